"""Batched aviary on one GPU: the Python owner of a ``gpd_sim`` (include/gpd.h).

``BatchedAviarySim`` holds the device state of ``n_envs`` identical aviaries (each with
``drones_per_env`` drones) and the caller-visible I/O buffers (torch tensors in HBM).  Every
call enqueues HIP work on the current torch stream of the sim's device; nothing here
computes physics on the CPU.
"""
import contextlib
import ctypes
import gc
import warnings

import numpy as np
import torch

from . import _lib
from .assets import default_params, model_id, parse_urdf
from .enums import ActionType, DroneModel, Physics

_ACTS = {ActionType.RPM: _lib.GPD_ACT_RPM, ActionType.ONE_D_RPM: _lib.GPD_ACT_ONE_D_RPM,
         ActionType.PID: _lib.GPD_ACT_PID, ActionType.VEL: _lib.GPD_ACT_VEL,
         ActionType.ONE_D_PID: _lib.GPD_ACT_ONE_D_PID}
PID_ACTS = (ActionType.PID, ActionType.VEL, ActionType.ONE_D_PID)
_TASKS = {"none": _lib.GPD_TASK_NONE, "hover": _lib.GPD_TASK_HOVER, "multihover": _lib.GPD_TASK_MULTIHOVER}
_AERO = {"gnd": _lib.GPD_F_GND, "drag": _lib.GPD_F_DRAG, "dw": _lib.GPD_F_DW, "geom": _lib.GPD_F_GEOM_WRENCH,
         "bullet": _lib.GPD_F_BULLET, "no_plane": _lib.GPD_F_NO_PLANE,
         "no_drone_contact": _lib.GPD_F_NO_DRONE_CONTACT}
_PHYSICS = {
    Physics.DYN: (),
    Physics.PYB: ("bullet",),
    Physics.PYB_GND: ("bullet", "gnd"),
    Physics.PYB_DRAG: ("bullet", "drag"),
    Physics.PYB_DW: ("bullet", "dw"),
    Physics.PYB_GND_DRAG_DW: ("bullet", "gnd", "drag", "dw"),
}
# cmd_step modes: (GPD_CMD_*, action width, actions in the sim's real dtype (else float32))
_CMD_MODES = {"rpm": (_lib.GPD_CMD_RPM, 4, True), "vel": (_lib.GPD_CMD_VEL, 4, False),
              "waypoint": (_lib.GPD_CMD_WAYPOINT, 7, True)}
_warned = set()


def _warn_once(key, msg):
    if key not in _warned:
        _warned.add(key)
        warnings.warn(msg, stacklevel=3)


def physics_flags(physics=Physics.DYN, aero=()):
    """Map a reference ``Physics`` value (+ extra force terms) to GPD_F_* flags.

    DYN is the reference's explicit integrator (BaseAviary.py:352-353).  The PYB* values apply
    the reference's forces (``_physics`` / ``_groundEffect`` / ``_drag`` / ``_downwash``,
    :679-811) to a restated Bullet3 multibody base step (``p.stepSimulation``, :369-370; SURVEY
    §8 f3): default damping, world-frame angular velocity, exponential-map orientation, and the
    collision cylinder's contact with the ground plane (``plane.urdf``, BaseAviary.py:484) and,
    in envs of several drones, with the env's other drones (every drone is a colliding body,
    :486-491; envs of more than 64 drones raise NotImplementedError unless ``no_drone_contact``).
    Known deviations of the contact restatement from pybullet (parity unpinned):
    one point per pair (Bullet keeps a 4-point manifold), and the pair rows are solved before the
    plane rows instead of in one island solve, so a drone resting on another that rests on the
    plane sinks into it until the ERP push balances (~1 cm).  ``aero`` adds terms by name
    (``gnd``, ``drag``, ``dw``, ``geom``, ``bullet``, ``no_plane``, ``no_drone_contact``), e.g.
    the aero terms on the DYN integrator (BASELINE config 3), ``no_plane`` for the reference's
    commented-out plane collision filter (:500-503), or ``no_drone_contact``.
    """
    physics = Physics(physics)
    terms = set(_PHYSICS[physics]) | set(aero)
    unknown = terms - set(_AERO)
    if unknown:
        raise ValueError(f"unknown aero terms {sorted(unknown)}; expected a subset of {sorted(_AERO)}")
    for t in ("no_plane", "no_drone_contact"):
        if t in terms and "bullet" not in terms:
            raise ValueError(f"'{t}' applies to the Physics.PYB* modes only (Physics.DYN has no contacts)")
    flags = 0
    for t in terms:
        flags |= _AERO[t]
    return flags


@contextlib.contextmanager
def graph_capture(graph, device):
    """``torch.cuda.graph(graph)`` on ``device`` with the cyclic garbage collector out of the way.

    Under capture (torch's global capture mode) destroying a ``torch.cuda.CUDAGraph`` is an error,
    and it is raised from the graph's destructor, which ends the process.  A graph held by a dead
    reference cycle (an object whose closures refer back to it, say) is destroyed whenever the
    cyclic collector next runs - possibly in the middle of a later capture; ``torch.cuda.graph``
    no longer collects on entry.  So: collect before the capture, keep the collector off during it."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.device(device), torch.cuda.graph(graph):
            yield
    finally:
        if was_enabled:
            gc.enable()


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_raw_stream_fn = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _raw_stream(index):
    """The current stream of device `index` as an integer handle (torch's raw accessor when this
    build has it: the eager step() is host-bound, and the Stream object costs a microsecond)."""
    if _raw_stream_fn is not None:
        return _raw_stream_fn(index)
    return torch.cuda.current_stream(index).cuda_stream


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


STATE_COLS = 12   # KIN observation: pos, rpy, vel, ang_v (BaseRLAviary.py:313-316) before the history


def pack_layout(n_envs, drones_per_env, obs_width, align=256):
    """Byte layout of a sim's output pack, ``gpd_pack_layout_of`` (include/gpd.h) restated:
    {field: (offset, nbytes)} for obs | reward | terminated | truncated | terminal_state |
    terminal_obs (each 256-B aligned), "prefix" = the end of the truncated flags,
    "prefix_aligned" = that rounded up to 256, "record" = the end of terminal_state (one rank's
    hand-off record, ``shard.LearnerHandoff``) and "total"."""
    E, D, W = n_envs, drones_per_env, obs_width
    out, off = {}, 0
    for name, nbytes in (("obs", E * D * W * 4), ("reward", E * 4), ("terminated", E), ("truncated", E),
                         ("terminal_state", E * D * STATE_COLS * 4), ("terminal_obs", E * D * W * 4)):
        out[name] = (off, nbytes)
        if name == "truncated":
            out["prefix"] = off + nbytes
            out["prefix_aligned"] = -(-(off + nbytes) // align) * align
        off += -(-nbytes // align) * align
        if name == "terminal_state":
            out["record"] = off
    out["total"] = off
    return out


def seq_segments(data_ptrs, slot_bytes):
    """Split a sequence of action tensors, given by their addresses, into the longest runs one
    ``gpd_step_seq`` call can express: ``[(base, n_slots, n_steps), ...]`` with tensor ``k`` of a
    run at ``base + (k % n_slots) * slot_bytes``.  A run grows while the tensors follow each other
    in memory; the first return to ``base`` fixes ``n_slots``, and the run then lasts as long as
    the tensors keep cycling through those slots.  Unrelated tensors are runs of one step."""
    ptrs = [int(p) for p in data_ptrs]
    out, i = [], 0
    while i < len(ptrs):
        base, n_slots, k = ptrs[i], None, 1
        while i + k < len(ptrs):
            p = ptrs[i + k]
            if n_slots is None and p == base:
                n_slots = k
            if p != base + (k % n_slots if n_slots else k) * slot_bytes:
                break
            k += 1
        out.append((base, n_slots or k, k))
        i += k
    return out


def env_param_rows(params, n_envs, env_params=None):
    """``gpd_env_params`` rows [E, 11] float64 (column order ``_lib.ENV_PARAM_NAMES``): the values of
    ``params`` (a ``_lib.DroneParams``) for every env, with the columns named in the dict
    ``env_params`` ({name: array[E] or scalar}) replaced."""
    rows = np.empty((int(n_envs), len(_lib.ENV_PARAM_NAMES)), dtype=np.float64)
    for k, name in enumerate(_lib.ENV_PARAM_NAMES):
        rows[:, k] = getattr(params, name)
    unknown = set(env_params or ()) - set(_lib.ENV_PARAM_NAMES)
    if unknown:
        raise ValueError(f"unknown env_params names {sorted(unknown)}; expected a subset of "
                         f"{list(_lib.ENV_PARAM_NAMES)}")
    for name, val in (env_params or {}).items():
        rows[:, _lib.ENV_PARAM_NAMES.index(name)] = np.broadcast_to(np.asarray(val, dtype=np.float64), (int(n_envs),))
    return np.ascontiguousarray(rows)


def _dptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


# set_pid_coefficients' keywords, in the order of a gain row's six triples (_lib.PID_GAIN_FIELDS)
PID_GAIN_KEYWORDS = ("p_coeff_pos", "i_coeff_pos", "d_coeff_pos", "p_coeff_att", "i_coeff_att", "d_coeff_att")


def pid_gain_rows(n_envs, drones_per_env, base, **coeffs):
    """``gpd_set_pid_gains`` rows [N, 18] float64 (N = ``n_envs * drones_per_env``; a row is the six
    coefficient triples in ``gpd_pid_params``' order).  ``base`` is a ``_lib.PidParams`` (its six
    triples for every drone) or an [N, 18] array.  Each keyword of ``set_pid_coefficients``
    (``p_coeff_pos`` ... ``d_coeff_att``) replaces its triple: shape (3,), (E, 3), (E, 1, 3) or
    (E, D, 3); ``None`` keeps the base.  Any other shape, and any non-finite value, is a ValueError."""
    E, D = int(n_envs), int(drones_per_env)
    if E < 1 or D < 1:
        raise ValueError(f"n_envs and drones_per_env must be >= 1, got {n_envs}, {drones_per_env}")
    unknown = set(coeffs) - set(PID_GAIN_KEYWORDS)
    if unknown:
        raise ValueError(f"unknown coefficient names {sorted(unknown)}; expected a subset of {list(PID_GAIN_KEYWORDS)}")
    rows = np.empty((E, D, 6, 3), dtype=np.float64)
    if isinstance(base, _lib.PidParams):
        for k, field in enumerate(_lib.PID_GAIN_FIELDS):
            rows[:, :, k, :] = np.array(list(getattr(base, field)), dtype=np.float64)
    else:
        b = np.asarray(base, dtype=np.float64)
        if b.shape != (E * D, _lib.PID_GAIN_COMPS):
            raise ValueError(f"base must be a PidParams or an array of shape {(E * D, _lib.PID_GAIN_COMPS)}, "
                             f"got shape {b.shape}")
        rows[:] = b.reshape(E, D, 6, 3)
    for k, name in enumerate(PID_GAIN_KEYWORDS):
        val = coeffs.get(name)
        if val is None:
            continue
        v = np.asarray(val, dtype=np.float64)
        if v.shape == (3,):
            v = v.reshape(1, 1, 3)
        elif v.shape == (E, 3):
            v = v.reshape(E, 1, 3)
        elif v.shape not in ((E, 1, 3), (E, D, 3)):
            raise ValueError(f"{name} must have shape (3,), ({E}, 3), ({E}, 1, 3) or ({E}, {D}, 3), got {v.shape}")
        rows[:, :, k, :] = v
    rows = np.ascontiguousarray(rows.reshape(E * D, _lib.PID_GAIN_COMPS))
    if not np.isfinite(rows).all():
        n, c = np.argwhere(~np.isfinite(rows))[0]
        raise ValueError(f"non-finite gain in row {n}, column {c}")
    return rows


_DERIVED = ("gravity", "hover_rpm", "max_rpm", "max_thrust", "max_xy_torque", "max_z_torque", "gnd_eff_h_clip")


def env_derive(params, rows):
    """``gpd_env_derive`` (host-only): the derived constants of ``rows`` [n, 11] on the drone
    ``params``, as a dict of [n] float64 arrays."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, len(_lib.ENV_PARAM_NAMES)))
    n = rows.shape[0]
    out = (_lib.Constants * max(n, 1))()
    _lib.check("gpd_env_derive", _lib.load().gpd_env_derive(ctypes.byref(params), _dptr(rows), n, out))
    return {name: np.array([getattr(out[i], name) for i in range(n)], dtype=np.float64) for name in _DERIVED}


def _mix32(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    return x ^ (x >> 16)


def reset_pool_draw(seed, stream, env, episode, n):
    """``gpd_reset_pool_draw`` restated in Python ints: the index in [0, n) that env ``env`` draws
    at its ``episode``-th auto-reset from a reset pool of ``n`` entries (``stream`` 1: parameter
    rows, 2: poses).  uint32 arithmetic, then one 32x32 -> 64 multiply."""
    seed, stream, env, episode, n = int(seed), int(stream), int(env), int(episode), int(n)
    if n < 1:
        return 0
    h = _mix32((seed ^ (0x9e3779b9 * stream)) & 0xffffffff)
    h = _mix32((h + env) & 0xffffffff)
    h = _mix32((h + episode) & 0xffffffff)
    return (h * n) >> 32


class BatchedAviarySim:
    """``n_envs`` x ``drones_per_env`` Crazyflie-class drones stepped in lockstep on one GPU.

    ``env_params`` ({name: array[E]} over any subset of ``_lib.ENV_PARAM_NAMES``) and / or
    ``initial_xyzs`` / ``initial_rpys`` of shape (E, D, 3) make the sim heterogeneous (``sim.het``):
    every env with its own drone parameters, every drone of every env with its own start pose
    (``gpd_create_het``).  Het sims run Physics.DYN (with any of the gnd / drag / dw / geom terms) and
    the RPM action types; anything else raises NotImplementedError.

    ``reset_pool=dict(env_params={name: array[P]}, initial_xyzs=(Q, D, 3), initial_rpys=(Q, D, 3),
    seed=0)`` (every key optional) also makes the sim heterogeneous and gives each env a new drone and
    start pose, drawn from the pools on the device, at every auto-reset (:meth:`set_reset_pool`)."""

    def __init__(self, n_envs, drones_per_env=1, drone_model=DroneModel.CF2X, urdf_path=None,
                 pyb_freq=240, ctrl_freq=30, act=ActionType.RPM, task="hover",
                 physics=Physics.DYN, aero=(), precision="f64", autoreset=True, episode_len_sec=8,
                 initial_xyzs=None, initial_rpys=None, device=None, tuning=None, env_params=None,
                 reset_pool=None):
        self._lib = _lib.load()
        act = ActionType(act)
        if env_params is not None or reset_pool is not None \
                or any(a is not None and np.ndim(a) == 3 for a in (initial_xyzs, initial_rpys)):
            # a heterogeneous sim: what it cannot run is refused, never silently dropped
            if physics_flags(physics, aero) & _lib.GPD_F_BULLET:
                raise NotImplementedError(
                    f"per-env parameters / start poses with {Physics(physics)}"
                    f"{' + bullet' if 'bullet' in aero else ''}: the PYB* contact solves hold mass and inertia in "
                    "derived rows; pass physics=Physics.DYN (aero terms gnd / drag / dw / geom are supported)")
            if act in PID_ACTS:
                raise NotImplementedError(f"per-env parameters / start poses with {act}: DSLPIDControl is tuned for "
                                          "the nominal drone; use ActionType.RPM or ActionType.ONE_D_RPM")
            if int(drones_per_env) > 64:
                raise NotImplementedError("per-env parameters / start poses need drones_per_env <= 64 (the "
                                          "multi-wave step kernel has no per-env parameters)")
        if not torch.cuda.is_available():
            raise _lib.GpdLibraryError("BatchedAviarySim needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if precision not in ("f32", "f64"):
            raise ValueError("precision must be 'f32' or 'f64'")
        if precision == "f32":
            _warn_once("f32", "precision='f32' does not meet the 1e-5 state-parity gate over 5 s (open-loop "
                       "attitude dynamics amplify float32 rounding to 1e-5..2e-4; DESIGN.md §5); f64 is the "
                       "reference's precision and costs about the same on MI355X")
        self.drone_model = DroneModel(drone_model)
        self.params = parse_urdf(urdf_path, self.drone_model) if urdf_path else default_params(self.drone_model)
        self.params.model = model_id(self.drone_model)
        self.n_envs, self.drones_per_env = int(n_envs), int(drones_per_env)
        self.act_type = act
        self.task = task
        self.precision = precision
        self.real_dtype = torch.float32 if precision == "f32" else torch.float64
        cfg = _lib.Config()
        cfg.n_envs = self.n_envs
        cfg.drones_per_env = self.drones_per_env
        cfg.pyb_freq = int(pyb_freq)
        cfg.ctrl_freq = int(ctrl_freq)
        cfg.act_type = _ACTS[act]
        cfg.task = _TASKS[task]
        cfg.physics_flags = physics_flags(physics, aero)
        if cfg.physics_flags & _lib.GPD_F_BULLET and self.drones_per_env > 64 \
                and not cfg.physics_flags & _lib.GPD_F_NO_DRONE_CONTACT:
            # a physics term is never dropped silently: the multi-wave kernels do not restate it
            raise NotImplementedError(
                f"{Physics(physics)} with {self.drones_per_env} drones per env: the drone <-> drone contact is "
                "implemented for envs of up to 64 drones; pass aero=('no_drone_contact',) to run larger "
                "PYB* envs without it")
        cfg.precision = _lib.GPD_F32 if precision == "f32" else _lib.GPD_F64
        cfg.autoreset = 1 if autoreset else 0
        cfg.episode_len_sec = float(episode_len_sec)
        # launch tuning (gpd_config: drones_per_block, step_waves, store_policy; 0 = automatic) and
        # the PYB* contact solver's numSolverIterations / solverResidualThreshold (0 = pybullet's)
        for name, val in (tuning or {}).items():
            if name == "solver_residual":
                cfg.solver_residual = float(val)
                continue
            if name not in ("drones_per_block", "step_waves", "store_policy", "solver_iterations"):
                raise ValueError(f"unknown tuning field {name!r}")
            setattr(cfg, name, int(val))
        keep = []
        het_poses = {}
        for name, arr in (("init_xyzs_host", initial_xyzs), ("init_rpys_host", initial_rpys)):
            if arr is not None:
                a = np.asarray(arr, dtype=np.float64)
                if a.ndim == 3:      # (E, D, 3): per-env start poses
                    het_poses[name] = self._pose_table(a)
                    continue
                a = np.ascontiguousarray(a.reshape(self.drones_per_env, 3))
                keep.append(a)
                setattr(cfg, name, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        self.physics_flags = cfg.physics_flags
        self.het = env_params is not None or bool(het_poses) or reset_pool is not None
        self._pool_rows = np.empty((0, len(_lib.ENV_PARAM_NAMES)))
        handle = ctypes.c_void_p()
        if self.het:
            self._env_rows = env_param_rows(self.params, self.n_envs, env_params)
            with torch.cuda.device(self.device):
                rc = self._lib.gpd_create_het(ctypes.byref(self.params), ctypes.byref(cfg), _dptr(self._env_rows),
                                              _dptr(het_poses.get("init_xyzs_host")),
                                              _dptr(het_poses.get("init_rpys_host")), ctypes.byref(handle))
            if rc == _lib.GPD_EUNSUPPORTED:
                raise NotImplementedError(self._lib.gpd_last_error().decode(errors="replace"))
            _lib.check("gpd_create_het", rc)
        else:
            with torch.cuda.device(self.device):
                _lib.check("gpd_create", self._lib.gpd_create(ctypes.byref(self.params), ctypes.byref(cfg),
                                                              ctypes.byref(handle)))
        self._h = handle
        k = _lib.Constants()
        _lib.check("gpd_get_constants", self._lib.gpd_get_constants(self._h, ctypes.byref(k)))
        self.constants = k
        self.n_drones = k.n_drones
        self.obs_width = k.obs_width
        self.act_width = k.act_width
        self.pyb_steps_per_ctrl = k.pyb_steps_per_ctrl
        E, D, W = self.n_envs, self.drones_per_env, self.obs_width
        dev = self.device
        # every per-step output lives in ONE device buffer ("out pack"), so that a sharded run hands
        # a step to the learner with a single collective over the kernel's own output bytes
        # (shard.LearnerHandoff): [obs | reward | terminated | truncated | terminal_obs], each field
        # 256-B aligned; the terminal rows come last so that a hand-off without them is a prefix
        self.pack_layout = pack_layout(E, D, W)
        L = self.pack_layout
        self.out_pack = torch.zeros((L["total"],), dtype=torch.uint8, device=dev)
        self.obs = self._field("obs", torch.float32, (E, D, W))
        self.reward = self._field("reward", torch.float32, (E,))
        self.terminated = self._field("terminated", torch.uint8, (E,))
        self.truncated = self._field("truncated", torch.uint8, (E,))
        self.terminal_obs = self._field("terminal_obs", torch.float32, (E, D, W))
        # the sim-owned output buffers never move: their ctypes pointers are built once (the eager
        # step() is host-bound at 4096 envs, a few microseconds per call)
        self._step_fn = self._lib.gpd_step
        self._out_ptrs = (_ptr(self.obs), _ptr(self.reward), _ptr(self.terminated), _ptr(self.truncated))
        self._tobs_ptr = _ptr(self.terminal_obs)
        self._obs20 = None              # cmd_step's [E, D, 20] rows, allocated on first use (not in out_pack)
        self.reset()
        if reset_pool is not None:
            self.set_reset_pool(reset_pool)

    # ------------------------------------------------------------------ heterogeneous sims
    def _pose_table(self, arr):
        a = np.asarray(arr, dtype=np.float64)
        if a.shape != (self.n_envs, self.drones_per_env, 3):
            raise ValueError(f"per-env poses must have shape ({self.n_envs}, {self.drones_per_env}, 3), got {a.shape}")
        return np.ascontiguousarray(a)

    def _need_het(self, what):
        if not self.het:
            raise ValueError(f"{what} needs a heterogeneous sim: create it with env_params= or (E, D, 3) start poses")

    def set_env_params(self, env_params):
        """Replace the per-env drone parameters (``gpd_set_env_params``): ``env_params`` is a dict
        {name: array[E]}; names it leaves out keep their current per-env values.  A synchronous
        upload that changes no launch geometry: a captured graph stays valid.  Acts from the next step."""
        self._need_het("set_env_params")
        rows = self._rows_in_force()
        fresh = env_param_rows(self.params, self.n_envs, env_params)
        for name in env_params:
            k = _lib.ENV_PARAM_NAMES.index(name)
            rows[:, k] = fresh[:, k]
        with torch.cuda.device(self.device):
            self._call("gpd_set_env_params", _dptr(rows))
        self._env_rows = rows

    def set_initial_poses(self, xyzs=None, rpys=None):
        """Replace the per-env start poses (``gpd_set_env_init``), each (E, D, 3) or None to keep.
        They take effect at the next reset or auto-reset; MultiHover targets follow them."""
        self._need_het("set_initial_poses")
        x = self._pose_table(xyzs) if xyzs is not None else None
        r = self._pose_table(rpys) if rpys is not None else None
        with torch.cuda.device(self.device):
            self._call("gpd_set_env_init", _dptr(x), _dptr(r))

    def set_reset_pool(self, reset_pool):
        """Install the pools an env draws its next drone and start pose from at each auto-reset
        (``gpd_set_reset_pool``), or clear them with None.  ``reset_pool`` is a dict, every key
        optional: ``env_params`` {name: array[P]} (names left out take the nominal drone, as
        ``env_param_rows`` does), ``initial_xyzs`` / ``initial_rpys`` (Q, D, 3), ``seed``.  Without
        ``env_params`` the parameters are never redrawn, without ``initial_xyzs`` the poses.  The
        draw is :func:`reset_pool_draw` of (seed, stream, env, episode number); :meth:`reset` draws
        nothing.  A synchronous upload.  What the old pools drew stays in force as the env's own row
        and pose.  Replacing a pool by another of any size keeps a captured graph valid; turning
        a pool on or off launches another kernel, so graphs captured before must be re-captured.
        Checkpoints carry neither pools nor draws."""
        self._need_het("set_reset_pool")
        pool = dict(reset_pool or {})
        unknown = set(pool) - {"env_params", "initial_xyzs", "initial_rpys", "seed"}
        if unknown:
            raise ValueError(f"unknown reset_pool keys {sorted(unknown)}")
        ep = pool.get("env_params")
        rows = np.empty((0, len(_lib.ENV_PARAM_NAMES)))
        if ep is not None:
            sizes = {np.size(v) for v in ep.values() if np.ndim(v) > 0}
            if len(sizes) > 1:
                raise ValueError(f"reset_pool env_params arrays differ in length: {sorted(sizes)}")
            rows = env_param_rows(self.params, sizes.pop() if sizes else 1, ep)
        poses = []
        for name in ("initial_xyzs", "initial_rpys"):
            a = pool.get(name)
            if a is not None:
                a = np.asarray(a, dtype=np.float64)
                if a.ndim != 3 or a.shape[1:] != (self.drones_per_env, 3):
                    raise ValueError(f"reset_pool {name} must have shape (Q, {self.drones_per_env}, 3), got {a.shape}")
                a = np.ascontiguousarray(a)
            poses.append(a)
        x, r = poses
        if r is not None and (x is None or r.shape != x.shape):
            raise ValueError("reset_pool initial_rpys needs initial_xyzs of the same shape")
        in_force = self._rows_in_force()
        with torch.cuda.device(self.device):
            self._call("gpd_set_reset_pool", _dptr(rows) if len(rows) else None, len(rows), _dptr(x), _dptr(r),
                       0 if x is None else x.shape[0], int(pool.get("seed", 0)) & 0xffffffff)
        self._env_rows, self._pool_rows = in_force, rows

    def reset_draws(self):
        """[E, 3] int32 on the device (``gpd_get_reset_draws``): each env's episode number (0 at
        create, +1 at each auto-reset), parameter-pool row in force and pose-pool index in force;
        -1 = not drawn (the env's create / set_env_params / set_initial_poses value)."""
        self._need_het("reset_draws")
        out = torch.empty((self.n_envs, 3), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._call("gpd_get_reset_draws", _ptr(out), _stream(self.device))
        return out

    def env_table(self):
        """Diagnostic (``gpd_get_env_table``): the device's per-env constant table, [E, 18] float64
        on the host."""
        self._need_het("env_table")
        out = np.empty((self.n_envs, 18), dtype=np.float64)
        with torch.cuda.device(self.device):
            self._call("gpd_get_env_table", _dptr(out))
        return out

    def _rows_in_force(self):
        """[E, 11]: the pool row where an env's drawn row index is >= 0, its own row otherwise."""
        if not self.het:
            return env_param_rows(self.params, self.n_envs)
        rows = self._env_rows.copy()
        if len(self._pool_rows):
            idx = self.reset_draws()[:, 1].cpu().numpy()
            rows[idx >= 0] = self._pool_rows[idx[idx >= 0]]
        return rows

    @property
    def env_params(self):
        """The per-env parameters in force as {name: array[E]} (every env nominal on a plain sim):
        with a reset pool, the drawn pool row of the envs that have drawn one."""
        rows = self._rows_in_force()
        return {name: rows[:, k].copy() for k, name in enumerate(_lib.ENV_PARAM_NAMES)}

    @property
    def env_constants(self):
        """Per-env derived constants (BaseAviary.py:117-128) from ``gpd_env_derive``: a dict of [E]
        float64 arrays (gravity, hover_rpm, max_rpm, max_thrust, max_xy_torque, max_z_torque,
        gnd_eff_h_clip)."""
        return env_derive(self.params, self._rows_in_force())

    def _field(self, name, dtype, shape):
        off, n = self.pack_layout[name]
        return self.out_pack[off:off + n].view(dtype).view(shape)

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None):
            self._lib.gpd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args):
        _lib.check(name, getattr(self._lib, name)(self._h, *args))

    # ------------------------------------------------------------------ RL surface
    def reset(self, env_mask=None):
        """BaseAviary.reset (:220-255) for all envs or the envs where ``env_mask`` is true."""
        m = None
        if env_mask is not None:
            m = torch.as_tensor(env_mask, device=self.device).to(torch.uint8).contiguous()
            assert m.numel() == self.n_envs
        with torch.cuda.device(self.device):
            self._call("gpd_reset", _ptr(m), _ptr(self.obs), _stream(self.device))
        return self.obs

    def step(self, actions, terminal_obs=True):
        """BaseAviary.step (:259-383) for every env; ``actions`` [E, D, A] float32 on the device.

        Returns the sim-owned (obs, reward, terminated, truncated) tensors; they are
        overwritten by the next call.  With autoreset, ``self.terminal_obs`` holds the final
        rows of the envs that finished in this step."""
        a = actions
        if not (isinstance(a, torch.Tensor) and a.device == self.device and a.dtype == torch.float32
                and a.is_contiguous()):
            a = torch.as_tensor(a, dtype=torch.float32, device=self.device).contiguous()
        if a.numel() != self.n_drones * self.act_width:
            raise ValueError(f"actions must have {self.n_envs}x{self.drones_per_env}x{self.act_width} elements")
        tptr = self._tobs_ptr if terminal_obs else None
        if torch.cuda.current_device() == self.device.index:
            rc = self._step_fn(self._h, a.data_ptr(), *self._out_ptrs, tptr, _raw_stream(self.device.index))
        else:
            with torch.cuda.device(self.device):
                rc = self._step_fn(self._h, a.data_ptr(), *self._out_ptrs, tptr, _stream(self.device))
        if rc != 0:
            self._step_failed("gpd_step", rc)
        return self.obs, self.reward, self.terminated, self.truncated

    def step_seq(self, action_slots, n_steps, terminal_obs=True):
        """``n_steps`` consecutive :meth:`step` calls issued from native code (``gpd_step_seq``):
        step t reads ``action_slots[t % P]`` of ``action_slots`` [P, E, D, A] (float32, on the
        device); the output tensors hold the last step's results."""
        a = action_slots
        if not (isinstance(a, torch.Tensor) and a.device == self.device and a.dtype == torch.float32
                and a.is_contiguous() and a.numel() % (self.n_drones * self.act_width) == 0):
            raise ValueError("step_seq needs contiguous float32 action slots [P, E, D, A] on the sim's device")
        P = a.numel() // (self.n_drones * self.act_width)
        self._step_seq_at(a.data_ptr(), P, n_steps, terminal_obs)
        return self.obs, self.reward, self.terminated, self.truncated

    def _step_seq_at(self, base, n_slots, n_steps, terminal_obs):
        tptr = self._tobs_ptr if terminal_obs else None
        with torch.cuda.device(self.device):
            rc = self._lib.gpd_step_seq(self._h, ctypes.c_void_p(base), int(n_slots), int(n_steps), *self._out_ptrs,
                                        tptr, _stream(self.device))
        if rc != 0:
            self._step_failed("gpd_step_seq", rc)

    def capture_graph(self, actions_seq, terminal_obs=True):
        """Record ``len(actions_seq)`` consecutive :meth:`step` calls into one HIP graph
        (``torch.cuda.CUDAGraph``).  Each ``replay()`` advances every env by that many steps,
        reading the given action tensors (refill them in place between replays).  The launches
        have fixed arguments - the ring head and step counters live in device memory - so one
        recorded sequence stays valid for any number of replays.  Capture records only; the sim
        does not advance until the first replay.

        Tensors that follow each other in memory, or cycle through such a run of slots
        (``[pool[k % P] for k in range(K)]``, one tensor repeated), are recorded as one
        ``gpd_step_seq`` call (:func:`seq_segments`), which the sims of the three-wave step kernel
        run as one fused launch per 256 steps; unrelated tensors are one launch each."""
        seq = []
        for a in actions_seq:
            if not (isinstance(a, torch.Tensor) and a.device == self.device and a.dtype == torch.float32
                    and a.is_contiguous() and a.numel() == self.n_drones * self.act_width):
                raise ValueError("capture_graph needs contiguous float32 action tensors on the sim's device")
            seq.append(a)
        segments = seq_segments([a.data_ptr() for a in seq], self.n_drones * self.act_width * 4)
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, self.device):
            k = 0
            for base, n_slots, n_steps in segments:
                if n_steps == 1:
                    self.step(seq[k], terminal_obs=terminal_obs)
                else:
                    self._step_seq_at(base, n_slots, n_steps, terminal_obs)
                k += n_steps
        return g

    # ------------------------------------------------------------------ command step (CtrlAviary / VelocityAviary)
    def cmd_step(self, actions, mode="rpm"):
        """One ``env.step()`` of the reference's CtrlAviary / VelocityAviary for every env, in one
        launch (``gpd_cmd_step``).  ``mode``:

        * ``"rpm"``: ``actions`` [E, D, 4] in the sim's real dtype, clipped to [0, MAX_RPM]
          (CtrlAviary.py:140);
        * ``"vel"``: ``actions`` [E, D, 4] float32 velocity commands through DSLPIDControl
          (VelocityAviary.py:148-168);
        * ``"waypoint"``: ``actions`` [E, D, 7] real = target_pos(3), target yaw, target_vel(3):
          ``DSLPIDControl.computeControl`` on the device (the loop of the reference's examples/pid.py).

        ``"vel"`` and ``"waypoint"`` need a sim created with a PID action type.  Returns the
        sim-owned [E, D, 20] state vectors (real dtype), overwritten by the next call.  No
        reward / done flags / auto-reset; the RL step's action history is left alone."""
        try:
            code, width, real = _CMD_MODES[mode]
        except KeyError:
            raise ValueError(f"mode must be one of {sorted(_CMD_MODES)}, got {mode!r}") from None
        dtype = self.real_dtype if real else torch.float32
        a = actions
        if not (isinstance(a, torch.Tensor) and a.device == self.device and a.dtype == dtype and a.is_contiguous()):
            a = torch.as_tensor(a, dtype=dtype, device=self.device).contiguous()
        if a.numel() != self.n_drones * width:
            raise ValueError(f"actions must have {self.n_envs}x{self.drones_per_env}x{width} elements")
        if self.het:
            raise NotImplementedError("cmd_step is not supported on a heterogeneous sim (the command step kernels "
                                      "read the sim-wide drone parameters)")
        with torch.cuda.device(self.device):
            self._call("gpd_cmd_step", code, _ptr(a), _ptr(self._cmd_rows()), _stream(self.device))
        return self._obs20

    def _cmd_rows(self):
        if self._obs20 is None:
            self._obs20 = torch.zeros((self.n_envs, self.drones_per_env, 20), dtype=self.real_dtype,
                                      device=self.device)
        return self._obs20

    def capture_cmd_graph(self, actions_seq, mode="rpm"):
        """:meth:`capture_graph` for :meth:`cmd_step`: ``len(actions_seq)`` consecutive command
        steps in one HIP graph.  gpd_cmd_step keeps no host state (the step counters live in
        device memory), so a recorded sequence stays valid for any number of replays; the action
        tensors must already be what ``cmd_step`` passes on (device, dtype, contiguous)."""
        _, width, real = _CMD_MODES[mode]
        dtype = self.real_dtype if real else torch.float32
        for a in actions_seq:
            if not (isinstance(a, torch.Tensor) and a.device == self.device and a.dtype == dtype
                    and a.is_contiguous() and a.numel() == self.n_drones * width):
                raise ValueError(f"capture_cmd_graph needs contiguous {dtype} action tensors on the sim's device")
        self._cmd_rows()    # allocated outside the capture
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, self.device):
            for a in actions_seq:
                self.cmd_step(a, mode)
        return g

    def cmd_rollout(self, actions, mode="rpm", record_every=1, record=True, metrics=False, max_steps_per_launch=0):
        """``T`` consecutive :meth:`cmd_step` calls with the on-device controller in the loop, in one
        launch per ``max_steps_per_launch`` steps (``gpd_cmd_rollout``; 0 = the library's default of
        256): the drones stay in registers between the steps.  ``actions`` [T, E, D, w] with
        ``cmd_step``'s widths and dtypes for ``mode``.

        Returns ``(traj, obs20, metrics)``: ``traj`` [T // record_every, E, D, 20], the state vectors
        after steps ``record_every``, ``2 * record_every``, ... (None with ``record=False``);
        ``obs20`` the sim-owned [E, D, 20] buffer ``cmd_step`` returns, holding the last step's rows;
        ``metrics`` [E, D, 2] (``"waypoint"`` only, None unless asked for): the sum over the steps
        of the squared distance to the step's target position, and the largest distance.  ``traj``
        and ``metrics`` are fresh tensors.  The sim ends exactly where T ``cmd_step`` calls leave it."""
        try:
            code, width, real = _CMD_MODES[mode]
        except KeyError:
            raise ValueError(f"mode must be one of {sorted(_CMD_MODES)}, got {mode!r}") from None
        dtype = self.real_dtype if real else torch.float32
        a = actions
        if not (isinstance(a, torch.Tensor) and a.device == self.device and a.dtype == dtype and a.is_contiguous()):
            a = torch.as_tensor(a, dtype=dtype, device=self.device).contiguous()
        per = self.n_drones * width
        if a.dim() < 1 or a.numel() != a.shape[0] * per:
            raise ValueError(f"actions must have Tx{self.n_envs}x{self.drones_per_env}x{width} elements")
        T, E, D = int(a.shape[0]), self.n_envs, self.drones_per_env
        if int(record_every) < 1:
            raise ValueError(f"record_every must be >= 1, got {record_every}")
        if metrics and mode != "waypoint":
            raise ValueError("metrics=True needs mode='waypoint' (the tracking error is measured against the "
                             "waypoints' target positions)")
        if self.het:
            raise NotImplementedError("cmd_rollout is not supported on a heterogeneous sim (the command step kernels "
                                      "read the sim-wide drone parameters)")
        traj = torch.empty((T // int(record_every), E, D, 20), dtype=self.real_dtype, device=self.device) \
            if record else None
        met = torch.zeros((E, D, 2), dtype=self.real_dtype, device=self.device) if metrics else None
        with torch.cuda.device(self.device):
            self._call("gpd_cmd_rollout", code, _ptr(a), T, int(record_every), _ptr(traj), _ptr(self._cmd_rows()),
                       _ptr(met), int(max_steps_per_launch), _stream(self.device))
        return traj, self._obs20, met

    def adjacency(self, radius=np.inf):
        """BaseAviary._getAdjacencyMatrix (:658-675) of every env: [E, D, D] uint8 on the device."""
        out = torch.empty((self.n_envs, self.drones_per_env, self.drones_per_env), dtype=torch.uint8,
                          device=self.device)
        with torch.cuda.device(self.device):
            self._call("gpd_adjacency", float(radius), _ptr(out), _stream(self.device))
        return out

    # ------------------------------------------------------------------ raw physics
    def integrate(self, rpm, record=False):
        """Raw DYN substeps: ``rpm`` [T, N, 4] (real dtype) -> optional trajectory [T, N, 20]."""
        r = torch.as_tensor(rpm, dtype=self.real_dtype, device=self.device).contiguous()
        T = r.shape[0]
        assert r.numel() == T * self.n_drones * 4
        traj = torch.empty((T, self.n_drones, 20), dtype=self.real_dtype, device=self.device) if record else None
        with torch.cuda.device(self.device):
            self._call("gpd_integrate", _ptr(r), int(T), _ptr(traj), _stream(self.device))
        return traj

    def state20(self):
        """BaseAviary._getDroneStateVector (:541-561) for every drone, [N, 20]."""
        out = torch.empty((self.n_drones, 20), dtype=self.real_dtype, device=self.device)
        with torch.cuda.device(self.device):
            self._call("gpd_get_state20", _ptr(out), _stream(self.device))
        return out

    def nonfinite(self):
        """Per-env non-finite guard (the reference has none): bool [E] on the device,
        True where any drone of the env holds a non-finite state component."""
        out = torch.empty((self.n_envs,), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._call("gpd_nonfinite", _ptr(out), _stream(self.device))
        return out.bool()

    def raw_state(self):
        out = torch.empty((self.n_drones, 20), dtype=self.real_dtype, device=self.device)
        with torch.cuda.device(self.device):
            self._call("gpd_get_raw_state", _ptr(out), _stream(self.device))
        return out

    def set_raw_state(self, raw):
        r = torch.as_tensor(raw, dtype=self.real_dtype, device=self.device).contiguous()
        assert r.numel() == self.n_drones * 20
        with torch.cuda.device(self.device):
            self._call("gpd_set_raw_state", _ptr(r), _stream(self.device))

    # ------------------------------------------------------------------ DSLPIDControl (PID types)
    def ctrl_state(self):
        """Per-drone controller state [N, 9]: integral_pos_e, integral_rpy_e, last_rpy
        (DSLPIDControl.py:65-78); only for the PID / VEL / ONE_D_PID action types."""
        out = torch.empty((self.n_drones, _lib.CTRL_COMPS), dtype=self.real_dtype, device=self.device)
        with torch.cuda.device(self.device):
            self._call("gpd_get_ctrl_state", _ptr(out), _stream(self.device))
        return out

    def set_ctrl_state(self, cs):
        t = torch.as_tensor(cs, dtype=self.real_dtype, device=self.device).contiguous()
        assert t.numel() == self.n_drones * _lib.CTRL_COMPS
        with torch.cuda.device(self.device):
            self._call("gpd_set_ctrl_state", _ptr(t), _stream(self.device))

    def set_pid_coefficients(self, p_coeff_pos=None, i_coeff_pos=None, d_coeff_pos=None,
                             p_coeff_att=None, i_coeff_att=None, d_coeff_att=None):
        """BaseControl.setPIDCoefficients (control/BaseControl.py:138-177) for every drone."""
        q = getattr(self, "_pid", None) or _lib.default_pid_params()
        for name, val in (("p_coeff_for", p_coeff_pos), ("i_coeff_for", i_coeff_pos), ("d_coeff_for", d_coeff_pos),
                          ("p_coeff_tor", p_coeff_att), ("i_coeff_tor", i_coeff_att), ("d_coeff_tor", d_coeff_att)):
            if val is not None:
                v = np.asarray(val, dtype=np.float64).reshape(3)
                getattr(q, name)[:] = v.tolist()
        with torch.cuda.device(self.device):
            _lib.check("gpd_set_pid_params", self._lib.gpd_set_pid_params(self._h, ctypes.byref(q)))
        self._pid = q

    def set_pid_gains(self, **coeffs):
        """Every drone's own DSLPIDControl coefficients (``gpd_set_pid_gains``): starts from the gains
        in force (:meth:`pid_gains`) and replaces the triples given, each broadcast from (3,), (E, 3),
        (E, 1, 3) or (E, D, 3) (:func:`pid_gain_rows`; the keywords of :meth:`set_pid_coefficients`).
        While the table is in force, ``cmd_step`` / ``cmd_rollout`` in the ``"vel"`` and ``"waypoint"``
        modes run each drone's controller on its own row, and :meth:`step` is refused (the RL step
        reads the sim-wide coefficients).  Installing the first table or clearing it changes which
        kernel the command step launches: recapture a graph recorded on the other side; a later
        call that only changes values keeps a captured graph valid.  Synchronous."""
        rows = pid_gain_rows(self.n_envs, self.drones_per_env, self._pid_gain_rows(), **coeffs)
        with torch.cuda.device(self.device):
            self._call("gpd_set_pid_gains", _dptr(rows))

    def _pid_gain_rows(self):
        rows = np.empty((self.n_drones, _lib.PID_GAIN_COMPS), dtype=np.float64)
        self._call("gpd_get_pid_gains", _dptr(rows))
        return rows

    def pid_gains(self):
        """The coefficients in force for every drone (``gpd_get_pid_gains``): a dict of (E, D, 3)
        float64 arrays under the keywords of :meth:`set_pid_gains`; the table's values as stored, or
        the sim-wide triples repeated when no table is in force."""
        rows = self._pid_gain_rows().reshape(self.n_envs, self.drones_per_env, 6, 3)
        return {name: np.ascontiguousarray(rows[:, :, k, :]) for k, name in enumerate(PID_GAIN_KEYWORDS)}

    def clear_pid_gains(self):
        """Put the sim-wide coefficients (:meth:`set_pid_coefficients`) back in force for every drone."""
        self._call("gpd_set_pid_gains", None)

    def _step_failed(self, name, rc):
        """The library's refusal of an RL step while a gain table is in force (it launches nothing;
        whether a table is in force is the library's to know) as NotImplementedError; else GpdError."""
        msg = self._lib.gpd_last_error().decode(errors="replace")
        if rc == _lib.GPD_EUNSUPPORTED and "gain table" in msg:
            raise NotImplementedError(f"{msg}: call clear_pid_gains() first")
        _lib.check(name, rc)

    def step_counters(self):
        out = torch.empty((self.n_envs,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._call("gpd_get_step_counters", _ptr(out), _stream(self.device))
        return out

    def set_step_counters(self, sc):
        t = torch.as_tensor(sc, dtype=torch.int32, device=self.device).contiguous()
        with torch.cuda.device(self.device):
            self._call("gpd_set_step_counters", _ptr(t), _stream(self.device))

    def save_state(self):
        n = self._lib.gpd_state_bytes(self._h)
        buf = ctypes.create_string_buffer(n)
        with torch.cuda.device(self.device):
            self._call("gpd_save_state", ctypes.cast(buf, ctypes.c_void_p), _stream(self.device))
        return buf.raw

    def load_state(self, blob):
        n = self._lib.gpd_state_bytes(self._h)
        if len(blob) != n:
            raise ValueError(f"state blob has {len(blob)} bytes, expected {n}")
        buf = ctypes.create_string_buffer(blob, n)
        with torch.cuda.device(self.device):
            self._call("gpd_load_state", ctypes.cast(buf, ctypes.c_void_p), _stream(self.device))
