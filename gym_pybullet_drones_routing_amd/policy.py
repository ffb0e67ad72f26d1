"""Fused rollout policy: the ctypes binding of ``include/gpd_policy.h`` (``libgpd_policy.so``).

The caller of the env step in the reference is stable-baselines3 PPO (``examples/learn.py:52-94``):
per env.step its rollout runs the MlpPolicy actor and critic ([64, 64] tanh), samples
Normal(mu, exp(log_std)), clips the action to the Box, writes the rollout buffer and, after the
step, bootstraps time-limit truncations with V(terminal_observation).  ``MlpPolicyKernel`` does
all of that in ONE HIP kernel per step (``gpd_policy_rollout_step``) reading the torch module's
parameters in place, and GAE in one more per rollout (``gpd_policy_gae``).  There is no torch
fallback: without the library every call raises ``GpdLibraryError``.
"""
import ctypes
import os
import pathlib

import torch

from ._lib import GpdError, GpdLibraryError

LIB_PATH = pathlib.Path(os.environ.get("GPD_POLICY_LIB") or (pathlib.Path(__file__).resolve().parent /
                                                               "libgpd_policy.so"))
GPD_POLICY_ABI_VERSION = 2
GROUP_ROWS = 16                 # rows per Philox call counter (the kernel's row group)
HIDDEN = 64
MAX_OBS = 192
MAX_ACT = 8
EXPORTED = ("gpd_policy_rollout_step", "gpd_policy_gae", "gpd_policy_abi_version", "gpd_policy_last_error",
            "gpd_policy_n_params", "gpd_policy_ppo_grad_workspace", "gpd_policy_ppo_grad")
PARAM_NAMES = ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "pi_w3", "pi_b3", "vf_w1", "vf_b1", "vf_w2", "vf_b2", "vf_w3",
               "vf_b3", "log_std")


class MlpPolicyStruct(ctypes.Structure):
    _fields_ = [("n_obs", ctypes.c_int), ("n_act", ctypes.c_int)] + [(n, ctypes.c_void_p) for n in PARAM_NAMES]


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise GpdLibraryError(f"{LIB_PATH} is missing: run `python -m gym_pybullet_drones_routing_amd._build` "
                              "(or __graft_entry__.build())")
    try:
        lib = ctypes.CDLL(str(LIB_PATH))
    except OSError as exc:
        raise GpdLibraryError(f"cannot load {LIB_PATH}: {exc}") from exc
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.gpd_policy_abi_version.restype = ci
    lib.gpd_policy_abi_version.argtypes = []
    lib.gpd_policy_last_error.restype = ctypes.c_char_p
    lib.gpd_policy_last_error.argtypes = []
    lib.gpd_policy_rollout_step.restype = ci
    lib.gpd_policy_rollout_step.argtypes = [ctypes.POINTER(MlpPolicyStruct), ci, vp, vp, vp, vp, vp, vp, ci, vp, ci,
                                            vp, vp, vp, vp, ctypes.c_float, vp, vp, vp]
    lib.gpd_policy_gae.restype = ci
    lib.gpd_policy_gae.argtypes = [ci, ci, vp, vp, vp, vp, ctypes.c_double, ctypes.c_double, vp, vp, vp]
    cf = ctypes.c_float
    lib.gpd_policy_n_params.restype = ci
    lib.gpd_policy_n_params.argtypes = [ci, ci]
    lib.gpd_policy_ppo_grad_workspace.restype = ctypes.c_size_t
    lib.gpd_policy_ppo_grad_workspace.argtypes = [ci, ci, ci, ci]
    lib.gpd_policy_ppo_grad.restype = ci
    lib.gpd_policy_ppo_grad.argtypes = [ctypes.POINTER(MlpPolicyStruct), ci, vp, vp, vp, vp, vp, vp, cf, cf, cf, vp, vp,
                                        vp, ctypes.c_size_t, ci, vp]
    if lib.gpd_policy_abi_version() != GPD_POLICY_ABI_VERSION:
        raise GpdLibraryError(f"{LIB_PATH} has ABI {lib.gpd_policy_abi_version()}, expected {GPD_POLICY_ABI_VERSION}")
    _lib = lib
    return lib


def _check(name, rc):
    if rc != 0:
        raise GpdError(name, rc, _lib.gpd_policy_last_error().decode(errors="replace"))


def _linears(seq):
    lin = [m for m in seq if isinstance(m, torch.nn.Linear)]
    acts = [m for m in seq if not isinstance(m, torch.nn.Linear)]
    if len(lin) != 3 or not all(isinstance(a, torch.nn.Tanh) for a in acts) or len(acts) != 2 \
            or lin[0].out_features != HIDDEN or lin[1].in_features != HIDDEN or lin[1].out_features != HIDDEN \
            or lin[2].in_features != HIDDEN:
        raise ValueError("the fused policy runs SB3 MlpPolicy networks: Linear(n, 64) Tanh Linear(64, 64) Tanh "
                         "Linear(64, m)")
    return lin


def _module_struct(module):
    """``module`` (``.pi``, ``.vf``, ``.log_std``) -> (gpd_mlp_policy struct over its parameters' device
    addresses, the 13 parameters in the struct's field order, n_obs, n_act, device)."""
    pi, vf = _linears(module.pi), _linears(module.vf)
    if vf[2].out_features != 1:
        raise ValueError("the critic has one output")
    n_obs, n_act = pi[0].in_features, pi[2].out_features
    if vf[0].in_features != n_obs:
        raise ValueError("actor and critic read the same observation")
    if not 1 <= n_obs <= MAX_OBS or not 1 <= n_act <= MAX_ACT:
        raise ValueError(f"n_obs must be in [1, {MAX_OBS}] and n_act in [1, {MAX_ACT}]")
    params = [p for lin in pi + vf for p in (lin.weight, lin.bias)] + [module.log_std]
    dev = params[0].device
    for p in params:
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev or dev.type != "cuda":
            raise ValueError("the fused policy reads contiguous float32 parameters on the GPU")
    st = MlpPolicyStruct()
    st.n_obs, st.n_act = n_obs, n_act
    for n, p in zip(PARAM_NAMES, params):
        setattr(st, n, p.data_ptr())
    return st, params, n_obs, n_act, dev


def _ptr(t, name, dtype, device=None, numel=None):
    """The address of ``t``, a contiguous ``dtype`` tensor on the GPU (on ``device``, if given), optionally of
    ``numel`` = (rows, width) elements."""
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()) or (device is not None and t.device != device):
        raise ValueError(f"{name} must be a contiguous {dtype} tensor on {device}" if device is not None else
                         f"{name} must be a contiguous float32 device tensor")
    if numel is not None and t.numel() != numel[0] * numel[1]:
        raise ValueError(f"{name} must hold {numel[0]} x {numel[1]} elements, has {t.numel()}")
    return ctypes.c_void_p(t.data_ptr())


def _as_int64(x):
    """``x`` mod 2^64 as the int64 with the same bits (the device words are uint64, torch's int64)."""
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return x - (1 << 64) if x >= 1 << 63 else x


class MlpPolicyKernel:
    """The actor-critic ``module`` (``.pi``, ``.vf`` as Linear-Tanh-Linear-Tanh-Linear, ``.log_std``;
    examples/learn.py's ``ActorCritic``) as one rollout kernel per step.  The parameters are read
    in place: an optimizer step that updates them in place is seen by the next call (and by a
    captured graph).  ``seed``: the 64-bit Philox key, taken mod 2^64 (``rng[0]`` holds it as int64
    two's complement: the kernel reads both 32-bit halves); the call counters (one per group of 16
    rows) live on the device (``rng``), sized for ``max_rows`` rows (grown by a call with more rows,
    which a captured graph must not do)."""

    def __init__(self, module, seed=0, max_rows=1 << 16):
        self._lib = load()
        # the parameters are kept alive: the struct holds their addresses
        self._st, self._params, self.n_obs, self.n_act, self.device = _module_struct(module)
        dev = self.device
        # {key, 0, call counter of row group 0, 1, ...} (include/gpd_policy.h)
        self.rng = torch.zeros(2 + -(-int(max_rows) // GROUP_ROWS), dtype=torch.int64, device=dev)
        self.rng[0] = _as_int64(seed)

    @property
    def rng_groups(self):
        return self.rng.numel() - 2

    def _fit(self, n_rows):
        need = -(-n_rows // GROUP_ROWS)
        if need > self.rng_groups:
            if torch.cuda.is_current_stream_capturing():
                raise ValueError(f"{n_rows} rows need {need} row-group counters, the rng holds {self.rng_groups}: "
                                 "pass max_rows >= the largest batch before capturing a graph")
            grown = torch.zeros(2 + need, dtype=torch.int64, device=self.device)
            grown[:self.rng.numel()] = self.rng
            grown[self.rng.numel():] = self.rng[2]      # new groups join at the batch's call count
            self.rng = grown

    @property
    def calls(self):
        """Sampling calls made so far (row group 0's device counter; reading it synchronises)."""
        return int(self.rng[2])

    def set_calls(self, n):
        """Rewind / advance the Philox call counters of every row group (the same key and counter draw
        the same numbers)."""
        self.rng[2:] = int(n)

    def _rows(self, t, width, name):
        return None if t is None else _ptr(t, name, torch.float32, numel=(self._n, width))

    def step(self, obs=None, act_env=None, buf_obs=None, buf_act=None, buf_logp=None, buf_val=None,
             deterministic=False, prev=None, gamma=0.99, buf_rew=None, buf_done=None, n_rows=None):
        """One rollout step (gpd_policy_rollout_step); ``prev`` = (reward, terminated, truncated,
        terminal_obs) of the previous env.step, written to ``buf_rew`` / ``buf_done``."""
        src = obs if obs is not None else (prev[3] if prev is not None else None)
        if src is None:
            raise ValueError("nothing to do: neither obs nor prev")
        self._n = int(n_rows) if n_rows is not None else src.numel() // self.n_obs
        self._fit(self._n)
        args = [self._rows(obs, self.n_obs, "obs"), self._rows(act_env, self.n_act, "act_env"),
                self._rows(buf_obs, self.n_obs, "buf_obs"), self._rows(buf_act, self.n_act, "buf_act"),
                self._rows(buf_logp, 1, "buf_logp"), self._rows(buf_val, 1, "buf_val")]
        if prev is not None:
            rew, te, tr, tobs = prev
            for t, nm in ((te, "terminated"), (tr, "truncated")):
                if not (t.is_cuda and t.dtype == torch.uint8 and t.numel() == self._n):
                    raise ValueError(f"{nm} must be a uint8 device tensor of {self._n} flags")
            pv = [self._rows(rew, 1, "reward"), ctypes.c_void_p(te.data_ptr()), ctypes.c_void_p(tr.data_ptr()),
                  self._rows(tobs, self.n_obs, "terminal_obs")]
            outs = [self._rows(buf_rew, 1, "buf_rew"), self._rows(buf_done, 1, "buf_done")]
        else:
            pv, outs = [None] * 4, [None, None]
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check("gpd_policy_rollout_step", self._lib.gpd_policy_rollout_step(
            ctypes.byref(self._st), self._n, *args, 1 if deterministic else 0, ctypes.c_void_p(self.rng.data_ptr()),
            self.rng_groups, *pv, float(gamma), *outs, ctypes.c_void_p(stream)))

    def gae(self, rew, val, done, last_val, gamma, lam, adv, ret):
        """GAE over a rollout, bit-identical to examples/learn.py's torch loop: [T, E] tensors."""
        T, E = rew.shape
        for t in (rew, val, done, adv, ret):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (T, E)):
                raise ValueError("GAE buffers must be contiguous float32 [T, E] device tensors")
        if last_val.numel() != E:
            raise ValueError("last_val must hold E values")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check("gpd_policy_gae", self._lib.gpd_policy_gae(
            T, E, *(ctypes.c_void_p(t.data_ptr()) for t in (rew, val, done, last_val)), float(gamma), float(lam),
            ctypes.c_void_p(adv.data_ptr()), ctypes.c_void_p(ret.data_ptr()), ctypes.c_void_p(stream)))


class PpoGradKernel:
    """The PPO minibatch gradient of the actor-critic ``module`` in HIP (``gpd_policy_ppo_grad``): the
    gather of the minibatch's rows, both forward passes, the clipped surrogate + value loss of
    examples/learn.py, the backward pass and the gradient-norm clip, with no autograd graph and no
    optimizer: ``grad_step`` leaves the clipped gradient in ``grad`` (flat, ``PARAM_NAMES`` order),
    whose per-parameter views are installed as each parameter's ``.grad``, so ``opt.step()`` follows.
    Owns ``grad``, ``stats`` (policy loss, value loss, gradient norm before clipping, clip fraction)
    and the workspace, sized for minibatches of up to ``max_rows`` rows.  ``max_blocks``: 0 = the
    library's grid, otherwise its cap (the same inputs and max_blocks give the same bits)."""

    def __init__(self, module, max_rows, max_blocks=0):
        self._lib = load()
        self._st, self._params, self.n_obs, self.n_act, self.device = _module_struct(module)
        self.max_rows, self.max_blocks = int(max_rows), int(max_blocks)
        if self.max_rows < 1 or self.max_blocks < 0:
            raise ValueError("max_rows must be >= 1 and max_blocks >= 0")
        self.n_params = self._lib.gpd_policy_n_params(self.n_obs, self.n_act)
        if self.n_params != sum(p.numel() for p in self._params):
            raise GpdLibraryError(f"{LIB_PATH} counts {self.n_params} parameters, the module has "
                                  f"{sum(p.numel() for p in self._params)}")
        # the workspace grows with the rows (more 16-row groups, up to the grid's cap)
        self._ws_bytes = self._lib.gpd_policy_ppo_grad_workspace(self.n_obs, self.n_act, self.max_rows,
                                                                 self.max_blocks)
        if self._ws_bytes == 0:
            raise GpdError("gpd_policy_ppo_grad_workspace", -1,
                           self._lib.gpd_policy_last_error().decode(errors="replace"))
        self.workspace = torch.empty(self._ws_bytes // 4, dtype=torch.float32, device=self.device)
        self.grad = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        self.stats = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.views, off = [], 0
        for p in self._params:
            self.views.append(self.grad[off:off + p.numel()].view_as(p))
            off += p.numel()
        self.install()

    def install(self):
        """Make the views of ``grad`` the parameters' ``.grad`` (again, e.g. after
        ``zero_grad(set_to_none=True)``)."""
        for p, v in zip(self._params, self.views):
            p.grad = v

    def _buf(self, t, name, dtype=torch.float32):
        return _ptr(t, name, dtype, self.device)

    def grad_step(self, idx, obs, act, logp, adv, ret, clip, vf_coef, max_grad_norm, n_rows=None):
        """One minibatch: rows ``idx`` (int64 device tensor, or None for rows 0 .. n_rows - 1) of the
        flattened rollout buffers ``obs [N, n_obs]``, ``act [N, n_act]``, ``logp``, ``adv``, ``ret [N]``.
        Asynchronous on the current stream and capturable.  The indices are not checked on the host
        (that would read them back): the caller keeps them inside the buffers."""
        N = logp.numel()
        if obs.numel() != N * self.n_obs or act.numel() != N * self.n_act or adv.numel() != N or ret.numel() != N:
            raise ValueError(f"the buffers must hold the same {N} rows: obs {tuple(obs.shape)}, act {tuple(act.shape)}, "
                             f"adv {tuple(adv.shape)}, ret {tuple(ret.shape)}")
        n = int(idx.numel()) if idx is not None else int(N if n_rows is None else n_rows)
        if not 1 <= n <= self.max_rows or (idx is None and n > N):
            raise ValueError(f"a minibatch of {n} rows: this kernel was built for 1 .. {self.max_rows} rows "
                             f"of buffers that hold them")
        ip = self._buf(idx, "idx", torch.int64) if idx is not None else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check("gpd_policy_ppo_grad", self._lib.gpd_policy_ppo_grad(
            ctypes.byref(self._st), n, ip, self._buf(obs, "obs"), self._buf(act, "act"), self._buf(logp, "logp"),
            self._buf(adv, "adv"), self._buf(ret, "ret"), float(clip), float(vf_coef), float(max_grad_norm),
            ctypes.c_void_p(self.grad.data_ptr()), ctypes.c_void_p(self.stats.data_ptr()),
            ctypes.c_void_p(self.workspace.data_ptr()), self._ws_bytes, self.max_blocks, ctypes.c_void_p(stream)))
