"""Oracle envs with their own drone parameters: the reference for heterogeneous sims.

Test infrastructure only.  The reference's vector of env objects lets each env parse its own URDF
(``BaseAviary.py:97-128, 982-1014``) and take its own ``initial_xyzs`` / ``initial_rpys``;
``het_env`` does the same to one ``oracle.ref_aviary.RefAviary``: it overrides the attributes the
DYN paths read (``ref_aviary.py:186-204, 287-353``) from one ``gpd_env_params`` row, with the
derived values recomputed by the formulas of ``oracle/params.derived``.
"""
import math

import numpy as np

from oracle.params import G, derived
from oracle.ref_aviary import RefAviary

NAMES = ("m", "arm", "thrust2weight", "ixx", "iyy", "izz", "kf", "km",
         "gnd_eff_coeff", "drag_coeff_xy", "drag_coeff_z")
DERIVED = ("gravity", "hover_rpm", "max_rpm", "max_thrust", "max_xy_torque", "max_z_torque", "gnd_eff_h_clip")


def nominal_row(model="cf2x"):
    p = derived(model)
    return {k: p[k] for k in NAMES}


def derive(row, model="cf2x"):
    """``oracle.params.derived`` with the per-env fields of ``row`` (a dict over NAMES) in place
    of the model's: raw + derived constants exactly as BaseAviary.__init__ computes them (:117-128)."""
    p = derived(model)
    p.update({k: float(row[k]) for k in NAMES})
    p["gravity"] = G * p["m"]                                                     # :117
    p["hover_rpm"] = math.sqrt(p["gravity"] / (4 * p["kf"]))                      # :118
    p["max_rpm"] = math.sqrt((p["thrust2weight"] * p["gravity"]) / (4 * p["kf"]))  # :119
    p["max_thrust"] = 4 * p["kf"] * p["max_rpm"] ** 2                              # :120
    if model == "cf2p":
        p["max_xy_torque"] = p["arm"] * p["kf"] * p["max_rpm"] ** 2                # :124
    else:
        p["max_xy_torque"] = (2 * p["arm"] * p["kf"] * p["max_rpm"] ** 2) / math.sqrt(2)  # :122,126
    p["max_z_torque"] = 2 * p["km"] * p["max_rpm"] ** 2                            # :127
    p["gnd_eff_h_clip"] = 0.25 * p["prop_radius"] * math.sqrt(
        (15 * p["max_rpm"] ** 2 * p["kf"] * p["gnd_eff_coeff"]) / p["max_thrust"])  # :128
    return p


def apply_row(env, row):
    """Give ``env`` the drone of ``row`` (what re-parsing another URDF would)."""
    p = derive(row, env.MODEL)
    env.P = p
    env.M, env.L, env.KF, env.KM = p["m"], p["arm"], p["kf"], p["km"]
    env.GRAVITY = p["gravity"]
    env.J = np.diag([p["ixx"], p["iyy"], p["izz"]])
    env.J_INV = np.linalg.inv(env.J)
    env.HOVER_RPM = np.float64(p["hover_rpm"])
    env.GND_EFF_COEFF = p["gnd_eff_coeff"]
    env.GND_EFF_H_CLIP = p["gnd_eff_h_clip"]
    env.DRAG_COEFF = np.array([p["drag_coeff_xy"], p["drag_coeff_xy"], p["drag_coeff_z"]])
    return env


def apply_poses(env, xyzs=None, rpys=None):
    """New INIT_XYZS / INIT_RPYS (effective at the next reset); MultiHover targets follow
    (MultiHoverAviary.py:71)."""
    n = env.NUM_DRONES
    if xyzs is not None:
        env.INIT_XYZS = np.array(xyzs, dtype=np.float64).reshape(n, 3)
        if env.TASK == "multihover":
            env.TARGET_POS = env.INIT_XYZS + np.array([[0, 0, 1 / (i + 1)] for i in range(n)])
    if rpys is not None:
        env.INIT_RPYS = np.array(rpys, dtype=np.float64).reshape(n, 3)
    return env


def het_env(row, **kw):
    """A RefAviary whose drone is ``row`` (dict over NAMES); ``kw`` as RefAviary's (``initial_xyzs``,
    ``initial_rpys``, ``task``, ``aero``, ...)."""
    return apply_row(RefAviary(**kw), row)


def rows_of(params, e):
    """Row e of a {name: array[E]} dict (``assets.randomized_params``'s form)."""
    nom = None
    out = {}
    for k in NAMES:
        if k in params:
            out[k] = float(params[k][e])
        else:
            nom = nom or nominal_row()
            out[k] = nom[k]
    return out


def random_rows(rng, n, frac=0.3, model="cf2x"):
    """{name: array[n]}: every parameter uniform in [1-frac, 1+frac] x nominal, drawn in NAMES order."""
    nom = nominal_row(model)
    return {k: nom[k] * rng.uniform(1.0 - frac, 1.0 + frac, n) for k in NAMES}
