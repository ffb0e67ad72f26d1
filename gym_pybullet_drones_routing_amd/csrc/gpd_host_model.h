// gpd_host_model.h — the HIP-free host model of the C ABI (include/gpd.h): the last-error string,
// the built-in drone and controller parameters, the derived constants of an env row, the reset
// template of a pose (the Bullet orientation round trip in double) and the checks of the per-env
// tables.  Standard library and gpd.h only, so that a plain C++ compiler can build and check it
// without a GPU (tests/host_model_driver.cpp); gpd.hip includes it and stays the only translation
// unit of libgpd.so.  Everything has internal linkage: the library exports none of it.
#ifndef GPD_HOST_MODEL_H
#define GPD_HOST_MODEL_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>

#include "../../include/gpd.h"

namespace {

thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// ---- host restatements of the Bullet helpers (double), for the reset template only
inline void h_quat_to_mat(const double q[4], double m[9]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double d = x * x + y * y + z * z + w * w, s = 2.0 / d;
  const double xs = x * s, ys = y * s, zs = z * s;
  const double wx = w * xs, wy = w * ys, wz = w * zs, xx = x * xs, xy = x * ys, xz = x * zs;
  const double yy = y * ys, yz = y * zs, zz = z * zs;
  m[0] = 1.0 - (yy + zz); m[1] = xy - wz; m[2] = xz + wy;
  m[3] = xy + wz; m[4] = 1.0 - (xx + zz); m[5] = yz - wx;
  m[6] = xz - wy; m[7] = yz + wx; m[8] = 1.0 - (xx + yy);
}
inline void h_mat_to_quat(const double m[9], double q[4]) {
  const double tr = m[0] + m[4] + m[8];
  double t[4];
  if (tr > 0.0) {
    double s = std::sqrt(tr + 1.0);
    t[3] = s * 0.5; s = 0.5 / s;
    t[0] = (m[7] - m[5]) * s; t[1] = (m[2] - m[6]) * s; t[2] = (m[3] - m[1]) * s;
  } else {
    const int i = m[0] < m[4] ? (m[4] < m[8] ? 2 : 1) : (m[0] < m[8] ? 2 : 0);
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    double s = std::sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
    t[i] = s * 0.5; s = 0.5 / s;
    t[3] = (m[k * 3 + j] - m[j * 3 + k]) * s;
    t[j] = (m[j * 3 + i] + m[i * 3 + j]) * s;
    t[k] = (m[k * 3 + i] + m[i * 3 + k]) * s;
  }
  for (int a = 0; a < 4; ++a) q[a] = t[a];
}
inline void h_roundtrip(const double q[4], double out[4]) {
  double m[9];
  h_quat_to_mat(q, m);
  h_mat_to_quat(m, out);
}
inline void h_euler(const double q[4], double rpy[3]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double sarg = -2.0 * (x * z - w * y);
  if (sarg <= -0.99999) {
    rpy[0] = 0.0; rpy[1] = -0.5 * M_PI; rpy[2] = 2.0 * std::atan2(x, -y);
  } else if (sarg >= 0.99999) {
    rpy[0] = 0.0; rpy[1] = 0.5 * M_PI; rpy[2] = 2.0 * std::atan2(-x, y);
  } else {
    rpy[1] = std::asin(std::fmin(1.0, std::fmax(-1.0, sarg)));
    rpy[0] = std::atan2(2.0 * (y * z + w * x), w * w - x * x - y * y + z * z);
    rpy[2] = std::atan2(2.0 * (x * y + w * z), w * w + x * x - y * y - z * z);
  }
}
inline void h_quat_from_euler(const double rpy[3], double q[4]) {  // btQuaternion::setEulerZYX
  const double hy = rpy[2] * 0.5, hp = rpy[1] * 0.5, hr = rpy[0] * 0.5;
  const double cy = std::cos(hy), sy = std::sin(hy), cp = std::cos(hp), sp = std::sin(hp);
  const double cr = std::cos(hr), sr = std::sin(hr);
  q[0] = sr * cp * cy - cr * sp * sy;
  q[1] = cr * sp * cy + sr * cp * sy;
  q[2] = cr * cp * sy - sr * sp * cy;
  q[3] = cr * cp * cy + sr * sp * sy;
}

// the reset template of one drone: INIT_XYZS and the orientation the client stores
// (BaseAviary.py:194-207, :486-491, :509-519)
inline void pose_template(const double xyz[3], const double rpy[3], double t[10]) {
  double q0[4], qraw[4], qn[4], e[3];
  h_quat_from_euler(rpy, q0);
  h_roundtrip(q0, qraw);  // loadURDF stores the orientation through a btTransform
  h_roundtrip(qraw, qn);  // readback (:517)
  h_euler(qn, e);         // :518
  t[0] = xyz[0]; t[1] = xyz[1]; t[2] = xyz[2];
  t[3] = qraw[0]; t[4] = qraw[1]; t[5] = qraw[2]; t[6] = qraw[3];
  t[7] = e[0]; t[8] = e[1]; t[9] = e[2];
}

// [n][D][10] templates and [n][D][3] targets from n x D poses (a sim's one set, a het sim's envs,
// or a reset pool)
inline void pose_tables(int task, size_t n_sets, int D, const double* xyzs, const double* rpys, double* tmpl,
                        double* target) {
  for (size_t e = 0; e < n_sets; ++e)
    for (int d = 0; d < D; ++d) {
      const size_t n = e * D + d;
      const double* xyz = &xyzs[n * 3];
      pose_template(xyz, &rpys[n * 3], &tmpl[n * 10]);
      double* tg = &target[n * 3];
      tg[0] = tg[1] = tg[2] = 0.0;
      if (task == GPD_TASK_HOVER) {           // HoverAviary.py:51
        tg[2] = 1.0;
      } else if (task == GPD_TASK_MULTIHOVER) {  // MultiHoverAviary.py:71
        tg[0] = xyz[0]; tg[1] = xyz[1]; tg[2] = xyz[2] + 1.0 / (d + 1);
      }
    }
}

inline gpd_env_params env_row_of(const gpd_drone_params& P) {
  return gpd_env_params{P.m, P.arm, P.thrust2weight, P.ixx, P.iyy, P.izz, P.kf, P.km,
                        P.gnd_eff_coeff, P.drag_coeff_xy, P.drag_coeff_z};
}

// self.MAX_RPM**2 as Python evaluates it: libm's pow(x, 2.0), which is not correctly rounded in
// every libm and then differs from x*x in the last bit (seen on one row in a thousand); the
// exponent is opaque so that the compiler cannot turn the call into a multiply
inline double py_square(double x) {
  volatile double two = 2.0;
  return std::pow(x, two);
}

// BaseAviary.py:117-128 for one env row, operation for operation (no FP contraction).
// (gpd.hip's derive_constants derives a sim's own gpd_constants from the same lines but squares
// MAX_RPM with x*x, where this squares with py_square; the two can differ in the last bit for
// user-supplied parameters, and gpd_get_constants / Consts::ge_clip on the one side, the env
// table on the other are pinned to their own: do not merge them)
inline void derive_row(const gpd_drone_params& base, const gpd_env_params& r, gpd_constants& K) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  std::memset(&K, 0, sizeof(K));
  K.gravity = 9.8 * r.m;
  K.hover_rpm = std::sqrt(K.gravity / (4 * r.kf));
  K.max_rpm = std::sqrt((r.thrust2weight * K.gravity) / (4 * r.kf));
  const double mr2 = py_square(K.max_rpm);
  K.max_thrust = 4 * r.kf * mr2;
  K.max_xy_torque = base.model == GPD_MODEL_CF2P ? r.arm * r.kf * mr2 : (2 * r.arm * r.kf * mr2) / std::sqrt(2.0);
  K.max_z_torque = 2 * r.km * mr2;
  K.gnd_eff_h_clip = 0.25 * base.prop_radius * std::sqrt((15 * mr2 * r.kf * r.gnd_eff_coeff) / K.max_thrust);
}

// gpd_constants::trunc_step_counter: truncated iff step_counter / PYB_FREQ > EPISODE_LEN_SEC
// (HoverAviary.py:114), so the smallest step counter for which that holds
inline int trunc_step_counter(double episode_len_sec, int pyb_freq) {
  long long sc = (long long)std::floor(episode_len_sec * pyb_freq);
  if (sc < 0) sc = 0;
  while (sc > 0 && (double)(sc - 1) / pyb_freq > episode_len_sec) --sc;
  while (!((double)sc / pyb_freq > episode_len_sec)) ++sc;
  return (int)std::min<long long>(sc, 0x7fffffff);
}

inline int check_env_rows(const char* fn, const gpd_env_params* rows, int n, const char* unit = "env") {
  static const char* const names[11] = {"m", "arm", "thrust2weight", "ixx", "iyy", "izz", "kf", "km",
                                        "gnd_eff_coeff", "drag_coeff_xy", "drag_coeff_z"};
  for (int e = 0; e < n; ++e) {
    const double* f = &rows[e].m;
    for (int k = 0; k < 11; ++k) {
      const bool aero = k >= 8;   // the three aero coefficients may be 0
      if (!std::isfinite(f[k]) || f[k] < 0.0 || (!aero && f[k] == 0.0))
        return fail(GPD_EINVAL, std::string(fn) + ": env_params field " + names[k] + " of " + unit + " " + std::to_string(e) +
                                    " must be finite and " + (aero ? ">= 0" : "> 0"));
    }
  }
  return GPD_OK;
}
static_assert(sizeof(gpd_env_params) == 11 * sizeof(double), "gpd_env_params is 11 packed doubles");

inline int check_poses(const char* fn, const char* what, const double* p, long long n_drones, int D,
                       const char* unit = "env") {
  if (!p) return GPD_OK;
  for (long long i = 0; i < n_drones * 3; ++i)
    if (!std::isfinite(p[i]))
      return fail(GPD_EINVAL, std::string(fn) + ": " + what + " of " + unit + " " + std::to_string(i / (3LL * D)) +
                                  " drone " + std::to_string((i / 3) % D) + " is not finite");
  return GPD_OK;
}

// gpd_default_params
inline int default_params(int model, gpd_drone_params* out) {
  if (!out) return fail(GPD_EINVAL, "gpd_default_params: out is NULL");
  gpd_drone_params p;
  std::memset(&p, 0, sizeof(p));
  p.model = model;
  // <properties> common to the three URDFs (cf2x.urdf:5)
  p.gnd_eff_coeff = 11.36859; p.drag_coeff_xy = 9.1785e-7; p.drag_coeff_z = 10.311e-7;
  p.dw_coeff_1 = 2267.18; p.dw_coeff_2 = .16; p.dw_coeff_3 = -.11;
  p.collision_h = .025; p.collision_r = .06; p.collision_z_offset = 0.0;  // collision cylinder
  double pp[4][3];
  if (model == GPD_MODEL_CF2X || model == GPD_MODEL_CF2P) {             // cf2x.urdf / cf2p.urdf
    p.arm = 0.0397; p.kf = 3.16e-10; p.km = 7.94e-12; p.thrust2weight = 2.25; p.max_speed_kmh = 30;
    p.prop_radius = 2.31348e-2; p.m = 0.027;
    if (model == GPD_MODEL_CF2X) {
      p.ixx = 1.4e-5; p.iyy = 1.4e-5; p.izz = 2.17e-5;
      const double c[4][3] = {{0.028, -0.028, 0}, {-0.028, -0.028, 0}, {-0.028, 0.028, 0}, {0.028, 0.028, 0}};
      std::memcpy(pp, c, sizeof(pp));
    } else {
      p.ixx = 2.3951e-5; p.iyy = 2.3951e-5; p.izz = 3.2347e-5;
      const double c[4][3] = {{0.0397, 0, 0}, {0, 0.0397, 0}, {-0.0397, 0, 0}, {0, -0.0397, 0}};
      std::memcpy(pp, c, sizeof(pp));
    }
  } else if (model == GPD_MODEL_RACE) {                                   // racer.urdf
    p.arm = 0.109; p.kf = 8.47e-9; p.km = 2.13e-11; p.thrust2weight = 4.17; p.max_speed_kmh = 200;
    p.prop_radius = 12.7e-2; p.m = 0.830; p.ixx = .003113; p.iyy = .003113; p.izz = .003113;
    const double c[4][3] = {{0.0850, 0.0675, 0}, {-0.0850, 0.0675, 0}, {-0.085, -0.0675, 0}, {0.085, -0.0675, 0}};
    std::memcpy(pp, c, sizeof(pp));
  } else {
    return fail(GPD_EINVAL, "gpd_default_params: unknown drone model");
  }
  std::memcpy(p.prop_pos, pp, sizeof(pp));
  *out = p;
  return GPD_OK;
}

// gpd_default_pid_params (line numbers: DSLPIDControl.py)
inline int default_pid_params(gpd_pid_params* out) {
  if (!out) return fail(GPD_EINVAL, "gpd_default_pid_params: out is NULL");
  gpd_pid_params q;
  std::memset(&q, 0, sizeof(q));
  const double pf[3] = {.4, .4, 1.25}, iff[3] = {.05, .05, .05}, df[3] = {.2, .2, .5};       // :37-39
  const double pt[3] = {70000., 70000., 60000.}, it[3] = {.0, .0, 500.}, dtq[3] = {20000., 20000., 12000.};  // :40-42
  const double mix[4][3] = {{-.5, -.5, -1}, {-.5, .5, 1}, {.5, .5, -1}, {.5, -.5, 1}};     // :48-53 (CF2X)
  for (int i = 0; i < 3; ++i) {
    q.p_coeff_for[i] = pf[i]; q.i_coeff_for[i] = iff[i]; q.d_coeff_for[i] = df[i];
    q.p_coeff_tor[i] = pt[i]; q.i_coeff_tor[i] = it[i]; q.d_coeff_tor[i] = dtq[i];
  }
  q.pwm2rpm_scale = 0.2685; q.pwm2rpm_const = 4070.3; q.min_pwm = 20000; q.max_pwm = 65535;  // :43-46
  std::memcpy(q.mixer, mix, sizeof(mix));
  q.gravity = 9.8 * 0.027;  // g * m of cf2x.urdf:11 (BaseControl.py:35)
  q.kf = 3.16e-10;          // cf2x.urdf:5 (BaseControl.py:37)
  *out = q;
  return GPD_OK;
}

}  // namespace

#endif  // GPD_HOST_MODEL_H
