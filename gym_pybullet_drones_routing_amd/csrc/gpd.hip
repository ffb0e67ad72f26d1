// gpd.hip — C ABI (include/gpd.h) of the batched quadrotor DYN path on MI355X (gfx950).
//
// Host side: validates the configuration (BaseAviary.__init__ checks, BaseAviary.py:79-80),
// derives the model constants in double exactly as BaseAviary.py:117-128 does, builds the
// reset template (INIT_XYZS / INIT_RPYS through the Bullet orientation round trip,
// BaseAviary.py:194-207, :486-491, :509-519), owns the SoA device state and launches the
// kernels of gpd_kernels.h on the caller's stream.  The parts of that which need no HIP (the
// orientation round trip, the derived constants of an env row, the table checks, the built-in
// parameters, the last-error string) are gpd_host_model.h; here are the sim, the kernel choice,
// the launches and the entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/gpd.h"
#include "gpd_host_model.h"
#include "gpd_kernels.h"
#include "gpd_handoff.h"

using namespace gpd;

static_assert(GPD_ACT_RPM == ACT_RPM && GPD_ACT_ONE_D_RPM == ACT_ONE_D_RPM && GPD_ACT_PID == ACT_PID &&
                  GPD_ACT_VEL == ACT_VEL && GPD_ACT_ONE_D_PID == ACT_ONE_D_PID,
              "action type codes of gpd.h and the kernels must agree");
static_assert(GPD_CMD_RPM == CMD_RPM && GPD_CMD_VEL == CMD_VEL && GPD_CMD_WAYPOINT == CMD_WAYPOINT,
              "command mode codes of gpd.h and the kernels must agree");
constexpr int kCtrlComps = 9;
constexpr size_t kLdsBytes = 160 * 1024;   // LDS per workgroup on gfx950

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) return fail(GPD_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct gpd_sim {
  gpd_drone_params P;
  gpd_pid_params pid;
  gpd_config cfg;
  gpd_constants K;
  int E, D, N, A, W, nsub, ring_len, prec, tpb;
  long long npad;
  void* d_state = nullptr;
  void* d_ctrl = nullptr;         // tiled [npad/64][9][64] DSLPIDControl state (PID action types)
  float* d_ring = nullptr;
  int2* d_ctr = nullptr;          // [E] {step_counter, ring head} + [E].x: last action in the ring
  void* d_init = nullptr;
  void* d_target = nullptr;
  void* d_consts = nullptr;       // Consts<real> in device memory
  int tile_bytes = 0;             // dynamic LDS of the step kernel
  int seq_lds = 0;                // dynamic LDS of step_seq_kernel (tile + the rate chains' hand-off buffers);
                                  // 0: the sim is not seq_fused (prepare_step_kernel)
  int wt = 0;                     // SimView::wt (write-through store policy)
  int nc_magic = 0;               // SimView::nc_magic
  bool duo = false;               // step launches step_kernel_duo (two or three waves per block)
  bool wide = false;              // step_kernel_wide / integrate_kernel_wide, one env per workgroup: D > 64,
                                  // or an observation row too long for the one-wave kernels' LDS tile
  int step_waves = 1;             // waves per step block (1, 2, or 3 with the io wave)
  bool stream = false;            // streaming cache policies (step_kernel STREAM): batches past the MALL
  bool generic_pf = false;        // the run-time-flag step kernel even where a flag set is compiled in
                                  // (its static LDS + the observation tile would not fit: upload_tables)
  DwPairs dw_pairs{0, 0};         // SimView::dw_pairs
  // drone <-> drone contact (PYB*, 1 < D <= 64; SimView::dc*): pairs per env, p / P magic, the
  // [P] pair table, the row store of pairs past a block's first 64 (blocks x stride reals)
  int dcP = 0, dc_pmagic = 0;
  int* d_dc_tab = nullptr;
  void* d_dc_rows = nullptr;
  long long dc_row_stride = 0;
  double bound_xy;
  std::vector<double> init_tmpl;  // [D][10]; het: [E][D][10]
  std::vector<double> target;     // [D][3]; het: [E][D][3]
  // heterogeneous sim (gpd_create_het; kernels in gpd_step_het.h)
  bool het = false;
  void* d_etab = nullptr;         // [kHetCols][epad] per-env constants in the sim's real type
  long long epad = 0;             // E rounded up to 64
  std::vector<gpd_env_params> env_rows;   // [E]
  std::vector<double> het_xyz, het_rpy;   // [E][D][3]
  // reset pools (gpd_set_reset_pool; the pooled tail of step_kernel_het)
  bool pool_on = false;           // step launches the pooled instantiation
  int* d_draws = nullptr;         // [E][3] {episode number, row index, pose index}
  void* d_pool = nullptr;         // ResetPool<real>: allocated at create, rewritten by every set
  void* d_pool_rows = nullptr;    // [P][kHetCols]
  void* d_pool_init = nullptr;    // [Q][D][10]
  void* d_pool_target = nullptr;  // [Q][D][3]
  std::vector<gpd_env_params> pool_rows;    // [P] host copies: fold_draws makes a drawn row / pose
  std::vector<double> pool_xyz, pool_rpy;   // [Q][D][3] the env's own before the pool is replaced
  // per-drone controller gains (gpd_set_pid_gains; the PG instantiations of the command step kernels)
  void* d_gains = nullptr;        // tiled [npad/64][18][64], allocated at the first install, freed at destroy
  bool gains_on = false;          // a table is in force: the controller modes launch the _pg kernels
  std::vector<double> gains;      // [N][18] the table's values as stored (rounded to the sim's real type)
};

namespace {

// ---- the run-time choices that become template arguments, each made in one place.  f is a
// generic lambda; it is instantiated for every value listed here, so a caller whose kernels
// exist for fewer (the RPM action types only, say) asks the narrower helper.
// the sim's real type: f(R{})
template <typename F>
auto by_real(const gpd_sim* s, F&& f) {
  return s->prec == GPD_F64 ? f(double{}) : f(float{});
}
template <int V>
using int_c = std::integral_constant<int, V>;
// act code -> ACT_*: f(int_c<ACT>{})
template <typename F>
auto with_act(int act, F&& f) {
  switch (act) {
    case GPD_ACT_RPM: return f(int_c<ACT_RPM>{});
    case GPD_ACT_ONE_D_RPM: return f(int_c<ACT_ONE_D_RPM>{});
    case GPD_ACT_PID: return f(int_c<ACT_PID>{});
    case GPD_ACT_VEL: return f(int_c<ACT_VEL>{});
    default: return f(int_c<ACT_ONE_D_PID>{});
  }
}
// the same for the kernels that serve the RPM action types only (het, duo)
template <typename F>
auto with_rpm_act(int act, F&& f) {
  return act == GPD_ACT_RPM ? f(int_c<ACT_RPM>{}) : f(int_c<ACT_ONE_D_RPM>{});
}
// D -> MAXT, the block size bound of the multi-wave (wide) kernels: f(int_c<MAXT>{})
template <typename F>
auto with_maxt(int D, F&& f) {
  if (D <= 256) return f(int_c<256>{});
  if (D <= 512) return f(int_c<512>{});
  return f(int_c<1024>{});
}

template <typename R>
Consts<R> make_consts(const gpd_sim* s) {
  const gpd_drone_params& P = s->P;
  Consts<R> c;
  c.dt = (R)s->K.pyb_timestep;
  c.hdt = (R)(0.5 * s->K.pyb_timestep);
  c.hdt2 = (R)((0.5 * s->K.pyb_timestep) * (0.5 * s->K.pyb_timestep));
  c.m = (R)P.m;
  c.gravity = (R)s->K.gravity;
  c.kf = (R)P.kf;
  c.km = (R)P.km;
  c.L = (R)P.arm;
  c.Ls2 = (R)(P.arm / std::sqrt(2.0));
  c.jx = (R)P.ixx; c.jy = (R)P.iyy; c.jz = (R)P.izz;
  c.ijx = (R)(1.0 / P.ixx); c.ijy = (R)(1.0 / P.iyy); c.ijz = (R)(1.0 / P.izz);
  c.ge_coeff = (R)P.gnd_eff_coeff;
  c.prop_r = (R)P.prop_radius;
  c.ge_clip = (R)s->K.gnd_eff_h_clip;
  c.drag_xy = (R)P.drag_coeff_xy;
  c.drag_z = (R)P.drag_coeff_z;
  c.two_pi = (R)(2.0 * M_PI);
  c.dw1 = (R)P.dw_coeff_1; c.dw2 = (R)P.dw_coeff_2; c.dw3 = (R)P.dw_coeff_3;
  c.dwk1 = (R)(P.dw_coeff_1 * ((P.prop_radius / 4) * (P.prop_radius / 4)));
  c.inv_m = (R)(1.0 / P.m);
  c.rpm2rad = (R)(2.0 * M_PI / 60.0);
  for (int k = 0; k < 4; ++k) {
    c.rx[k] = (R)P.prop_pos[k][0];
    c.ry[k] = (R)P.prop_pos[k][1];
    c.rz[k] = (R)P.prop_pos[k][2];
  }
  for (int k = 0; k < 10; ++k) c.init0[k] = (R)s->init_tmpl[k];
  for (int k = 0; k < 3; ++k) c.target0[k] = (R)s->target[k];
  c.hover_f32 = (float)s->K.hover_rpm;
  c.model = P.model;
  // the Bullet integrator always places the thrust at the prop links (_physics :698-705)
  c.flags = s->cfg.physics_flags | ((s->cfg.physics_flags & GPD_F_BULLET) ? GPD_F_GEOM_WRENCH : 0);
  c.lin_damp = (R)0.04;      // btMultiBody() m_linearDamping (not removed: BaseAviary.py:492-494)
  c.ang_damp = (R)0.04;      // btMultiBody() m_angularDamping
  c.max_vel = (R)100.0;      // btMultiBody() m_maxCoordinateVelocity
  c.ang_thr2 = (R)((0.125 * M_PI) * (0.125 * M_PI));   // (ANGULAR_MOTION_THRESHOLD / 2)^2
  // ground-plane contact (plane_contact; constants restated in oracle/bullet_mb.py)
  c.cyl_r = (R)P.collision_r;
  c.cyl_hh = (R)(P.collision_h / 2);
  c.cyl_zoff = (R)P.collision_z_offset;
  {
    const double r = P.collision_r + 0.001, h = P.collision_h / 2 + 0.001;   // + URDF shape margin
    c.brk = (R)(0.02 * std::sqrt(r * r + r * r + h * h));                   // 0.02 x motion disc
  }
  c.slop = (R)1e-5;          // m_linearSlop (pybullet)
  c.erp = (R)0.08;           // m_erp2 (pybullet contactERP)
  c.mu = (R)(0.5 * 1.0);     // drone default friction x plane.urdf lateral_friction
  c.plane_half = (R)15.0;    // plane.urdf collision box 30 x 30
  c.resid = (R)1e-7;         // m_leastSquaresResidualThreshold (pybullet)
  {
    // drone <-> drone contact (drone_contact, gpd_dcontact.h; oracle/bullet_mb.py drone_contact)
    const double bs = std::sqrt(P.collision_r * P.collision_r + (P.collision_h / 2) * (P.collision_h / 2));
    const double reach = 2.0 * bs + (double)c.brk;
    c.dd_reach2 = (R)(reach * reach);
    c.dd_mu = (R)(0.5 * 0.5);   // drone x drone default friction
  }
  c.iters = 50;              // m_numIterations (pybullet numSolverIterations)
  // setPhysicsEngineParameter(numSolverIterations=, solverResidualThreshold=) (gpd_config)
  if (s->cfg.solver_iterations > 0) c.iters = s->cfg.solver_iterations;
  if (s->cfg.solver_residual != 0.0) c.resid = (R)s->cfg.solver_residual;
  c.nsub = s->nsub;
  const gpd_pid_params& Q = s->pid;
  PidConsts<R>& k = c.pid;
  for (int i = 0; i < 3; ++i) {
    k.p_for[i] = (R)Q.p_coeff_for[i]; k.i_for[i] = (R)Q.i_coeff_for[i]; k.d_for[i] = (R)Q.d_coeff_for[i];
    k.p_tor[i] = (R)Q.p_coeff_tor[i]; k.i_tor[i] = (R)Q.i_coeff_tor[i]; k.d_tor[i] = (R)Q.d_coeff_tor[i];
  }
  k.pwm2rpm_scale = (R)Q.pwm2rpm_scale; k.pwm2rpm_const = (R)Q.pwm2rpm_const;
  k.min_pwm = (R)Q.min_pwm; k.max_pwm = (R)Q.max_pwm;
  for (int j = 0; j < 4; ++j)
    for (int i = 0; i < 3; ++i) k.mixer[j * 3 + i] = (R)Q.mixer[j][i];
  k.gravity = (R)Q.gravity; k.kf = (R)Q.kf;
  k.ctrl_dt = (R)s->K.ctrl_timestep;
  k.speed_limit = 0.03 * P.max_speed_kmh * (1000.0 / 3600.0);
  return c;
}

template <typename R>
SimView<R> make_view(const gpd_sim* s) {
  SimView<R> v;
  v.state = (R*)s->d_state;
  v.ctrl = (R*)s->d_ctrl;
  v.ring = s->d_ring;
  v.ctr = s->d_ctr;
  v.init = (const R*)s->d_init;
  v.target = (const R*)s->d_target;
  v.npad = s->npad;
  v.N = s->N; v.D = s->D; v.A = s->A; v.W = s->W; v.tpb = s->tpb; v.ring_len = s->ring_len;
  v.task = s->cfg.task;
  v.autoreset = s->cfg.autoreset;
  v.trunc_sc = s->K.trunc_step_counter;
  v.wt = s->wt;
  v.nc_magic = s->nc_magic;
  v.dw_pairs = s->dw_pairs;
  v.bound_xy = (R)s->bound_xy;
  v.dcP = s->dcP;
  v.dc_pmagic = s->dc_pmagic;
  v.dc_tab = s->d_dc_tab;
  v.dc_rows = s->d_dc_rows;
  v.dc_row_stride = s->dc_row_stride;
  return v;
}

// The step_kernel instantiation of a sim: action type x (D > 1) x (plain DYN fast path).  The
// fast specialisation exists for the RPM action types only (the bench path).
// Physics-flag sets compiled into their own kernels (pf_on): the BASELINE configs' combinations
// (config 3: ground effect + drag; config 4: downwash) and Physics.PYB / PYB_GND_DRAG_DW (single-
// and multi-drone envs) for the RPM action types, plain DYN and Physics.PYB for the single-drone
// PID types; every other combination tests Consts::flags at run time.  The PYB flag sets run the
// register-resident contact solve (gpd_device.h plane_contact_regs), the run-time kernels the
// LDS one.
constexpr int kPfAero = F_GND | F_DRAG;
constexpr int kPfPyb = F_BULLET | F_GEOM;
constexpr int kPfPybAll = F_BULLET | F_GEOM | F_GND | F_DRAG | F_DW;
template <typename R, int ACT>
const void* step_fn_act(bool multi, int flags, bool stream) {
  if (multi) {
    switch (flags) {
      case 0: return (const void*)step_kernel<R, ACT, true, 0>;
      case F_DW: return (const void*)step_kernel<R, ACT, true, F_DW>;
      case kPfPyb: return (const void*)step_kernel<R, ACT, true, kPfPyb>;   // MultiHoverAviary's default physics
      case kPfPybAll: return (const void*)step_kernel<R, ACT, true, kPfPybAll>;
      // the same without the drone <-> drone contact (aero "no_drone_contact"): the kernels
      // compiled without it, as fast as before it existed
      case kPfPyb | F_NO_DC: return (const void*)step_kernel<R, ACT, true, kPfPyb | F_NO_DC>;
      case kPfPybAll | F_NO_DC: return (const void*)step_kernel<R, ACT, true, kPfPybAll | F_NO_DC>;
      default: return (const void*)step_kernel<R, ACT, true, kPfRuntime>;
    }
  }
  switch (flags) {
    case 0: return stream ? (const void*)step_kernel<R, ACT, false, 0, true> : (const void*)step_kernel<R, ACT, false, 0>;
    case kPfAero: return (const void*)step_kernel<R, ACT, false, kPfAero>;
    case kPfPyb: return (const void*)step_kernel<R, ACT, false, kPfPyb>;
    case kPfPybAll: return (const void*)step_kernel<R, ACT, false, kPfPybAll>;
    default: return (const void*)step_kernel<R, ACT, false, kPfRuntime>;
  }
}
template <typename R, int ACT>
const void* step_fn_pid(bool multi, int flags) {
  if (multi) return (const void*)step_kernel<R, ACT, true, kPfRuntime>;
  switch (flags) {
    case 0: return (const void*)step_kernel<R, ACT, false, 0>;
    case kPfPyb: return (const void*)step_kernel<R, ACT, false, kPfPyb>;
    default: return (const void*)step_kernel<R, ACT, false, kPfRuntime>;
  }
}
// het sims (gpd_step_het.h): the flag sets compiled in as step_fn_act chooses them (plain DYN,
// ground effect + drag, downwash in multi-drone envs), the other DYN combinations at run time
// POOL: empty, or PoolArgs<R> for a sim with a reset pool (the same flag sets, the pooled tail)
template <typename R, int ACT, typename... POOL>
const void* step_het_fn_act(bool multi, int flags) {
  if (multi) {
    switch (flags) {
      case 0: return (const void*)step_kernel_het<R, ACT, true, 0, POOL...>;
      case F_DW: return (const void*)step_kernel_het<R, ACT, true, F_DW, POOL...>;
      default: return (const void*)step_kernel_het<R, ACT, true, kPfRuntime, POOL...>;
    }
  }
  switch (flags) {
    case 0: return (const void*)step_kernel_het<R, ACT, false, 0, POOL...>;
    case kPfAero: return (const void*)step_kernel_het<R, ACT, false, kPfAero, POOL...>;
    default: return (const void*)step_kernel_het<R, ACT, false, kPfRuntime, POOL...>;
  }
}
// the one-wave step_kernel of an action type: the RPM types' flag-set list or the PID types' own
template <typename R>
const void* step_fn(int act, bool multi, int flags, bool stream) {
  return with_act(act, [&](auto a) {
    constexpr int ACT = decltype(a)::value;
    if constexpr (act_is_pid(ACT)) return step_fn_pid<R, ACT>(multi, flags);
    else return step_fn_act<R, ACT>(multi, flags, stream);
  });
}
template <typename R>
const void* step_kernel_fn(const gpd_sim* s) {
  const int act = s->cfg.act_type;
  const bool multi = s->D > 1;
  if (s->het)
    return with_rpm_act(act, [&](auto a) {
      constexpr int ACT = decltype(a)::value;
      return s->pool_on ? step_het_fn_act<R, ACT, PoolArgs<R>>(multi, s->cfg.physics_flags)
                        : step_het_fn_act<R, ACT>(multi, s->cfg.physics_flags);
    });
  if (s->duo)   // two waves, or three with the io wave
    return with_rpm_act(act, [&](auto a) {
      constexpr int ACT = decltype(a)::value;
      return s->step_waves == 3 ? (const void*)step_kernel_duo<R, ACT, true> : (const void*)step_kernel_duo<R, ACT, false>;
    });
  // the flags the kernel sees (Consts::flags, make_consts)
  const int pf = s->generic_pf ? kPfRuntime
                              : s->cfg.physics_flags | ((s->cfg.physics_flags & GPD_F_BULLET) ? GPD_F_GEOM_WRENCH : 0);
  return step_fn<R>(act, multi, pf, s->stream);
}

// gpd_step_seq's fused form (step_seq_kernel, gpd_step_seq.h): the sims whose step is
// step_kernel_duo<R, ACT, true>, one launch per kSeqStepsPerLaunch steps (gpd_cmd_rollout's default).
// f64 only: hipcc contracts the f32 instantiation's multiply-adds differently from the per-step
// kernel's (observations differ in last bits after 40 steps), so f32 sims keep the per-step loop
// and the f32 kernel is not built.  The kernel's hand-off buffers grow with the block's drones and
// the substeps (seq_lds_bytes); a sim whose buffers do not fit the workgroup's LDS beside the tile
// keeps the per-step loop as well (prepare_step_kernel decides: seq_lds).
constexpr int kSeqStepsPerLaunch = 256;
inline bool seq_kind(const gpd_sim* s) { return s->duo && s->step_waves == 3 && s->prec == GPD_F64; }
inline bool seq_fused(const gpd_sim* s) { return seq_kind(s) && s->seq_lds > 0; }
template <typename R>
const void* step_seq_fn(const gpd_sim* s) {
  if constexpr (sizeof(R) == 8)
    return with_rpm_act(s->cfg.act_type, [](auto a) { return (const void*)step_seq_kernel<R, decltype(a)::value>; });
  else
    return nullptr;
}
// the launches gpd_step_seq issues for n_steps steps
inline int step_seq_launches(const gpd_sim* s, int n_steps) {
  if (n_steps <= 0) return 0;
  return seq_fused(s) && n_steps >= 2 ? (n_steps + kSeqStepsPerLaunch - 1) / kSeqStepsPerLaunch : n_steps;
}

// static LDS of the run-time-flag step kernel of an action type (the one-wave kernel every sim
// that is not wide can fall back to: upload_tables)
template <typename R>
size_t runtime_step_lds(int act, bool multi) {
  const void* f = step_fn<R>(act, multi, kPfRuntime, false);
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, f) != hipSuccess) {
    (void)hipGetLastError();
    return kLdsBytes;
  }
  return fa.sharedSizeBytes;
}

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the kernel, not to a sim: it is only ever
// raised, so a later sim that needs less does not lower it under a live sim that needs more
inline hipError_t raise_dynamic_lds(const void* f, int bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, int> set_to;   // by device and kernel
  int dev = 0;
  if (const hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  int& cur = set_to[{dev, f}];
  if (bytes <= cur) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) cur = bytes;
  return e;
}

// the LDS budget and dynamic-LDS attribute of the step kernel the sim launches (again when a reset
// pool turns on or off: another instantiation)
template <typename R>
int prepare_step_kernel(gpd_sim* s) {
  if (s->wide) return GPD_OK;   // step_kernel_wide: no observation tile
  // the step kernel's static LDS (the PYB flag-set kernels park 44 KB of per-lane values around
  // the contact solve, gpd_device.h bullet_substep) beside the observation tile must fit the
  // workgroup's LDS; a long action history (high ctrl_freq) that leaves no room for it gets the
  // run-time-flag kernel, which solves the contact with its rows in 20 KB of LDS
  const void* f = step_kernel_fn<R>(s);
  hipFuncAttributes fa;
  HIP_TRY(hipFuncGetAttributes(&fa, f));
  if (fa.sharedSizeBytes + (size_t)s->tile_bytes > kLdsBytes && !s->generic_pf) {
    s->generic_pf = true;
    f = step_kernel_fn<R>(s);
    HIP_TRY(hipFuncGetAttributes(&fa, f));
  }
  if (fa.sharedSizeBytes + (size_t)s->tile_bytes > kLdsBytes && s->het)   // (gpd_create_het's host-side bound is the
    // first line of defence; this is the kernel's own figure)
    return fail(GPD_EUNSUPPORTED, "gpd_create_het: the action history does not fit the one-wave step kernel's "
                                  "observation tile beside its static LDS");
  if (fa.sharedSizeBytes + (size_t)s->tile_bytes > kLdsBytes)
    return fail(GPD_EUNSUPPORTED, "gpd_create: ctrl_freq too high for drone <-> drone contact (observation tile + "
                                  "the step kernel's LDS exceed 160 KiB; GPD_F_NO_DRONE_CONTACT lifts the limit)");
  // the observation tile can exceed the 64 KiB default dynamic-LDS limit for long histories
  if (s->tile_bytes > 65536) HIP_TRY(raise_dynamic_lds(f, s->tile_bytes));
  // gpd_step_seq's fused kernel keeps its action history in the same tile, with the rate chains'
  // hand-off buffers behind it
  s->seq_lds = 0;
  if (seq_kind(s)) {
    const void* fs = step_seq_fn<R>(s);
    const size_t need = seq_lds_bytes(s->tile_bytes, s->nsub, s->tpb, sizeof(R));
    HIP_TRY(hipFuncGetAttributes(&fa, fs));
    if (fa.sharedSizeBytes + need <= kLdsBytes) {
      s->seq_lds = (int)need;
      if (need > 65536) HIP_TRY(raise_dynamic_lds(fs, (int)need));
    }
  }
  return GPD_OK;
}

template <typename R>
int upload_tables(gpd_sim* s) {
  std::vector<R> ini(s->init_tmpl.begin(), s->init_tmpl.end());
  std::vector<R> tgt(s->target.begin(), s->target.end());
  const Consts<R> c = make_consts<R>(s);
  HIP_TRY(hipMemcpy(s->d_init, ini.data(), ini.size() * sizeof(R), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->d_target, tgt.data(), tgt.size() * sizeof(R), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->d_consts, &c, sizeof(c), hipMemcpyHostToDevice));
  return prepare_step_kernel<R>(s);
}

inline unsigned grid_for(long long n, int tpb) { return (unsigned)((n + tpb - 1) / tpb); }
inline size_t real_size(const gpd_sim* s) { return s->prec == GPD_F64 ? sizeof(double) : sizeof(float); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// Device buffer sizes in bytes, one definition each: create's allocation and clearing, save / load.
inline size_t state_buf_bytes(const gpd_sim* s) { return (size_t)kStateComps * s->npad * real_size(s); }
inline size_t ctrl_buf_bytes(const gpd_sim* s) { return (size_t)kCtrlComps * s->npad * real_size(s); }
inline size_t ring_buf_bytes(const gpd_sim* s) { return (size_t)s->ring_len * s->npad * s->A * sizeof(float); }
inline size_t ctr_buf_bytes(const gpd_sim* s) { return (size_t)s->E * sizeof(int2); }   // (+ one int2: the ring mark)
inline size_t tmpl_buf_bytes(const gpd_sim* s) { return s->init_tmpl.size() * real_size(s); }
inline size_t target_buf_bytes(const gpd_sim* s) { return s->target.size() * real_size(s); }
inline size_t etab_buf_bytes(const gpd_sim* s) { return (size_t)kHetCols * s->epad * real_size(s); }
inline size_t pool_desc_bytes(const gpd_sim* s) {
  return by_real(s, [](auto r) { return sizeof(ResetPool<decltype(r)>); });
}

// step_kernel_wide: the contact instantiation (DC) is the one-wave one (D <= 64)
template <typename R>
const void* step_wide_fn(int act, int D, bool dc) {
  return with_act(act, [&](auto a) {
    constexpr int ACT = decltype(a)::value;
    if (dc) return (const void*)step_kernel_wide<R, ACT, kWave, true>;
    return with_maxt(D, [](auto m) { return (const void*)step_kernel_wide<R, ACT, decltype(m)::value>; });
  });
}
template <typename R>
const void* integrate_wide_fn(int D, bool traj) {
  return with_maxt(D, [&](auto m) {
    constexpr int MAXT = decltype(m)::value;
    return traj ? (const void*)integrate_kernel_wide<R, true, MAXT> : (const void*)integrate_kernel_wide<R, false, MAXT>;
  });
}

// last_clipped_action back from the ring (store_drone_step) before anything reads or replaces
// state[16..19]; a no-op launch when no step ran since the last settle
template <typename R>
int settle_last(gpd_sim* s, hipStream_t st) {
  if (!(s->wt & 4)) return GPD_OK;
  const SimView<R> v = make_view<R>(s);
  const Consts<R>* c = (const Consts<R>*)s->d_consts;
  // a het sim: the env's own float32 hover constant
  const R* hover_env = s->het ? (const R*)s->d_etab + kHetHover * s->epad : nullptr;
  hipLaunchKernelGGL((last_from_ring_kernel<R>), dim3(grid_for(s->N, 256)), dim3(256), 0, st, v, c, hover_env);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(s->d_ctr + s->E, 0, sizeof(int2), st));
  return GPD_OK;
}
inline int settle_last_any(gpd_sim* s, hipStream_t st) {
  return by_real(s, [&](auto r) { return settle_last<decltype(r)>(s, st); });
}

template <typename R>
int launch_step(gpd_sim* s, const float* actions, float* obs, float* reward, uint8_t* term, uint8_t* trunc,
                float* terminal_obs, hipStream_t st) {
  StepIO<R> io;
  io.actions = actions; io.obs = obs; io.reward = reward; io.term = term; io.trunc = trunc;
  io.terminal_obs = terminal_obs;
  const SimView<R> v = make_view<R>(s);
  const Consts<R>* c = (const Consts<R>*)s->d_consts;
  if (s->wide) {
    // drone <-> drone contact: the one-wave instantiation with the contact solve (D <= 64)
    const void* f = step_wide_fn<R>(s->cfg.act_type, s->D, s->dcP > 0);
    void* args[] = {(void*)&v, (void*)&io, (void*)&c};
    const int ge = s->tpb / s->D;   // envs per workgroup
    HIP_TRY(hipLaunchKernel(f, dim3((s->E + ge - 1) / ge), dim3((s->tpb + kWave - 1) / kWave * kWave), args, 0, st));
    return GPD_OK;
  }
  const unsigned grid = grid_for(s->N, s->tpb);
  const size_t lds = (size_t)s->tile_bytes;
  if (s->het) {
    typedef void (*HetFn)(R*, const float*, int2*, const Consts<R>*, const R*, int, int, long long, SimView<R>,
                          StepIO<R>);
    if (s->pool_on) {
      typedef void (*PoolFn)(R*, const float*, int2*, const Consts<R>*, const R*, int, int, long long, SimView<R>,
                             StepIO<R>, PoolArgs<R>);
      const PoolFn fp = (PoolFn)step_kernel_fn<R>(s);
      const PoolArgs<R> pa{(const ResetPool<R>*)s->d_pool, s->d_draws};
      hipLaunchKernelGGL(fp, dim3(grid), dim3(kWave), lds, st, v.state, io.actions, v.ctr, c, (const R*)s->d_etab,
                         v.N, v.tpb, s->epad, v, io, pa);
      HIP_TRY(hipGetLastError());
      return GPD_OK;
    }
    const HetFn fh = (HetFn)step_kernel_fn<R>(s);
    hipLaunchKernelGGL(fh, dim3(grid), dim3(kWave), lds, st, v.state, io.actions, v.ctr, c, (const R*)s->d_etab, v.N,
                       v.tpb, s->epad, v, io);
    HIP_TRY(hipGetLastError());
    return GPD_OK;
  }
  typedef void (*StepFn)(R*, const float*, int2*, const Consts<R>*, long long, int, int, SimView<R>, StepIO<R>);
  const StepFn f = (StepFn)step_kernel_fn<R>(s);
  hipLaunchKernelGGL(f, dim3(grid), dim3(s->step_waves * kWave), lds, st, v.state, io.actions, v.ctr, c, v.npad,
                     v.N, v.tpb, v, io);
  HIP_TRY(hipGetLastError());
  return GPD_OK;
}

// n_steps >= 2 steps of a seq_fused sim: step t reads slot (t % n_slots) of actions
template <typename R>
int launch_step_seq(gpd_sim* s, const float* actions, int n_slots, int n_steps, float* obs, float* reward,
                    uint8_t* term, uint8_t* trunc, float* terminal_obs, hipStream_t st) {
  StepIO<R> io;
  io.actions = actions; io.obs = obs; io.reward = reward; io.term = term; io.trunc = trunc;
  io.terminal_obs = terminal_obs;
  const SimView<R> v = make_view<R>(s);
  const Consts<R>* c = (const Consts<R>*)s->d_consts;
  typedef void (*SeqFn)(R*, const float*, int2*, const Consts<R>*, long long, int, int, SimView<R>, StepIO<R>, int, int,
                        int, int);
  const SeqFn f = (SeqFn)step_seq_fn<R>(s);
  const unsigned grid = grid_for(s->N, s->tpb);
  for (int t0 = 0; t0 < n_steps; t0 += kSeqStepsPerLaunch) {
    const int steps = std::min(kSeqStepsPerLaunch, n_steps - t0);
    hipLaunchKernelGGL(f, dim3(grid), dim3(4 * kWave), (size_t)s->seq_lds, st, v.state, actions, v.ctr, c, v.npad,
                       v.N, v.tpb, v, io, n_slots, t0 % n_slots, steps, seq_hand_off_at(s->tile_bytes));
    HIP_TRY(hipGetLastError());
  }
  return GPD_OK;
}

template <typename R>
int launch_integrate(gpd_sim* s, const void* rpm, int n_sub, void* traj, hipStream_t st) {
  const int rc = settle_last<R>(s, st);   // the raw substeps read and store last_clipped_action
  if (rc != GPD_OK) return rc;
  const SimView<R> v = make_view<R>(s);
  const Consts<R>* c = (const Consts<R>*)s->d_consts;
  const unsigned grid = grid_for(s->N, s->tpb);
  // plain DYN (the raw-integrator bench) compiled without flag tests; everything else at run time
  const bool plain = s->cfg.physics_flags == 0;
  const R* r = (const R*)rpm;
  R* tr = (R*)traj;
  if (s->wide && s->D > kWave) {   // (long-history envs of <= 64 drones: the one-wave kernels, no tile)
    const void* fw = integrate_wide_fn<R>(s->D, tr != nullptr);
    void* args[] = {(void*)&v, (void*)&c, (void*)&r, (void*)&n_sub, (void*)&tr};
    HIP_TRY(hipLaunchKernel(fw, dim3(s->E), dim3((s->D + kWave - 1) / kWave * kWave), args, 0, st));
    return GPD_OK;
  }
  if (s->het) {
    const bool multi = s->D > 1;
    const void* fh;
    if (tr) fh = multi ? (const void*)integrate_kernel_het<R, true, kPfRuntime, true>
                       : (const void*)integrate_kernel_het<R, false, kPfRuntime, true>;
    else if (multi) fh = plain ? (const void*)integrate_kernel_het<R, true, 0, false>
                               : (const void*)integrate_kernel_het<R, true, kPfRuntime, false>;
    else fh = plain ? (const void*)integrate_kernel_het<R, false, 0, false>
                    : (const void*)integrate_kernel_het<R, false, kPfRuntime, false>;
    const R* etab = (const R*)s->d_etab;
    long long epad = s->epad;
    void* hargs[] = {(void*)&v, (void*)&c, (void*)&etab, (void*)&epad, (void*)&r, (void*)&n_sub, (void*)&tr};
    HIP_TRY(hipLaunchKernel(fh, dim3(grid), dim3(kWave), hargs, 0, st));
    return GPD_OK;
  }
  const void* f;
  if (tr) {
    f = s->D > 1 ? (const void*)integrate_kernel<R, true, kPfRuntime, true>
                 : (const void*)integrate_kernel<R, false, kPfRuntime, true>;
  } else if (s->D > 1) {
    f = plain ? (const void*)integrate_kernel<R, true, 0, false> : (const void*)integrate_kernel<R, true, kPfRuntime, false>;
  } else {
    f = plain ? (s->N >= (1 << 19) ? (const void*)integrate_kernel<R, false, 0, false, true>
                                    : (const void*)integrate_kernel<R, false, 0, false>)
              : (const void*)integrate_kernel<R, false, kPfRuntime, false>;
  }
  void* args[] = {(void*)&v, (void*)&c, (void*)&r, (void*)&n_sub, (void*)&tr};
  HIP_TRY(hipLaunchKernel(f, dim3(grid), dim3(kWave), args, 0, st));
  HIP_TRY(hipGetLastError());
  return GPD_OK;
}

// gpd_cmd_step / gpd_cmd_rollout.  Instantiations: the RPM mode on plain DYN and on the run-time
// flags, the controller modes on the run-time flags only (every one that carries the contact code
// is expensive to compile), and the controller modes once more with PG, which read the kernels'
// last argument while a per-drone gain table is in force (gpd_set_pid_gains).  K names the kernel:
// CmdStepK or CmdRolloutK, the same choice on either.
template <typename K, bool MULTI>
const void* cmd_fn_multi(bool plain, bool ctrl, bool pg) {
  if (pg) return K::template fn<MULTI, kPfRuntime, true, true>();
  if (ctrl) return K::template fn<MULTI, kPfRuntime, true, false>();
  return plain ? K::template fn<MULTI, 0, false, false>() : K::template fn<MULTI, kPfRuntime, false, false>();
}
template <typename K>
const void* cmd_fn(bool multi, bool plain, bool ctrl, bool pg) {
  return multi ? cmd_fn_multi<K, true>(plain, ctrl, pg) : cmd_fn_multi<K, false>(plain, ctrl, pg);
}
template <typename R>
struct CmdStepK {
  template <bool MULTI, int PF, bool CTRL, bool PG>
  static const void* fn() { return (const void*)cmd_step_kernel<R, MULTI, PF, CTRL, PG>; }
};
template <typename R>
struct CmdRolloutK {
  template <bool MULTI, int PF, bool CTRL, bool PG>
  static const void* fn() { return (const void*)cmd_rollout_kernel<R, MULTI, PF, CTRL, PG>; }
};
template <typename R>
const void* cmd_step_wide_fn(int D, bool ctrl, bool pg) {
  return with_maxt(D, [&](auto m) {
    constexpr int MAXT = decltype(m)::value;
    if (pg) return (const void*)cmd_step_kernel_wide<R, MAXT, true, true>;
    return ctrl ? (const void*)cmd_step_kernel_wide<R, MAXT, true> : (const void*)cmd_step_kernel_wide<R, MAXT, false>;
  });
}

template <typename R>
int launch_cmd_step(gpd_sim* s, int mode, const void* actions, void* obs20, hipStream_t st) {
  // (no settle_last launch: a pending last-action-in-the-ring mark belongs to a sim without drag,
  // where the step reads no last_clipped_action; the kernel replaces the value and clears the mark)
  const SimView<R> v = make_view<R>(s);
  const Consts<R>* c = (const Consts<R>*)s->d_consts;
  const bool ctrl = mode != GPD_CMD_RPM;
  R max_rpm = (R)s->K.max_rpm;
  R* o = (R*)obs20;
  const bool pg = ctrl && s->gains_on;
  const R* g = pg ? (const R*)s->d_gains : nullptr;   // read by the PG instantiations only
  void* args[] = {(void*)&v, (void*)&c, (void*)&actions, (void*)&mode, (void*)&max_rpm, (void*)&o, (void*)&g};
  if (s->D > kWave) {
    const void* fw = cmd_step_wide_fn<R>(s->D, ctrl, pg);
    HIP_TRY(hipLaunchKernel(fw, dim3(s->E), dim3((s->D + kWave - 1) / kWave * kWave), args, 0, st));
    return GPD_OK;
  }
  const void* f = cmd_fn<CmdStepK<R>>(s->D > 1, s->cfg.physics_flags == 0, ctrl, pg);
  HIP_TRY(hipLaunchKernel(f, dim3(grid_for(s->N, s->tpb)), dim3(kWave), args, 0, st));
  return GPD_OK;
}

template <typename R>
int launch_cmd_rollout(gpd_sim* s, int mode, const void* actions, int n_steps, int record_every, void* traj,
                       void* obs20, void* metrics, int chunk, hipStream_t st) {
  const size_t row_bytes = (size_t)s->N * (mode == GPD_CMD_WAYPOINT ? 7 : 4) *
                           (mode == GPD_CMD_VEL ? sizeof(float) : sizeof(R));   // one step's commands
  const size_t rows20 = (size_t)s->N * 20;
  const char* act = (const char*)actions;
  R* tr = (R*)traj;
  R* m = (R*)metrics;
  if (s->D > kWave) {
    // envs of 65 .. 1024 drones: the command step's own wide kernel, one launch per step, storing a
    // recorded step's rows straight into traj; the tracking figures from a pass over the stored
    // positions behind every step
    const SimView<R> v = make_view<R>(s);
    for (int t = 0; t < n_steps; ++t) {
      const int g = t + 1;
      const bool rec = tr && g % record_every == 0, last = g == n_steps;
      R* dst = rec ? tr + (size_t)(g / record_every - 1) * rows20 : (last ? (R*)obs20 : nullptr);
      const int rc = launch_cmd_step<R>(s, mode, act + (size_t)t * row_bytes, dst, st);
      if (rc != GPD_OK) return rc;
      if (rec && last && obs20)
        HIP_TRY(hipMemcpyAsync(obs20, dst, rows20 * sizeof(R), hipMemcpyDeviceToDevice, st));
      if (m) {
        hipLaunchKernelGGL((cmd_track_kernel<R>), dim3(grid_for(s->N, 256)), dim3(256), 0, st, v,
                           (const R*)(act + (size_t)t * row_bytes), m, t > 0 ? 1 : 0);
        HIP_TRY(hipGetLastError());
      }
    }
    return GPD_OK;
  }
  const SimView<R> v = make_view<R>(s);
  const Consts<R>* c = (const Consts<R>*)s->d_consts;
  const bool pg = mode != GPD_CMD_RPM && s->gains_on;
  const void* f = cmd_fn<CmdRolloutK<R>>(s->D > 1, s->cfg.physics_flags == 0, mode != GPD_CMD_RPM, pg);
  const R* g = pg ? (const R*)s->d_gains : nullptr;   // read by the PG instantiations only
  R max_rpm = (R)s->K.max_rpm;
  for (int t0 = 0; t0 < n_steps; t0 += chunk) {
    int n = n_steps - t0 < chunk ? n_steps - t0 : chunk;
    const void* a = act + (size_t)t0 * row_bytes;
    int rec_phase = t0 % record_every, carry = t0 > 0 ? 1 : 0;
    long long rec_row = t0 / record_every;
    R* o = t0 + n == n_steps ? (R*)obs20 : nullptr;
    void* args[] = {(void*)&v, (void*)&c, (void*)&a, (void*)&mode, (void*)&max_rpm, (void*)&n, (void*)&record_every,
                    (void*)&rec_phase, (void*)&rec_row, (void*)&tr, (void*)&o, (void*)&m, (void*)&carry, (void*)&g};
    HIP_TRY(hipLaunchKernel(f, dim3(grid_for(s->N, s->tpb)), dim3(kWave), args, 0, st));
  }
  return GPD_OK;
}

template <typename R>
int launch_adjacency(gpd_sim* s, double radius, uint8_t* out, hipStream_t st) {
  const SimView<R> v = make_view<R>(s);
  const long long total = (long long)s->N * s->D;
  hipLaunchKernelGGL((adjacency_kernel<R>), dim3(grid_for(total, 256)), dim3(256), 0, st, v, radius, out);
  HIP_TRY(hipGetLastError());
  return GPD_OK;
}

template <typename R>
int launch_reset(gpd_sim* s, const uint8_t* mask, float* obs, hipStream_t st) {
  const SimView<R> v = make_view<R>(s);
  if (s->het)   // every drone's own template
    hipLaunchKernelGGL((reset_kernel<R, true>), dim3(grid_for(s->N, 256)), dim3(256), 0, st, v, mask, obs);
  else
    hipLaunchKernelGGL((reset_kernel<R, false>), dim3(grid_for(s->N, 256)), dim3(256), 0, st, v, mask, obs);
  HIP_TRY(hipGetLastError());
  return GPD_OK;
}

template <typename R>
int launch_state20(gpd_sim* s, void* out, int raw, hipStream_t st) {
  const int rc = settle_last<R>(s, st);
  if (rc != GPD_OK) return rc;
  const SimView<R> v = make_view<R>(s);
  hipLaunchKernelGGL((state20_kernel<R>), dim3(grid_for(s->N, 256)), dim3(256), 0, st, v, (R*)out, raw);
  HIP_TRY(hipGetLastError());
  return GPD_OK;
}

template <typename R>
int launch_nonfinite(gpd_sim* s, uint8_t* flags, hipStream_t st) {
  const SimView<R> v = make_view<R>(s);
  HIP_TRY(hipMemsetAsync(flags, 0, (size_t)s->E, st));
  hipLaunchKernelGGL((nonfinite_kernel<R>), dim3(grid_for(s->N, 256)), dim3(256), 0, st, v, flags);
  HIP_TRY(hipGetLastError());
  return GPD_OK;
}

template <typename R>
int launch_set_raw(gpd_sim* s, const void* in, hipStream_t st) {
  if (s->wt & 4) HIP_TRY(hipMemsetAsync(s->d_ctr + s->E, 0, sizeof(int2), st));   // all 20 replaced
  const SimView<R> v = make_view<R>(s);
  hipLaunchKernelGGL((set_raw_kernel<R>), dim3(grid_for(s->N, 256)), dim3(256), 0, st, v, (const R*)in);
  HIP_TRY(hipGetLastError());
  return GPD_OK;
}

void free_sim(gpd_sim* s) {
  if (!s) return;
  for (void* p : {s->d_state, s->d_ctrl, (void*)s->d_ring, (void*)s->d_ctr, s->d_init, s->d_target, s->d_consts, s->d_etab,
                  (void*)s->d_draws, s->d_pool, s->d_pool_rows, s->d_pool_init, s->d_pool_target, (void*)s->d_dc_tab,
                  s->d_dc_rows, s->d_gains})
    if (p) (void)hipFree(p);
  delete s;
}

// ---- heterogeneous sims (gpd_create_het)
// static LDS of step_kernel_het beside the observation tile: 0 for single-drone envs, 7.5 KiB for
// f64 multi-drone ones (positions, reward / distance / flag reduction, the downwash pair buffer)
constexpr size_t kHetStaticLds = 8192;

struct HetArgs {
  const gpd_env_params* rows;   // [E] or null
  const double* xyzs;           // [E][D][3] or null
  const double* rpys;           // [E][D][3] or null
};

// [E][D][10] templates and [E][D][3] targets from the stored het poses
void het_templates(gpd_sim* s) {
  pose_tables(s->cfg.task, (size_t)s->E, s->D, s->het_xyz.data(), s->het_rpy.data(), s->init_tmpl.data(),
              s->target.data());
}

// the kHetCols constants of one row: derived in double with make_consts' expressions, rounded once
// to R; put(col, value) places them (the env table's SoA columns, a reset pool's row-major rows)
template <typename R, typename Put>
void env_row_consts(const gpd_drone_params& base, const gpd_env_params& r, Put put) {
  gpd_constants K;
  derive_row(base, r, K);
  put(kHetM, (R)r.m); put(kHetGravity, (R)K.gravity); put(kHetInvM, (R)(1.0 / r.m));
  put(kHetKf, (R)r.kf); put(kHetKm, (R)r.km); put(kHetL, (R)r.arm); put(kHetLs2, (R)(r.arm / std::sqrt(2.0)));
  put(kHetJx, (R)r.ixx); put(kHetJy, (R)r.iyy); put(kHetJz, (R)r.izz);
  put(kHetIjx, (R)(1.0 / r.ixx)); put(kHetIjy, (R)(1.0 / r.iyy)); put(kHetIjz, (R)(1.0 / r.izz));
  put(kHetHover, (R)(double)(float)K.hover_rpm);   // float32(HOVER_RPM), exact in either real type
  put(kHetGeCoeff, (R)r.gnd_eff_coeff); put(kHetGeClip, (R)K.gnd_eff_h_clip);
  put(kHetDragXy, (R)r.drag_coeff_xy); put(kHetDragZ, (R)r.drag_coeff_z);
}

// the per-env constant table
template <typename R>
int upload_env_table(gpd_sim* s) {
  std::vector<R> tab((size_t)kHetCols * s->epad, R(0));
  for (int e = 0; e < s->E; ++e)
    env_row_consts<R>(s->P, s->env_rows[e], [&](int col, R v) { tab[(size_t)col * s->epad + e] = v; });
  HIP_TRY(hipMemcpy(s->d_etab, tab.data(), tab.size() * sizeof(R), hipMemcpyHostToDevice));
  return GPD_OK;
}

// ---- reset pools (gpd_set_reset_pool)
// Drawn rows / poses become the env's own (host copies included) and every index goes back to -1;
// the episode numbers stay.  Called, after a device synchronise, before anything replaces the
// pools or the env tables.  which: bit 0 rows, bit 1 poses.
int fold_draws(gpd_sim* s, int which) {
  std::vector<int> dr((size_t)s->E * 3);
  HIP_TRY(hipMemcpy(dr.data(), s->d_draws, dr.size() * sizeof(int), hipMemcpyDeviceToHost));
  const size_t D3 = (size_t)s->D * 3;
  for (int e = 0; e < s->E; ++e) {
    int* d = &dr[(size_t)e * 3];
    if ((which & 1) && d[1] >= 0) {
      if ((size_t)d[1] < s->pool_rows.size()) s->env_rows[e] = s->pool_rows[d[1]];
      d[1] = -1;
    }
    if ((which & 2) && d[2] >= 0) {
      if (((size_t)d[2] + 1) * D3 <= s->pool_xyz.size()) {
        std::copy_n(&s->pool_xyz[d[2] * D3], D3, &s->het_xyz[e * D3]);
        std::copy_n(&s->pool_rpy[d[2] * D3], D3, &s->het_rpy[e * D3]);
      }
      d[2] = -1;
    }
  }
  HIP_TRY(hipMemcpy(s->d_draws, dr.data(), dr.size() * sizeof(int), hipMemcpyHostToDevice));
  return GPD_OK;
}

template <typename R>
int upload_pool(gpd_sim* s, unsigned seed) {
  const int P = (int)s->pool_rows.size(), D = s->D;
  const size_t Q = s->pool_xyz.size() / ((size_t)D * 3);
  std::vector<R> rows((size_t)P * kHetCols);
  for (int i = 0; i < P; ++i)
    env_row_consts<R>(s->P, s->pool_rows[i], [&](int col, R v) { rows[(size_t)i * kHetCols + col] = v; });
  std::vector<double> tmpl(Q * D * 10), tgt(Q * D * 3);
  pose_tables(s->cfg.task, Q, D, s->pool_xyz.data(), s->pool_rpy.data(), tmpl.data(), tgt.data());
  const std::vector<R> ini(tmpl.begin(), tmpl.end()), tg(tgt.begin(), tgt.end());
  for (void** p : {&s->d_pool_rows, &s->d_pool_init, &s->d_pool_target}) {
    if (*p) HIP_TRY(hipFree(*p));
    *p = nullptr;
  }
  if (P > 0) {
    HIP_TRY(hipMalloc(&s->d_pool_rows, rows.size() * sizeof(R)));
    HIP_TRY(hipMemcpy(s->d_pool_rows, rows.data(), rows.size() * sizeof(R), hipMemcpyHostToDevice));
  }
  if (Q > 0) {
    HIP_TRY(hipMalloc(&s->d_pool_init, ini.size() * sizeof(R)));
    HIP_TRY(hipMalloc(&s->d_pool_target, tg.size() * sizeof(R)));
    HIP_TRY(hipMemcpy(s->d_pool_init, ini.data(), ini.size() * sizeof(R), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_pool_target, tg.data(), tg.size() * sizeof(R), hipMemcpyHostToDevice));
  }
  const ResetPool<R> desc{(const R*)s->d_pool_rows, (const R*)s->d_pool_init, (const R*)s->d_pool_target, P, (int)Q,
                          seed};
  HIP_TRY(hipMemcpy(s->d_pool, &desc, sizeof(desc), hipMemcpyHostToDevice));
  const bool on = P > 0 || Q > 0;
  if (on != s->pool_on) {   // another step kernel instantiation: its LDS budget and attribute
    s->pool_on = on;
    return prepare_step_kernel<R>(s);
  }
  return GPD_OK;
}

template <typename R>
int env_table_to_host(gpd_sim* s, double* out) {
  std::vector<R> tab((size_t)kHetCols * s->epad);
  HIP_TRY(hipMemcpy(tab.data(), s->d_etab, tab.size() * sizeof(R), hipMemcpyDeviceToHost));
  for (int e = 0; e < s->E; ++e)
    for (int c = 0; c < kHetCols; ++c) out[(size_t)e * kHetCols + c] = (double)tab[(size_t)c * s->epad + e];
  return GPD_OK;
}

// ---- the create path (gpd_create, gpd_create_het), in stages.  fn is the entry point's name, for
// the messages; the sim is held by a SimPtr from its allocation on, so every early return frees it.
struct SimDeleter { void operator()(gpd_sim* s) const { free_sim(s); } };
using SimPtr = std::unique_ptr<gpd_sim, SimDeleter>;

// what every sim needs of its configuration: all before the first device call
int validate_config(const std::string& fn, const gpd_drone_params* params, const gpd_config& C) {
  if (C.n_envs < 1) return fail(GPD_EINVAL, fn + ": n_envs must be >= 1");
  if (C.drones_per_env < 1 || C.drones_per_env > kWideMax)
    return fail(GPD_EINVAL, fn + ": drones_per_env must be in [1, 1024]");
  if (C.pyb_freq < 1 || C.ctrl_freq < 1) return fail(GPD_EINVAL, fn + ": frequencies must be >= 1");
  if (C.pyb_freq % C.ctrl_freq != 0)
    return fail(GPD_EINVAL, "[ERROR] in BaseAviary.__init__(), pyb_freq is not divisible by env_freq.");
  if (C.ctrl_freq / 2 < 1)
    return fail(GPD_EUNSUPPORTED, fn + ": ctrl_freq//2 == 0 gives an empty action buffer (unsupported)");
  if (C.act_type < GPD_ACT_RPM || C.act_type > GPD_ACT_ONE_D_PID) return fail(GPD_EINVAL, fn + ": bad act_type");
  const bool pid = act_is_pid(C.act_type);
  if (pid && params->model != GPD_MODEL_CF2X && params->model != GPD_MODEL_CF2P)  // BaseRLAviary.py:75-78
    return fail(GPD_EUNSUPPORTED,
                "[ERROR] in BaseRLAviary.__init()__, no controller is available for the specified drone_model");
  if (C.task < GPD_TASK_NONE || C.task > GPD_TASK_MULTIHOVER) return fail(GPD_EINVAL, fn + ": bad task");
  if (C.task == GPD_TASK_HOVER && C.drones_per_env != 1)
    return fail(GPD_EINVAL, fn + ": HoverAviary is single-drone (drones_per_env must be 1)");
  if (C.precision != GPD_F32 && C.precision != GPD_F64) return fail(GPD_EINVAL, fn + ": bad precision");
  if (C.solver_iterations < 0 || C.solver_iterations > 1000)
    return fail(GPD_EINVAL, fn + ": solver_iterations must be 0 (default) or in [1, 1000]");
  if (!std::isfinite(C.solver_residual)) return fail(GPD_EINVAL, fn + ": solver_residual must be finite");
  if ((C.physics_flags & GPD_F_BULLET) && C.drones_per_env > kWave && !(C.physics_flags & GPD_F_NO_DRONE_CONTACT))
    return fail(GPD_EUNSUPPORTED,
                fn + ": drone <-> drone contact is implemented for envs of up to 64 drones; pass "
                "GPD_F_NO_DRONE_CONTACT (aero 'no_drone_contact') for larger PYB* envs");
  if (C.physics_flags & ~(GPD_F_GND | GPD_F_DRAG | GPD_F_DW | GPD_F_GEOM_WRENCH | GPD_F_BULLET | GPD_F_NO_PLANE |
                          GPD_F_NO_DRONE_CONTACT))
    return fail(GPD_EINVAL, fn + ": unknown physics flag");
  if (params->model < GPD_MODEL_CF2X || params->model > GPD_MODEL_RACE)
    return fail(GPD_EINVAL, fn + ": unknown drone model");
  if ((long long)C.n_envs * C.drones_per_env > (1LL << 31) - 64) return fail(GPD_EINVAL, fn + ": too many drones");
  return GPD_OK;
}

// a sim of a validated configuration, its shape filled in and nothing on the device yet
SimPtr new_sim(const gpd_drone_params* params, const gpd_config& C, bool het) {
  SimPtr s(new gpd_sim());
  s->P = *params;
  s->cfg = C;
  s->cfg.init_xyzs_host = nullptr;
  s->cfg.init_rpys_host = nullptr;
  s->E = C.n_envs;
  s->D = C.drones_per_env;
  s->N = C.n_envs * C.drones_per_env;
  s->A = act_width(C.act_type);
  default_pid_params(&s->pid);
  s->ring_len = C.ctrl_freq / 2;  // ACTION_BUFFER_SIZE = int(ctrl_freq//2)  BaseRLAviary.py:66
  s->W = 12 + s->ring_len * s->A;
  s->nsub = C.pyb_freq / C.ctrl_freq;
  s->prec = C.precision;
  s->het = het;
  return s;
}

// The launch policy: the block shape, the wide / duo / stream kernels, the store policy, nc_magic
// and the downwash pairs.  The thresholds are measured; the comments carry the figures.
int plan_launch(const std::string& fn, gpd_sim* s) {
  const gpd_config& C = s->cfg;
  const long long Nll = s->N;
  // Drones per 64-lane block.  A wave's time is set by its serial instruction stream, not by
  // how many of its lanes are active, while a CU streams the observation rows of its blocks at
  // a limited store-issue rate; so when there are too few drones to give every CU a full wave,
  // blocks are thinned (down to 16 drones) to spread the rows over all 256 CUs.
  {
    const int full = (kWave / s->D) * s->D;
    const long long per_cu = (Nll + 255) / 256;
    int want = (int)std::min<long long>(full, std::max<long long>(16, per_cu));
    if (s->D > 1 && (C.physics_flags & GPD_F_DW)) {
      // downwash envs: the per-substep pair work is spread over a block's lanes, and about four
      // blocks per CU measured best (scripts/geom_probe_multi.py, D = 8, staggered init:
      // 512 envs 8 drones/block 13.2 us vs 16: 14.7; 2048 envs 16: 16.1 vs 64: 23.2;
      // 8192 envs 64: 27.3 vs 16: 50.3)
      want = (int)std::min<long long>(full, Nll / 1024);
    }
    want = std::max(s->D, (want / s->D) * s->D);
    if (C.drones_per_block > 0) want = std::max(s->D, std::min(full, (C.drones_per_block / s->D) * s->D));
    s->tpb = want;
    // envs of more than 64 drones: one env per multi-wave workgroup (step_kernel_wide).  Also an
    // observation row too long for the one-wave kernels (their LDS tile of 64 rows beside the
    // run-time-flag kernel's static LDS: a long action history, e.g. RPM actions at ctrl_freq 480):
    // the wide kernel copies the history columns without a tile (with the drone <-> drone contact
    // in its one-wave instantiation, D <= 64)
    const size_t tile = (size_t)step_tile_bytes(s->A, s->ring_len);
    const size_t lds_rt = s->D > kWave || s->het ? 0   // (a het sim never launches that kernel)
                          : (C.precision == GPD_F64 ? runtime_step_lds<double>(C.act_type, s->D > 1)
                                                    : runtime_step_lds<float>(C.act_type, s->D > 1));
    s->wide = s->D > kWave || tile + lds_rt > (size_t)kLdsBytes;
    if (s->het) s->wide = false;   // gpd_create_het checked D and the tile against step_kernel_het's LDS
    // envs of up to 32 drones share the wave, up to 64 / D of them, as many as leave ~2048
    // workgroups (the history copy's loads in flight: 4096 single-drone envs at ctrl_freq 480
    // 37.8 us per step with one env per workgroup, 86.7 with 64; 65536 envs 591 / 213 us);
    // gpd_config::drones_per_block overrides
    if (s->wide) {
      int ge = 1;
      if (s->D <= kWave / 2) {
        const int gmax = kWave / s->D;
        ge = C.drones_per_block > 0 ? C.drones_per_block / s->D : (int)std::min<long long>(gmax, C.n_envs / 2048);
        ge = std::max(1, std::min(gmax, ge));
      }
      s->tpb = ge * s->D;
    }
  }
  s->npad = ((long long)s->N + 63) / 64 * 64;
  {
    // downwash pairs over idle lanes: only for thin blocks whose pairs fit the LDS buffer
    const int D = s->D, n = s->tpb * D;
    if (D > 1 && (C.physics_flags & GPD_F_DW) && s->tpb < kWave && n <= kPairMax) {
      const int m = ((1 << 20) + D - 1) / D;
      bool ok = true;
      for (int p = 0; p < n && ok; ++p) ok = ((p * m) >> 20) == p / D;
      if (ok) s->dw_pairs = DwPairs{n, m};
    }
  }
  {
    // write-through (sc1) stores for the obs rows (bit 0) and the state (bit 1), default both:
    // measured on one MI355X, 4096 envs 8.60 -> 8.37 us/step and 65536 envs 15.3 -> 13.7 us,
    // large N unchanged (gpd_config::store_policy overrides).  State only while its byte
    // offsets fit the 32-bit buffer offset (re-applied after the wave-count policies below).
    s->wt = C.store_policy > 0 ? ((C.store_policy - 1) & 3) : 3;
    // bit 2: the step kernels leave last_clipped_action in the ring (store_drone_step) where
    // the step never reads it back: RPM action types (the ring holds the very actions it maps),
    // no drag (the only reader, on the first substep)
    if ((C.act_type == GPD_ACT_RPM || C.act_type == GPD_ACT_ONE_D_RPM) && !(C.physics_flags & GPD_F_DRAG)) s->wt |= 4;
  }
  s->bound_xy = C.task == GPD_TASK_MULTIHOVER ? 2.0 : 1.5;
  s->tile_bytes = step_tile_bytes(s->A, s->ring_len);
  {
    // division-free row/column split of the copy-out (t / NC for t <= 64)
    const int NC = s->A == 4 ? 3 + s->ring_len : 12 + s->ring_len * s->A;
    s->nc_magic = (65536 + NC - 1) / NC;
    for (int t = 0; t <= kWave && !s->wide; ++t)   // (the wide kernel has no tile copy-out)
      if ((t * s->nc_magic) >> 16 != t / NC)
        return fail(GPD_EUNSUPPORTED, fn + ": observation width not supported by the tile copy-out");
    // two-wave step (step_kernel_duo) for the plain-DYN single-drone RPM path while the launch
    // is latency-bound: up to 64K drones (<= 4 blocks per CU).  Measured on one MI355X
    // (scripts/geom_probe.py): 4096 envs 6.28 -> 5.71 us/step, 16384 envs 7.48 -> 6.49,
    // 65536 envs 10.45 -> 10.31, but 262144 envs 35.8 -> 38.1 (bandwidth-bound: the second
    // wave only adds occupancy pressure).  Its 128-lane copy-out needs t / NC for t <= 128.
    // A third (io) wave takes the history columns off the pose wave (step_waves = 3): measured
    // (scripts/geom_probe.py, gpurun_out r2n) 2048 envs 5.30 -> 5.24 us/step, 4096 envs 5.40 ->
    // 5.33, but 8192 envs 5.72 -> 5.90 and 16384 envs 6.23 -> 7.20: with fuller blocks the
    // two-wave copy-out overlaps other blocks' work anyway.
    // gpd_config::step_waves overrides (1, 2 or 3).
    const bool duo_ok = !s->het && !s->wide && s->D == 1 && C.physics_flags == 0 &&
                        (C.act_type == GPD_ACT_RPM || C.act_type == GPD_ACT_ONE_D_RPM);
    int waves = !duo_ok || s->N > 65536 ? 1 : (s->N <= 4096 ? 3 : 2);
    if (C.step_waves > 0) waves = duo_ok ? std::min(3, C.step_waves) : 1;
    for (int t = 0; t <= 2 * kWave && waves == 2; ++t)
      if ((t * s->nc_magic) >> 16 != t / NC) waves = 1;
    s->step_waves = waves;
    s->duo = waves >= 2;
    // streaming cache policies for the single-wave plain-DYN kernel once a step's working set
    // (~820 B per drone: state, ring, rows) is well past the 256 MB Infinity Cache (>= 512K drones;
    // 262144 envs = 215 MB stay with the default policies, 1M envs 194 -> 145 us with STREAM,
    // 4096 envs 4.93 -> 6.31 us had it been used there)
    s->stream = !s->het && !s->duo && !s->wide && s->D == 1 && C.physics_flags == 0 &&
                (C.act_type == GPD_ACT_RPM || C.act_type == GPD_ACT_ONE_D_RPM) && s->N >= (1 << 19);
    // the multi-wave kernels store their state plainly (measured 4096 envs 5.47 -> 5.37 us/step);
    // the single-wave kernel keeps write-through state stores (262144 envs 36.7 -> 35.9 us)
    if (s->duo && C.store_policy <= 0) s->wt &= ~2;
    // the io-wave kernel writes each observation row in two parts from two waves (12 state columns,
    // history columns): write-through row stores leave those lines partially written twice, +0.29 MB
    // of HBM writes per launch at 4096 envs (PMC/alg 1.232 -> 1.143 with plain row stores and
    // write-through state, store_policy 3; step time 4.93 vs 4.97 us, within the run-to-run spread:
    // profiles/r3/pmc4096, profiles/r3/policy_4096.log)
    if (waves == 3 && C.store_policy <= 0) s->wt = (s->wt & ~1) | 2;
    // write-through state stores address the whole state through one buffer resource with 32-bit
    // offsets (store_drone_wt): whatever the policy above chose, never past 2 GiB of state
    const size_t state_bytes = (size_t)kStateComps * s->npad * (C.precision == GPD_F64 ? 8 : 4);
    if (state_bytes >= 0x7fffffffULL) s->wt &= ~2;
  }
  if (s->tile_bytes > kLdsBytes && !s->wide)
    return fail(GPD_EUNSUPPORTED, fn + ": ctrl_freq too high for drone <-> drone contact (observation tile "
                                  "exceeds 160 KiB of LDS; GPD_F_NO_DRONE_CONTACT lifts the limit)");
  return GPD_OK;
}

// gpd_constants: the derived constants (BaseAviary.py:117-128) and the sim's shape.
// (gpd_host_model.h's derive_row derives a het sim's env rows from the same lines but squares
// MAX_RPM as Python's **2 does, with libm's pow, where this squares with x*x; the two can differ in
// the last bit for user-supplied parameters, and gpd_get_constants and Consts::ge_clip are pinned
// to this one: do not merge them)
void derive_constants(gpd_sim* s) {
  const gpd_drone_params& P = s->P;
  const gpd_config& C = s->cfg;
  gpd_constants& K = s->K;
  std::memset(&K, 0, sizeof(K));
  K.gravity = 9.8 * P.m;
  K.hover_rpm = std::sqrt(K.gravity / (4 * P.kf));
  K.max_rpm = std::sqrt((P.thrust2weight * K.gravity) / (4 * P.kf));
  K.max_thrust = 4 * P.kf * (K.max_rpm * K.max_rpm);
  K.max_xy_torque = P.model == GPD_MODEL_CF2P ? P.arm * P.kf * (K.max_rpm * K.max_rpm)
                                              : (2 * P.arm * P.kf * (K.max_rpm * K.max_rpm)) / std::sqrt(2.0);
  K.max_z_torque = 2 * P.km * (K.max_rpm * K.max_rpm);
  K.gnd_eff_h_clip = 0.25 * P.prop_radius *
                     std::sqrt((15 * (K.max_rpm * K.max_rpm) * P.kf * P.gnd_eff_coeff) / K.max_thrust);
  K.pyb_timestep = 1.0 / C.pyb_freq;
  K.ctrl_timestep = 1.0 / C.ctrl_freq;
  K.pyb_steps_per_ctrl = s->nsub;
  K.action_buffer_size = s->ring_len;
  K.obs_width = s->W;
  K.act_width = s->A;
  K.n_drones = s->N;
  K.drones_per_block = s->tpb;
  K.lanes_per_block = s->step_waves * kWave;
  K.trunc_step_counter = trunc_step_counter(C.episode_len_sec, C.pyb_freq);
}

// The reset template and the targets: INIT_XYZS / INIT_RPYS (BaseAviary.py:194-197; C's tables or
// the default layout) through pose_tables.  One set of D poses for the sim; on a het sim one per
// env, C's set for every env unless the per-env tables replace it.  C is the caller's config:
// the sim's copy keeps no host pointers.
void build_templates(gpd_sim* s, const gpd_config& C, const HetArgs* het) {
  const gpd_drone_params& P = s->P;
  const size_t D3 = (size_t)s->D * 3;
  std::vector<double> xyz(D3), rpy(D3, 0.0);
  for (int d = 0; d < s->D; ++d) {
    xyz[d * 3 + 0] = d * 4 * P.arm;
    xyz[d * 3 + 1] = d * 4 * P.arm;
    xyz[d * 3 + 2] = P.collision_h / 2 - P.collision_z_offset + .1;
  }
  if (C.init_xyzs_host) xyz.assign(C.init_xyzs_host, C.init_xyzs_host + D3);
  if (C.init_rpys_host) rpy.assign(C.init_rpys_host, C.init_rpys_host + D3);
  const size_t TE = s->het ? (size_t)s->E : 1;   // template / target tables: per env on a het sim
  s->init_tmpl.assign(TE * s->D * 10, 0.0);
  s->target.assign(TE * s->D * 3, 0.0);
  if (!s->het) {
    pose_tables(C.task, 1, s->D, xyz.data(), rpy.data(), s->init_tmpl.data(), s->target.data());
    return;
  }
  s->epad = ((long long)s->E + 63) / 64 * 64;
  if (het->rows) s->env_rows.assign(het->rows, het->rows + s->E);
  else s->env_rows.assign((size_t)s->E, env_row_of(P));
  s->het_xyz.resize((size_t)s->N * 3);
  s->het_rpy.resize((size_t)s->N * 3);
  for (int e = 0; e < s->E; ++e) {
    std::copy_n(het->xyzs ? het->xyzs + e * D3 : xyz.data(), D3, &s->het_xyz[e * D3]);
    std::copy_n(het->rpys ? het->rpys + e * D3 : rpy.data(), D3, &s->het_rpy[e * D3]);
  }
  het_templates(s);
}

// hipMalloc on the create path: GPD_ENOMEM under the caller's message
int dev_alloc(void** p, size_t bytes, const std::string& msg) {
  if (hipMalloc(p, bytes) == hipSuccess) return GPD_OK;
  (void)hipGetLastError();
  return fail(GPD_ENOMEM, msg);
}

// drone <-> drone contact (gpd_dcontact.h DcHook / dc_solve): the pair table of an env and the
// row store for a block's contacts past its first 64 (up to kDcPts per pair: the closest point
// and the face manifold)
int alloc_drone_contact(const std::string& fn, gpd_sim* s) {
  const int D = s->D, P = D * (D - 1) / 2;
  const int npairs = (s->tpb / D) * P;
  s->dcP = P;
  s->dc_pmagic = ((1 << 24) + P - 1) / P;   // exact for p < npairs <= 32 (D - 1) <= 2016 (p P < 2^24)
  for (int p = 0; p < npairs; ++p)
    if (((p * s->dc_pmagic) >> 24) != p / P)
      return fail(GPD_EUNSUPPORTED, fn + ": drone contact pair layout not supported");
  std::vector<int> tab;
  tab.reserve(P);
  for (int i = 0; i < D; ++i)
    for (int j = i + 1; j < D; ++j) tab.push_back(i | (j << 8));   // bullet_mb.drone_contacts' order
  int rc = dev_alloc((void**)&s->d_dc_tab, (size_t)P * sizeof(int), fn + ": drone contact pair table");
  if (rc != GPD_OK) return rc;
  if (hipMemcpy(s->d_dc_tab, tab.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    return fail(GPD_ENOMEM, fn + ": drone contact pair table");
  }
  if (npairs * kDcPts > kDcRegRows * kWave) {
    const int row_reals = by_real(s, [](auto r) { return dc_row_reals<decltype(r)>(); });
    const int chunks = (npairs * kDcPts + kWave - 1) / kWave - kDcRegRows;
    s->dc_row_stride = (long long)chunks * kWave * row_reals;
    const long long blocks = ((long long)s->N + s->tpb - 1) / s->tpb;
    rc = dev_alloc(&s->d_dc_rows, (size_t)(blocks * s->dc_row_stride) * real_size(s), fn + ": drone contact row store");
  }
  return rc;
}

int alloc_device(const std::string& fn, gpd_sim* s) {
  const std::string msg = fn + ": hipMalloc failed";
  int rc = dev_alloc(&s->d_state, state_buf_bytes(s), msg);
  if (rc == GPD_OK) rc = dev_alloc((void**)&s->d_ring, ring_buf_bytes(s), msg);
  if (rc == GPD_OK) rc = dev_alloc((void**)&s->d_ctr, ctr_buf_bytes(s) + sizeof(int2), msg);
  if (rc == GPD_OK) rc = dev_alloc(&s->d_init, tmpl_buf_bytes(s), msg);
  if (rc == GPD_OK) rc = dev_alloc(&s->d_target, target_buf_bytes(s), msg);
  if (rc == GPD_OK) rc = dev_alloc(&s->d_consts, by_real(s, [](auto r) { return sizeof(Consts<decltype(r)>); }), msg);
  if (rc == GPD_OK && act_is_pid(s->cfg.act_type)) rc = dev_alloc(&s->d_ctrl, ctrl_buf_bytes(s), msg);
  if (rc == GPD_OK && s->het) rc = dev_alloc(&s->d_etab, etab_buf_bytes(s), msg);
  if (rc == GPD_OK && s->het) rc = dev_alloc((void**)&s->d_draws, (size_t)s->E * 3 * sizeof(int), msg);
  if (rc == GPD_OK && s->het) rc = dev_alloc(&s->d_pool, pool_desc_bytes(s), msg);
  const int pf = s->cfg.physics_flags;
  if (rc == GPD_OK && (pf & GPD_F_BULLET) && s->D > 1 && !(pf & GPD_F_NO_DRONE_CONTACT)) rc = alloc_drone_contact(fn, s);
  return rc;
}

// the tables onto the device, every buffer cleared, every env reset
int upload_and_reset(const std::string& fn, gpd_sim* s) {
  int rc = by_real(s, [&](auto r) { return upload_tables<decltype(r)>(s); });
  if (rc == GPD_OK && s->het) rc = by_real(s, [&](auto r) { return upload_env_table<decltype(r)>(s); });
  if (rc == GPD_OK && s->het) {   // no pool; every env in episode 0 on its own row and pose
    std::vector<int> dr((size_t)s->E * 3, -1);
    for (int e = 0; e < s->E; ++e) dr[(size_t)e * 3] = 0;
    if (hipMemset(s->d_pool, 0, pool_desc_bytes(s)) != hipSuccess ||
        hipMemcpy(s->d_draws, dr.data(), dr.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(GPD_EHIP, "gpd_create_het: reset pool state");
  }
  if (rc != GPD_OK) return rc;
  if (hipMemset(s->d_state, 0, state_buf_bytes(s)) != hipSuccess ||
      hipMemset(s->d_ring, 0, ring_buf_bytes(s)) != hipSuccess ||
      hipMemset(s->d_ctr, 0, ctr_buf_bytes(s) + sizeof(int2)) != hipSuccess ||
      (s->d_ctrl && hipMemset(s->d_ctrl, 0, ctrl_buf_bytes(s)) != hipSuccess))
    return fail(GPD_EHIP, fn + ": hipMemset failed");
  rc = by_real(s, [&](auto r) { return launch_reset<decltype(r)>(s, nullptr, nullptr, 0); });
  if (rc == GPD_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(GPD_EHIP, fn + ": initial reset failed");
  return rc;
}

// gpd_create (het null) and gpd_create_het, which has checked what only a het sim needs
int create_impl(const std::string& fn, const gpd_drone_params* params, const gpd_config* cfg, const HetArgs* het,
                gpd_sim** out) {
  if (!params || !cfg || !out) return fail(GPD_EINVAL, fn + ": NULL argument");
  *out = nullptr;
  int rc = validate_config(fn, params, *cfg);
  if (rc != GPD_OK) return rc;
  SimPtr s = new_sim(params, *cfg, het != nullptr);
  rc = plan_launch(fn, s.get());
  if (rc != GPD_OK) return rc;
  derive_constants(s.get());
  build_templates(s.get(), *cfg, het);
  rc = alloc_device(fn, s.get());
  if (rc == GPD_OK) rc = upload_and_reset(fn, s.get());
  if (rc != GPD_OK) return rc;
  *out = s.release();
  return GPD_OK;
}

// gpd_set_pid_gains: the [N][18] table rounded once to the sim's real type, tiled [npad/64][18][64]
// (padding drones: zeros, never read)
template <typename R>
int install_gains(gpd_sim* sim, const double* gains) {
  const size_t N = (size_t)sim->N;
  std::vector<double> stored(N * kGainComps);
  std::vector<R> tiled((size_t)kGainComps * (size_t)sim->npad, R(0));
  for (size_t n = 0; n < N; ++n)
    for (int k = 0; k < kGainComps; ++k) {
      const R x = (R)gains[n * kGainComps + k];
      tiled[(size_t)tidx((long long)n, k, kGainComps)] = x;
      stored[n * kGainComps + k] = (double)x;
      if (!std::isfinite(x))   // a finite double past float's range rounds to infinity
        return fail(GPD_EINVAL, "gpd_set_pid_gains: non-finite value in row " + std::to_string(n) + ", column " +
                                    std::to_string(k) + " (out of float32 range)");
    }
  const size_t bytes = tiled.size() * sizeof(R);
  HIP_TRY(hipDeviceSynchronize());
  if (!sim->d_gains && hipMalloc(&sim->d_gains, bytes) != hipSuccess) {
    sim->d_gains = nullptr;
    return fail(GPD_ENOMEM, "gpd_set_pid_gains: device allocation of the gain table failed");
  }
  HIP_TRY(hipMemcpy(sim->d_gains, tiled.data(), bytes, hipMemcpyHostToDevice));
  sim->gains.swap(stored);
  sim->gains_on = true;
  return GPD_OK;
}

// ---- argument checks shared by paired entry points; fn is the entry point's name.  The order of
// the checks is part of the interface: callers see the first failure.
int need_het(const char* fn, const gpd_sim* sim) {
  if (sim->het) return GPD_OK;
  return fail(GPD_EINVAL, std::string(fn) + ": not a het sim (create it with gpd_create_het)");
}

// gpd_step and gpd_step_seq (gpd_step: one slot)
int check_step_args(const char* fn, const gpd_sim* sim, const float* actions, const float* obs, const float* reward,
                    const uint8_t* terminated, const uint8_t* truncated, const float* terminal_obs, int n_slots = 1,
                    int n_steps = 0) {
  const auto err = [fn](int code, const std::string& what) { return fail(code, std::string(fn) + what); };
  if (!sim || !actions || !obs || !reward || !terminated || !truncated)
    return err(GPD_EINVAL, ": NULL argument");
  if (n_slots < 1 || n_steps < 0) return err(GPD_EINVAL, ": n_slots must be >= 1, n_steps >= 0");
  if (sim->A == 4 && !aligned16(actions)) return err(GPD_EINVAL, ": actions must be 16-byte aligned");
  if (sim->A == 4 && (!aligned16(obs) || (terminal_obs && !aligned16(terminal_obs))))
    return err(GPD_EINVAL, ": obs buffers must be 16-byte aligned");
  if (sim->gains_on)
    return err(GPD_EUNSUPPORTED, ": a per-drone gain table is in force (gpd_set_pid_gains) and the RL step "
                                 "reads the sim-wide coefficients; clear the table with gpd_set_pid_gains(sim, NULL)");
  return GPD_OK;
}

// gpd_cmd_step and gpd_cmd_rollout (gpd_cmd_step: a rollout of one step that records nothing)
int check_cmd_args(const char* fn, const gpd_sim* sim, int mode, const void* actions, const void* obs20,
                   int n_steps = 1, int record_every = 1, int max_steps_per_launch = 0, const void* traj = nullptr,
                   const void* metrics = nullptr) {
  const auto err = [fn](int code, const std::string& what) { return fail(code, std::string(fn) + what); };
  if (mode != GPD_CMD_RPM && mode != GPD_CMD_VEL && mode != GPD_CMD_WAYPOINT)
    return err(GPD_EINVAL, ": unknown mode " + std::to_string(mode) +
                           " (GPD_CMD_RPM, GPD_CMD_VEL or GPD_CMD_WAYPOINT)");
  if (n_steps < 0) return err(GPD_EINVAL, ": n_steps < 0");
  if (record_every < 1) return err(GPD_EINVAL, ": record_every must be >= 1");
  if (max_steps_per_launch < 0)
    return err(GPD_EINVAL, ": max_steps_per_launch must be 0 (the default, 256) or >= 1");
  if (!sim) return err(GPD_EINVAL, ": NULL sim");
  if (n_steps > 0 && !actions) return err(GPD_EINVAL, ": NULL actions");
  if (sim->het)
    return err(GPD_EUNSUPPORTED, ": not supported on a het sim (the command step kernels read the "
                                 "sim-wide drone parameters)");
  if (mode != GPD_CMD_RPM && !sim->d_ctrl)
    return err(GPD_EINVAL, ": the VEL and WAYPOINT modes run DSLPIDControl, and the sim's action type "
                           "has no controller (create it with a PID action type)");
  if (metrics && mode != GPD_CMD_WAYPOINT)
    return err(GPD_EINVAL, ": metrics needs GPD_CMD_WAYPOINT (the tracking error is measured "
                           "against the waypoint rows' target positions)");
  // RPM and VEL rows are loaded as 16-byte vectors, the state20 rows stored as such
  if (mode != GPD_CMD_WAYPOINT && actions && !aligned16(actions))
    return err(GPD_EINVAL, ": actions must be 16-byte aligned");
  if (traj && !aligned16(traj)) return err(GPD_EINVAL, ": traj must be 16-byte aligned");
  if (obs20 && !aligned16(obs20)) return err(GPD_EINVAL, ": obs20 must be 16-byte aligned");
  if (metrics && !aligned16(metrics)) return err(GPD_EINVAL, ": metrics must be 16-byte aligned");
  return GPD_OK;
}

}  // namespace

extern "C" {

int gpd_abi_version(void) { return GPD_ABI_VERSION; }

const char* gpd_last_error(void) { return g_err.c_str(); }

int gpd_default_params(int model, gpd_drone_params* out) { return default_params(model, out); }

int gpd_create(const gpd_drone_params* params, const gpd_config* cfg, gpd_sim** out) {
  return create_impl("gpd_create", params, cfg, nullptr, out);
}

int gpd_create_het(const gpd_drone_params* params, const gpd_config* cfg, const gpd_env_params* env_params_host,
                   const double* init_xyzs_host, const double* init_rpys_host, gpd_sim** out) {
  if (!params || !cfg || !out) return fail(GPD_EINVAL, "gpd_create_het: NULL argument");
  *out = nullptr;
  const gpd_config& C = *cfg;
  // what a het sim supports, then every row and pose: all before the first device call
  if (C.n_envs < 1) return fail(GPD_EINVAL, "gpd_create_het: n_envs must be >= 1");
  if (C.drones_per_env < 1) return fail(GPD_EINVAL, "gpd_create_het: drones_per_env must be >= 1");
  if (C.physics_flags & GPD_F_BULLET)
    return fail(GPD_EUNSUPPORTED, "gpd_create_het: GPD_F_BULLET (Physics.PYB*) is not supported with per-env "
                                  "parameters: the contact solves hold mass and inertia in derived rows; use the DYN "
                                  "integrator (Physics.DYN)");
  if (C.physics_flags & ~kHetFlags) return fail(GPD_EINVAL, "gpd_create_het: unknown or contact-only physics flag");
  if (C.act_type != GPD_ACT_RPM && C.act_type != GPD_ACT_ONE_D_RPM)
    return fail(GPD_EUNSUPPORTED, "gpd_create_het: the PID action types are not supported with per-env parameters "
                                  "(DSLPIDControl is tuned for the nominal drone); use GPD_ACT_RPM or GPD_ACT_ONE_D_RPM");
  if (C.drones_per_env > kWave)
    return fail(GPD_EUNSUPPORTED, "gpd_create_het: drones_per_env > 64 needs the multi-wave step kernel, which has no "
                                  "per-env parameters");
  if (C.ctrl_freq >= 2 &&
      (size_t)step_tile_bytes(act_width(C.act_type), C.ctrl_freq / 2) + kHetStaticLds > kLdsBytes)
    return fail(GPD_EUNSUPPORTED, "gpd_create_het: the action history (ctrl_freq // 2 slots) does not fit the one-wave "
                                  "step kernel's observation tile; the multi-wave kernel has no per-env parameters");
  const long long N = (long long)C.n_envs * C.drones_per_env;
  int rc = env_params_host ? check_env_rows("gpd_create_het", env_params_host, C.n_envs) : GPD_OK;
  if (rc == GPD_OK) rc = check_poses("gpd_create_het", "init_xyzs", init_xyzs_host, N, C.drones_per_env);
  if (rc == GPD_OK) rc = check_poses("gpd_create_het", "init_rpys", init_rpys_host, N, C.drones_per_env);
  if (rc != GPD_OK) return rc;
  const HetArgs het{env_params_host, init_xyzs_host, init_rpys_host};
  return create_impl("gpd_create_het", params, cfg, &het, out);   // the shared checks under this entry point's name
}

int gpd_set_env_params(gpd_sim* sim, const gpd_env_params* rows_host) {
  if (!sim || !rows_host) return fail(GPD_EINVAL, "gpd_set_env_params: NULL argument");
  if (need_het("gpd_set_env_params", sim) != GPD_OK) return GPD_EINVAL;
  int rc = check_env_rows("gpd_set_env_params", rows_host, sim->E);
  if (rc != GPD_OK) return rc;
  // a last action still in the ring (store-policy bit 2) is rebuilt from the env's hover column:
  // settle it with the rows the steps ran on, before they are replaced
  rc = settle_last_any(sim, 0);
  if (rc != GPD_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  rc = fold_draws(sim, 1);   // every row index back to -1: the rows in force are the new ones
  if (rc != GPD_OK) return rc;
  sim->env_rows.assign(rows_host, rows_host + sim->E);
  return by_real(sim, [&](auto r) { return upload_env_table<decltype(r)>(sim); });
}

int gpd_set_env_init(gpd_sim* sim, const double* xyzs_host, const double* rpys_host) {
  if (!sim) return fail(GPD_EINVAL, "gpd_set_env_init: NULL sim");
  if (need_het("gpd_set_env_init", sim) != GPD_OK) return GPD_EINVAL;
  int rc = check_poses("gpd_set_env_init", "init_xyzs", xyzs_host, sim->N, sim->D);
  if (rc == GPD_OK) rc = check_poses("gpd_set_env_init", "init_rpys", rpys_host, sim->N, sim->D);
  if (rc != GPD_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  rc = fold_draws(sim, 2);   // a NULL table keeps the poses in force; every pose index back to -1
  if (rc != GPD_OK) return rc;
  if (xyzs_host) sim->het_xyz.assign(xyzs_host, xyzs_host + (size_t)sim->N * 3);
  if (rpys_host) sim->het_rpy.assign(rpys_host, rpys_host + (size_t)sim->N * 3);
  het_templates(sim);
  return by_real(sim, [&](auto r) { return upload_tables<decltype(r)>(sim); });
}

int gpd_env_derive(const gpd_drone_params* base, const gpd_env_params* rows, int n, gpd_constants* out) {
  if (!base || !rows || !out || n < 0) return fail(GPD_EINVAL, "gpd_env_derive: NULL argument or n < 0");
  for (int i = 0; i < n; ++i) derive_row(*base, rows[i], out[i]);
  return GPD_OK;
}

int gpd_reset_pool_draw(unsigned seed, int stream, long long env, int episode, int n) {
  if (n < 1) return 0;
  return pool_draw(seed, (unsigned)stream, (unsigned)env, (unsigned)episode, (unsigned)n);
}

int gpd_set_reset_pool(gpd_sim* sim, const gpd_env_params* rows_host, int n_rows, const double* xyzs_host,
                       const double* rpys_host, int n_poses, unsigned seed) {
  if (!sim) return fail(GPD_EINVAL, "gpd_set_reset_pool: NULL sim");
  if (need_het("gpd_set_reset_pool", sim) != GPD_OK) return GPD_EINVAL;
  if (n_rows < 0 || n_poses < 0) return fail(GPD_EINVAL, "gpd_set_reset_pool: n_rows and n_poses must be >= 0");
  if (n_rows > 0 && !rows_host) return fail(GPD_EINVAL, "gpd_set_reset_pool: rows_host is NULL but n_rows > 0");
  if (n_poses > 0 && !xyzs_host) return fail(GPD_EINVAL, "gpd_set_reset_pool: xyzs_host is NULL but n_poses > 0");
  const long long nq = (long long)n_poses * sim->D;
  int rc = check_env_rows("gpd_set_reset_pool", rows_host, n_rows, "pool row");
  if (rc == GPD_OK) rc = check_poses("gpd_set_reset_pool", "xyzs", n_poses ? xyzs_host : nullptr, nq, sim->D, "pool pose");
  if (rc == GPD_OK) rc = check_poses("gpd_set_reset_pool", "rpys", n_poses ? rpys_host : nullptr, nq, sim->D, "pool pose");
  if (rc != GPD_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  rc = fold_draws(sim, 3);   // what the old pools gave stays in force, as the env's own
  if (rc != GPD_OK) return rc;
  sim->pool_rows.assign(rows_host, rows_host + n_rows);
  sim->pool_xyz.assign(xyzs_host, xyzs_host + nq * 3);
  if (n_poses && rpys_host) sim->pool_rpy.assign(rpys_host, rpys_host + nq * 3);
  else sim->pool_rpy.assign((size_t)nq * 3, 0.0);
  return by_real(sim, [&](auto r) { return upload_pool<decltype(r)>(sim, seed); });
}

int gpd_get_reset_draws(gpd_sim* sim, int* out_dev, void* stream) {
  if (!sim || !out_dev) return fail(GPD_EINVAL, "gpd_get_reset_draws: NULL argument");
  if (need_het("gpd_get_reset_draws", sim) != GPD_OK) return GPD_EINVAL;
  HIP_TRY(hipMemcpyAsync(out_dev, sim->d_draws, (size_t)sim->E * 3 * sizeof(int), hipMemcpyDeviceToDevice,
                         (hipStream_t)stream));
  return GPD_OK;
}

int gpd_get_env_table(gpd_sim* sim, double* out_host) {
  if (!sim || !out_host) return fail(GPD_EINVAL, "gpd_get_env_table: NULL argument");
  if (need_het("gpd_get_env_table", sim) != GPD_OK) return GPD_EINVAL;
  HIP_TRY(hipDeviceSynchronize());
  return by_real(sim, [&](auto r) { return env_table_to_host<decltype(r)>(sim, out_host); });
}

int gpd_destroy(gpd_sim* sim) {
  if (!sim) return fail(GPD_EINVAL, "gpd_destroy: NULL sim");
  (void)hipDeviceSynchronize();
  free_sim(sim);
  return GPD_OK;
}

int gpd_get_constants(const gpd_sim* sim, gpd_constants* out) {
  if (!sim || !out) return fail(GPD_EINVAL, "gpd_get_constants: NULL argument");
  *out = sim->K;
  return GPD_OK;
}

int gpd_reset(gpd_sim* sim, const uint8_t* env_mask, float* obs, void* stream) {
  if (!sim) return fail(GPD_EINVAL, "gpd_reset: NULL sim");
  return by_real(sim, [&](auto r) { return launch_reset<decltype(r)>(sim, env_mask, obs, (hipStream_t)stream); });
}

int gpd_step(gpd_sim* sim, const float* actions, float* obs, float* reward, uint8_t* terminated,
             uint8_t* truncated, float* terminal_obs, void* stream) {
  const int rc = check_step_args("gpd_step", sim, actions, obs, reward, terminated, truncated, terminal_obs);
  if (rc != GPD_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  return by_real(sim, [&](auto r) {
    return launch_step<decltype(r)>(sim, actions, obs, reward, terminated, truncated, terminal_obs, st);
  });
}

int gpd_step_seq(gpd_sim* sim, const float* actions, int n_slots, int n_steps, float* obs, float* reward,
                 uint8_t* terminated, uint8_t* truncated, float* terminal_obs, void* stream) {
  const int rc = check_step_args("gpd_step_seq", sim, actions, obs, reward, terminated, truncated, terminal_obs, n_slots,
                                 n_steps);
  if (rc != GPD_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t slot = (size_t)sim->N * sim->A;
  return by_real(sim, [&](auto r) {
    if (seq_fused(sim) && n_steps >= 2)
      return launch_step_seq<decltype(r)>(sim, actions, n_slots, n_steps, obs, reward, terminated, truncated,
                                          terminal_obs, st);
    for (int t = 0; t < n_steps; ++t) {
      const float* a = actions + (size_t)(t % n_slots) * slot;
      const int rc = launch_step<decltype(r)>(sim, a, obs, reward, terminated, truncated, terminal_obs, st);
      if (rc != GPD_OK) return rc;
    }
    return (int)GPD_OK;
  });
}

int gpd_step_seq_plan(const gpd_sim* sim, int n_steps) {
  if (!sim) return fail(GPD_EINVAL, "gpd_step_seq_plan: NULL sim");
  return step_seq_launches(sim, n_steps);
}

int gpd_integrate(gpd_sim* sim, const void* rpm, int n_sub, void* traj, void* stream) {
  if (!sim || !rpm) return fail(GPD_EINVAL, "gpd_integrate: NULL argument");
  if (n_sub < 0) return fail(GPD_EINVAL, "gpd_integrate: n_sub < 0");
  if (n_sub == 0) return GPD_OK;
  return by_real(sim, [&](auto r) { return launch_integrate<decltype(r)>(sim, rpm, n_sub, traj, (hipStream_t)stream); });
}

int gpd_cmd_step(gpd_sim* sim, int mode, const void* actions, void* obs20, void* stream) {
  const int rc = check_cmd_args("gpd_cmd_step", sim, mode, actions, obs20);
  if (rc != GPD_OK) return rc;
  return by_real(sim, [&](auto r) { return launch_cmd_step<decltype(r)>(sim, mode, actions, obs20, (hipStream_t)stream); });
}

int gpd_cmd_rollout(gpd_sim* sim, int mode, const void* actions, int n_steps, int record_every, void* traj,
                    void* obs20, void* metrics, int max_steps_per_launch, void* stream) {
  const int rc = check_cmd_args("gpd_cmd_rollout", sim, mode, actions, obs20, n_steps, record_every,
                                max_steps_per_launch, traj, metrics);
  if (rc != GPD_OK) return rc;
  if (n_steps == 0) return GPD_OK;
  const int chunk = max_steps_per_launch == 0 ? 256 : max_steps_per_launch;
  hipStream_t st = (hipStream_t)stream;
  return by_real(sim, [&](auto r) {
    return launch_cmd_rollout<decltype(r)>(sim, mode, actions, n_steps, record_every, traj, obs20, metrics, chunk, st);
  });
}

int gpd_adjacency(gpd_sim* sim, double radius, uint8_t* out, void* stream) {
  if (!sim) return fail(GPD_EINVAL, "gpd_adjacency: NULL sim");
  if (!out) return fail(GPD_EINVAL, "gpd_adjacency: NULL out");
  if (std::isnan(radius)) return fail(GPD_EINVAL, "gpd_adjacency: radius is NaN");
  return by_real(sim, [&](auto r) { return launch_adjacency<decltype(r)>(sim, radius, out, (hipStream_t)stream); });
}

int gpd_get_state20(gpd_sim* sim, void* out, void* stream) {
  if (!sim || !out) return fail(GPD_EINVAL, "gpd_get_state20: NULL argument");
  return by_real(sim, [&](auto r) { return launch_state20<decltype(r)>(sim, out, 0, (hipStream_t)stream); });
}

int gpd_get_raw_state(gpd_sim* sim, void* out, void* stream) {
  if (!sim || !out) return fail(GPD_EINVAL, "gpd_get_raw_state: NULL argument");
  return by_real(sim, [&](auto r) { return launch_state20<decltype(r)>(sim, out, 1, (hipStream_t)stream); });
}

int gpd_nonfinite(gpd_sim* sim, uint8_t* env_flags, void* stream) {
  if (!sim || !env_flags) return fail(GPD_EINVAL, "gpd_nonfinite: NULL argument");
  return by_real(sim, [&](auto r) { return launch_nonfinite<decltype(r)>(sim, env_flags, (hipStream_t)stream); });
}

int gpd_set_raw_state(gpd_sim* sim, const void* in, void* stream) {
  if (!sim || !in) return fail(GPD_EINVAL, "gpd_set_raw_state: NULL argument");
  return by_real(sim, [&](auto r) { return launch_set_raw<decltype(r)>(sim, in, (hipStream_t)stream); });
}

int gpd_default_pid_params(gpd_pid_params* out) { return default_pid_params(out); }

int gpd_set_pid_params(gpd_sim* sim, const gpd_pid_params* params) {
  if (!sim || !params) return fail(GPD_EINVAL, "gpd_set_pid_params: NULL argument");
  if (!act_is_pid(sim->cfg.act_type))
    return fail(GPD_EINVAL, "gpd_set_pid_params: the sim's action type has no controller");
  sim->pid = *params;
  HIP_TRY(hipDeviceSynchronize());
  return by_real(sim, [&](auto r) { return upload_tables<decltype(r)>(sim); });
}

int gpd_set_pid_gains(gpd_sim* sim, const double* gains) {
  if (!sim) return fail(GPD_EINVAL, "gpd_set_pid_gains: NULL sim");
  if (!act_is_pid(sim->cfg.act_type))
    return fail(GPD_EINVAL, "gpd_set_pid_gains: the sim's action type has no controller");
  if (!gains) {   // the sim-wide coefficients are back in force; the buffer and its address stay
    sim->gains_on = false;
    return GPD_OK;
  }
  const size_t N = (size_t)sim->N;
  for (size_t n = 0; n < N; ++n)
    for (int k = 0; k < kGainComps; ++k)
      if (!std::isfinite(gains[n * kGainComps + k]))
        return fail(GPD_EINVAL, "gpd_set_pid_gains: non-finite value in row " + std::to_string(n) + ", column " +
                                    std::to_string(k));
  return by_real(sim, [&](auto r) { return install_gains<decltype(r)>(sim, gains); });
}

int gpd_get_pid_gains(gpd_sim* sim, double* out) {
  if (!sim || !out) return fail(GPD_EINVAL, "gpd_get_pid_gains: NULL argument");
  if (!act_is_pid(sim->cfg.act_type))
    return fail(GPD_EINVAL, "gpd_get_pid_gains: the sim's action type has no controller");
  const size_t N = (size_t)sim->N;
  if (sim->gains_on) {
    std::memcpy(out, sim->gains.data(), N * kGainComps * sizeof(double));
    return GPD_OK;
  }
  // no table: the sim-wide triples as the kernels read them (rounded to the sim's real type)
  const gpd_pid_params& Q = sim->pid;
  const double* tri[6] = {Q.p_coeff_for, Q.i_coeff_for, Q.d_coeff_for, Q.p_coeff_tor, Q.i_coeff_tor, Q.d_coeff_tor};
  double row[kGainComps];
  for (int k = 0; k < kGainComps; ++k) {
    const double x = tri[k / 3][k % 3];
    row[k] = by_real(sim, [&](auto r) { return (double)(decltype(r))x; });
  }
  for (size_t n = 0; n < N; ++n) std::memcpy(out + n * kGainComps, row, sizeof(row));
  return GPD_OK;
}

int gpd_get_ctrl_state(gpd_sim* sim, void* out, void* stream) {
  if (!sim || !out) return fail(GPD_EINVAL, "gpd_get_ctrl_state: NULL argument");
  if (!sim->d_ctrl) return fail(GPD_EINVAL, "gpd_get_ctrl_state: the sim's action type has no controller");
  const unsigned g = grid_for(sim->N, 256);
  hipStream_t st = (hipStream_t)stream;
  by_real(sim, [&](auto r) {
    using R = decltype(r);
    hipLaunchKernelGGL((soa_to_rows_kernel<R>), dim3(g), dim3(256), 0, st, (const R*)sim->d_ctrl, sim->npad, kCtrlComps,
                       sim->N, (R*)out);
  });
  HIP_TRY(hipGetLastError());
  return GPD_OK;
}

int gpd_set_ctrl_state(gpd_sim* sim, const void* in, void* stream) {
  if (!sim || !in) return fail(GPD_EINVAL, "gpd_set_ctrl_state: NULL argument");
  if (!sim->d_ctrl) return fail(GPD_EINVAL, "gpd_set_ctrl_state: the sim's action type has no controller");
  const unsigned g = grid_for(sim->N, 256);
  hipStream_t st = (hipStream_t)stream;
  by_real(sim, [&](auto r) {
    using R = decltype(r);
    hipLaunchKernelGGL((rows_to_soa_kernel<R>), dim3(g), dim3(256), 0, st, (const R*)in, sim->npad, kCtrlComps, sim->N,
                       (R*)sim->d_ctrl);
  });
  HIP_TRY(hipGetLastError());
  return GPD_OK;
}

int gpd_get_step_counters(gpd_sim* sim, int32_t* out, void* stream) {
  if (!sim || !out) return fail(GPD_EINVAL, "gpd_get_step_counters: NULL argument");
  HIP_TRY(hipMemcpy2DAsync(out, sizeof(int32_t), sim->d_ctr, sizeof(int2), sizeof(int32_t), (size_t)sim->E,
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return GPD_OK;
}

int gpd_set_step_counters(gpd_sim* sim, const int32_t* in, void* stream) {
  if (!sim || !in) return fail(GPD_EINVAL, "gpd_set_step_counters: NULL argument");
  const int rc = settle_last_any(sim, (hipStream_t)stream);   // the ring-derived value reads them
  if (rc != GPD_OK) return rc;
  HIP_TRY(hipMemcpy2DAsync(sim->d_ctr, sizeof(int2), in, sizeof(int32_t), sizeof(int32_t), (size_t)sim->E,
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return GPD_OK;
}

namespace {
// checkpoint sections: state, controller state (PID types), action ring, counters
struct Section { void* dev; size_t bytes; };
// blob header: everything that fixes the section sizes and meaning
constexpr size_t kBlobHeader = 64;
void blob_header(const gpd_sim* sim, int64_t h[kBlobHeader / 8]) {
  const int64_t v[kBlobHeader / 8] = {(int64_t)GPD_ABI_VERSION, (int64_t)sim->N, (int64_t)sim->E, (int64_t)sim->D,
                                      (int64_t)sim->cfg.act_type, (int64_t)sim->prec, (int64_t)sim->ring_len,
                                      (int64_t)sim->npad};
  for (size_t i = 0; i < kBlobHeader / 8; ++i) h[i] = v[i];
}
int sections(gpd_sim* sim, Section out[4]) {
  out[0] = {sim->d_state, state_buf_bytes(sim)};
  out[1] = {sim->d_ctrl, sim->d_ctrl ? ctrl_buf_bytes(sim) : 0};
  out[2] = {sim->d_ring, ring_buf_bytes(sim)};
  out[3] = {sim->d_ctr, ctr_buf_bytes(sim)};
  return 4;
}
}  // namespace

size_t gpd_state_bytes(const gpd_sim* sim) {
  if (!sim) return 0;
  Section sec[4];
  const int ns = sections(const_cast<gpd_sim*>(sim), sec);
  size_t total = kBlobHeader;
  for (int i = 0; i < ns; ++i) total += sec[i].bytes;
  return total;
}

int gpd_save_state(gpd_sim* sim, void* blob_host, void* stream) {
  if (!sim || !blob_host) return fail(GPD_EINVAL, "gpd_save_state: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  char* b = (char*)blob_host;
  int64_t hdr[kBlobHeader / 8];
  blob_header(sim, hdr);
  std::memcpy(b, hdr, kBlobHeader);
  const int rc = settle_last_any(sim, st);
  if (rc != GPD_OK) return rc;
  size_t off = kBlobHeader;
  Section sec[4];
  const int ns = sections(sim, sec);
  for (int i = 0; i < ns; ++i) {
    if (sec[i].bytes) HIP_TRY(hipMemcpyAsync(b + off, sec[i].dev, sec[i].bytes, hipMemcpyDeviceToHost, st));
    off += sec[i].bytes;
  }
  HIP_TRY(hipStreamSynchronize(st));
  return GPD_OK;
}

int gpd_load_state(gpd_sim* sim, const void* blob_host, void* stream) {
  if (!sim || !blob_host) return fail(GPD_EINVAL, "gpd_load_state: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const char* b = (const char*)blob_host;
  int64_t hdr[kBlobHeader / 8], mine[kBlobHeader / 8];
  std::memcpy(hdr, b, kBlobHeader);
  blob_header(sim, mine);
  if (std::memcmp(hdr, mine, kBlobHeader) != 0)
    return fail(GPD_EINVAL, "gpd_load_state: blob does not match this sim");
  size_t off = kBlobHeader;
  Section sec[4];
  const int ns = sections(sim, sec);
  for (int i = 0; i < ns; ++i) {
    if (sec[i].bytes) HIP_TRY(hipMemcpyAsync(sec[i].dev, b + off, sec[i].bytes, hipMemcpyHostToDevice, st));
    off += sec[i].bytes;
  }
  if (sim->wt & 4) HIP_TRY(hipMemsetAsync(sim->d_ctr + sim->E, 0, sizeof(int2), st));   // saved settled
  HIP_TRY(hipStreamSynchronize(st));
  return GPD_OK;
}

// ---- config-5 learner hand-off (gpd_handoff.h; SURVEY §8(e), caller examples/learn.py:52-94)
namespace {
constexpr long long kPackAlign = 256;
inline long long align_up(long long n) { return (n + kPackAlign - 1) / kPackAlign * kPackAlign; }

int check_layout(const gpd_pack_layout* L, const char* fn) {
  if (!L) return fail(GPD_EINVAL, std::string(fn) + ": NULL layout");
  if (L->n_envs < 1 || L->drones_per_env < 1 || L->obs_width < kHandoffStateCols ||
      L->state_cols != kHandoffStateCols)
    return fail(GPD_EINVAL, std::string(fn) + ": layout not made by gpd_pack_layout_of");
  gpd_pack_layout ref;
  gpd_pack_layout_of(L->n_envs, L->drones_per_env, L->obs_width, &ref);
  if (std::memcmp(&ref, L, sizeof(ref)) != 0)
    return fail(GPD_EINVAL, std::string(fn) + ": layout offsets differ from gpd_pack_layout_of's");
  return GPD_OK;
}

HandoffView handoff_view(const gpd_pack_layout* L, long long stride, int n_ranks) {
  HandoffView v;
  v.obs = L->obs; v.reward = L->reward; v.term = L->terminated; v.trunc = L->truncated;
  v.tstate = L->terminal_state; v.tobs = L->terminal_obs; v.stride = stride;
  v.E = L->n_envs; v.D = L->drones_per_env; v.W = L->obs_width; v.G = n_ranks;
  return v;
}
}  // namespace

int gpd_pack_layout_of(int n_envs, int drones_per_env, int obs_width, gpd_pack_layout* out) {
  if (!out || n_envs < 1 || drones_per_env < 1 || obs_width < kHandoffStateCols)
    return fail(GPD_EINVAL, "gpd_pack_layout_of: invalid argument");
  const long long E = n_envs, D = drones_per_env, W = obs_width;
  gpd_pack_layout L;
  std::memset(&L, 0, sizeof(L));
  L.n_envs = n_envs; L.drones_per_env = drones_per_env; L.obs_width = obs_width;
  L.state_cols = kHandoffStateCols;
  long long off = 0;
  L.obs = off;            off += align_up(E * D * W * 4);
  L.reward = off;         off += align_up(E * 4);
  L.terminated = off;     off += align_up(E);
  L.truncated = off;
  L.prefix = off + E;
  L.prefix_aligned = align_up(L.prefix);
  off += align_up(E);
  L.terminal_state = off; off += align_up(E * D * kHandoffStateCols * 4);
  L.record = off;
  L.terminal_obs = off;   off += align_up(E * D * W * 4);
  L.total = off;
  *out = L;
  return GPD_OK;
}

int gpd_handoff_pack(uint8_t* pack, const gpd_pack_layout* layout, void* stream) {
  const int rc = check_layout(layout, "gpd_handoff_pack");
  if (rc != GPD_OK) return rc;
  if (!pack) return fail(GPD_EINVAL, "gpd_handoff_pack: NULL pack");
  const HandoffView v = handoff_view(layout, layout->record, 1);
  const long long n = (long long)v.E * v.D * kHandoffStateCols;
  if (n >= (1ll << 31)) return fail(GPD_EINVAL, "gpd_handoff_pack: shard too large");
  hipLaunchKernelGGL(handoff_pack_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, pack, v);
  HIP_TRY(hipGetLastError());
  return GPD_OK;
}

int gpd_handoff_unpack(const uint8_t* gathered, int n_ranks, long long stride, const gpd_pack_layout* layout,
                       float* obs, float* reward, uint8_t* terminated, uint8_t* truncated, float* terminal_obs,
                       void* stream) {
  const int rc = check_layout(layout, "gpd_handoff_unpack");
  if (rc != GPD_OK) return rc;
  if (!gathered || !obs || !reward || !terminated || !truncated || n_ranks < 1)
    return fail(GPD_EINVAL, "gpd_handoff_unpack: NULL output or n_ranks < 1");
  if (stride != layout->prefix_aligned && stride != layout->record)
    return fail(GPD_EINVAL, "gpd_handoff_unpack: stride must be the layout's prefix_aligned or record");
  if (terminal_obs && stride != layout->record)
    return fail(GPD_EINVAL, "gpd_handoff_unpack: terminal rows need whole records (stride = record)");
  const HandoffView v = handoff_view(layout, stride, n_ranks);
  const long long rows = (long long)v.E * v.D;
  if (rows * v.W * n_ranks >= (1ll << 31))
    return fail(GPD_EINVAL, "gpd_handoff_unpack: gathered batch too large");
  hipStream_t st = (hipStream_t)stream;
  const bool vec4 = v.W % 4 == 0 && aligned16(obs) && (!terminal_obs || aligned16(terminal_obs)) && aligned16(gathered);
  const long long nvec = rows * v.W / (vec4 ? 4 : 1) * n_ranks;
  const long long nthr = std::max(nvec, (long long)v.E * n_ranks);
  const dim3 grid(grid_for(nthr, 256)), block(256);
  const auto k = vec4 ? (terminal_obs ? handoff_unpack_kernel<4, true> : handoff_unpack_kernel<4, false>)
                      : (terminal_obs ? handoff_unpack_kernel<1, true> : handoff_unpack_kernel<1, false>);
  hipLaunchKernelGGL(k, grid, block, 0, st, gathered, v, obs, reward, terminated, truncated, terminal_obs);
  HIP_TRY(hipGetLastError());
  return GPD_OK;
}

#ifdef GPD_STAMPS
// diagnostic build only: copy the phase stamps of the last step launches to the host
int gpd_debug_stamps(unsigned long long* out_host, int n_blocks) {
  if (n_blocks > 65536) n_blocks = 65536;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_stamps), (size_t)n_blocks * kStampPhases * 8, 0,
                              hipMemcpyDeviceToHost));
  return GPD_OK;
}
#endif

#ifdef GPD_CONTACT_STATS
// diagnostic build only: read and clear the contact-solve histogram (kPcHist counters)
int gpd_debug_contact_hist(unsigned long long* out_host) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_pc_hist), kPcHist * 8, 0, hipMemcpyDeviceToHost));
  static unsigned long long zero[kPcHist] = {};
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_pc_hist), zero, kPcHist * 8, 0, hipMemcpyHostToDevice));
  return GPD_OK;
}
#endif

}  // extern "C"
