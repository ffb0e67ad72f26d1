// gpd_step_cmd.h — the command step (gpd_cmd_step): one env.step() of the reference's CtrlAviary /
// VelocityAviary for every env in one launch, and the adjacency helper (gpd_adjacency).
//   CMD_RPM       CtrlAviary._preprocessAction (envs/CtrlAviary.py:140): np.clip(a, 0, MAX_RPM)
//   CMD_VEL       VelocityAviary._preprocessAction (envs/VelocityAviary.py:148-168), the VEL branch
//                 of BaseRLAviary (:208-223) line for line
//   CMD_WAYPOINT  DSLPIDControl.computeControl(target_pos, target_rpy=(0, 0, yaw), target_vel) on the
//                 state of the last readback: the control loop of examples/pid.py on the device
// then PYB_STEPS_PER_CTRL substeps on those RPMs (BaseAviary.py:343-372), the final readback and
// the 20-float state vectors (_getDroneStateVector :541-561) as the observation.  No reward, no
// done flag, no auto-reset, and the action ring of the RL step is left alone.
// Needs substeps_cmd, state20_row and load_rpm4 (gpd_step_parts.h) and wide_downwash (gpd_step_wide.h).
#pragma once
#include "gpd_step_wide.h"

namespace gpd {

enum : int { CMD_RPM = 0, CMD_VEL = 1, CMD_WAYPOINT = 2 };

// The command of one drone -> its four RPMs, in two halves so that the rollout (gpd_step_rollout.h)
// can load a step's row while the step before it integrates.  CTRL: the controller modes (VEL /
// WAYPOINT), else RPM; `mode` is wave-uniform.
// actions: RPM real [..][N][4] (the sim's precision: float64 controller outputs lose nothing),
// VEL float [..][N][4], WAYPOINT real [..][N][7] = target_pos(3) target_yaw target_vel(3).
// Register width of a command row: RPM 4 reals, VEL 4 floats (held as reals: exact), WAYPOINT 7 reals.
template <bool CTRL>
constexpr int cmd_row_regs() { return CTRL ? 7 : 4; }

// Command row `row` (= step * N + drone) into registers.  RPM and VEL rows are one aligned vector
// (host-checked base pointer); a waypoint row is 7 reals, not 16-byte aligned for odd drones:
// scalar loads.
template <typename R, bool CTRL>
__device__ __forceinline__ void cmd_row_load(const void* __restrict__ actions, int mode, long long row,
                                             R a[cmd_row_regs<CTRL>()]) {
  if (!CTRL) {
    load_rpm4((const R*)actions + row * 4, a);
  } else if (mode == CMD_VEL) {
    float q[4];
    load_rpm4((const float*)actions + row * 4, q);
    a[0] = (R)q[0]; a[1] = (R)q[1]; a[2] = (R)q[2]; a[3] = (R)q[3];
    a[4] = a[5] = a[6] = R(0);
  } else {
    const R* w = (const R*)actions + row * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) a[k] = w[k];
  }
}

// The controller modes: DSLPIDControl.computeControl on the state of the last readback; cs is the
// drone's controller state, updated in place.  targets(pos, rpy, tpos, tyaw, tvel) fills in the
// command's targets: from the row in registers (cmd_row_to_rpm) or straight from memory
// (cmd_to_rpm; a single step has no row to prefetch, and holding the 7 reals across the mode
// branch spills in the f64 kernels).
// k: the constants the controller runs on: Consts::pid, or the lane's own copy of it with its
// drone's gain row (pid_with_gains).
template <typename R, typename F>
__device__ __forceinline__ void cmd_ctrl_rpm(const PidConsts<R>& k, const Drone<R>& s, R cs[9], R rpm[4], F&& targets) {
  R qn[4], Rm[9], rpy[3];
  readback_fused(s.qx, s.qy, s.qz, s.qw, qn, Rm);
  quat_to_euler(qn, rpy[0], rpy[1], rpy[2]);
  const R pos[3] = {s.px, s.py, s.pz}, vel[3] = {s.vx, s.vy, s.vz};
  R tpos[3], tvel[3], tyaw;
  targets(pos, rpy, tpos, tyaw, tvel);
  dsl_pid<R, false>(k, pos, Rm, rpy, vel, tpos, tyaw, tvel, cs, rpm);
}

// The row in registers -> RPMs.
template <typename R, bool CTRL>
__device__ __forceinline__ void cmd_row_to_rpm(const PidConsts<R>& k, int mode, const R a[cmd_row_regs<CTRL>()], R max_rpm,
                                               const Drone<R>& s, R cs[9], R rpm[4]) {
  if (!CTRL) {
#pragma unroll
    for (int k = 0; k < 4; ++k) rpm[k] = np_clip(a[k], R(0), max_rpm);
  } else {
    cmd_ctrl_rpm(k, s, cs, rpm, [&](const R pos[3], const R rpy[3], R tpos[3], R& tyaw, R tvel[3]) {
      if (mode == CMD_VEL) {
        const float af[4] = {(float)a[0], (float)a[1], (float)a[2], (float)a[3]};
        pid_targets<R, ACT_VEL>(k, af, pos, rpy, tpos, tyaw, tvel);
      } else {
        tpos[0] = a[0]; tpos[1] = a[1]; tpos[2] = a[2];
        tyaw = a[3];
        tvel[0] = a[4]; tvel[1] = a[5]; tvel[2] = a[6];
      }
    });
  }
}

// Drone n's command of a single step -> RPMs.
template <typename R, bool CTRL>
__device__ __forceinline__ void cmd_to_rpm(const PidConsts<R>& k, int mode, const void* __restrict__ actions, long long n,
                                           R max_rpm, const Drone<R>& s, R cs[9], R rpm[4]) {
  if (!CTRL) {
    R a[4];
    cmd_row_load<R, false>(actions, mode, n, a);
    cmd_row_to_rpm<R, false>(k, mode, a, max_rpm, s, cs, rpm);
  } else {
    cmd_ctrl_rpm(k, s, cs, rpm, [&](const R pos[3], const R rpy[3], R tpos[3], R& tyaw, R tvel[3]) {
      if (mode == CMD_VEL) {
        float a[4];
        load_rpm4((const float*)actions + n * 4, a);
        pid_targets<R, ACT_VEL>(k, a, pos, rpy, tpos, tyaw, tvel);
      } else {
        const R* w = (const R*)actions + n * 7;
        tpos[0] = w[0]; tpos[1] = w[1]; tpos[2] = w[2];
        tyaw = w[3];
        tvel[0] = w[4]; tvel[1] = w[5]; tvel[2] = w[6];
      }
    });
  }
}

// Copy-out of a one-wave block's state20 rows: the rows are [nact][20] reals, contiguous in HBM
// and a multiple of 16 bytes long, staged column-major in LDS (tile[col][lane], kPad apart: the
// lanes' writes and the transposed reads are bank-conflict free) and streamed out with
// coalesced 16-byte stores (2 doubles / 4 floats, never across a row: 20 is a multiple of both).
// Measured against every lane storing its own row (20 scalar stores at a 160-byte stride), on the
// build that still launched settle_last in front of this kernel (not the shipped 10.9 / 14.5 us
// one): the same at 4096 envs, 18.2 vs 19.6 us per step at 65536
// (profiles/cmd_step/probe_settle_launch_rowlane_ab.txt).
template <typename R>
__device__ __forceinline__ void rows20_copy_out(const R* tile, int lane, int nact, R* __restrict__ dst) {
  constexpr int G = 16 / (int)sizeof(R);
  typedef R gpd_vec __attribute__((ext_vector_type(G)));
  const int total = nact * (20 / G);
#pragma unroll 2
  for (int i = lane; i < total; i += kWave) {
    const int el = i * G, row = el / 20, col = el - row * 20;
    gpd_vec q;
#pragma unroll
    for (int g = 0; g < G; ++g) q[g] = tile[(col + g) * kPad + row];
    reinterpret_cast<gpd_vec*>(dst)[i] = q;
  }
}

// The block's state20 rows (state20_row of every lane) through the LDS tile `rows` to dst.
template <typename R>
__device__ __forceinline__ void rows20_stage_out(R* rows, int tid, int nact, const Drone<R>& s, const R last[4],
                                                 R* __restrict__ dst) {
  R o[20];
  state20_row(s, last, o);
#pragma unroll
  for (int k = 0; k < 20; ++k) rows[k * kPad + tid] = o[k];
  wave_lds_sync();
  rows20_copy_out(rows, tid, nact, dst);
}

// The command step stores last_clipped_action into the state itself, so it takes back the mark an
// RL step may have left (mark_last_in_ring: "state[16..19] is stale, the value is in the ring").
// Such sims have no drag (SimView::wt bit 2), so nothing in this step reads the stale columns, and
// no block reads the mark: drone 0's lane clears it, as drone 0's lane of the RL step sets it.
template <typename R>
__device__ __forceinline__ void unmark_last_in_ring(const SimView<R>& v, long long n) {
  if ((v.wt & 4) && n == 0) v.ctr[v.N / v.D] = make_int2(0, 0);
}

// ---------------------------------------------------------------------------------------
// Per-drone controller gains (gpd_set_pid_gains).  The table is tiled like v.ctrl,
// [npad/64][18][64] reals: column k of drone n at tidx(n, k, 18), so a wave's load of one column
// is one contiguous 64-real line.  A row is gpd_pid_params' six triples in its order:
// P/I/D_COEFF_FOR, P/I/D_COEFF_TOR.
constexpr int kGainComps = 18;

// Drone n's row into registers: issued beside the loads of its state and controller state.
template <typename R>
__device__ __forceinline__ void pid_gains_load(const R* __restrict__ gains, long long n, R g[kGainComps]) {
#pragma unroll
  for (int k = 0; k < kGainComps; ++k) g[k] = gains[tidx(n, k, kGainComps)];
}

// The lane's own controller constants: the sim-wide block with the six triples replaced by the
// drone's row.  Everything else (PWM constants, mixer, gravity, kf, ctrl_dt, speed_limit) stays
// wave-uniform.
template <typename R>
__device__ __forceinline__ PidConsts<R> pid_with_gains(const PidConsts<R>& base, const R g[kGainComps]) {
  PidConsts<R> k = base;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    k.p_for[i] = g[i];     k.i_for[i] = g[3 + i];  k.d_for[i] = g[6 + i];
    k.p_tor[i] = g[9 + i]; k.i_tor[i] = g[12 + i]; k.d_tor[i] = g[15 + i];
  }
  return k;
}

// The one-wave kernels keep the lane's constants in an LDS slot of its own and hand the controller
// a reference to it: dsl_pid then reads its constants through a pointer to a PidConsts, the form in
// which the no-table instantiation reads Consts::pid, and 18 reals per lane stay out of the
// registers across the rollout's step loop.  The slot is read back under the lane id from mbcnt,
// which equals tid in these one-wave blocks but which the compiler does not know to: it does not
// forward the stored values into the controller, and (unlike an asm statement) the index is no
// scheduling boundary, so the loads that follow issue ahead of the staging's waits.  8 bytes of
// padding: the slots' stride is 78 (f64) / 42 (f32) dwords, two lanes per bank at worst.
// The whole PidConsts is staged, its wave-uniform part (19 reals + the speed limit) 64 times: 15 KB
// of the 19.5 KB (f64) are copies, loaded by every lane from one address.  A shared copy of that
// part would need the controller to read two structs, a form the no-table kernel does not have.
// COMPILER DEPENDENCE: that a table of the sim-wide gains is bit-identical to no table
// (tests/test_gpu_pid_gains.py) rests on this form and on where the kernels call it, i.e. on how
// the hipcc it was developed with orders operands before it contracts a*b + c*d in the Bullet code,
// which is compiled with contraction left to it.  Another compiler may break that test without any
// change here; the robust remedy is explicit contraction in that shared code.
template <typename R>
struct LanePid {
  PidConsts<R> k;
  R pad[8 / sizeof(R)];
};
template <typename R>
__device__ __forceinline__ const PidConsts<R>& pid_stage_lane(LanePid<R>* tile, int tid, const PidConsts<R>& base,
                                                              const R g[kGainComps]) {
  tile[tid].k = pid_with_gains(base, g);
  const int slot = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));   // == tid (one-wave blocks)
  return tile[slot].k;
}

// ---------------------------------------------------------------------------------------
// gpd_cmd_step for envs of up to 64 drones: one wave per block, the geometry of integrate_kernel
// (whole envs per block, v.tpb drones), one control step as step_kernel runs it.
// PF: 0 (plain DYN) or kPfRuntime; CTRL: the instantiation runs the controller (VEL / WAYPOINT).
// PG: a per-drone gain table is in force and the controller runs on the drone's own row of `gains`;
// else on Consts::pid, and `gains` (the last kernel argument, null) is never read.
template <typename R, bool MULTI, int PF, bool CTRL, bool PG = false>
__global__ __launch_bounds__(kWave) void cmd_step_kernel(SimView<R> v, const Consts<R>* __restrict__ cp,
                                                         const void* __restrict__ actions, int mode, R max_rpm,
                                                         R* __restrict__ obs20, const R* __restrict__ gains) {
  static_assert(CTRL || !PG, "the gain table is read by the controller modes only");
  __shared__ R sx[MULTI ? 2 * kWave : 1], sy[MULTI ? 2 * kWave : 1], sz[MULTI ? 2 * kWave : 1];
  __shared__ R rows[20 * kPad];   // the block's state20 rows, column-major (rows20_copy_out)
  const Consts<R>& c = *cp;
  const int tid = threadIdx.x;
  const int D = MULTI ? v.D : 1;
  const int d = MULTI ? tid % D : 0;
  const int base = tid - d;
  const long long n0 = (long long)blockIdx.x * v.tpb;
  const long long n = n0 + tid;
  const long long nleft = v.N - n0;
  const int nact = (int)(nleft < v.tpb ? nleft : v.tpb);   // drones owned by this block
  const bool active = tid < nact;
  const long long nn = active ? n : n0;   // inactive lanes: the block's first drone (step_kernel)
  // PG: the row's loads, the controller state's and the staging stand ahead of every load the no-table
  // kernel has: what follows is then that kernel's code in that kernel's order, and the compiler's
  // choices in it (which product of a sum it contracts) stay the same.  As compiled:
  // on single-drone envs the state's 13 loads, next in the block, issue in the same batch, ahead of
  // the staging's waits (one round trip; the four last_clipped_action loads of a sim with drag sit
  // behind a branch and issue after them).  On multi-drone envs the pair-table code (branches
  // and dependent loads of its own, in the no-table kernel too) stands between the staging and the
  // state's loads: there the staging's round trip comes on top of those the no-table kernel has.
  const PidConsts<R>* pk = nullptr;
  R cs_pg[PG ? 9 : 1];
  if constexpr (PG) {
    __shared__ LanePid<R> lane_pid[kWave];
    R g[kGainComps];
    pid_gains_load(gains, nn, g);
#pragma unroll
    for (int k = 0; k < 9; ++k) cs_pg[k] = v.ctrl[tidx(nn, k, 9)];
    pk = &pid_stage_lane(lane_pid, tid, c.pid, g);
  }
  const bool drag = pf_on<PF>(c.flags, F_DRAG);
  const DcPairs dcp = dc_enabled<MULTI, PF>(c.flags) ? dc_pairs_for(v, tid, nact) : dc_pairs_none();
  Drone<R> s;
  R last[4];
  load_drone(v, nn, s, last, drag);
  DynK<R> dk = dyn_consts(c);
  R rpm[4];
  R cs[9];
  if constexpr (PG) {
#pragma unroll
    for (int k = 0; k < 9; ++k) cs[k] = cs_pg[k];
  } else if (CTRL) {
#pragma unroll
    for (int k = 0; k < 9; ++k) cs[k] = v.ctrl[tidx(nn, k, 9)];
  }
  if constexpr (PG) {
    cmd_to_rpm<R, CTRL>(*pk, mode, actions, nn, max_rpm, s, cs, rpm);
  } else {
    cmd_to_rpm<R, CTRL>(c.pid, mode, actions, nn, max_rpm, s, cs, rpm);
  }
  // the same RPMs and wrench drive every substep
  R W[4];
  rpm_wrench<R, PF>(rpm, dk, c, W);
  substeps_cmd<R, MULTI, PF>(s, rpm, W, last, c, dk, sx, sy, sz, tid, base, D, dcp);
  if (obs20) rows20_stage_out(rows, tid, nact, s, last, obs20 + n0 * 20);
  if (!active) return;
  store_drone(v, n, s, last);
  unmark_last_in_ring(v, n);
  if (CTRL) {
#pragma unroll
    for (int k = 0; k < 9; ++k) v.ctrl[tidx(n, k, 9)] = cs[k];
  }
  if (d == 0) {   // step_counter += PYB_STEPS_PER_CTRL (:382); the ring head stays
    int* sc = &v.ctr[MULTI ? n / D : n].x;
    *sc = *sc + dk.nsub;
  }
}

// gpd_cmd_step for envs of 65 .. 1024 drones: one env per workgroup of ceil(D / 64) waves
// (integrate_kernel_wide), rows stored per lane.  PG and gains as cmd_step_kernel's.
template <typename R, int MAXT, bool CTRL, bool PG = false>
__global__ __launch_bounds__(MAXT) void cmd_step_kernel_wide(SimView<R> v, const Consts<R>* __restrict__ cp,
                                                             const void* __restrict__ actions, int mode, R max_rpm,
                                                             R* __restrict__ obs20, const R* __restrict__ gains) {
  static_assert(CTRL || !PG, "the gain table is read by the controller modes only");
  __shared__ R sx[MAXT], sy[MAXT], sz[MAXT];
  const Consts<R>& c = *cp;
  const int D = v.D;
  const int d = threadIdx.x;
  const bool active = d < D;
  const long long n = (long long)blockIdx.x * D + (active ? d : (d & ~(kWave - 1)));   // (step_kernel_wide)
  Drone<R> s;
  R last[4];
  load_drone(v, n, s, last, true);
  DynK<R> dk = dyn_consts(c);
  const int nw = (D + kWave - 1) / kWave;
  R rpm[4];
  R cs[9];
  if (CTRL) {
#pragma unroll
    for (int k = 0; k < 9; ++k) cs[k] = v.ctrl[tidx(n, k, 9)];
  }
  if constexpr (PG) {
    R g[kGainComps];
    pid_gains_load(gains, n, g);
    const PidConsts<R> pk = pid_with_gains(c.pid, g);
    cmd_to_rpm<R, CTRL>(pk, mode, actions, n, max_rpm, s, cs, rpm);
  } else {
    cmd_to_rpm<R, CTRL>(c.pid, mode, actions, n, max_rpm, s, cs, rpm);
  }
  R W[4];
  rpm_wrench<R, kPfRuntime>(rpm, dk, c, W);
  for (int it = 0; it < dk.nsub; ++it) {
    const R dw = wide_downwash(s, sx, sy, sz, d, active, 0, D, c, dk.flags);
    if (nw > 1) dyn_substep<R, kPfRuntime, true, 16>(s, rpm, W, last, dw, c, dk);
    else dyn_substep<R, kPfRuntime, true, 1>(s, rpm, W, last, dw, c, dk);
#pragma unroll
    for (int k = 0; k < 4; ++k) last[k] = rpm[k];
  }
  if (!active) return;
  if (obs20) state20_store(s, last, obs20 + n * 20);
  store_drone(v, n, s, last);
  unmark_last_in_ring(v, n);
  if (CTRL) {
#pragma unroll
    for (int k = 0; k < 9; ++k) v.ctrl[tidx(n, k, 9)] = cs[k];
  }
  if (d == 0) {
    int* sc = &v.ctr[blockIdx.x].x;
    *sc = *sc + dk.nsub;
  }
}

// ---------------------------------------------------------------------------------------
// gpd_adjacency: BaseAviary._getAdjacencyMatrix (:658-675) of every env from the stored
// positions, one thread per (env, i, j): 1 on the diagonal, else |pos_i - pos_j| < radius with
// np.linalg.norm's rounding of each product and sum (no FP contraction).  radius = inf: all ones.
template <typename R>
__global__ __launch_bounds__(256) void adjacency_kernel(SimView<R> v, double radius, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long D = v.D, total = (long long)v.N * D;
  if (idx >= total) return;
  const long long ni = idx / D;              // drone i (global)
  const int j = (int)(idx - ni * D);
  const long long nj = ni / D * D + j;       // drone j of the same env
  uint8_t adj = 1;
  if (ni != nj) {
    const R dx = v.state[tidx(ni, 0, kStateComps)] - v.state[tidx(nj, 0, kStateComps)];
    const R dy = v.state[tidx(ni, 1, kStateComps)] - v.state[tidx(nj, 1, kStateComps)];
    const R dz = v.state[tidx(ni, 2, kStateComps)] - v.state[tidx(nj, 2, kStateComps)];
    const R dist = g_sqrt((dx * dx + dy * dy) + dz * dz);
    adj = (double)dist < radius ? 1 : 0;
  }
  out[idx] = adj;
}

}  // namespace gpd
