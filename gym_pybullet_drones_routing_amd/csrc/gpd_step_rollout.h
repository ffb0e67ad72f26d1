// gpd_step_rollout.h — the closed-loop rollout (gpd_cmd_rollout): n_steps consecutive command
// steps (gpd_step_cmd.h) of every env in one launch.  Envs do not interact, so a block keeps its
// drones, their controller state and last_clipped_action in registers for the whole flight: the
// state goes through HBM once per launch instead of once per step, and the state20 rows are
// stored only on the steps the caller records.  The commands of the flight are a
// [n_steps][N][w] tensor; the next step's row is loaded while the current step's substeps run.
// The per-step arithmetic is cmd_step_kernel's: the same clip / cmd_ctrl_rpm (here on a row
// already in registers, cmd_row_to_rpm).  The substep loop and the staging of the state20 rows are
// written out here although substeps_cmd (gpd_step_parts.h) and rows20_stage_out (gpd_step_cmd.h)
// define them for cmd_step_kernel: as calls they change this kernel's schedule, and the
// single-drone RPM rollout measured 1.4 % slower (profiles/step_parts/).  A fix to either goes to
// the helper AND here.
// Needs cmd_step_kernel's helpers (gpd_step_cmd.h).
#pragma once
#include "gpd_step_cmd.h"

namespace gpd {

// One step's tracking figures: |pos - target|^2 added to the sum, its root folded into the max.
// Every product and sum rounded (np.linalg.norm's operations, as adjacency_kernel).
template <typename R>
__device__ __forceinline__ void track_accumulate(R px, R py, R pz, R tx, R ty, R tz, R& sum2, R& dmax) {
#pragma clang fp contract(off)
  const R dx = px - tx, dy = py - ty, dz = pz - tz;
  const R d2 = (dx * dx + dy * dy) + dz * dz;
  sum2 = sum2 + d2;
  const R dist = g_sqrt(d2);
  dmax = dist > dmax ? dist : dmax;
}

// ---------------------------------------------------------------------------------------
// gpd_cmd_rollout for envs of up to 64 drones: cmd_step_kernel's block (one wave, whole envs,
// v.tpb drones) running n_steps steps.  PF and CTRL as cmd_step_kernel's.
//   actions    the launch's first command row ([n_steps][N][w])
//   rec_every  record every rec_every-th step of the flight into traj (null: none); rec_phase
//              steps of the flight since the last recorded one and rec_row recorded rows precede
//              this launch (a flight longer than one launch continues its count)
//   obs20      the rows after the launch's last step (null on all but a flight's last launch)
//   metrics    [N][2] tracking sum / max over the WAYPOINT targets (null: none); carry != 0
//              continues the values there, else the flight starts at zero
//   gains      PG: the per-drone gain table (gpd_step_cmd.h); a lane loads its drone's row once per
//              launch, in the batch of its state loads, and stages its controller constants in its
//              LDS slot (pid_stage_lane), where the controller reads them on every step of the launch
//              (PG as cmd_step_kernel's; else null and never read)
template <typename R, bool MULTI, int PF, bool CTRL, bool PG = false>
__global__ __launch_bounds__(kWave) void cmd_rollout_kernel(SimView<R> v, const Consts<R>* __restrict__ cp,
                                                            const void* __restrict__ actions, int mode, R max_rpm,
                                                            int n_steps, int rec_every, int rec_phase,
                                                            long long rec_row, R* __restrict__ traj,
                                                            R* __restrict__ obs20, R* __restrict__ metrics, int carry,
                                                            const R* __restrict__ gains) {
  static_assert(CTRL || !PG, "the gain table is read by the controller modes only");
  constexpr int CW = cmd_row_regs<CTRL>();
  __shared__ R sx[MULTI ? 2 * kWave : 1], sy[MULTI ? 2 * kWave : 1], sz[MULTI ? 2 * kWave : 1];
  __shared__ R rows[20 * kPad];   // the block's state20 rows, column-major (rows20_copy_out)
  const Consts<R>& c = *cp;
  const int tid = threadIdx.x;
  const int D = MULTI ? v.D : 1;
  const int d = MULTI ? tid % D : 0;
  const int base = tid - d;
  const long long N = v.N;
  const long long n0 = (long long)blockIdx.x * v.tpb;
  const long long n = n0 + tid;
  const long long nleft = N - n0;
  const int nact = (int)(nleft < v.tpb ? nleft : v.tpb);   // drones owned by this block
  const bool active = tid < nact;
  const long long nn = active ? n : n0;   // inactive lanes: the block's first drone (step_kernel)
  // PG: the lane's controller constants for the whole launch, staged ahead of every load the
  // no-table kernel has (cmd_step_kernel).  The controller state, the command row and the carried
  // metrics load behind the staging's waits here: once per launch, not once per step.
  const PidConsts<R>* pk = nullptr;
  if constexpr (PG) {
    __shared__ LanePid<R> lane_pid[kWave];
    R g[kGainComps];
    pid_gains_load(gains, nn, g);
    pk = &pid_stage_lane(lane_pid, tid, c.pid, g);
  }
  const bool drag = pf_on<PF>(c.flags, F_DRAG);
  const DcPairs dcp = dc_enabled<MULTI, PF>(c.flags) ? dc_pairs_for(v, tid, nact) : dc_pairs_none();
  Drone<R> s;
  R last[4];
  load_drone(v, nn, s, last, drag);
  R nxt[CW];
  cmd_row_load<R, CTRL>(actions, mode, nn, nxt);
  DynK<R> dk = dyn_consts(c);
  R cs[9];
  if (CTRL) {
#pragma unroll
    for (int k = 0; k < 9; ++k) cs[k] = v.ctrl[tidx(nn, k, 9)];
  }
  R msum = R(0), mmax = R(0);
  if (CTRL && metrics && carry) {
    msum = metrics[nn * 2];
    mmax = metrics[nn * 2 + 1];
  }
  for (int t = 0; t < n_steps; ++t) {
    R cur[CW];
#pragma unroll
    for (int k = 0; k < CW; ++k) cur[k] = nxt[k];
    // the next step's row is in flight while this step's substeps run
    if (t + 1 < n_steps) cmd_row_load<R, CTRL>(actions, mode, (long long)(t + 1) * N + nn, nxt);
    R rpm[4];
    if constexpr (PG) cmd_row_to_rpm<R, CTRL>(*pk, mode, cur, max_rpm, s, cs, rpm);
    else cmd_row_to_rpm<R, CTRL>(c.pid, mode, cur, max_rpm, s, cs, rpm);
    // the same RPMs and wrench drive every substep; the drag of substep 1 sees the previous step's
    // RPMs (BaseAviary.py:359-372), here handed over in `last`
    R W[4];
    rpm_wrench<R, PF>(rpm, dk, c, W);
    if (PF == 0) {   // the write-only world ang_v from the last substep only
      for (int it = 0; it < dk.nsub - 1; ++it)
        substep_block<R, MULTI, PF, false>(s, rpm, W, last, c, dk, sx, sy, sz, tid, base, D, DwPairs{0, 0}, nullptr, dcp);
      substep_block<R, MULTI, PF, true>(s, rpm, W, last, c, dk, sx, sy, sz, tid, base, D, DwPairs{0, 0}, nullptr, dcp);
#pragma unroll
      for (int k = 0; k < 4; ++k) last[k] = rpm[k];
    } else {         // one copy of the substep (cmd_step_kernel)
      for (int it = 0; it < dk.nsub; ++it) {
        substep_block<R, MULTI, PF, true>(s, rpm, W, last, c, dk, sx, sy, sz, tid, base, D, DwPairs{0, 0}, nullptr, dcp);
#pragma unroll
        for (int k = 0; k < 4; ++k) last[k] = rpm[k];   // self.last_clipped_action = clipped_action  :372
      }
    }
    if (CTRL && metrics) track_accumulate(s.px, s.py, s.pz, cur[0], cur[1], cur[2], msum, mmax);
    if (traj && ++rec_phase == rec_every) {   // wave-uniform
      rec_phase = 0;
      R o[20];
      state20_row(s, last, o);
#pragma unroll
      for (int k = 0; k < 20; ++k) rows[k * kPad + tid] = o[k];
      wave_lds_sync();
      rows20_copy_out(rows, tid, nact, traj + (rec_row * N + n0) * 20);
      ++rec_row;
      wave_lds_sync();   // the tile is rewritten by the next recorded step (and by obs20's rows)
    }
  }
  if (obs20) {
    R o[20];
    state20_row(s, last, o);
#pragma unroll
    for (int k = 0; k < 20; ++k) rows[k * kPad + tid] = o[k];
    wave_lds_sync();
    rows20_copy_out(rows, tid, nact, obs20 + n0 * 20);
  }
  if (!active) return;
  store_drone(v, n, s, last);
  unmark_last_in_ring(v, n);
  if (CTRL) {
#pragma unroll
    for (int k = 0; k < 9; ++k) v.ctrl[tidx(n, k, 9)] = cs[k];
    if (metrics) {
      metrics[n * 2] = msum;
      metrics[n * 2 + 1] = mmax;
    }
  }
  if (d == 0) {   // step_counter += n_steps * PYB_STEPS_PER_CTRL; the ring head stays
    int* sc = &v.ctr[MULTI ? n / D : n].x;
    *sc = *sc + dk.nsub * n_steps;
  }
}

// The tracking figures of one step on envs of more than 64 drones, where gpd_cmd_rollout issues
// cmd_step_kernel_wide once per step: one thread per drone, the positions the step just stored
// against the step's waypoint row (track_accumulate: the one-wave kernel's operations).
template <typename R>
__global__ __launch_bounds__(256) void cmd_track_kernel(SimView<R> v, const R* __restrict__ wp, R* __restrict__ metrics,
                                                        int carry) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= v.N) return;
  R msum = R(0), mmax = R(0);
  if (carry) {
    msum = metrics[n * 2];
    mmax = metrics[n * 2 + 1];
  }
  const R* st = v.state + tidx(n, 0, kStateComps);
  const R* w = wp + n * 7;
  track_accumulate(st[0 * 64], st[1 * 64], st[2 * 64], w[0], w[1], w[2], msum, mmax);
  metrics[n * 2] = msum;
  metrics[n * 2 + 1] = mmax;
}

}  // namespace gpd
