// gpd_step.h — the one-wave step: the observation tile's size and copy-out, and step_kernel
// (gpd_step: one env.step() per launch).  Needs the loads / stores and stamps of gpd_layout.h and
// the phases of gpd_step_parts.h; the duo, wide and het kernels reuse what is defined here.
#pragma once
#include "gpd_step_parts.h"

namespace gpd {

// Bytes of dynamic LDS the step kernel needs for its observation tile: the row's columns
// (state, history, current action).  A == 4 keeps float4 columns (state 3, history+action L);
// A == 1 / 3 keep float columns (state 12, history+action L*A).
__host__ __device__ inline int step_tile_bytes(int A, int ring_len) {
  return A == 4 ? (3 + ring_len) * kPad * 16 : (12 + ring_len * A) * kPad * 4;
}

// Copy-out of the observation tile: the block's nact rows of NC columns (float4 columns for
// A == 4, float otherwise), streamed by NL lanes with coalesced (write-through with wt & 1)
// stores; rows flagged in done_rows also go to terminal_obs (their non-state columns - the
// state part was stored from registers).  t / NC is (t * nc_magic) >> 16 for t <= NL.  U tile
// elements per lane per batch (LDS reads in flight); lanes past the end are masked off.
template <int A, int NL, int U = 6, int AUX = kAuxWt>
__device__ __forceinline__ void tile_copy_out(const float4* tile4, const float* tilef, int lane, int nact, int NC,
                                              int nc_magic, int wt, unsigned long long done_rows, float* obs,
                                              float* terminal_obs, long long n0) {
  // lane `lane` streams tile elements g = lane, lane+NL, ... (row-major over the block's rows).
  // A lane whose element index passes the end reads the last element and stores nothing (an
  // exec-masked store; re-storing the last element instead would send up to NL*U writes of one
  // 16-byte word through one L2 channel).  Rows of envs that finished this step are also
  // written to terminal_obs (state columns from the extra tile columns).
  const int total = nact * NC;
  const int drow = (NL * nc_magic) >> 16, dcol = NL - drow * NC;
  int row = (lane * nc_magic) >> 16;
  int col = lane - row * NC;
  const int last_row = nact - 1, last_col = NC - 1;
  const int ncs = A == 4 ? 3 : 12;  // state columns
  using E = std::conditional_t<A == 4, float4, float>;   // a tile element
  constexpr int EB = sizeof(E);
  const E* tile = A == 4 ? reinterpret_cast<const E*>(tile4) : reinterpret_cast<const E*>(tilef);
  for (int g0 = lane; g0 - lane < total; g0 += U * NL) {
    E val[U];
    int idx[U];
    int rr[U], cc[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      ok[u] = g0 + u * NL < total;
      rr[u] = ok[u] ? row : last_row;
      cc[u] = ok[u] ? col : last_col;
      val[u] = tile[__umul24(cc[u], kPad) + rr[u]];   // 24-bit multiply: full-rate VALU
      idx[u] = ok[u] ? g0 + u * NL : total - 1;
      col += dcol; row += drow;
      if (col >= NC) { col -= NC; ++row; }
    }
    GPD_STAMP(8);
    E* dst = reinterpret_cast<E*>(obs) + n0 * NC;
    if (wt & 1) {
      // masked-off elements get an offset past num_records: the buffer unit drops the store
      // (no exec-mask branch per element)
      const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(dst, 0, total * EB, 0x00020000);
#pragma unroll
      for (int u = 0; u < U; ++u) store_wt<AUX>(r, ok[u] ? idx[u] * EB : total * EB, val[u]);
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (ok[u]) dst[idx[u]] = val[u];
    }
    GPD_STAMP(9);
    if (done_rows) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (ok[u] && ((done_rows >> rr[u]) & 1ull)) {
          if (cc[u] >= ncs) reinterpret_cast<E*>(terminal_obs)[n0 * NC + idx[u]] = val[u];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// gpd_step: one env.step() for every env (BaseAviary.py:259-383) in ONE launch.
// ACT: action type (GPD_ACT_*); PID types run DSLPIDControl before the substeps.
// PF: the physics flags compiled in (pf_on): 0 = plain DYN (the bench path, aero / PYB-wrench code
// compiled out), a flag set for the BASELINE configs' combinations, kPfRuntime for the rest.
// The history DMA, the ring append, the terminal-row store and the reset are the helpers of
// gpd_step_parts.h.  The action load, the peeled substep loop, the final readback, the hover
// terms, the env reduction and the tile fill are written out here although the same header
// defines them (step_kernel_het and step_kernel_wide call those): as calls they inline to the
// same instructions but to another register allocation and schedule in some instantiations, and
// this kernel's code is kept as tuned (scripts/kernel_diff.py, profiles/step_parts/).  A fix
// to one of those phases goes to the helper AND here (and to step_kernel_duo's pose wave); the
// peeled loop exists here and in step_kernel_het (see there).
template <typename R, int ACT, bool MULTI, int PF, bool STREAM = false>
// STREAM: the cache policies for batches far past the Infinity Cache (kAuxWtStream above).
// The leading scalar arguments duplicate the SimView / StepIO fields the first loads need: the
// library is built with kernarg preloading, so they arrive in SGPRs at wave launch instead of
// through an s_load round trip on the kernel-argument segment before the first state load.
__global__ __launch_bounds__(kWave) void step_kernel(R* __restrict__ state_p, const float* __restrict__ actions_p,
                                                     int2* __restrict__ ctr_p, const Consts<R>* __restrict__ cp,
                                                     long long npad_p, int n_p, int tpb_p, SimView<R> v, StepIO<R> io) {
  v.state = state_p; v.ctr = ctr_p; v.npad = npad_p; v.N = n_p; v.tpb = tpb_p;
  io.actions = actions_p;
  constexpr int A = act_width(ACT);
  extern __shared__ float4 tile4[];          // A == 4: [3+L][kPad] float4
  float* tilef = reinterpret_cast<float*>(tile4);  // A == 1, 3: [12+L*A][kPad] float
  __shared__ R sx[MULTI ? 2 * kWave : 1], sy[MULTI ? 2 * kWave : 1], sz[MULTI ? 2 * kWave : 1];
  // per-drone reward / distance in the compute precision: MultiHoverAviary sums both in fp64
  // (MultiHoverAviary.py:75-106) and tests the summed distance against 1e-4
  __shared__ R srew[MULTI ? 2 * kWave : 1], sdist[MULTI ? 2 * kWave : 1];
  __shared__ int sflag[MULTI ? 2 * kWave : 1];
  __shared__ R spair[MULTI ? kPairMax : 1];
  GPD_RSTAMP(11);
  GPD_STAMP(0);
#ifdef GPD_CONTACT_STATS
  const unsigned long long tk0 = __builtin_readcyclecounter();
#endif
  const Consts<R>& c = *cp;
  const int tid = threadIdx.x;
  const int D = MULTI ? v.D : 1;
  const int d = MULTI ? tid % D : 0;
  const int base = tid - d;
  const long long n0 = (long long)blockIdx.x * v.tpb;
  const long long n = n0 + tid;
  const int nact = (int)((v.N - n0) < v.tpb ? (v.N - n0) : v.tpb);  // drones owned by this block
  const bool active = tid < nact;
  // inactive lanes compute on the block's first drone and store nothing: a copy of a drone the
  // block integrates anyway, so a wave-uniform solve (the PYB contact) never waits for a drone
  // of another block (with drone 0's copies, every block paid drone 0's contact iterations)
  const long long nn = active ? n : n0;
  const long long e = MULTI ? nn / D : nn;
  const bool drag = pf_on<PF>(c.flags, F_DRAG);
  // drone <-> drone contact: the block's pair layout (the pair table loads go out with the state's)
  const DcPairs dcp = dc_enabled<MULTI, PF>(c.flags) ? dc_pairs_for(v, tid, nact) : dc_pairs_none();

  Drone<R> s;
  R last[4];
  load_drone<R, STREAM>(v, nn, s, last, drag);
  const int2 cv = v.ctr[e];
  const int sc = cv.x;        // step_counter
  const int head = cv.y;      // ring slot receiving this step's action
  float a[A];
  if (A == 4) {
    const float4 a4 = *reinterpret_cast<const float4*>(io.actions + nn * 4);
    a[0] = a4.x; a[1] = a4.y; a[2] = a4.z; a[3] = a4.w;
  } else {
#pragma unroll
    for (int j = 0; j < A; ++j) a[j] = io.actions[nn * A + j];
  }

  // the constants of the whole step, loaded in one batch while the state loads are in flight
  DynK<R> dk = dyn_consts(c);
  // warm the scalar cache with the kernel-argument lines the rest of the step reads (ring /
  // counters, task fields + obs pointers, done-flag pointers): one batch of misses now, in the
  // shadow of the state loads, instead of serialised misses behind later branches
  asm volatile("" ::"s"(v.ring), "s"(v.task), "s"(io.trunc));
#ifdef GPD_STAMPS
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // diagnostic: loads landed
  GPD_STAMP(10);
#endif
  R rpm[4];
  R cs[9];  // controller state (PID types)
  if (!act_is_pid(ACT)) {
    // _preprocessAction: rpm = HOVER_RPM*(1+0.05*a)  (BaseRLAviary.py:191-192, :224-225)
#pragma unroll
    for (int k = 0; k < 4; ++k) rpm[k] = (R)action_to_rpm(dk.hover_f32, a[A == 4 ? k : 0]);
  } else {
    // PID / VEL / ONE_D_PID (BaseRLAviary.py:193-235): DSLPIDControl on the state vector of
    // the last readback (_getDroneStateVector :559-561)
#pragma unroll
    for (int k = 0; k < 9; ++k) cs[k] = v.ctrl[tidx(nn, k, 9)];
    R qn[4], Rm[9], rpy[3];
    readback_fused(s.qx, s.qy, s.qz, s.qw, qn, Rm);
    quat_to_euler(qn, rpy[0], rpy[1], rpy[2]);
    const R pos[3] = {s.px, s.py, s.pz}, vel[3] = {s.vx, s.vy, s.vz};
    R tpos[3], tvel[3], tyaw;
    pid_targets<R, ACT>(c.pid, a, pos, rpy, tpos, tyaw, tvel);
    dsl_pid<R, ACT != ACT_VEL>(c.pid, pos, Rm, rpy, vel, tpos, tyaw, tvel, cs, rpm);
  }

  const int nh = v.ring_len - 1;
  // history ring -> obs tile: the L-1 oldest actions (LDS-DMA).  Issued after the first
  // substep: hipcc waits vmcnt(0) at the next use of an ordinary load while an LDS-DMA is in
  // flight, so issuing it before the state/action loads were consumed would put the DMA round
  // trip on the critical path.  Issued there it overlaps the remaining substeps.
  auto history_dma = [&]() {
    gpd::history_dma<A, STREAM ? kAuxDmaStream : 0>(v.ring, nn, head, v.ring_len, nh, tile4, tilef);
  };
  // propeller wrench: the same RPMs drive every substep of the control step (:349-367)
  R W[4];
  rpm_wrench<R, PF>(rpm, dk, c, W);
  // substeps 1..nsub-1 skip the (write-only) world ang_v; the last one produces it
  // (the first substep is peeled so the loop body stays one basic block)
  if (PF != kPfRuntime && (PF & F_BULLET) != 0) {
    // Bullet flag sets: ONE copy of the substep (its plane and pair solves are most of the kernel's
    // code; peeled first / last copies would triple it past the instruction cache the SQC shares
    // between two CUs; profiles/r4/loop/).  The world ang_v is a three-register copy here, so every
    // substep makes it.  The multi-drone kernels issue the history DMA after the substeps: a
    // drone-contact call waits for every memory operation in flight (multi2pyb 62.0 vs 62.7-63.0 us,
    // 8-drone 527-532 vs 536-538 us, profiles/r4/dc_call/).
    for (int it = 0; it < dk.nsub; ++it) {
      substep_block<R, MULTI, PF, true>(s, rpm, W, last, c, dk, sx, sy, sz, tid, base, D, v.dw_pairs, spair, dcp);
#pragma unroll
      for (int k = 0; k < 4; ++k) last[k] = rpm[k];   // self.last_clipped_action = clipped_action  :372
      if (it == 0 && !MULTI) history_dma();
    }
    if (MULTI) history_dma();
  } else {
    if (dk.nsub > 1) {
      substep_block<R, MULTI, PF, false>(s, rpm, W, last, c, dk, sx, sy, sz, tid, base, D, v.dw_pairs, spair, dcp);
#pragma unroll
      for (int k = 0; k < 4; ++k) last[k] = rpm[k];   // self.last_clipped_action = clipped_action  :372
      GPD_STAMP(1);
      history_dma();
      for (int it = 1; it < dk.nsub - 1; ++it)
        substep_block<R, MULTI, PF, false>(s, rpm, W, last, c, dk, sx, sy, sz, tid, base, D, v.dw_pairs, spair, dcp);
    }
    substep_block<R, MULTI, PF, true>(s, rpm, W, last, c, dk, sx, sy, sz, tid, base, D, v.dw_pairs, spair, dcp);
#pragma unroll
    for (int k = 0; k < 4; ++k) last[k] = rpm[k];
    if (dk.nsub == 1) history_dma();
  }
  GPD_STAMP(2);
  // final readback (:374) -> obs / reward / done
  R qn[4], Rm[9];
  readback_fused(s.qx, s.qy, s.qz, s.qw, qn, Rm);
  AttitudeArgs<R> att = attitude_args(qn);
  bool tilted, up_unused;   // |roll| or |pitch| > 0.4, decided exactly near the limit (attitude_decide)
  attitude_decide<R, true, false>(s.qx, s.qy, s.qz, s.qw, att, tilted, up_unused);
  float roll, pitch, yaw;
  obs_euler_f32(qn, att, roll, pitch, yaw);

  // ---- task hooks, evaluated before step_counter += PYB_STEPS_PER_CTRL (:376-382)
  float reward = -1.0f;
  bool term = false, trunc = false;
  if (v.task != TASK_NONE) {
    const R* tg = MULTI ? v.target + d * 3 : c.target0;
    const R tx = tg[0] - s.px, ty = tg[1] - s.py, tz = tg[2] - s.pz;
    // |e|^2 gives the reward max(0, 2 - |e|^4); the done test is made on |e| itself, as the
    // reference's np.linalg.norm(...) < .0001 (HoverAviary.py:92, MultiHoverAviary.py:101-104)
    const R d2 = tx * tx + ty * ty + tz * tz;
    const R dist = g_sqrt(d2);
    R r = R(2) - d2 * d2;
    r = r > R(0) ? r : R(0);
    const bool oob = g_abs(s.px) > v.bound_xy || g_abs(s.py) > v.bound_xy || s.pz > R(2) || tilted;
    if (MULTI) {
      srew[tid] = r;
      sdist[tid] = dist;
      sflag[tid] = oob ? 1 : 0;
      wave_lds_sync();   // one-wave block; no __syncthreads(): its fence would wait for the history DMA
      if (d == 0) {
        // MultiHoverAviary: summed reward, sum of distances < 1e-4, any drone out of bounds
        R rs = R(0), ds = R(0);
        int anyo = 0;
        for (int j = 0; j < D; ++j) { rs += srew[base + j]; ds += sdist[base + j]; anyo |= sflag[base + j]; }
        reward = (float)rs;
        term = ds < R(1e-4);
        trunc = anyo != 0 || sc >= v.trunc_sc;
        sflag[tid] = (term ? 1 : 0) | (trunc ? 2 : 0);
        srew[tid] = reward;
      }
      wave_lds_sync();
      const int fl = sflag[base];
      term = fl & 1;
      trunc = (fl >> 1) & 1;
      reward = (float)srew[base];
    } else {
      reward = (float)r;
      term = dist < R(1e-4);
      trunc = oob || sc >= v.trunc_sc;
    }
  }
  const bool done = term || trunc;
  const bool do_reset = done && v.autoreset;

  float row12[12] = {(float)s.px, (float)s.py, (float)s.pz, roll, pitch, yaw,
                     (float)s.vx, (float)s.vy, (float)s.vz, (float)s.ax, (float)s.ay, (float)s.az};
  GPD_STAMP(3);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // history DMA has landed in the tile
  GPD_STAMP(4);
  // current action into the ring (deque.append); issued after the wait above so that the wait
  // does not also cover this store's write acknowledgement.  The DMA never reads slot `head`.
  if (active) ring_append<A>(v.ring, n, head, v.ring_len, a);


  const int NC = A == 4 ? 3 + v.ring_len : 12 + v.ring_len * A;  // tile columns (float4 / float)
  if (do_reset) {
    // the terminal row's state part is stored straight from registers (finished envs are rare;
    // its history and action columns equal the reset row's and go out with the tile copy-out);
    // the env goes back to INIT_XYZS / INIT_RPYS (_housekeeping :458-477; SB3 DummyVecEnv keeps
    // the last obs as terminal_observation)
    if (active && io.terminal_obs != nullptr) row12_store<A>(io.terminal_obs + n * v.W, row12);
    reset_to_template(MULTI ? v.init + d * 10 : c.init0, s, last, row12);
  }
  // bit r set <=> tile row r belongs to an env that finished this step (tile rows are lanes)
  const unsigned long long done_rows = __ballot(do_reset && active && io.terminal_obs != nullptr);

  GPD_STAMP(5);
  // ---- state columns + current action into the tile, then coalesced copy-out of the rows
  if (A == 4) {
    tile4[0 * kPad + tid] = make_float4(row12[0], row12[1], row12[2], row12[3]);
    tile4[1 * kPad + tid] = make_float4(row12[4], row12[5], row12[6], row12[7]);
    tile4[2 * kPad + tid] = make_float4(row12[8], row12[9], row12[10], row12[11]);
    tile4[(3 + nh) * kPad + tid] = make_float4(a[0], a[1], a[2], a[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) tilef[k * kPad + tid] = row12[k];
#pragma unroll
    for (int j = 0; j < A; ++j) tilef[(12 + nh * A + j) * kPad + tid] = a[j];
  }
  __syncthreads();
  GPD_STAMP(6);
  tile_copy_out<A, kWave, 6, STREAM ? kAuxWtStream : kAuxWt>(tile4, tilef, tid, nact, NC, v.nc_magic, v.wt, done_rows,
                                                             io.obs, io.terminal_obs, n0);
  GPD_STAMP(7);
  GPD_RSTAMP(12);
#ifdef GPD_CONTACT_STATS
  if (tid == 0 && blockIdx.x < 4096) atomicAdd(&g_pc_hist[256 + 4096 + blockIdx.x], __builtin_readcyclecounter() - tk0);
#endif
  if (!active) return;
  store_drone_step<R, STREAM ? kAuxWtStream : kAuxWt>(v, n, s, last);
  mark_last_in_ring(v, n);
  if (act_is_pid(ACT)) {
#pragma unroll
    for (int k = 0; k < 9; ++k) v.ctrl[tidx(n, k, 9)] = cs[k];
  }
  if (d == 0) {
    io.reward[e] = reward;
    io.term[e] = term ? 1 : 0;
    io.trunc[e] = trunc ? 1 : 0;
    v.ctr[e] = make_int2(do_reset ? 0 : sc + dk.nsub, head + 1 == v.ring_len ? 0 : head + 1);
  }
}

}  // namespace gpd
