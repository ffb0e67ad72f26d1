// gpd_step_het.h — the heterogeneous ("het") sim: every env has its own drone parameters
// (gpd_env_params) and every drone of every env its own start pose (gpd_create_het).  The kernels
// here run the phases of step_kernel / integrate_kernel (gpd_step_parts.h) on per-lane model
// constants; the physics itself is the unchanged device functions of gpd_device.h, called on a
// lane-local Consts.  gpd_reset and the last_clipped_action settle are the shared reset_kernel /
// last_from_ring_kernel (gpd_step_wide.h), told to use the per-drone template / per-env hover
// column.  A het sim runs the DYN integrator only (no F_BULLET), the RPM action types, D <= 64; it
// never selects the duo, io-wave, STREAM or wide kernels.
//
// Tables (owned by the sim, uploaded by the host, never derived on the device):
//   etab   real [kHetCols][epad]  SoA of the per-env constants the substeps read, derived on the
//                                 host in double with make_consts' expressions and rounded once to
//                                 the sim's real type; epad = E rounded up to 64.  Column
//                                 kHetHover holds float32(HOVER_RPM) (exact in either real type).
//   init   real [E][D][10]        reset templates (pos, stored quat, rpy), SimView::init
//   target real [E][D][3]         task targets, SimView::target
// A lane loads its env's kHetCols columns right behind its state loads (one batch of loads in
// flight); single-drone envs read 64 consecutive elements per column.  The downwash coefficients
// stay sim-wide: in the thin-block pair path (substep_block, pairs.n > 0) a lane evaluates dw_pair
// for a drone of ANOTHER env, so they must come from the shared constant block.
//
// Reset pools (gpd_set_reset_pool): a pool of P drones (rows [P][kHetCols], row-major: one lane
// reads one row) and a pool of Q start poses (templates [Q][D][10], targets [Q][D][3]), derived on
// the host by the code that derives the tables above.  The pooled instantiations of step_kernel_het
// (POOL = one PoolArgs) give an env that auto-resets its next drone and pose: pool_draw, a pure
// function of (seed, env, episode number), picks the indices; the env's own lanes copy the row
// into etab[:, e] and the pose into init[e] / target[e].  draws [E][3] int32 holds {episode number,
// row index in force, pose index in force}, -1 = the env's own (not drawn) value.
#pragma once
#include "gpd_step.h"

namespace gpd {

enum : int {
  kHetM = 0, kHetGravity, kHetInvM, kHetKf, kHetKm, kHetL, kHetLs2, kHetJx, kHetJy, kHetJz,
  kHetIjx, kHetIjy, kHetIjz, kHetHover, kHetGeCoeff, kHetGeClip, kHetDragXy, kHetDragZ, kHetCols
};
// the physics terms a het sim may carry (gpd_create_het rejects every other flag)
constexpr int kHetFlags = F_GND | F_DRAG | F_DW | F_GEOM;

// The lane's Consts: the sim-wide fields the DYN path reads from the shared block (scalar loads),
// the per-env ones from env e's table columns (vector loads).  Fields the DYN path never reads
// (the Bullet contact constants, the PID block, init0 / target0) stay zero.
template <typename R>
__device__ __forceinline__ Consts<R> het_consts(const Consts<R>& c, const R* __restrict__ etab, long long epad,
                                                long long e) {
  Consts<R> lc = {};
  const R* col = etab + e;
  lc.m = col[kHetM * epad]; lc.gravity = col[kHetGravity * epad]; lc.inv_m = col[kHetInvM * epad];
  lc.kf = col[kHetKf * epad]; lc.km = col[kHetKm * epad]; lc.L = col[kHetL * epad]; lc.Ls2 = col[kHetLs2 * epad];
  lc.jx = col[kHetJx * epad]; lc.jy = col[kHetJy * epad]; lc.jz = col[kHetJz * epad];
  lc.ijx = col[kHetIjx * epad]; lc.ijy = col[kHetIjy * epad]; lc.ijz = col[kHetIjz * epad];
  lc.hover_f32 = (float)col[kHetHover * epad];
  lc.ge_coeff = col[kHetGeCoeff * epad]; lc.ge_clip = col[kHetGeClip * epad];
  lc.drag_xy = col[kHetDragXy * epad]; lc.drag_z = col[kHetDragZ * epad];
  lc.dt = c.dt; lc.hdt = c.hdt; lc.hdt2 = c.hdt2;
  lc.prop_r = c.prop_r; lc.two_pi = c.two_pi;
  lc.dw1 = c.dw1; lc.dw2 = c.dw2; lc.dw3 = c.dw3; lc.dwk1 = c.dwk1;
#pragma unroll
  for (int k = 0; k < 4; ++k) { lc.rx[k] = c.rx[k]; lc.ry[k] = c.ry[k]; lc.rz[k] = c.rz[k]; }
  lc.rpm2rad = c.rpm2rad;
  lc.model = c.model; lc.flags = c.flags; lc.nsub = c.nsub;
  return lc;
}

// The pool draw (gpd_reset_pool_draw is this function): uint32 arithmetic, then one 32x32 -> 64
// multiply that maps the hash to [0, n).  stream: 1 = parameter rows, 2 = poses; k: the env's
// episode number (1 at its first auto-reset).
__host__ __device__ __forceinline__ unsigned pool_mix32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__host__ __device__ __forceinline__ int pool_draw(unsigned seed, unsigned stream, unsigned e, unsigned k, unsigned n) {
  unsigned h = pool_mix32(seed ^ (0x9e3779b9u * stream));
  h = pool_mix32(h + e);
  h = pool_mix32(h + k);
  return (int)(((unsigned long long)h * n) >> 32);
}
enum : unsigned { kPoolStreamRows = 1, kPoolStreamPoses = 2 };
template <typename T, typename... Rest>
__device__ __forceinline__ const T& first_arg(const T& a, const Rest&...) { return a; }

// The pool descriptor, in device memory at an address that never changes: replacing a pool by
// another of any size rewrites these fields and leaves a captured graph valid.
template <typename R>
struct ResetPool {
  const R* rows;     // [P][kHetCols]
  const R* init;     // [Q][D][10]
  const R* target;   // [Q][D][3]
  int P, Q;          // 0: parameters / poses are never redrawn
  unsigned seed;
};
template <typename R>
struct PoolArgs {
  const ResetPool<R>* pool;
  int* draws;        // [E][3]
};

// ---------------------------------------------------------------------------------------
// gpd_step of a het sim: step_kernel's phases (gpd_step.h) with the lane's own constants, reset
// template (v.init + nn*10) and task target (v.target + nn*3), and no drone contact.  PF as in
// step_kernel: 0, F_GND|F_DRAG, F_DW (multi) compiled in, kPfRuntime for the other DYN flag sets.
// POOL is empty (a sim without a reset pool: the kernel and its arguments as they always were) or
// one PoolArgs<R> (the pooled instantiation: the same code plus the pooled tail below).
template <typename R, int ACT, bool MULTI, int PF, typename... POOL>
__global__ __launch_bounds__(kWave) void step_kernel_het(R* __restrict__ state_p, const float* __restrict__ actions_p,
                                                         int2* __restrict__ ctr_p, const Consts<R>* __restrict__ cp,
                                                         const R* __restrict__ etab, int n_p, int tpb_p,
                                                         long long epad, SimView<R> v, StepIO<R> io,
                                                         POOL... pool_args) {
  static_assert(sizeof...(POOL) <= 1, "POOL is empty or one PoolArgs<R>");
  constexpr bool kPool = sizeof...(POOL) == 1;
  static_assert(!act_is_pid(ACT), "het sims take the RPM action types only");
  static_assert(PF == kPfRuntime || (PF & ~kHetFlags) == 0, "het sims run the DYN integrator only");
  v.state = state_p; v.ctr = ctr_p; v.N = n_p; v.tpb = tpb_p;
  io.actions = actions_p;
  constexpr int A = act_width(ACT);
  extern __shared__ float4 tile4[];          // A == 4: [3+L][kPad] float4
  float* tilef = reinterpret_cast<float*>(tile4);  // A == 1: [12+L][kPad] float
  __shared__ R sx[MULTI ? 2 * kWave : 1], sy[MULTI ? 2 * kWave : 1], sz[MULTI ? 2 * kWave : 1];
  __shared__ R srew[MULTI ? 2 * kWave : 1], sdist[MULTI ? 2 * kWave : 1];
  __shared__ int sflag[MULTI ? 2 * kWave : 1];
  __shared__ R spair[MULTI ? kPairMax : 1];
  const Consts<R>& c = *cp;
  const int tid = threadIdx.x;
  const int D = MULTI ? v.D : 1;
  const int d = MULTI ? tid % D : 0;
  const int base = tid - d;
  const long long n0 = (long long)blockIdx.x * v.tpb;
  const long long n = n0 + tid;
  const int nact = (int)((v.N - n0) < v.tpb ? (v.N - n0) : v.tpb);  // drones owned by this block
  const bool active = tid < nact;
  // inactive lanes compute on the block's first drone (state AND env parameters) and store nothing
  const long long nn = active ? n : n0;
  const long long e = MULTI ? nn / D : nn;
  const bool drag = pf_on<PF>(c.flags, F_DRAG);
  const DcPairs dcp = dc_pairs_none();

  Drone<R> s;
  R last[4];
  load_drone<R, false>(v, nn, s, last, drag);
  const Consts<R> lc = het_consts(c, etab, epad, e);   // same batch of loads as the state's
  const int2 cv = v.ctr[e];
  const int sc = cv.x;        // step_counter
  const int head = cv.y;      // ring slot receiving this step's action
  // pooled: the env's draws and the pool descriptor in the entry batch of loads, so that the
  // pooled tail does not start with two dependent round trips (descriptor, then draws)
  ResetPool<R> pool = {};
  int* draws_e = nullptr;
  int episode = 0, pi = -1, qi = -1;
  if constexpr (kPool) {
    const PoolArgs<R> pa = first_arg(pool_args...);
    pool = *pa.pool;
    draws_e = pa.draws + e * 3;
    episode = draws_e[0]; pi = draws_e[1]; qi = draws_e[2];
  }
  float a[A];
  action_load<A>(io.actions, nn, a);

  DynK<R> dk = dyn_consts(lc);
  dk.flags &= kHetFlags;   // known to the compiler: the Bullet substep is dead code here
  asm volatile("" ::"s"(v.ring), "s"(v.task), "s"(io.trunc));
  R rpm[4];
  // _preprocessAction: rpm = HOVER_RPM*(1+0.05*a) with the ENV's float32 hover constant
#pragma unroll
  for (int k = 0; k < 4; ++k) rpm[k] = (R)action_to_rpm(dk.hover_f32, a[A == 4 ? k : 0]);

  const int nh = v.ring_len - 1;
  R W[4];
  rpm_wrench<R, PF>(rpm, dk, lc, W);
  // the peeled substep loop with the history DMA after the first substep, written out as in
  // step_kernel: through a shared helper the f64 gnd + drag instantiation rounds the state
  // differently in the last bit, and a het sim on nominal rows must stay bit-equal to step_kernel.
  // (The form tried: a __forceinline__ template taking the hook as a callable by forwarding
  // reference, `F&& after_first`, called with this lambda; every other argument as substep_block's.
  // The f64 instruction counts stayed the same; which operation rounds differently was not traced.)
  auto dma = [&]() { history_dma<A, 0>(v.ring, nn, head, v.ring_len, nh, tile4, tilef); };
  if (dk.nsub > 1) {
    substep_block<R, MULTI, PF, false>(s, rpm, W, last, lc, dk, sx, sy, sz, tid, base, D, v.dw_pairs, spair, dcp);
#pragma unroll
    for (int k = 0; k < 4; ++k) last[k] = rpm[k];   // self.last_clipped_action = clipped_action  :372
    dma();
    for (int it = 1; it < dk.nsub - 1; ++it)
      substep_block<R, MULTI, PF, false>(s, rpm, W, last, lc, dk, sx, sy, sz, tid, base, D, v.dw_pairs, spair, dcp);
  }
  substep_block<R, MULTI, PF, true>(s, rpm, W, last, lc, dk, sx, sy, sz, tid, base, D, v.dw_pairs, spair, dcp);
#pragma unroll
  for (int k = 0; k < 4; ++k) last[k] = rpm[k];
  if (dk.nsub == 1) dma();
  // final readback (:374) -> obs / reward / done
  float roll, pitch, yaw;
  const bool tilted = obs_angles(s, roll, pitch, yaw);

  // ---- task hooks, evaluated before step_counter += PYB_STEPS_PER_CTRL (:376-382)
  float reward = -1.0f;
  bool term = false, trunc = false;
  if (v.task != TASK_NONE) {
    R r, dist;
    bool oob;
    // the drone's own target (MultiHover: INIT_XYZS + (0,0,1/(i+1)))
    hover_terms(v.target + nn * 3, s, v.bound_xy, tilted, r, dist, oob);
    if (MULTI) {
      env_reduce(srew, sdist, sflag, tid, d, base, D, r, dist, oob, sc, v.trunc_sc, reward, term, trunc);
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
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // history DMA has landed in the tile
  if (active) ring_append<A>(v.ring, n, head, v.ring_len, a);

  const int NC = A == 4 ? 3 + v.ring_len : 12 + v.ring_len * A;  // tile columns (float4 / float)
  const R* tmpl = v.init + nn * 10;   // the drone's own start pose
  if constexpr (kPool) {
    // The pooled tail: the env's next drone and pose.  The reward, flags and terminal row above are
    // the old drone's and the old target's.  The branch is wave-uniform and, at real episode
    // lengths, skipped by almost every wave.  Only lanes of env e's own block ever read or write
    // env e's columns of etab, init, target and draws, and they read them at the kernel's entry,
    // so no ordering against other blocks is needed; the next launch sees the stores.
    // The lane then resets itself through ONE reset_to_template call on a selected pointer.  That
    // form is the one found to leave the substeps' rounding alone: with the drawn template handed
    // over in registers (a second call, or an override after the plain call), and also with the
    // state pinned by an empty asm in front of the tail, some instantiation (f64 gnd + drag, f64
    // plain, f32 gnd + drag) came out one ulp away from its non-pooled twin on nominal rows, as the
    // note at the substep loop above describes; tests/test_gpu_pool.py holds every instantiation
    // family to bit-equality.
    if (__ballot(do_reset && active) != 0ull) {
      const bool mine = do_reset && active;
      const bool new_row = mine && d == 0 && pool.P > 0;
      const bool new_pose = mine && pool.Q > 0;
      // every lane of the env makes the env's draws itself: a pure function of (seed, e, episode)
      const unsigned k = (unsigned)episode + 1u;
      if (pool.P > 0) pi = pool_draw(pool.seed, kPoolStreamRows, (unsigned)e, k, (unsigned)pool.P);
      if (pool.Q > 0) qi = pool_draw(pool.seed, kPoolStreamPoses, (unsigned)e, k, (unsigned)pool.Q);
      // all of the copies' loads first (one round trip), then their stores
      R prow[kHetCols], ptmpl[10], ptgt[3];
      const long long q = (long long)qi * D + d;
      if (new_row) {
        const R* row = pool.rows + (long long)pi * kHetCols;
#pragma unroll
        for (int c2 = 0; c2 < kHetCols; ++c2) prow[c2] = row[c2];
      }
      if (new_pose) {
        tmpl = pool.init + q * 10;   // the drawn start pose
#pragma unroll
        for (int c2 = 0; c2 < 10; ++c2) ptmpl[c2] = pool.init[q * 10 + c2];
#pragma unroll
        for (int c2 = 0; c2 < 3; ++c2) ptgt[c2] = pool.target[q * 3 + c2];
      }
      if (new_row) {
        // etab[:, e] <- the pool row (ordinary vector stores).  last_clipped_action needs no
        // care: the env's hover column changes only here, at a reset, where the step counter
        // becomes 0 and last_from_ring_kernel / settle_last_any therefore write 0 whatever
        // the hover column holds; the next step stores a last action made with the new one.
        R* col = const_cast<R*>(etab) + e;
#pragma unroll
        for (int c2 = 0; c2 < kHetCols; ++c2) col[c2 * epad] = prow[c2];
      }
      if (new_pose) {
        // init[e][d] / target[e][d] <- the drawn pose: gpd_reset goes back to the pose in force
        R* ini = const_cast<R*>(v.init) + nn * 10;
        R* tgt = const_cast<R*>(v.target) + nn * 3;
#pragma unroll
        for (int c2 = 0; c2 < 10; ++c2) ini[c2] = ptmpl[c2];
#pragma unroll
        for (int c2 = 0; c2 < 3; ++c2) tgt[c2] = ptgt[c2];
      }
      if (mine && d == 0) { draws_e[0] = (int)k; draws_e[1] = pi; draws_e[2] = qi; }
    }
  }
  if (do_reset) {
    if (active && io.terminal_obs != nullptr) row12_store<A>(io.terminal_obs + n * v.W, row12);
    reset_to_template(tmpl, s, last, row12);
  }
  const unsigned long long done_rows = __ballot(do_reset && active && io.terminal_obs != nullptr);

  tile_fill_state<A>(tile4, tilef, tid, row12);
  tile_fill_action<A>(tile4, tilef, tid, nh, a);
  __syncthreads();
  tile_copy_out<A, kWave, 6, kAuxWt>(tile4, tilef, tid, nact, NC, v.nc_magic, v.wt, done_rows, io.obs,
                                     io.terminal_obs, n0);
  if (!active) return;
  store_drone_step<R, kAuxWt>(v, n, s, last);
  mark_last_in_ring(v, n);
  if (d == 0) {
    io.reward[e] = reward;
    io.term[e] = term ? 1 : 0;
    io.trunc[e] = trunc ? 1 : 0;
    v.ctr[e] = make_int2(do_reset ? 0 : sc + dk.nsub, head + 1 == v.ring_len ? 0 : head + 1);
  }
}

// ---------------------------------------------------------------------------------------
// gpd_integrate of a het sim: integrate_kernel's loop (gpd_step_wide.h) with the lane's own
// constants.  PF: 0 (plain DYN) or kPfRuntime; TRAJ: record the [n_sub][N][20] trajectory.
template <typename R, bool MULTI, int PF, bool TRAJ>
__global__ __launch_bounds__(kWave) void integrate_kernel_het(SimView<R> v, const Consts<R>* __restrict__ cp,
                                                              const R* __restrict__ etab, long long epad,
                                                              const R* __restrict__ rpm_in, int n_sub,
                                                              R* __restrict__ traj) {
  __shared__ R sx[MULTI ? 2 * kWave : 1], sy[MULTI ? 2 * kWave : 1], sz[MULTI ? 2 * kWave : 1];
  const Consts<R>& c = *cp;
  const int tid = threadIdx.x;
  const int D = MULTI ? v.D : 1;
  const int d = MULTI ? tid % D : 0;
  const int base = tid - d;
  const long long n0 = (long long)blockIdx.x * v.tpb;
  const long long n = n0 + tid;
  const bool active = tid < v.tpb && n < v.N;
  const long long nn = active ? n : n0;   // the block's first drone (step_kernel_het)
  const long long e = MULTI ? nn / D : nn;
  Drone<R> s;
  R last[4];
  load_drone<R, false>(v, nn, s, last, true);
  const Consts<R> lc = het_consts(c, etab, epad, e);
  const long long N = v.N;
  DynK<R> dk = dyn_consts(lc);
  dk.flags &= kHetFlags;
  const DcPairs dcp = dc_pairs_none();
  auto load4 = [&](int t, R out[4]) { load_rpm4(rpm_in + ((long long)t * N + nn) * 4, out); };
  R nxt[4], nxt2[4];
  if (n_sub > 0) load4(0, nxt);
  if (n_sub > 1) load4(1, nxt2);
  for (int t = 0; t < n_sub; ++t) {
    R rpm[4] = {nxt[0], nxt[1], nxt[2], nxt[3]};
#pragma unroll
    for (int k = 0; k < 4; ++k) nxt[k] = nxt2[k];
    if (t + 2 < n_sub) load4(t + 2, nxt2);
    R W[4];
    rpm_wrench<R, PF>(rpm, dk, lc, W);
    substep_block<R, MULTI, PF>(s, rpm, W, last, lc, dk, sx, sy, sz, tid, base, D, DwPairs{0, 0}, nullptr, dcp);
#pragma unroll
    for (int k = 0; k < 4; ++k) last[k] = rpm[k];
    if (TRAJ && active) state20_store(s, last, traj + ((long long)t * N + n) * 20);
  }
  if (!active || n_sub == 0) return;
  store_drone<R, false>(v, n, s, last);
}

}  // namespace gpd
