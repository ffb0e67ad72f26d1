// gpd_step_het.h — the heterogeneous ("het") sim: every env has its own drone parameters
// (gpd_env_params) and every drone of every env its own start pose (gpd_create_het).  The kernels
// here are the one-wave step_kernel / integrate_kernel bodies (gpd_step.h, gpd_step_wide.h) with
// per-lane model constants; the physics itself is the unchanged device functions of gpd_device.h,
// called on a lane-local Consts.  A het sim runs the DYN integrator only (no F_BULLET), the RPM
// action types, D <= 64; it never selects the duo, io-wave, STREAM or wide kernels.
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

// ---------------------------------------------------------------------------------------
// gpd_step of a het sim: step_kernel's body (gpd_step.h) with the lane's own constants, reset
// template (v.init + nn*10) and task target (v.target + nn*3).  PF as in step_kernel: 0,
// F_GND|F_DRAG, F_DW (multi) compiled in, kPfRuntime for the other DYN flag sets.
template <typename R, int ACT, bool MULTI, int PF>
__global__ __launch_bounds__(kWave) void step_kernel_het(R* __restrict__ state_p, const float* __restrict__ actions_p,
                                                         int2* __restrict__ ctr_p, const Consts<R>* __restrict__ cp,
                                                         const R* __restrict__ etab, int n_p, int tpb_p,
                                                         long long epad, SimView<R> v, StepIO<R> io) {
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
  float a[A];
  if (A == 4) {
    const float4 a4 = *reinterpret_cast<const float4*>(io.actions + nn * 4);
    a[0] = a4.x; a[1] = a4.y; a[2] = a4.z; a[3] = a4.w;
  } else {
#pragma unroll
    for (int j = 0; j < A; ++j) a[j] = io.actions[nn * A + j];
  }

  DynK<R> dk = dyn_consts(lc);
  dk.flags &= kHetFlags;   // known to the compiler: the Bullet substep is dead code here
  asm volatile("" ::"s"(v.ring), "s"(v.task), "s"(io.trunc));
  R rpm[4];
  // _preprocessAction: rpm = HOVER_RPM*(1+0.05*a) with the ENV's float32 hover constant
#pragma unroll
  for (int k = 0; k < 4; ++k) rpm[k] = (R)action_to_rpm(dk.hover_f32, a[A == 4 ? k : 0]);

  const int nh = v.ring_len - 1;
  auto history_dma = [&]() {   // as step_kernel's: after the first substep
    for (int k = 0; k < nh; ++k) {
      int slot = head + 1 + k;
      slot -= slot >= v.ring_len ? v.ring_len : 0;
      const float* src = v.ring + ridx(nn, slot, v.ring_len, A);
      if (A == 4) {
        __builtin_amdgcn_global_load_lds((gbl_void_ptr)src, (lds_void_ptr)(tile4 + (3 + k) * kPad), 16, 0, 0);
      } else {
#pragma unroll
        for (int j = 0; j < A; ++j)
          __builtin_amdgcn_global_load_lds((gbl_void_ptr)(src + j), (lds_void_ptr)(tilef + (12 + k * A + j) * kPad), 4,
                                           0, 0);
      }
    }
  };
  R W[4];
  rpm_wrench<R, PF>(rpm, dk, lc, W);
  if (dk.nsub > 1) {
    substep_block<R, MULTI, PF, false>(s, rpm, W, last, lc, dk, sx, sy, sz, tid, base, D, v.dw_pairs, spair, dcp);
#pragma unroll
    for (int k = 0; k < 4; ++k) last[k] = rpm[k];   // self.last_clipped_action = clipped_action  :372
    history_dma();
    for (int it = 1; it < dk.nsub - 1; ++it)
      substep_block<R, MULTI, PF, false>(s, rpm, W, last, lc, dk, sx, sy, sz, tid, base, D, v.dw_pairs, spair, dcp);
  }
  substep_block<R, MULTI, PF, true>(s, rpm, W, last, lc, dk, sx, sy, sz, tid, base, D, v.dw_pairs, spair, dcp);
#pragma unroll
  for (int k = 0; k < 4; ++k) last[k] = rpm[k];
  if (dk.nsub == 1) history_dma();
  // final readback (:374) -> obs / reward / done
  R qn[4], Rm[9];
  readback_fused(s.qx, s.qy, s.qz, s.qw, qn, Rm);
  AttitudeArgs<R> att = attitude_args(qn);
  bool tilted, up_unused;
  attitude_decide<R, true, false>(s.qx, s.qy, s.qz, s.qw, att, tilted, up_unused);
  float roll, pitch, yaw;
  obs_euler_f32(qn, att, roll, pitch, yaw);

  // ---- task hooks, evaluated before step_counter += PYB_STEPS_PER_CTRL (:376-382)
  float reward = -1.0f;
  bool term = false, trunc = false;
  if (v.task != TASK_NONE) {
    const R* tg = v.target + nn * 3;   // the drone's own target (MultiHover: INIT_XYZS + (0,0,1/(i+1)))
    const R tx = tg[0] - s.px, ty = tg[1] - s.py, tz = tg[2] - s.pz;
    const R d2 = tx * tx + ty * ty + tz * tz;
    const R dist = g_sqrt(d2);
    R r = R(2) - d2 * d2;
    r = r > R(0) ? r : R(0);
    const bool oob = g_abs(s.px) > v.bound_xy || g_abs(s.py) > v.bound_xy || s.pz > R(2) || tilted;
    if (MULTI) {
      srew[tid] = r;
      sdist[tid] = dist;
      sflag[tid] = oob ? 1 : 0;
      wave_lds_sync();
      if (d == 0) {
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
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // history DMA has landed in the tile
  if (active) {
    float* ring_cur = v.ring + ridx(n, head, v.ring_len, A);
    if (A == 4) *reinterpret_cast<float4*>(ring_cur) = make_float4(a[0], a[1], a[2], a[3]);
    else
#pragma unroll
      for (int j = 0; j < A; ++j) ring_cur[j] = a[j];
  }

  const int NC = A == 4 ? 3 + v.ring_len : 12 + v.ring_len * A;  // tile columns (float4 / float)
  if (do_reset) {
    if (active && io.terminal_obs != nullptr) {
      float* trow = io.terminal_obs + n * v.W;
      if (A == 4) {
        float4* t4 = reinterpret_cast<float4*>(trow);
        t4[0] = make_float4(row12[0], row12[1], row12[2], row12[3]);
        t4[1] = make_float4(row12[4], row12[5], row12[6], row12[7]);
        t4[2] = make_float4(row12[8], row12[9], row12[10], row12[11]);
      } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) trow[k] = row12[k];
      }
    }
    const R* ini = v.init + nn * 10;   // the drone's own start pose
    s.px = ini[0]; s.py = ini[1]; s.pz = ini[2];
    s.qx = ini[3]; s.qy = ini[4]; s.qz = ini[5]; s.qw = ini[6];
    s.vx = s.vy = s.vz = R(0);
    s.wx = s.wy = s.wz = R(0);
    s.ax = s.ay = s.az = R(0);
#pragma unroll
    for (int k = 0; k < 4; ++k) last[k] = R(0);
    row12[0] = (float)ini[0]; row12[1] = (float)ini[1]; row12[2] = (float)ini[2];
    row12[3] = (float)ini[7]; row12[4] = (float)ini[8]; row12[5] = (float)ini[9];
#pragma unroll
    for (int k = 6; k < 12; ++k) row12[k] = 0.0f;
  }
  const unsigned long long done_rows = __ballot(do_reset && active && io.terminal_obs != nullptr);

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
// gpd_integrate of a het sim: integrate_kernel's body (gpd_step_wide.h) with the lane's own
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
  auto load4 = [&](int t, R out[4]) {   // a drone's 4 RPMs: one aligned 4*sizeof(R)-byte vector
    const R* src = rpm_in + ((long long)t * N + nn) * 4;
    typedef double gpd_d2 __attribute__((ext_vector_type(2)));
    typedef float gpd_f4 __attribute__((ext_vector_type(4)));
    if (sizeof(R) == 8) {
      const gpd_d2 a = reinterpret_cast<const gpd_d2*>(src)[0], b = reinterpret_cast<const gpd_d2*>(src)[1];
      out[0] = (R)a.x; out[1] = (R)a.y; out[2] = (R)b.x; out[3] = (R)b.y;
    } else {
      const gpd_f4 a = *reinterpret_cast<const gpd_f4*>(src);
      out[0] = (R)a.x; out[1] = (R)a.y; out[2] = (R)a.z; out[3] = (R)a.w;
    }
  };
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
    if (TRAJ && active) {
      R qn[4], roll, pitch, yaw;   // the literal Bullet readback (as state20)
      quat_readback(s.qx, s.qy, s.qz, s.qw, qn);
      quat_to_euler(qn, roll, pitch, yaw);
      R* o = traj + ((long long)t * N + n) * 20;
      o[0] = s.px; o[1] = s.py; o[2] = s.pz;
      o[3] = qn[0]; o[4] = qn[1]; o[5] = qn[2]; o[6] = qn[3];
      o[7] = roll; o[8] = pitch; o[9] = yaw;
      o[10] = s.vx; o[11] = s.vy; o[12] = s.vz;
      o[13] = s.ax; o[14] = s.ay; o[15] = s.az;
      o[16] = last[0]; o[17] = last[1]; o[18] = last[2]; o[19] = last[3];
    }
  }
  if (!active || n_sub == 0) return;
  store_drone<R, false>(v, n, s, last);
}

// gpd_reset of a het sim: reset_kernel (gpd_step_wide.h) with the drone's own template, v.init + n*10.
template <typename R>
__global__ __launch_bounds__(256) void reset_kernel_het(SimView<R> v, const uint8_t* __restrict__ mask, float* obs) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= v.N) return;
  const long long e = n / v.D;
  const int d = (int)(n - e * v.D);
  if (mask && mask[e] == 0) return;
  const R* ini = v.init + n * 10;
  Drone<R> s;
  s.px = ini[0]; s.py = ini[1]; s.pz = ini[2];
  s.qx = ini[3]; s.qy = ini[4]; s.qz = ini[5]; s.qw = ini[6];
  s.vx = s.vy = s.vz = R(0);
  s.wx = s.wy = s.wz = R(0);
  s.ax = s.ay = s.az = R(0);
  R last[4] = {R(0), R(0), R(0), R(0)};
  store_drone(v, n, s, last);
  const int head = v.ctr[e].y;
  if (d == 0) v.ctr[e].x = 0;
  if (obs) {
    float* orow = obs + n * v.W;
    orow[0] = (float)ini[0]; orow[1] = (float)ini[1]; orow[2] = (float)ini[2];
    orow[3] = (float)ini[7]; orow[4] = (float)ini[8]; orow[5] = (float)ini[9];
    for (int k = 6; k < 12; ++k) orow[k] = 0.0f;
    const int A = v.A;
    for (int k = 0; k < v.ring_len; ++k) {   // oldest first: the slot about to be overwritten
      int slot = head + k;
      slot -= slot >= v.ring_len ? v.ring_len : 0;
      const float* src = v.ring + ridx(n, slot, v.ring_len, A);
      for (int j = 0; j < A; ++j) orow[12 + k * A + j] = src[j];
    }
  }
}

// last_clipped_action back from the ring on a het sim: last_from_ring_kernel (gpd_step_wide.h)
// with the ENV's float32 hover constant from the table.
template <typename R>
__global__ __launch_bounds__(256) void last_from_ring_kernel_het(SimView<R> v, const R* __restrict__ etab,
                                                                 long long epad) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= v.N) return;
  if (v.ctr[v.N / v.D].x == 0) return;
  const long long e = n / v.D;
  const int2 cv = v.ctr[e];
  R last[4] = {R(0), R(0), R(0), R(0)};
  if (cv.x != 0) {
    const int slot = cv.y == 0 ? v.ring_len - 1 : cv.y - 1;
    const float* a = v.ring + ridx(n, slot, v.ring_len, v.A);
    const float hover = (float)etab[kHetHover * epad + e];
    for (int k = 0; k < 4; ++k) last[k] = (R)action_to_rpm(hover, a[v.A == 4 ? k : 0]);
  }
  for (int k = 0; k < 4; ++k) v.state[tidx(n, 16 + k, kStateComps)] = last[k];
}

}  // namespace gpd
