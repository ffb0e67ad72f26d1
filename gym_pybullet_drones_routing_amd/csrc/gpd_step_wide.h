// gpd_step_wide.h — the remaining kernels: step_kernel_wide / integrate_kernel_wide (envs of more
// than 64 drones, or rows that overflow the one-wave tile), integrate_kernel (gpd_integrate: raw
// substeps with explicit RPMs) and the utility kernels (reset, state export / import, layout
// conversion).  Needs gpd_layout.h, DcHookT (gpd_dcontact.h) and the phases of gpd_step_parts.h
// (substep_block, action_load, obs_angles, hover_terms, reset_to_template, state20_store, load_rpm4).
#pragma once
#include "gpd_step_duo.h"

namespace gpd {

// ---------------------------------------------------------------------------------------
// Envs of more than 64 drones (MultiHoverAviary(num_drones=D), D <= kWideMax): one env per
// workgroup of ceil(D/64) waves.  (Also envs of any D whose observation rows overflow the one-wave
// kernels' LDS tile, gpd_create: up to 64 / D of them packed into one wave when D <= 32.)  The per-substep position exchange of _downwash
// (BaseAviary.py:785-811, O(D^2)) and the env's reward / done reductions go through LDS with
// workgroup barriers; lanes d >= D compute on drone 0 of the env and store nothing.  Physics
// flags are tested at run time; observation rows are stored straight from registers (history
// columns read from the ring), without the LDS tile of the one-wave kernels.  Same operations
// and order as step_kernel / integrate_kernel (tests/test_gpu_wide.py).
constexpr int kWideMax = 1024;

// t: the thread (its LDS slot), active: it owns a drone, base: its env's first slot
template <typename R>
__device__ __forceinline__ R wide_downwash(const Drone<R>& s, R* sx, R* sy, R* sz, int t, bool active, int base,
                                           int D, const Consts<R>& c, int flags) {
  R dw = R(0);
  if (flags & F_DW) {
    __syncthreads();                       // previous readers of sx/sy/sz are done
    if (active) { sx[t] = s.px; sy[t] = s.py; sz[t] = s.pz; }
    __syncthreads();
    dw = downwash_sum(s.px, s.py, s.pz, sx, sy, sz, base, D, c);
  }
  return dw;
}

// The history columns of the workgroup's observation rows (and terminal rows): ring slots
// head+1 .. head+L-1 of each drone, copied by every thread of the workgroup (ACT's A floats per
// slot, float4 items for A = 4), kWideU loads in flight per thread before their stores.  n0: the
// workgroup's first drone, nd: its drones; shead[env slot] = ring head | 1 << 30 when the env's
// terminal row is written.
constexpr int kWideU = 8;
constexpr int kWideTrow = 1 << 30;
template <typename R, int A>
__device__ __forceinline__ void wide_history(const SimView<R>& v, const StepIO<R>& io, long long n0, int nd, int D,
                                             const int* shead) {
  const int L = v.ring_len, Wd = v.W, H = L - 1, nth = blockDim.x;
  constexpr int G = A == 4 ? 4 : 1;              // floats per item
  const int per = H * (A / G);                   // items per drone
  const int total = nd * per;
  for (int i0 = 0; i0 < total; i0 += nth * kWideU) {
    float x[kWideU][G];
    long long dst[kWideU];
    bool tr[kWideU];
#pragma unroll
    for (int u = 0; u < kWideU; ++u) {
      const int i = i0 + u * nth + (int)threadIdx.x;
      dst[u] = -1;
      if (i < total) {
        const int dq = i / per, r = i - dq * per;
        const int k = G == 4 ? r : r / A, j = G == 4 ? 0 : r - k * A;
        const int hv = shead[dq / D], head = hv & (kWideTrow - 1);
        tr[u] = (hv & kWideTrow) != 0;
        int slot = head + 1 + k;
        slot -= slot >= L ? L : 0;
        const float* src = v.ring + ridx(n0 + dq, slot, L, A) + j;
        if (G == 4) {
          const float4 q = *reinterpret_cast<const float4*>(src);
          x[u][0] = q.x; x[u][G > 1 ? 1 : 0] = q.y; x[u][G > 2 ? 2 : 0] = q.z; x[u][G > 3 ? 3 : 0] = q.w;
        } else {
          x[u][0] = *src;
        }
        dst[u] = (n0 + dq) * Wd + 12 + k * A + j;
      }
    }
#pragma unroll
    for (int u = 0; u < kWideU; ++u) {
      if (dst[u] < 0) continue;
      if (G == 4) {
        const float4 q = make_float4(x[u][0], x[u][G > 1 ? 1 : 0], x[u][G > 2 ? 2 : 0], x[u][G > 3 ? 3 : 0]);
        *reinterpret_cast<float4*>(io.obs + dst[u]) = q;
        if (tr[u]) *reinterpret_cast<float4*>(io.terminal_obs + dst[u]) = q;
      } else {
        io.obs[dst[u]] = x[u][0];
        if (tr[u]) io.terminal_obs[dst[u]] = x[u][0];
      }
    }
  }
}

// MAXT: the workgroup size bound the instantiation is compiled for (256 / 512 / 1024 threads:
// the register budget per lane halves with each doubling, 1024 spills to scratch).
// DC: the drone <-> drone contact (DcHookT, the one-wave kernels' solve): one-wave workgroups
// (D <= 64, MAXT = 64) of a long-history PYB* env; its DcLds is static LDS, so only these
// instantiations carry it.
template <typename R, int ACT, int MAXT, bool DC = false>
__global__ __launch_bounds__(MAXT) void step_kernel_wide(SimView<R> v, StepIO<R> io, const Consts<R>* __restrict__ cp) {
  constexpr int A = act_width(ACT);
  __shared__ R sx[MAXT], sy[MAXT], sz[MAXT];
  __shared__ int sflag[MAXT];
  __shared__ int shead[kWave];
  const Consts<R>& c = *cp;
  const int D = v.D;
  // GE = v.tpb / D envs per workgroup: one for D > 32; up to 64 / D packed into one wave for the
  // small envs that run here because their observation rows overflow the one-wave kernels' LDS tile
  const int GE = v.tpb / D;
  const int t = threadIdx.x;
  const int g = t / D, d = t - g * D;           // env slot, drone in the env
  const long long e0 = (long long)blockIdx.x * GE, e = e0 + g;
  const long long nenv = v.N / D;
  const bool active = g < GE && e < nenv;
  const int slot0 = (g < GE ? g : 0) * D;       // the env's first LDS slot
  // lanes without a drone compute on the first drone of their own wave (a drone this wave
  // integrates anyway: the waves take turns in the contact solve) and store nothing
  const long long n = active ? e * D + d : e0 * D + (t & ~(kWave - 1));
  const long long es = active ? e : e0;
  const int nact = (int)(nenv - e0 < GE ? nenv - e0 : GE) * D;   // drones owned by this workgroup
  const DcPairs dcp = DC ? dc_pairs_for(v, t, nact) : dc_pairs_none();
  const bool drag = (c.flags & F_DRAG) != 0;
  Drone<R> s;
  R last[4];
  load_drone(v, n, s, last, drag);
  const int2 cv = v.ctr[es];
  const int sc = cv.x, head = cv.y;
  float a[A];
  action_load<A>(io.actions, n, a);
  DynK<R> dk = dyn_consts(c);
  R rpm[4];
  R cs[9];
  if (!act_is_pid(ACT)) {
#pragma unroll
    for (int k = 0; k < 4; ++k) rpm[k] = (R)action_to_rpm(dk.hover_f32, a[A == 4 ? k : 0]);
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) cs[k] = v.ctrl[tidx(n, k, 9)];
    R qn[4], Rm[9], rpy[3];
    readback_fused(s.qx, s.qy, s.qz, s.qw, qn, Rm);
    quat_to_euler(qn, rpy[0], rpy[1], rpy[2]);
    const R pos[3] = {s.px, s.py, s.pz}, vel[3] = {s.vx, s.vy, s.vz};
    R tpos[3], tvel[3], tyaw;
    pid_targets<R, ACT>(c.pid, a, pos, rpy, tpos, tyaw, tvel);
    dsl_pid<R, ACT != ACT_VEL>(c.pid, pos, Rm, rpy, vel, tpos, tyaw, tvel, cs, rpm);
  }
  R W[4];
  rpm_wrench<R, kPfRuntime>(rpm, dk, c, W);
  const int nw = (int)(blockDim.x / kWave);
  for (int it = 0; it < dk.nsub; ++it) {
    const R dw = wide_downwash(s, sx, sy, sz, t, active, slot0, D, c, dk.flags);
    if (DC) dyn_substep<R, kPfRuntime, true, 1, DcHookT<false>>(s, rpm, W, last, dw, c, dk, DcHookT<false>{t, dcp});
    else if (nw > 1) dyn_substep<R, kPfRuntime, true, 16>(s, rpm, W, last, dw, c, dk);
    else dyn_substep<R, kPfRuntime, true, 1>(s, rpm, W, last, dw, c, dk);
#pragma unroll
    for (int k = 0; k < 4; ++k) last[k] = rpm[k];   // self.last_clipped_action = clipped_action  :372
  }
  // final readback (:374) -> obs / reward / done
  float roll, pitch, yaw;
  const bool tilted = obs_angles(s, roll, pitch, yaw);
  float reward = -1.0f;
  bool term = false, trunc = false;
  if (v.task != TASK_NONE) {
    R r, dist;
    bool oob;
    hover_terms(v.target + (active ? d : 0) * 3, s, v.bound_xy, tilted, r, dist, oob);
    __syncthreads();
    if (active) { sx[t] = r; sy[t] = dist; sflag[t] = oob ? 1 : 0; }
    __syncthreads();
    if (active && d == 0) {   // MultiHoverAviary: the summed reward / distance in the reference's order
      R rs = R(0), ds = R(0);
      int anyo = 0;
      for (int j = slot0; j < slot0 + D; ++j) { rs += sx[j]; ds += sy[j]; anyo |= sflag[j]; }
      sflag[slot0] = (ds < R(1e-4) ? 1 : 0) | ((anyo != 0 || sc >= v.trunc_sc) ? 2 : 0);
      sx[slot0] = rs;
    }
    __syncthreads();
    const int fl = sflag[slot0];
    term = fl & 1;
    trunc = (fl >> 1) & 1;
    reward = (float)sx[slot0];
  }
  const bool done = term || trunc;
  const bool do_reset = done && v.autoreset;
  float row12[12] = {(float)s.px, (float)s.py, (float)s.pz, roll, pitch, yaw,
                     (float)s.vx, (float)s.vy, (float)s.vz, (float)s.ax, (float)s.ay, (float)s.az};
  const int L = v.ring_len, Wd = v.W;
  // history columns: ring slots head+1 .. head+L-1 (oldest first), then the current action
  // (BaseRLAviary.py:307-319); the same for the terminal row and the (reset) observation.  The
  // history columns are copied by the whole workgroup, kWideU independent loads per thread
  // before their stores: a lane copying its own row element by element waited out one memory
  // round trip per element (680 us per step for 4096 single-drone envs with a 240-step history)
  if (active && d == 0) shead[g] = head | ((do_reset && io.terminal_obs) ? kWideTrow : 0);
  // (also: every wave has read ctr[e] (kernel entry) before lane d == 0 overwrites it below;
  // without a task, downwash or contact no other workgroup barrier orders the two)
  __syncthreads();
  wide_history<R, A>(v, io, e0 * D, nact, D, shead);
  if (!active) return;
  float* orow = io.obs + n * Wd;
  float* trow = (do_reset && io.terminal_obs) ? io.terminal_obs + n * Wd : nullptr;
  for (int j = 0; j < A; ++j) {
    orow[12 + (L - 1) * A + j] = a[j];
    if (trow) trow[12 + (L - 1) * A + j] = a[j];
  }
  // deque.append (slot head is not read above); float by float: ring_append's 16-byte store costs
  // step_kernel_wide<double, ACT_VEL, 256> two more registers
  float* ring_cur = v.ring + ridx(n, head, L, A);
  for (int j = 0; j < A; ++j) ring_cur[j] = a[j];
  if (do_reset) {
    if (trow)
      for (int k = 0; k < 12; ++k) trow[k] = row12[k];
    reset_to_template(v.init + d * 10, s, last, row12);
  }
  for (int k = 0; k < 12; ++k) orow[k] = row12[k];
  store_drone_step(v, n, s, last);
  mark_last_in_ring(v, n);
  if (act_is_pid(ACT)) {
#pragma unroll
    for (int k = 0; k < 9; ++k) v.ctrl[tidx(n, k, 9)] = cs[k];
  }
  if (d == 0) {
    io.reward[e] = reward;
    io.term[e] = term ? 1 : 0;
    io.trunc[e] = trunc ? 1 : 0;
    v.ctr[e] = make_int2(do_reset ? 0 : sc + dk.nsub, head + 1 == L ? 0 : head + 1);
  }
}

// gpd_integrate for envs of more than 64 drones (see step_kernel_wide).
template <typename R, bool TRAJ, int MAXT>
__global__ __launch_bounds__(MAXT) void integrate_kernel_wide(SimView<R> v, const Consts<R>* __restrict__ cp,
                                                              const R* __restrict__ rpm_in, int n_sub,
                                                              R* __restrict__ traj) {
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
  const long long N = v.N;
  for (int t = 0; t < n_sub; ++t) {
    const R* src = rpm_in + ((long long)t * N + n) * 4;
    R rpm[4] = {src[0], src[1], src[2], src[3]};
    R W[4];
    rpm_wrench<R, kPfRuntime>(rpm, dk, c, W);
    const R dw = wide_downwash(s, sx, sy, sz, d, active, 0, D, c, dk.flags);
    if (nw > 1) dyn_substep<R, kPfRuntime, true, 16>(s, rpm, W, last, dw, c, dk);
    else dyn_substep<R, kPfRuntime, true, 1>(s, rpm, W, last, dw, c, dk);
#pragma unroll
    for (int k = 0; k < 4; ++k) last[k] = rpm[k];
    if (TRAJ && active) state20_store(s, last, traj + ((long long)t * N + n) * 20);
  }
  if (active && n_sub > 0) store_drone(v, n, s, last);
}

// ---------------------------------------------------------------------------------------
// gpd_integrate: n_sub raw substeps with explicit per-substep RPMs, each followed by a readback.
// PF as in step_kernel: 0 (plain DYN, the raw-integrator bench) or kPfRuntime; TRAJ: record the
// [n_sub][N][20] trajectory.
// STREAM (plain DYN batches past the Infinity Cache): nt loads of the once-read RPM stream and the
// state, nt stores of the state (as step_kernel's STREAM).
template <typename R, bool MULTI, int PF, bool TRAJ, bool STREAM = false>
__global__ __launch_bounds__(kWave) void integrate_kernel(SimView<R> v, const Consts<R>* __restrict__ cp,
                                                          const R* __restrict__ rpm_in, int n_sub, R* __restrict__ traj) {
  __shared__ R sx[MULTI ? 2 * kWave : 1], sy[MULTI ? 2 * kWave : 1], sz[MULTI ? 2 * kWave : 1];
  const Consts<R>& c = *cp;
  const int tid = threadIdx.x;
  const int D = MULTI ? v.D : 1;
  const int d = MULTI ? tid % D : 0;
  const int base = tid - d;
  const long long n = (long long)blockIdx.x * v.tpb + tid;
  const bool active = tid < v.tpb && n < v.N;
  const long long nn = active ? n : (long long)blockIdx.x * v.tpb;   // the block's first drone (step_kernel)
  const long long nleft = v.N - (long long)blockIdx.x * v.tpb;
  const int nact = (int)(nleft < v.tpb ? nleft : v.tpb);
  Drone<R> s;
  R last[4];
  load_drone<R, STREAM>(v, nn, s, last, true);
  const long long N = v.N;
  DynK<R> dk = dyn_consts(c);
  const DcPairs dcp = dc_enabled<MULTI, PF>(c.flags) ? dc_pairs_for(v, tid, nact) : dc_pairs_none();
  // RPMs are loaded two substeps ahead of their use (substeps t+1 and t+2 in flight while t
  // integrates): more bytes in flight per wave for the HBM stream.
  auto load4 = [&](int t, R out[4]) { load_rpm4<R, STREAM>(rpm_in + ((long long)t * N + nn) * 4, out); };
  R nxt[4], nxt2[4];
  if (n_sub > 0) load4(0, nxt);
  if (n_sub > 1) load4(1, nxt2);
  for (int t = 0; t < n_sub; ++t) {
    R rpm[4] = {nxt[0], nxt[1], nxt[2], nxt[3]};
#pragma unroll
    for (int k = 0; k < 4; ++k) nxt[k] = nxt2[k];
    if (t + 2 < n_sub) load4(t + 2, nxt2);
    R W[4];
    rpm_wrench<R, PF>(rpm, dk, c, W);
    substep_block<R, MULTI, PF>(s, rpm, W, last, c, dk, sx, sy, sz, tid, base, D, DwPairs{0, 0}, nullptr, dcp);
#pragma unroll
    for (int k = 0; k < 4; ++k) last[k] = rpm[k];
    // TRAJ: the trajectory variant (its readback / Euler registers stay out of the other)
    if (TRAJ && active) state20_store(s, last, traj + ((long long)t * N + n) * 20);
  }
  if (!active) return;
  if (n_sub == 0) return;
  store_drone<R, STREAM>(v, n, s, last);
}

// ---------------------------------------------------------------------------------------
// gpd_reset: masked re-initialisation (+ reset observation rows).  HET: v.init holds a template
// per drone of every env ([E][D][10], gpd_step_het.h), else one per drone of an env ([D][10]).
template <typename R, bool HET>
__global__ __launch_bounds__(256) void reset_kernel(SimView<R> v, const uint8_t* __restrict__ mask, float* obs) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= v.N) return;
  const long long e = n / v.D;
  const int d = (int)(n - e * v.D);
  if (mask && mask[e] == 0) return;
  const R* ini = v.init + (HET ? n : d) * 10;
  Drone<R> s;
  drone_from_template(ini, s);
  R last[4] = {R(0), R(0), R(0), R(0)};
  store_drone(v, n, s, last);
  const int head = v.ctr[e].y;
  if (d == 0) v.ctr[e].x = 0;
  if (obs) {
    float* orow = obs + n * v.W;
    row12_from_template(ini, orow);
    const int A = v.A;
    for (int k = 0; k < v.ring_len; ++k) {   // oldest first: the slot about to be overwritten
      int slot = head + k;
      slot -= slot >= v.ring_len ? v.ring_len : 0;
      const float* src = v.ring + ridx(n, slot, v.ring_len, A);
      for (int j = 0; j < A; ++j) orow[12 + k * A + j] = src[j];
    }
  }
}

// last_clipped_action back into the state (store_drone_step): when ctr[E].x is set, drone n's
// state[16..19] = action_to_rpm of its ring's newest slot (head - 1 after the step; the same
// float32 mapping as the step, _preprocessAction BaseRLAviary.py:191-192), or 0 when its env's
// step_counter is 0 (_housekeeping zeroes last_clipped_action, BaseAviary.py:466).  The caller
// clears the mark afterwards (stream order).  hover_env: a het sim's per-env column of
// float32(HOVER_RPM) values (etab's kHetHover, gpd_step_het.h), null for the sim-wide constant.
template <typename R>
__global__ __launch_bounds__(256) void last_from_ring_kernel(SimView<R> v, const Consts<R>* __restrict__ c,
                                                             const R* __restrict__ hover_env) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= v.N) return;
  if (v.ctr[v.N / v.D].x == 0) return;
  const long long e = n / v.D;
  const int2 cv = v.ctr[e];
  R last[4] = {R(0), R(0), R(0), R(0)};
  if (cv.x != 0) {
    const int slot = cv.y == 0 ? v.ring_len - 1 : cv.y - 1;
    const float* a = v.ring + ridx(n, slot, v.ring_len, v.A);
    const float hover = hover_env ? (float)hover_env[e] : c->hover_f32;
    for (int k = 0; k < 4; ++k) last[k] = (R)action_to_rpm(hover, a[v.A == 4 ? k : 0]);
  }
  for (int k = 0; k < 4; ++k) v.state[tidx(n, 16 + k, kStateComps)] = last[k];
}

// state20 (BaseAviary._getDroneStateVector :541-561, literal Bullet readback) / raw transposes
template <typename R>
__global__ __launch_bounds__(256) void state20_kernel(SimView<R> v, R* __restrict__ out, int raw) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= v.N) return;
  R* o = out + n * 20;
  if (raw) {
    for (int k = 0; k < 20; ++k) o[k] = v.state[tidx(n, k, kStateComps)];
    return;
  }
  Drone<R> s;
  R last[4];
  load_drone_full(v, n, s, last);
  state20_store(s, last, o);
}

// Per-env non-finite guard: flag[e] = 1 when any drone of env e holds a
// non-finite integrated state component (pos, stored quat, vel, rates, ang_v), e.g. after the
// downwash quotient's beta = 0 edge (BaseAviary.py:802-804).  flag is zeroed by the caller;
// several drones of one env may store the same 1.
template <typename R>
__global__ __launch_bounds__(256) void nonfinite_kernel(SimView<R> v, uint8_t* __restrict__ flag) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= v.N) return;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 16; ++k) bad = bad || !isfinite(v.state[tidx(n, k, kStateComps)]);
  if (bad) flag[n / v.D] = 1;
}

template <typename R>
__global__ __launch_bounds__(256) void set_raw_kernel(SimView<R> v, const R* __restrict__ in) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= v.N) return;
  for (int k = 0; k < 20; ++k) v.state[tidx(n, k, kStateComps)] = in[n * 20 + k];
}

// tiled SoA <-> [N][comps] rows (controller state access)
template <typename R>
__global__ __launch_bounds__(256) void soa_to_rows_kernel(const R* __restrict__ soa, long long npad, int comps, int N,
                                                          R* __restrict__ out) {
  (void)npad;
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  for (int k = 0; k < comps; ++k) out[n * comps + k] = soa[tidx(n, k, comps)];
}
template <typename R>
__global__ __launch_bounds__(256) void rows_to_soa_kernel(const R* __restrict__ in, long long npad, int comps, int N,
                                                          R* __restrict__ soa) {
  (void)npad;
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  for (int k = 0; k < comps; ++k) soa[tidx(n, k, comps)] = in[n * comps + k];
}

}  // namespace gpd
