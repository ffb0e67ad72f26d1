// gpd_step_parts.h — the phases of a step, one definition each: the kernels of gpd_step.h,
// gpd_step_duo.h, gpd_step_wide.h, gpd_step_cmd.h, gpd_step_rollout.h and gpd_step_het.h are
// sequences of these.  Every helper is __forceinline__ and takes the operands of the text it
// replaced with the same types and qualifiers; WHEN a phase runs (the DMA after the first substep,
// the wait before the ring store, ...) is the calling kernel's schedule and is explained there.
// step_kernel and step_kernel_duo call only the helpers that leave their machine code as it was
// and keep the other phases written out (see the note at step_kernel); step_seq_kernel
// (gpd_step_seq.h) follows step_kernel_duo in this, phase for phase.  So do, for one block
// each: step_kernel_het (the peeled substep loop: a last-bit change), cmd_rollout_kernel (substep
// loop and row staging: speed), step_kernel_wide (ring append: registers).  Each says so in place.
// Needs the layout and loads of gpd_layout.h, the device functions of gpd_device.h and DcHookT
// (gpd_dcontact.h).
#pragma once
#include "gpd_dcontact.h"

namespace gpd {

// One physics substep of every drone of the block, including the readback that precedes it
// (BaseAviary.py:343-372 loop body).  MULTI: envs have D > 1 drones and may need downwash.
template <typename R, bool MULTI, int PF, bool ANGV = true>
__device__ __forceinline__ void substep_block(Drone<R>& s, R rpm[4], R W[4], R last[4],
                                              const Consts<R>& c, DynK<R>& k, R* sx, R* sy, R* sz, int tid,
                                              int base, int D, DwPairs pairs, R* spair, const DcPairs& dcp) {
  R dw = R(0);
  if (MULTI && pf_on<PF>(k.flags, F_DW)) {
    sx[tid] = s.px; sy[tid] = s.py; sz[tid] = s.pz;
    wave_lds_sync();
    if (pairs.n > 0) {
      for (int p = tid; p < pairs.n; p += kWave) {
        const int i = (p * pairs.dmagic) >> 20;          // drone of the block
        const int j = p - i * D;                          // neighbour within its env
        const int ib = ((i * pairs.dmagic) >> 20) * D;   // the env's first drone in the block
        spair[p] = dw_pair(sx[i], sy[i], sz[i], sx[ib + j], sy[ib + j], sz[ib + j], c);
      }
      wave_lds_sync();
      if (tid * D < pairs.n)
        for (int j = 0; j < D; ++j) dw = dw + spair[tid * D + j];
    } else {
      dw = downwash_sum(s.px, s.py, s.pz, sx, sy, sz, base, D, c);
    }
    wave_lds_sync();
  }
  // the drone contact inlined in the compiled-in flag sets without downwash (DcHookT)
  constexpr bool kDcInl = PF != kPfRuntime && (PF & F_DW) == 0;
  if (MULTI) dyn_substep<R, PF, ANGV, 1, DcHookT<kDcInl>>(s, rpm, W, last, dw, c, k, DcHookT<kDcInl>{tid, dcp});
  else dyn_substep<R, PF, ANGV>(s, rpm, W, last, dw, c, k);
}

// The substeps of one command step (no downwash pair split, nothing between the substeps).  The
// drag of substep 1 sees the previous step's RPMs in `last` (BaseAviary.py:359-372).
template <typename R, bool MULTI, int PF>
__device__ __forceinline__ void substeps_cmd(Drone<R>& s, R rpm[4], R W[4], R last[4], const Consts<R>& c, DynK<R>& dk,
                                             R* sx, R* sy, R* sz, int tid, int base, int D, const DcPairs& dcp) {
  if (PF == 0) {   // the write-only world ang_v from the last substep only
    for (int it = 0; it < dk.nsub - 1; ++it)
      substep_block<R, MULTI, PF, false>(s, rpm, W, last, c, dk, sx, sy, sz, tid, base, D, DwPairs{0, 0}, nullptr, dcp);
    substep_block<R, MULTI, PF, true>(s, rpm, W, last, c, dk, sx, sy, sz, tid, base, D, DwPairs{0, 0}, nullptr, dcp);
#pragma unroll
    for (int k = 0; k < 4; ++k) last[k] = rpm[k];
  } else {         // one copy of the substep (its plane and pair solves are most of the kernel's code)
    for (int it = 0; it < dk.nsub; ++it) {
      substep_block<R, MULTI, PF, true>(s, rpm, W, last, c, dk, sx, sy, sz, tid, base, D, DwPairs{0, 0}, nullptr, dcp);
#pragma unroll
      for (int k = 0; k < 4; ++k) last[k] = rpm[k];   // self.last_clipped_action = clipped_action  :372
    }
  }
}

// ---- actions and the history ring
// Drone n's action row: A floats, one 16-byte load for A == 4.
template <int A>
__device__ __forceinline__ void action_load(const float* actions, long long n, float a[A]) {
  if (A == 4) {
    const float4 a4 = *reinterpret_cast<const float4*>(actions + n * 4);
    a[0] = a4.x; a[1] = a4.y; a[2] = a4.z; a[3] = a4.w;
  } else {
#pragma unroll
    for (int j = 0; j < A; ++j) a[j] = actions[n * A + j];
  }
}

// deque.append of the current action: ring slot `head` of drone n.
template <int A>
__device__ __forceinline__ void ring_append(float* ring, long long n, int head, int ring_len, const float a[A]) {
  float* ring_cur = ring + ridx(n, head, ring_len, A);
  if (A == 4) *reinterpret_cast<float4*>(ring_cur) = make_float4(a[0], a[1], a[2], a[3]);
  else
#pragma unroll
    for (int j = 0; j < A; ++j) ring_cur[j] = a[j];
}

// History ring -> obs tile (LDS-DMA): drone n's nh = L-1 oldest actions, slots head+1 .., into the
// tile columns behind the state's.  AUX: the DMA's cache policy.  (nh comes from the kernel, which
// uses it again for the action column: forming it here moves the subtraction in step_kernel.)
template <int A, int AUX>
__device__ __forceinline__ void history_dma(const float* ring, long long n, int head, int ring_len, int nh,
                                            float4* tile4, float* tilef) {
  for (int k = 0; k < nh; ++k) {
    int slot = head + 1 + k;
    slot -= slot >= ring_len ? ring_len : 0;
    const float* src = ring + ridx(n, slot, ring_len, A);
    if (A == 4) {
      __builtin_amdgcn_global_load_lds((gbl_void_ptr)src, (lds_void_ptr)(tile4 + (3 + k) * kPad), 16, 0, AUX);
    } else {
#pragma unroll
      for (int j = 0; j < A; ++j)
        __builtin_amdgcn_global_load_lds((gbl_void_ptr)(src + j), (lds_void_ptr)(tilef + (12 + k * A + j) * kPad), 4, 0,
                                         AUX);
    }
  }
}

// ---- the final readback (:374) and the task
// The observation's Euler angles in float32; returns whether |roll| or |pitch| > 0.4, decided
// exactly near the limit (attitude_decide).
template <typename R>
__device__ __forceinline__ bool obs_angles(const Drone<R>& s, float& roll, float& pitch, float& yaw) {
  R qn[4], Rm[9];
  readback_fused(s.qx, s.qy, s.qz, s.qw, qn, Rm);
  AttitudeArgs<R> att = attitude_args(qn);
  bool tilted, up_unused;
  attitude_decide<R, true, false>(s.qx, s.qy, s.qz, s.qw, att, tilted, up_unused);
  obs_euler_f32(qn, att, roll, pitch, yaw);
  return tilted;
}

// A drone's hover terms against its target row tg.  |e|^2 gives the reward max(0, 2 - |e|^4); the
// done test is made on |e| itself, as the reference's np.linalg.norm(...) < .0001
// (HoverAviary.py:92, MultiHoverAviary.py:101-104).
template <typename R>
__device__ __forceinline__ void hover_terms(const R* tg, const Drone<R>& s, R bound_xy, bool tilted, R& r, R& dist,
                                            bool& oob) {
  const R tx = tg[0] - s.px, ty = tg[1] - s.py, tz = tg[2] - s.pz;
  const R d2 = tx * tx + ty * ty + tz * tz;
  dist = g_sqrt(d2);
  r = R(2) - d2 * d2;
  r = r > R(0) ? r : R(0);
  oob = g_abs(s.px) > bound_xy || g_abs(s.py) > bound_xy || s.pz > R(2) || tilted;
}

// MultiHoverAviary's env figures in a one-wave block: summed reward, sum of distances < 1e-4, any
// drone out of bounds, each in the compute precision and in the reference's order
// (MultiHoverAviary.py:75-106).  Lane `base` is the env's first drone (d == 0).  One-wave block:
// no __syncthreads(), whose fence would wait for a history DMA in flight.
template <typename R>
__device__ __forceinline__ void env_reduce(R* srew, R* sdist, int* sflag, int tid, int d, int base, int D, R r, R dist,
                                           bool oob, int sc, int trunc_sc, float& reward, bool& term, bool& trunc) {
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
    trunc = anyo != 0 || sc >= trunc_sc;
    sflag[tid] = (term ? 1 : 0) | (trunc ? 2 : 0);
    srew[tid] = reward;
  }
  wave_lds_sync();
  const int fl = sflag[base];
  term = fl & 1;
  trunc = (fl >> 1) & 1;
  reward = (float)srew[base];
}

// ---- observation rows
// The 12 state columns of a row to trow; A == 4 rows are 16-byte aligned (W = 12 + 4 L).
template <int A>
__device__ __forceinline__ void row12_store(float* trow, const float row12[12]) {
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

// A drone at its reset template ini = pos(3) quat_raw(4) rpy(3) (_housekeeping :458-477).
template <typename R>
__device__ __forceinline__ void drone_from_template(const R* ini, Drone<R>& s) {
  s.px = ini[0]; s.py = ini[1]; s.pz = ini[2];
  s.qx = ini[3]; s.qy = ini[4]; s.qz = ini[5]; s.qw = ini[6];
  s.vx = s.vy = s.vz = R(0);
  s.wx = s.wy = s.wz = R(0);
  s.ax = s.ay = s.az = R(0);
}
// The state columns of the template's observation row.
template <typename R>
__device__ __forceinline__ void row12_from_template(const R* ini, float row12[12]) {
  row12[0] = (float)ini[0]; row12[1] = (float)ini[1]; row12[2] = (float)ini[2];
  row12[3] = (float)ini[7]; row12[4] = (float)ini[8]; row12[5] = (float)ini[9];
#pragma unroll
  for (int k = 6; k < 12; ++k) row12[k] = 0.0f;
}
// Auto-reset of a finished env's drone inside the step.
template <typename R>
__device__ __forceinline__ void reset_to_template(const R* ini, Drone<R>& s, R last[4], float row12[12]) {
  drone_from_template(ini, s);
#pragma unroll
  for (int k = 0; k < 4; ++k) last[k] = R(0);
  row12_from_template(ini, row12);
}

// Lane tid's state columns / current action into the obs tile (tile[col][lane], gpd_kernels.h).
template <int A>
__device__ __forceinline__ void tile_fill_state(float4* tile4, float* tilef, int tid, const float row12[12]) {
  if (A == 4) {
    tile4[0 * kPad + tid] = make_float4(row12[0], row12[1], row12[2], row12[3]);
    tile4[1 * kPad + tid] = make_float4(row12[4], row12[5], row12[6], row12[7]);
    tile4[2 * kPad + tid] = make_float4(row12[8], row12[9], row12[10], row12[11]);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) tilef[k * kPad + tid] = row12[k];
  }
}
template <int A>
__device__ __forceinline__ void tile_fill_action(float4* tile4, float* tilef, int tid, int nh, const float a[A]) {
  if (A == 4) {
    tile4[(3 + nh) * kPad + tid] = make_float4(a[0], a[1], a[2], a[3]);
  } else {
#pragma unroll
    for (int j = 0; j < A; ++j) tilef[(12 + nh * A + j) * kPad + tid] = a[j];
  }
}

// ---- state20 rows and RPM vectors
// The 20-float state vector of a drone (BaseAviary._getDroneStateVector :541-561) with the
// literal Bullet readback: exact gimbal branches.
template <typename R>
__device__ __forceinline__ void state20_row(const Drone<R>& s, const R last[4], R o[20]) {
  R qn[4], roll, pitch, yaw;
  quat_readback(s.qx, s.qy, s.qz, s.qw, qn);
  quat_to_euler(qn, roll, pitch, yaw);
  o[0] = s.px; o[1] = s.py; o[2] = s.pz;
  o[3] = qn[0]; o[4] = qn[1]; o[5] = qn[2]; o[6] = qn[3];
  o[7] = roll; o[8] = pitch; o[9] = yaw;
  o[10] = s.vx; o[11] = s.vy; o[12] = s.vz;
  o[13] = s.ax; o[14] = s.ay; o[15] = s.az;
  o[16] = last[0]; o[17] = last[1]; o[18] = last[2]; o[19] = last[3];
}
// ... stored by the drone's own lane (the kernels whose rows do not go through an LDS tile)
template <typename R>
__device__ __forceinline__ void state20_store(const Drone<R>& s, const R last[4], R* dst) {
  R o[20];
  state20_row(s, last, o);
#pragma unroll
  for (int k = 0; k < 20; ++k) dst[k] = o[k];
}

// A drone's 4 RPMs: one aligned 4*sizeof(R)-byte vector (a row of a [..][N][4] tensor whose base
// the host checked).  STREAM: non-temporal, for a stream read once.
template <typename R, bool STREAM = false>
__device__ __forceinline__ void load_rpm4(const R* src, R out[4]) {
  typedef double gpd_d2 __attribute__((ext_vector_type(2)));
  typedef float gpd_f4 __attribute__((ext_vector_type(4)));
  if (sizeof(R) == 8) {
    gpd_d2 a, b;
    if (STREAM) {
      a = __builtin_nontemporal_load(reinterpret_cast<const gpd_d2*>(src));
      b = __builtin_nontemporal_load(reinterpret_cast<const gpd_d2*>(src) + 1);
    } else {
      a = reinterpret_cast<const gpd_d2*>(src)[0];
      b = reinterpret_cast<const gpd_d2*>(src)[1];
    }
    out[0] = (R)a.x; out[1] = (R)a.y; out[2] = (R)b.x; out[3] = (R)b.y;
  } else {
    const gpd_f4 a = STREAM ? __builtin_nontemporal_load(reinterpret_cast<const gpd_f4*>(src))
                            : *reinterpret_cast<const gpd_f4*>(src);
    out[0] = (R)a.x; out[1] = (R)a.y; out[2] = (R)a.z; out[3] = (R)a.w;
  }
}

}  // namespace gpd
