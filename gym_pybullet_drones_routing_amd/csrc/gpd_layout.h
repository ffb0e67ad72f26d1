// gpd_layout.h — what every launch-level kernel shares: the HBM layout's views (SimView, StepIO;
// the layout itself is described at the head of gpd_kernels.h) and index functions, the drone
// loads and stores with their cache policies, the phase-stamp macros (GPD_STAMPS builds) and the
// LDS synchronisation helpers.  Needs Drone / Consts (gpd_device.h) and the action types
// (gpd_ctrl.h).
#pragma once
#include <type_traits>
#include "gpd_ctrl.h"
#include "gpd_device.h"

namespace gpd {

constexpr int kStateComps = 20;

// The step and integrate kernels put no minimum-waves-per-SIMD constraint (amdgpu_waves_per_eu)
// on the register allocation: forcing 4 waves on the integrate kernel spills to scratch and
// measured slower (scripts/ab_raw.sh).
constexpr int kWave = 64;
constexpr int kPad = kWave + 1;  // tile column stride (elements)

enum : int { TASK_NONE = 0, TASK_HOVER = 1, TASK_MULTIHOVER = 2 };

// Diagnostic build only (-DGPD_STAMPS, libgpd_stamps.so): lane 0 of every block records the
// shader clock at phase boundaries of step_kernel into g_stamps[block][phase].  The shipped
// library executes no stamp.
#ifdef GPD_STAMPS
constexpr int kStampPhases = 88;   // 0..10 shader clocks; 11 / 12: s_memrealtime (100 MHz) at entry / end;
                                   // 13: rate / io wave end (realtime); 14..16: HW_ID of waves 0..2;
                                   // 17..23: io wave phases (shader clocks);
                                   // 24 + 16 w + k: hand-off barrier k < 16 of step_kernel_duo (shader clocks),
                                   // w = 0 / 1 the rate wave's arrival / release, 2 / 3 the pose wave's
__device__ unsigned long long g_stamps[65536 * kStampPhases];
#define GPD_STAMP(k)                                                                      \
  do {                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    unsigned long long t_;                                                                \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");            \
    if (threadIdx.x == 0 && blockIdx.x < 65536) g_stamps[blockIdx.x * kStampPhases + (k)] = t_; \
    __builtin_amdgcn_sched_barrier(0);                                                    \
  } while (0)
#define GPD_RSTAMP(k)                                                                     \
  do {                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    unsigned long long t_;                                                                \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");        \
    if (threadIdx.x == 0 && blockIdx.x < 65536) g_stamps[blockIdx.x * kStampPhases + (k)] = t_; \
    __builtin_amdgcn_sched_barrier(0);                                                    \
  } while (0)
#define GPD_IOSTAMP(k)                                                                    \
  do {                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();                           \
    if (tid == 0 && blockIdx.x < 65536) g_stamps[blockIdx.x * kStampPhases + 17 + (k)] = t_; \
    __builtin_amdgcn_sched_barrier(0);                                                    \
  } while (0)
// (lane 0 of the calling wave; the arrival stamp sits in front of lds_barrier's own lgkmcnt(0))
#define GPD_HSTAMP(w, k)                                                                  \
  do {                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();                           \
    if (tid == 0 && blockIdx.x < 65536 && (k) < 16)                                       \
      g_stamps[blockIdx.x * kStampPhases + 24 + 16 * (w) + (k)] = t_;                     \
    __builtin_amdgcn_sched_barrier(0);                                                    \
  } while (0)
#else
#define GPD_HSTAMP(w, k) do {} while (0)
#define GPD_IOSTAMP(k) do {} while (0)
#define GPD_STAMP(k) do {} while (0)
#define GPD_RSTAMP(k) do {} while (0)
#endif

// Write-through (sc1) stores through a buffer resource.  Every launch ends with a release that
// writes the XCD L2's dirty lines back; rows stored write-through are already on their way to
// memory when the wave stores them, so less of that write-back is left for the kernel's end.
typedef int gpd_v4i __attribute__((ext_vector_type(4)));
typedef unsigned gpd_v2u __attribute__((ext_vector_type(2)));
typedef int gpd_v2i __attribute__((ext_vector_type(2)));
typedef float gpd_v4f __attribute__((ext_vector_type(4)));
// Cache policies of the step kernel's streams: the default one for cache-resident batches (the
// state, ring and rows of the last step are re-read from L2 / Infinity Cache), and STREAM for
// batches far past the 256 MB Infinity Cache: nt (nontemporal) on the state loads and the
// history LDS-DMA, sc1|nt on the write-through stores.  Measured (scripts/large_n_ab2.sh,
// profiles/r3/large_n_ab_nt.log, U[-1,1] actions): 1M envs 194 -> 145 us, 4M envs 780 -> 608 us;
// at 4096 envs the same bits cost 4.93 -> 6.31 us, hence the size-dependent choice (gpd.hip).
constexpr int kAuxWt = 16 /* sc1: write-through */, kAuxWtStream = 18, kAuxDmaStream = 2;
template <int AUX = kAuxWt>
__device__ __forceinline__ void store_wt(__amdgpu_buffer_rsrc_t r, int off, float4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gpd_v4i, v), r, off, 0, AUX);
}
template <int AUX = kAuxWt>
__device__ __forceinline__ void store_wt(__amdgpu_buffer_rsrc_t r, int off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, off, 0, AUX);
}
template <int AUX = kAuxWt>
__device__ __forceinline__ void store_wt(__amdgpu_buffer_rsrc_t r, int off, double v) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(gpd_v2u, v), r, off, 0, AUX);
}

typedef __attribute__((address_space(3))) void* lds_void_ptr;
typedef __attribute__((address_space(1))) void* gbl_void_ptr;
#define gpd_global __attribute__((address_space(1)))

// Downwash work split for blocks with idle lanes: with n > 0, the block's n = tpb*D drone
// pairs are spread over all 64 lanes (pair k: drone k/D of the block, neighbour k%D of its
// env), each force goes to LDS, and the drone's lane sums its D forces in the reference's
// order.  k/D = (k*dmagic) >> 20 (host-checked for k < n).
struct DwPairs {
  int n, dmagic;
};
constexpr int kPairMax = 256;

template <typename R>
struct SimView {
  R* state;               // [npad/64][20][64]
  R* ctrl;                // [npad/64][9][64] DSLPIDControl state (PID action types only, else null)
  float* ring;            // [npad/64][ring_len][64*A]
  int2* ctr;              // [E] {step_counter, ring head}
  const R* init;          // [D][10]
  const R* target;        // [D][3]
  long long npad;         // drones rounded up to whole 64-drone tiles
  int N, D, A, W, tpb, ring_len;
  int task, autoreset, trunc_sc;
  int wt;                 // write-through stores: bit 0 obs/terminal rows, bit 1 state (see store_wt);
                          // bit 2: last_clipped_action lives in the ring (store_drone_step)
  int nc_magic;           // floor(t / NC) == (t * nc_magic) >> 16 for 0 <= t < 64 (host-checked)
  DwPairs dw_pairs;       // downwash pair split (n = 0: one lane per drone loops over its env)
  R bound_xy;             // 1.5 (Hover) or 2.0 (MultiHover)
  // drone <-> drone contact (PYB*, D > 1; DcPairs): pairs per env D(D-1)/2 (0 = off), p / P magic,
  // the [P] pair table, the per-block row store for pairs past the first 64 of a block
  int dcP, dc_pmagic;
  const int* dc_tab;
  void* dc_rows;
  long long dc_row_stride;   // row-store reals per block
};

template <typename R>
struct StepIO {
  const float* actions;   // [N][A]
  float* obs;             // [N][W]
  float* reward;          // [E]
  uint8_t* term;          // [E]
  uint8_t* trunc;         // [E]
  float* terminal_obs;    // [N][W] or null
};

// Tiled SoA: component k of drone n lives at tile(n) * C*64 + k*64 + lane(n).  Every wave
// load / store of one component is still 64 consecutive elements, while each 64-drone tile's
// state (and history) is one contiguous stretch of HBM: a block streams a few large runs
// instead of one 512-B run from each of 20 (+14) widely separated arrays.
__host__ __device__ __forceinline__ long long tidx(long long n, int k, int C) {
  return (n >> 6) * (64LL * C) + k * 64 + (n & 63);
}
// ring slot `slot` of drone n (units of float, A floats per drone)
__host__ __device__ __forceinline__ long long ridx(long long n, int slot, int L, int A) {
  return ((n >> 6) * L + slot) * (64LL * A) + (n & 63) * A;
}

// Only what the dynamics reads: ang_v is write-only, last_clipped_action is read only by drag.
template <bool NT, typename R>
__device__ __forceinline__ R ldst(const R* p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}
template <typename R, bool NT = false>
__device__ __forceinline__ void load_drone(const SimView<R>& v, long long n, Drone<R>& s, R last[4], bool need_last) {
  const R* st = v.state + tidx(n, 0, kStateComps);
  s.px = ldst<NT>(st + 0 * 64); s.py = ldst<NT>(st + 1 * 64); s.pz = ldst<NT>(st + 2 * 64);
  s.qx = ldst<NT>(st + 3 * 64); s.qy = ldst<NT>(st + 4 * 64); s.qz = ldst<NT>(st + 5 * 64); s.qw = ldst<NT>(st + 6 * 64);
  s.vx = ldst<NT>(st + 7 * 64); s.vy = ldst<NT>(st + 8 * 64); s.vz = ldst<NT>(st + 9 * 64);
  s.wx = ldst<NT>(st + 10 * 64); s.wy = ldst<NT>(st + 11 * 64); s.wz = ldst<NT>(st + 12 * 64);
  s.ax = s.ay = s.az = R(0);
  if (need_last) {
    last[0] = st[16 * 64]; last[1] = st[17 * 64]; last[2] = st[18 * 64]; last[3] = st[19 * 64];
  } else {
    last[0] = last[1] = last[2] = last[3] = R(0);
  }
}

template <typename R>
__device__ __forceinline__ void load_drone_full(const SimView<R>& v, long long n, Drone<R>& s, R last[4]) {
  load_drone(v, n, s, last, true);
  const R* st = v.state + tidx(n, 0, kStateComps);
  s.ax = st[13 * 64]; s.ay = st[14 * 64]; s.az = st[15 * 64];
}

template <typename R, int AUX = kAuxWt>
__device__ __forceinline__ void store_drone_wt(const SimView<R>& v, long long n, const Drone<R>& s, const R last[4]) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(v.state, 0, (int)(kStateComps * v.npad * (long long)sizeof(R)), 0x00020000);
  int o = (int)(tidx(n, 0, kStateComps) * sizeof(R));
  const R vals[20] = {s.px, s.py, s.pz, s.qx, s.qy, s.qz, s.qw, s.vx, s.vy, s.vz,
                      s.wx, s.wy, s.wz, s.ax, s.ay, s.az, last[0], last[1], last[2], last[3]};
  const bool skip_last = (v.wt & 4) != 0;   // store_drone_step
#pragma unroll
  for (int k = 0; k < 20; ++k, o += 64 * (int)sizeof(R))
    if (k < 16 || !skip_last) store_wt<AUX>(r, o, vals[k]);
}

template <typename R, bool NT = false>
__device__ __forceinline__ void store_drone(const SimView<R>& v, long long n, const Drone<R>& s, const R last[4]) {
  R* st = v.state + tidx(n, 0, kStateComps);
  const R vals[20] = {s.px, s.py, s.pz, s.qx, s.qy, s.qz, s.qw, s.vx, s.vy, s.vz,
                      s.wx, s.wy, s.wz, s.ax, s.ay, s.az, last[0], last[1], last[2], last[3]};
#pragma unroll
  for (int k = 0; k < 20; ++k) {
    if (NT) __builtin_nontemporal_store(vals[k], st + k * 64);
    else st[k * 64] = vals[k];
  }
}

// The step kernels' state store.  With SimView::wt bit 2 (RPM / ONE_D_RPM action types without
// drag, where nothing in the step reads it) last_clipped_action is not stored: it equals
// action_to_rpm of the ring's newest slot, or 0 in an env that has not stepped since its reset,
// and last_from_ring_kernel writes it back before any reader of state[16..19] (32 B per drone
// and step less HBM traffic in f64).  The kernel marks that with ctr[E].x = 1 (mark_last_in_ring).
template <typename R, int AUX = kAuxWt>
__device__ __forceinline__ void store_drone_step(const SimView<R>& v, long long n, const Drone<R>& s,
                                                 const R last[4]) {
  if (v.wt & 2) {
    store_drone_wt<R, AUX>(v, n, s, last);
    return;
  }
  R* st = v.state + tidx(n, 0, kStateComps);
  st[0 * 64] = s.px; st[1 * 64] = s.py; st[2 * 64] = s.pz;
  st[3 * 64] = s.qx; st[4 * 64] = s.qy; st[5 * 64] = s.qz; st[6 * 64] = s.qw;
  st[7 * 64] = s.vx; st[8 * 64] = s.vy; st[9 * 64] = s.vz;
  st[10 * 64] = s.wx; st[11 * 64] = s.wy; st[12 * 64] = s.wz;
  st[13 * 64] = s.ax; st[14 * 64] = s.ay; st[15 * 64] = s.az;
  if (!(v.wt & 4)) {
    st[16 * 64] = last[0]; st[17 * 64] = last[1]; st[18 * 64] = last[2]; st[19 * 64] = last[3];
  }
}

// drone 0's lane of a step launch: the state's last_clipped_action columns are stale from here on.
// ctr[E] has a second writer: the command step (unmark_last_in_ring, gpd_step_cmd.h) stores the
// columns itself and clears the mark in-kernel, relying on the same invariant as this one: the mark
// is only ever set on sims whose steps read no last_clipped_action (wt bit 2: RPM types, no drag).
template <typename R>
__device__ __forceinline__ void mark_last_in_ring(const SimView<R>& v, long long n) {
  if ((v.wt & 4) && n == 0) v.ctr[v.N / v.D] = make_int2(1, 0);
}

// step_kernel_duo's forms of the two above: the drone's state address (st = v.state + tidx(n, 0,
// kStateComps), o its byte offset for the write-through form) and the ctr slot come from the
// caller, which forms them ahead of its final barrier.  Its envs are single drones, so the slot
// N / D is N.  (Separate functions: the other kernels' code stays as it was.)
template <typename R, int AUX = kAuxWt, typename P = R*>
__device__ __forceinline__ void store_drone_step_at(const SimView<R>& v, P st, int o, const Drone<R>& s,
                                                    const R last[4]) {
  if (v.wt & 2) {
    const __amdgpu_buffer_rsrc_t r =
        __builtin_amdgcn_make_buffer_rsrc(v.state, 0, (int)(kStateComps * v.npad * (long long)sizeof(R)), 0x00020000);
    const R vals[20] = {s.px, s.py, s.pz, s.qx, s.qy, s.qz, s.qw, s.vx, s.vy, s.vz,
                        s.wx, s.wy, s.wz, s.ax, s.ay, s.az, last[0], last[1], last[2], last[3]};
    const bool skip_last = (v.wt & 4) != 0;
#pragma unroll
    for (int k = 0; k < 20; ++k, o += 64 * (int)sizeof(R))
      if (k < 16 || !skip_last) store_wt<AUX>(r, o, vals[k]);
    return;
  }
  st[0 * 64] = s.px; st[1 * 64] = s.py; st[2 * 64] = s.pz;
  st[3 * 64] = s.qx; st[4 * 64] = s.qy; st[5 * 64] = s.qz; st[6 * 64] = s.qw;
  st[7 * 64] = s.vx; st[8 * 64] = s.vy; st[9 * 64] = s.vz;
  st[10 * 64] = s.wx; st[11 * 64] = s.wy; st[12 * 64] = s.wz;
  st[13 * 64] = s.ax; st[14 * 64] = s.ay; st[15 * 64] = s.az;
  if (!(v.wt & 4)) {
    st[16 * 64] = last[0]; st[17 * 64] = last[1]; st[18 * 64] = last[2]; st[19 * 64] = last[3];
  }
}
template <typename R>
__device__ __forceinline__ void mark_last_in_ring_single(const SimView<R>& v, long long n) {
  if ((v.wt & 4) && n == 0) v.ctr[v.N] = make_int2(1, 0);
}

// |target - pos|^2 of step_kernel_duo's task hook: tx*tx + ty*ty + tz*tz in the very operations
// the compiler has contracted it to in that kernel (f64: two chained fmas on ty*ty; f32: one
// fma and a rounded tz*tz), written out so that a change of the code around it cannot change
// how the sum is contracted, and with it the reward's last bit.  (The one-wave step_kernel keeps
// the plain expression; should a compiler contract that one differently, the kernel-form tests of
// tests/test_gpu_parity.py and tests/test_gpu_step_tail.py compare the rewards to a tolerance, and
// `bench.py --dump-outputs` of two builds shows the last bit.)
__device__ __forceinline__ double hover_d2(double tx, double ty, double tz) {
#pragma clang fp contract(off)
  return __builtin_fma(tz, tz, __builtin_fma(tx, tx, ty * ty));
}
__device__ __forceinline__ float hover_d2(float tx, float ty, float tz) {
#pragma clang fp contract(off)
  return __builtin_fmaf(ty, ty, tx * tx) + tz * tz;
}

// Workgroup barrier for LDS exchanges within a block (between its waves, or its lanes): waits for this wave's own
// LDS operations only.  __syncthreads() (a workgroup release fence) would also wait for every
// vector-memory operation in flight, including an LDS-DMA that nobody reads until much later.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// A wave-uniform pointer the compiler formed with vector instructions (a 64-bit multiply), back
// in scalar registers.
template <typename T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
  const unsigned long long x = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)x), hi = __builtin_amdgcn_readfirstlane((unsigned)(x >> 32));
  return (T*)(((unsigned long long)hi << 32) | lo);
}

// LDS exchange among the lanes of ONE wave (the step / integrate kernels' blocks are one wave):
// a wave's LDS instructions execute in order, so a later ds_read sees an earlier ds_write of
// any lane without a wait or a hardware barrier; the fence only keeps the compiler from
// reordering the accesses.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

}  // namespace gpd
