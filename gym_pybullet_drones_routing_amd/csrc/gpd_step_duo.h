// gpd_step_duo.h — step_kernel_duo and its helpers: the bench path's step (single-drone envs,
// plain DYN, RPM action types) with a drone's work split over two or three waves of a workgroup.
// Needs the layout, stores and lds_barrier of gpd_layout.h, tile_copy_out (gpd_step.h) and the
// rate / pose halves of a substep (gpd_device.h).
#pragma once
#include "gpd_step.h"

namespace gpd {

// ---------------------------------------------------------------------------------------
// step_kernel_duo: step_kernel<R, ACT, false, true> (single-drone envs, plain DYN, RPM action
// types: the bench path) with every drone's work split over TWO waves of one workgroup.
// With few envs per CU (4096 envs: one 16-drone wave per CU) a launch lasts as long as one
// wave's serial instruction stream, and a substep is ~115 issue-bound f64 instructions.
// Without aero terms it falls into two chains (rate_half / pose_half, gpd_device.h):
//   wave 1 (rates): ω' and the _integrateQ weights, handed over through LDS;
//   wave 0 (pose):  readback, v, p, and the quaternion update with those weights.
// One barrier per substep; the hand-off is double-buffered by substep parity, so wave 1
// computes substep k+1 while wave 0 finishes substep k.  Wave 1 also issues the history DMA
// behind its last substep (it lands while wave 0 finishes) and writes the current action (ring
// + tile); both waves stream the tile copy-out.  (Moving the final Euler angles to wave 1 as
// well measured slower: 5.56 -> 5.89 us at 4096 envs.)  Same operations as step_kernel<R, ACT, false, true>; results agree to
// rounding (tests/test_gpu_parity.py::test_duo_kernel_matches_single_wave).
// IO = true adds a third wave ("io wave") that writes the action-history columns of the
// observation rows (83 % of a row's bytes, independent of the physics: ring slots head+1.. and
// the current action) WHILE the pose / rate waves integrate, and appends the action to the
// ring.  The pose wave then stores only the 12 state columns of its rows straight from
// registers, so the LDS observation tile and its copy-out leave the critical path.
// Of the phases of gpd_step_parts.h the ring append, the terminal-row store and the reset are
// calls; the action load, the final readback and the tile fill stay written out, for the reason
// given at step_kernel (gpd_step.h).  The history DMAs and the hover terms are this kernel's own.
// step_seq_kernel (gpd_step_seq.h) runs the same waves for many steps per launch.  It shares
// pose_half and the rate pieces; the io wave's mapping, store and terminal passes, the hover hook,
// action -> wrench and the look-ahead rate loop are also written there: each was tried as one
// helper for both kernels and changed this kernel's instructions
// (profiles/step_seq_shared/README.md).  A fix to one of them goes to gpd_step_seq.h too.
// Two phases differ there on purpose (profiles/step_seq_rows/README.md): the pose wave's action ->
// thrust (the rate chains publish it) and the row's state columns with reward and flags (the io wave
// makes and stores them from what the pose wave publishes).  A change to obs_euler_f32 or
// rate_weights goes to seq_obs_euler_f32 / seq_rate_weights in gpd_step_seq.h too.
template <typename R, int ACT, bool IO>
__global__ __launch_bounds__(IO ? 3 * kWave : 2 * kWave) void step_kernel_duo(R* __restrict__ state_p,
                                                             const float* __restrict__ actions_p,
                                                             int2* __restrict__ ctr_p, const Consts<R>* __restrict__ cp,
                                                             long long npad_p, int n_p, int tpb_p, SimView<R> v,
                                                             StepIO<R> io) {
  static_assert(!act_is_pid(ACT), "the duo kernel serves the RPM action types");
  v.state = state_p; v.ctr = ctr_p; v.npad = npad_p; v.N = n_p; v.tpb = tpb_p;
  io.actions = actions_p;
  constexpr int A = act_width(ACT);
  // The f64 kernels run the substep loop in the order described at the two waves below.  The f32
  // kernels keep the plain order: hipcc packs and contracts the moved f32 expressions differently,
  // which changes last bits of their results.
  constexpr bool kAhead = sizeof(R) == 8;
  extern __shared__ float4 tile4[];
  float* tilef = reinterpret_cast<float*>(tile4);
  __shared__ R shand[2][5][kWave];        // rate_half -> pose_half, by substep parity
  __shared__ R sw[3][kWave];              // rpy_rates after the last substep
  __shared__ unsigned long long sdone;    // done-row mask of the block (tile rows)
  GPD_RSTAMP(11);
  GPD_STAMP(0);
  const Consts<R>& c = *cp;
  const int tid = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x) / kWave;   // wave-uniform
  const bool rate_wave = wave == 1;
  const long long n0 = (long long)blockIdx.x * v.tpb;
  const long long n = n0 + tid;
  const int nact = (int)((v.N - n0) < v.tpb ? (v.N - n0) : v.tpb);
  const bool active = tid < nact;
  const long long nn = active ? n : n0;  // inactive lanes compute on the block's first drone, store nothing
#ifdef GPD_STAMPS
  {   // diagnostic: which SIMD / CU each wave of the block runs on (HW_ID: SIMD_ID bits 5:4)
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);
    if (tid == 0 && blockIdx.x < 65536) g_stamps[blockIdx.x * kStampPhases + 14 + wave] = hw;
  }
#endif

  if (IO && wave == 2) {
    // ------------------------------------------------------------ wave 2: history columns
    // The history columns of a row are ring slots head+1 .. head+L-1 (oldest first,
    // BaseRLAviary.py:307-319) and the current action.  The wave appends the action to the
    // ring and the tile, follows the pose/rate waves' hand-off barriers, then DMAs the ring
    // slots into the tile and streams the tile, transposed (conflict-free thanks to the column
    // pad), into the rows' history columns with coalesced stores - beside the pose wave's last
    // substep and epilogue, which then stores only the 12 state columns.  The tile stays for
    // the terminal rows of envs that finish, known after the final barrier.
    const int L = v.ring_len;
    const int nsub = c.nsub;
    const int2 cv = v.ctr[nn];
    const int hd = cv.y;                          // ring slot receiving this step's action
    float a[A];
    if (A == 4) {
      const float4 a4 = *reinterpret_cast<const float4*>(io.actions + nn * 4);
      a[0] = a4.x; a[1] = a4.y; a[2] = a4.z; a[3] = a4.w;
    } else {
      a[0] = io.actions[nn];
    }
    // The current action goes into its tile column BEFORE the DMA is issued: a ds_write after
    // an LDS-DMA in flight makes the compiler wait for the whole DMA (vmcnt(0)) first.
    if (A == 4) tile4[(L - 1) * kPad + tid] = make_float4(a[0], a[1], a[2], a[3]);
    else tilef[(L - 1) * kPad + tid] = a[0];
    if (active) ring_append<A>(v.ring, n, hd, L, a);   // deque.append; the DMA never reads slot `head`
    // Everything the tail needs that does not depend on the DMA'd data is formed in the slack
    // the wave has at the hand-off barriers (its tail is the end of the block's critical path)
    // and pinned in registers across them:
    //   * the DMA source of a lane as a 32-bit byte offset on a wave-uniform base (the block's
    //     first 64-drone tile), stepped slot by slot with an add and a wrap;
    //   * for the common case of a block whose nact * L elements fit one pass of U per lane
    //     (`fits`): each element's LDS address, row and store offset;
    //   * the rows' buffer base and size.
    // Behind the last hand-off only m0 + global_load_lds per slot remain, behind vmcnt(0) only
    // the LDS reads and the stores.  Where it runs: the wave is the block's last to start and must
    // not be late at hand-off 0 (all of it in front of that barrier measured slower than no change,
    // profiles/r7/step_tail/), so one half runs behind hand-off 0 and the other behind hand-off 1,
    // each well inside a substep of the pose / rate waves.
    constexpr int U = 4;                          // elements per lane in flight per pass
    constexpr int EB = A == 4 ? 16 : 4;           // bytes of a tile element
    constexpr unsigned kSlotBytes = 64u * A * 4u; // one ring slot of a 64-drone tile
    const int total = nact * L;
    const int NC = A == 4 ? 3 + L : v.W;          // row stride in elements
    const int c0 = A == 4 ? 3 : 12;               // first history column
    const float rL = 1.0f / (float)L;             // (g + 0.5) / L: exact row index for g < 2^12
    const bool fits = total <= U * kWave;
    const bool wt_rows = (v.wt & 1) != 0;
    float* dst0;
    int nrec;
    const char* ring0;
    unsigned dma_lo, dma_hi, dma_cur;
    int off[U], row[U];
    lds_void_ptr la[U];
    // (lane, drone: opaque copies taken where a part runs, or the scheduler hoists the part's
    // arithmetic above the barrier in front of it)
    auto map_elem = [&](int u, int lane) {
      // an element past the end gets an offset past num_records, so the buffer unit drops its store
      const int g = lane + u * kWave;
      const bool ok = g < total;
      const int gg = ok ? g : total - 1;
      const int i = (int)(((float)gg + 0.5f) * rL), k = gg - i * L;
      row[u] = i;
      off[u] = ok ? (i * NC + c0 + k) * EB : nrec;
      la[u] = A == 4 ? (lds_void_ptr)(tile4 + (__umul24(k, kPad) + i)) : (lds_void_ptr)(tilef + (__umul24(k, kPad) + i));
    };
    auto pre_a = [&]() {
      int lane = tid;
      long long drone = nn;
      asm volatile("" : "+v"(lane), "+v"(drone));
      dst0 = uniform_ptr(io.obs + n0 * v.W);
      nrec = __builtin_amdgcn_readfirstlane(nact * v.W * 4);
      ring0 = uniform_ptr(reinterpret_cast<const char*>(v.ring + (n0 >> 6) * L * (64LL * A)));
      dma_lo = (unsigned)((((drone >> 6) - (n0 >> 6)) * L * 64 + (drone & 63)) * (A * 4));
      dma_hi = dma_lo + (unsigned)L * kSlotBytes;
      dma_cur = dma_lo + (unsigned)(hd + 1 == L ? 0 : hd + 1) * kSlotBytes;
      map_elem(0, lane);
      map_elem(1, lane);
      asm volatile("" : "+v"(dma_lo), "+v"(dma_hi), "+v"(dma_cur), "+v"(off[0]), "+v"(off[1]), "+v"(row[0]), "+v"(row[1]),
                   "+v"(la[0]), "+v"(la[1]), "+s"(ring0), "+s"(dst0), "+s"(nrec));
      // (the pinned scalars read back as wave-uniform, or the stores would loop over "distinct" bases)
      dst0 = uniform_ptr(dst0);
      nrec = __builtin_amdgcn_readfirstlane(nrec);
    };
    auto pre_b = [&]() {
      int lane = tid;
      asm volatile("" : "+v"(lane));
      map_elem(2, lane);
      map_elem(3, lane);
      asm volatile("" : "+v"(off[2]), "+v"(off[3]), "+v"(row[2]), "+v"(row[3]), "+v"(la[2]), "+v"(la[3]));
    };
    // This wave publishes nothing to the others, so its barriers skip lds_barrier's
    // lgkmcnt(0) wait: an LDS-DMA in flight holds that counter until it lands.
    // (an LDS-counter hand-off between the pose and rate waves, which would free this wave of
    // their barriers, measured 5.3 / 6.4 us against 4.9: profiles/r6/duo_flags/)
    GPD_IOSTAMP(0);
    asm volatile("s_barrier" ::: "memory");       // hand-off 0
    GPD_IOSTAMP(1);
    pre_a();
    if (nsub > 1) asm volatile("s_barrier" ::: "memory");   // hand-off 1
    pre_b();
    for (int k = 2; k < nsub; ++k) asm volatile("s_barrier" ::: "memory");   // hand-offs 2 .. nsub-1
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(dst0, 0, nrec, 0x00020000);
    auto tile_read4 = [&](int u) {
      return __builtin_bit_cast(float4, *(const __attribute__((address_space(3))) gpd_v4f*)la[u]);
    };
    auto tile_read1 = [&](int u) { return *(const __attribute__((address_space(3))) float*)la[u]; };
    // history ring -> tile (LDS-DMA) behind the last hand-off: an LDS-DMA in flight while the
    // pose / rate waves still exchange hand-offs slowed their substeps by ~850 cycles per launch
    // (phase stamps, 4096 envs), issued here it lands beside the pose wave's last substep and
    // epilogue.  Slot head+1+m of every drone of the block -> tile column m (one coalesced
    // 64-drone run per slot, lane-contiguous in LDS).
    for (int m = 0; m < L - 1; ++m) {
      const char* src = ring0 + dma_cur;
      if (A == 4) __builtin_amdgcn_global_load_lds((gbl_void_ptr)src, (lds_void_ptr)(tile4 + m * kPad), 16, 0, 0);
      else __builtin_amdgcn_global_load_lds((gbl_void_ptr)src, (lds_void_ptr)(tilef + m * kPad), 4, 0, 0);
      dma_cur += kSlotBytes;
      dma_cur = dma_cur == dma_hi ? dma_lo : dma_cur;
    }
    GPD_IOSTAMP(2);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA has landed in its tile
    GPD_IOSTAMP(3);
    // (the fits pass keeps its elements in registers for the terminal rows: an LDS read behind
    // the stores would make the compiler wait for every store in flight first)
    float4 v4[U];
    float v1[U];
    if (fits) {
      // one pass: LDS reads, then stores, both at the addresses formed at the hand-offs
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (A == 4) v4[u] = tile_read4(u);
        else v1[u] = tile_read1(u);
      }
      if (wt_rows) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (A == 4) store_wt(rsrc, off[u], v4[u]);
          else store_wt(rsrc, off[u], v1[u]);
        }
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (A == 4) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gpd_v4i, v4[u]), rsrc, off[u], 0, 0);
          else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v1[u]), rsrc, off[u], 0, 0);
        }
      }
    }
    // longer histories: U elements per lane in flight per pass, the mapping formed per pass
    for (int g0 = fits ? total : tid; g0 < total; g0 += U * kWave) {
      int poff[U];
      float4 p4[U];
      float p1[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int g = g0 + u * kWave;
        const bool ok = g < total;
        const int gg = ok ? g : total - 1;
        const int i = (int)(((float)gg + 0.5f) * rL), k = gg - i * L;
        const int e = i * NC + c0 + k;
        poff[u] = ok ? e * (A == 4 ? 16 : 4) : nact * v.W * 4;
        if (A == 4) p4[u] = tile4[__umul24(k, kPad) + i];
        else p1[u] = tilef[__umul24(k, kPad) + i];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (v.wt & 1) {
          if (A == 4) store_wt(rsrc, poff[u], p4[u]);
          else store_wt(rsrc, poff[u], p1[u]);
        } else {
          if (A == 4) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gpd_v4i, p4[u]), rsrc, poff[u], 0, 0);
          else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, p1[u]), rsrc, poff[u], 0, 0);
        }
      }
    }
    GPD_IOSTAMP(4);
    lds_barrier();     // final: sdone published by the pose wave
    GPD_IOSTAMP(5);
    const unsigned long long dr = sdone;
    if (dr) {
      float* const tdst = io.terminal_obs + n0 * v.W;
      if (fits) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (tid + u * kWave < total && ((dr >> row[u]) & 1ull)) {
            char* const t = reinterpret_cast<char*>(tdst) + off[u];
            if (A == 4) *reinterpret_cast<float4*>(t) = v4[u];
            else *reinterpret_cast<float*>(t) = v1[u];
          }
        }
      }
      for (int g = fits ? total : tid; g < total; g += kWave) {
        const int i = (int)(((float)g + 0.5f) * rL), k = g - i * L;
        if ((dr >> i) & 1ull) {
          const int e = i * NC + c0 + k;
          if (A == 4) reinterpret_cast<float4*>(tdst)[e] = tile4[__umul24(k, kPad) + i];
          else tdst[e] = tilef[__umul24(k, kPad) + i];
        }
      }
    }
#ifdef GPD_STAMPS
    {   // diagnostic: the io wave's end (realtime) into phase 13
      __builtin_amdgcn_sched_barrier(0);
      unsigned long long t_;
      asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");
      if (tid == 0 && blockIdx.x < 65536) g_stamps[blockIdx.x * kStampPhases + 13] = t_;
    }
#endif
    return;
  }

  float a[A];
  if (A == 4) {
    const float4 a4 = *reinterpret_cast<const float4*>(io.actions + nn * 4);
    a[0] = a4.x; a[1] = a4.y; a[2] = a4.z; a[3] = a4.w;
  } else {
#pragma unroll
    for (int j = 0; j < A; ++j) a[j] = io.actions[nn * A + j];
  }
  const R* st = v.state + tidx(nn, 0, kStateComps);
  // each wave issues its state loads first and only then pins the step's constants into VGPRs
  // (dyn_consts waits for the scalar loads): one exposed memory round trip, not two

  if (rate_wave) {
    // ------------------------------------------------------------ wave 1: body rates
    R wx = st[10 * 64], wy = st[11 * 64], wz = st[12 * 64];
    const int head = v.ctr[nn].y;
    DynK<R> dk = dyn_consts(c);   // the ring fields are first needed after the substeps
    const int nsub = dk.nsub, nh = v.ring_len - 1;
    const int NC = A == 4 ? 3 + v.ring_len : 12 + v.ring_len * A;
    R rpm[4], W[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) rpm[k] = (R)action_to_rpm(dk.hover_f32, a[A == 4 ? k : 0]);
    rpm_wrench<R, 0>(rpm, dk, c, W);
    if constexpr (kAhead) {
      // The recurrence runs one substep ahead of its weights.  Only ω_{k+1} -> ω_{k+2} (6 levels)
      // feeds the next substep; the weights of ω_{k+1} (9 levels) feed only the hand-off.  So the
      // wave publishes the weights first and runs the recurrence behind the LDS writes, on their
      // way to the barrier, where it covers the write acknowledgement.  The cost is at hand-off 0,
      // which two recurrence steps now precede: the rate wave reaches it ~200 cycles later (stamps:
      // 1 975 against 1 774) and the pose wave waits 270 there.  Hand-offs 1..6 come 15-30 cycles
      // sooner each and the last one, which no longer holds a recurrence, 240 sooner (536 against
      // 780 cycles), so hand-off 7 is reached ~100 cycles earlier.  (The two chains interleaved in
      // one block in front of the writes measured no gain: profiles/r8/substep_schedule/.)  The
      // last substep has no look-ahead: sw[] receives ω_nsub, no step past nsub is evaluated.
      rate_recur(wx, wy, wz, W, dk);   // ω_1
      for (int k = 0; k < nsub - 1; ++k) {
        R h[5], n2;
        const R cx = wx, cy = wy, cz = wz;   // ω_{k+1}
        const bool big = rate_weights(cx, cy, cz, dk, h, n2);
        rate_weights_big(big, n2, dk, h);
#pragma unroll
        for (int j = 0; j < 5; ++j) shand[k & 1][j][tid] = h[j];
        rate_recur(wx, wy, wz, W, dk);       // ω_{k+2}
        asm volatile("" : "+v"(wx), "+v"(wy), "+v"(wz));   // (complete in front of the barrier)
        GPD_HSTAMP(0, k);
        lds_barrier();   // hand-off k published
        GPD_HSTAMP(1, k);
      }
      {
        R h[5], n2;
        const bool big = rate_weights(wx, wy, wz, dk, h, n2);
        rate_weights_big(big, n2, dk, h);
#pragma unroll
        for (int j = 0; j < 5; ++j) shand[(nsub - 1) & 1][j][tid] = h[j];
        sw[0][tid] = wx; sw[1][tid] = wy; sw[2][tid] = wz;
        GPD_HSTAMP(0, nsub - 1);
        lds_barrier();   // last hand-off and the final rates published
        GPD_HSTAMP(1, nsub - 1);
      }
    } else {
      for (int k = 0; k < nsub; ++k) {
        R h[5];
        rate_half(wx, wy, wz, W, dk, h);
#pragma unroll
        for (int j = 0; j < 5; ++j) shand[k & 1][j][tid] = h[j];
        if (k == nsub - 1) { sw[0][tid] = wx; sw[1][tid] = wy; sw[2][tid] = wz; }
        GPD_HSTAMP(0, k);
        lds_barrier();   // hand-off k published
        GPD_HSTAMP(1, k);
      }
    }
    if (IO) {          // the io wave owns the history columns and the ring append
      lds_barrier();   // final
      return;
    }
    // history ring -> obs tile (LDS-DMA): issued once the last hand-off is out, it lands while
    // the pose wave finishes its last substep, the final readback and the task hooks.  The
    // env's ring slots are 64*A floats apart in its 64-drone tile.
    {
      const float* rb = v.ring + ridx(nn, 0, v.ring_len, A);
      int slot = head + 1 == v.ring_len ? 0 : head + 1;
      for (int m = 0; m < nh; ++m) {
        const float* src = rb + slot * (64 * A);
        if (A == 4) {
          __builtin_amdgcn_global_load_lds((gbl_void_ptr)src, (lds_void_ptr)(tile4 + (3 + m) * kPad), 16, 0, 0);
        } else {
#pragma unroll
          for (int j = 0; j < A; ++j)
            __builtin_amdgcn_global_load_lds((gbl_void_ptr)(src + j), (lds_void_ptr)(tilef + (12 + m * A + j) * kPad), 4,
                                             0, 0);
        }
        slot = slot + 1 == v.ring_len ? 0 : slot + 1;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // history DMA has landed in the tile
    // current action into the ring (deque.append); the DMA never reads `head`
    if (active) ring_append<A>(v.ring, n, head, v.ring_len, a);
    if (A == 4) {
      tile4[(3 + nh) * kPad + tid] = make_float4(a[0], a[1], a[2], a[3]);
    } else {
#pragma unroll
      for (int j = 0; j < A; ++j) tilef[(12 + nh * A + j) * kPad + tid] = a[j];
    }
    lds_barrier();     // tile complete, sdone published
    tile_copy_out<A, 2 * kWave, 3>(tile4, tilef, threadIdx.x, nact, NC, v.nc_magic, v.wt, sdone, io.obs,
                                io.terminal_obs, n0);
#ifdef GPD_STAMPS
    {   // diagnostic: the rate wave's end (realtime) into phase 13
      __builtin_amdgcn_sched_barrier(0);
      unsigned long long t_;
      asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");
      if (tid == 0 && blockIdx.x < 65536) g_stamps[blockIdx.x * kStampPhases + 13] = t_;
    }
#endif
    return;
  }

  // -------------------------------------------------------------- wave 0: pose
  Drone<R> s;
  R last[4];
  load_drone(v, nn, s, last, false);
  const int2 cv = v.ctr[nn];
  const int sc = cv.x;          // step_counter
  const int head = cv.y;        // ring slot receiving this step's action
  DynK<R> dk = dyn_consts(c, v.task, io.trunc);
  const TailK<R> tk = tail_consts(c, v.bound_xy);
  const int nsub = dk.nsub;
  const int NC = A == 4 ? 3 + v.ring_len : 12 + v.ring_len * A;
  // where the lane's results go: formed here, under the loads, not behind the final barrier
  // (global-address-space pointers: a generic pointer out of the pin would make flat stores)
  gpd_global R* st_out = (gpd_global R*)(v.state + tidx(nn, 0, kStateComps));
  int st_off = (int)(tidx(nn, 0, kStateComps) * sizeof(R));
  gpd_global float* rew_out = (gpd_global float*)(io.reward + nn);
  gpd_global uint8_t* term_out = (gpd_global uint8_t*)(io.term + nn);
  gpd_global uint8_t* trunc_out = (gpd_global uint8_t*)(io.trunc + nn);
  gpd_global gpd_v2i* ctr_out = (gpd_global gpd_v2i*)(v.ctr + nn);
  int head_next = head + 1 == v.ring_len ? 0 : head + 1;
  asm volatile("" : "+v"(st_out), "+v"(st_off), "+v"(rew_out), "+v"(term_out), "+v"(trunc_out), "+v"(ctr_out),
               "+v"(head_next));
#ifdef GPD_STAMPS
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // diagnostic: loads landed
  GPD_STAMP(10);
#endif
  R fz;
  {
    R rpm[4], W[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) rpm[k] = (R)action_to_rpm(dk.hover_f32, a[A == 4 ? k : 0]);
    rpm_wrench<R, 0>(rpm, dk, c, W);
    fz = W[0];
#pragma unroll
    for (int k = 0; k < 4; ++k) last[k] = rpm[k];   // self.last_clipped_action = clipped_action  :372
  }
  const R wnone[3] = {R(0), R(0), R(0)};
  auto hand_off = [&](int k, R h[5]) {
#pragma unroll
    for (int j = 0; j < 5; ++j) h[j] = shand[k & 1][j][tid];
  };
  if (nsub > 1) {
    GPD_HSTAMP(2, 0);
    lds_barrier();   // hand-off 0
    GPD_HSTAMP(3, 0);
    R h[5];
    hand_off(0, h);
    pose_half<R, false, true>(s, fz, h, wnone, dk);
    GPD_STAMP(1);
    for (int k = 1; k < nsub - 1; ++k) {
      GPD_HSTAMP(2, k);
      lds_barrier();   // hand-off k
      GPD_HSTAMP(3, k);
      hand_off(k, h);
      pose_half<R, false, false>(s, fz, h, wnone, dk);
    }
  }
  {
    GPD_HSTAMP(2, nsub - 1);
    lds_barrier();   // last hand-off + final rates
    GPD_HSTAMP(3, nsub - 1);
    R h[5];
    hand_off(nsub - 1, h);
    s.wx = sw[0][tid]; s.wy = sw[1][tid]; s.wz = sw[2][tid];
    const R w[3] = {s.wx, s.wy, s.wz};
    if (nsub > 1) pose_half<R, true, false>(s, fz, h, w, dk);
    else pose_half<R, true, true>(s, fz, h, w, dk);
  }
  GPD_STAMP(2);
  // final readback (:374) -> obs / reward / done
  R qn[4], Rm[9];
  if constexpr (kAhead) readback_fused_rare(s.qx, s.qy, s.qz, s.qw, qn, Rm);
  else readback_fused(s.qx, s.qy, s.qz, s.qw, qn, Rm);
  AttitudeArgs<R> att = attitude_args(qn);
  bool tilted, up_unused;   // |roll| or |pitch| > 0.4, decided exactly near the limit (attitude_decide)
  attitude_decide<R, true, false>(s.qx, s.qy, s.qz, s.qw, att, tilted, up_unused);
  float roll, pitch, yaw;
  obs_euler_f32(qn, att, roll, pitch, yaw);
  float reward = -1.0f;
  bool term = false, trunc = false;
  if (v.task != TASK_NONE) {
    const R tx = tk.tg[0] - s.px, ty = tk.tg[1] - s.py, tz = tk.tg[2] - s.pz;
    const R d2 = hover_d2(tx, ty, tz);
    R r = R(2) - d2 * d2;
    r = r > R(0) ? r : R(0);
    const bool oob = g_abs(s.px) > tk.bound_xy || g_abs(s.py) > tk.bound_xy || s.pz > R(2) || tilted;
    reward = (float)r;
    // np.linalg.norm(...) < .0001 (HoverAviary.py:92).  A squared distance more than 1 % away
    // from 1e-8 decides it (its root is then 0.5 % away from 1e-4, far beyond any rounding of
    // the root); only a wave with a lane inside that band takes the square root, so the result
    // is the root's comparison in every case and the 16-instruction dependent f64 root leaves
    // the epilogue.
    term = d2 < R(0.99e-8);
    const bool band = !(d2 < R(0.99e-8)) && !(d2 > R(1.01e-8));   // a NaN goes the root's way, too
    if (GPD_RARE(__ballot(band) != 0ull)) term = g_sqrt(d2) < R(1e-4);
    trunc = oob || sc >= v.trunc_sc;
  }
  const bool done = term || trunc;
  const bool do_reset = done && v.autoreset;
  GPD_STAMP(3);
  GPD_STAMP(4);
  float row12[12] = {(float)s.px, (float)s.py, (float)s.pz, roll, pitch, yaw,
                     (float)s.vx, (float)s.vy, (float)s.vz, (float)s.ax, (float)s.ay, (float)s.az};
  if (do_reset) {
    if (active && io.terminal_obs != nullptr) row12_store<A>(io.terminal_obs + n * v.W, row12);
    reset_to_template(tk.ini, s, last, row12);
  }
  const unsigned long long done_rows = __ballot(do_reset && active && io.terminal_obs != nullptr);
  // what the last stores write, formed before the final barrier (the stores stay behind it)
  int ctr_x = do_reset ? 0 : sc + nsub, term_b = term ? 1 : 0, trunc_b = trunc ? 1 : 0;
  asm volatile("" : "+v"(ctr_x), "+v"(term_b), "+v"(trunc_b));
  if (IO) {
    // the row's 12 state columns straight from registers; the io wave writes the rest
    GPD_STAMP(5);
    if (active) {
      if (A == 4) {
        const float4 r0 = make_float4(row12[0], row12[1], row12[2], row12[3]);
        const float4 r1 = make_float4(row12[4], row12[5], row12[6], row12[7]);
        const float4 r2 = make_float4(row12[8], row12[9], row12[10], row12[11]);
        if (v.wt & 1) {
          const __amdgpu_buffer_rsrc_t r =
              __builtin_amdgcn_make_buffer_rsrc(io.obs + n0 * v.W, 0, nact * v.W * 4, 0x00020000);
          const int o = tid * v.W * 4;
          store_wt(r, o, r0); store_wt(r, o + 16, r1); store_wt(r, o + 32, r2);
        } else {
          float4* o4 = reinterpret_cast<float4*>(io.obs + n * v.W);
          o4[0] = r0; o4[1] = r1; o4[2] = r2;
        }
      } else {
        float* orow = io.obs + n * v.W;
#pragma unroll
        for (int k = 0; k < 12; ++k) orow[k] = row12[k];
      }
    }
    if (tid == 0) sdone = done_rows;
    lds_barrier();   // final: sdone published (the io wave writes the terminal rows' history)
    GPD_STAMP(6);
    GPD_STAMP(8);
    GPD_STAMP(9);
  } else {
    if (A == 4) {
      tile4[0 * kPad + tid] = make_float4(row12[0], row12[1], row12[2], row12[3]);
      tile4[1 * kPad + tid] = make_float4(row12[4], row12[5], row12[6], row12[7]);
      tile4[2 * kPad + tid] = make_float4(row12[8], row12[9], row12[10], row12[11]);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) tilef[k * kPad + tid] = row12[k];
    }
    if (tid == 0) sdone = done_rows;
    GPD_STAMP(5);
    lds_barrier();     // tile complete, sdone published
    GPD_STAMP(6);
    tile_copy_out<A, 2 * kWave, 3>(tile4, tilef, threadIdx.x, nact, NC, v.nc_magic, v.wt, done_rows, io.obs,
                                io.terminal_obs, n0);
  }
  GPD_STAMP(7);
  GPD_RSTAMP(12);
  if (!active) return;
  store_drone_step_at<R, kAuxWt>(v, st_out, st_off, s, last);
  mark_last_in_ring_single(v, n);
  *rew_out = reward;
  *term_out = (uint8_t)term_b;
  *trunc_out = (uint8_t)trunc_b;
  *ctr_out = gpd_v2i{ctr_x, head_next};
}

}  // namespace gpd
