// gpd_step_seq.h — step_seq_kernel: n_steps consecutive steps of step_kernel_duo<R, ACT, true>
// (single-drone envs, plain DYN, RPM action types; four waves per block here) in ONE launch, for
// open-loop action sequences (gpd_step_seq, BatchedAviarySim.capture_graph).  The envs of this path
// do not interact, so a block keeps its drones for the whole sequence, as cmd_rollout_kernel does
// (gpd_step_rollout.h): the state, the step counters and the constants are loaded once and the
// state is stored once, the action history lives in the LDS tile, and the kernel boundary with its
// cold caches is paid once per launch instead of once per step.  Every step still stores what an
// env.step() returns (observation rows, reward, flags, terminal rows), so after the launch memory
// holds what n_steps launches of step_kernel_duo would have left, bit for bit.
// The arithmetic of the waves is step_kernel_duo's (gpd_step_duo.h).  The pose halves (pose_half,
// FMAX for this kernel's last one) and the rate pieces (gpd_device.h) are shared.  The io wave's
// mapping, store and terminal passes, the hover hook, action -> wrench and the look-ahead rate loop
// are written out in both: each was tried as one helper, which changed step_kernel_duo's
// instructions, and as a helper of this kernel alone, which cost it 0.8 % in the native launch loop
// (profiles/step_seq_shared/README.md).  A fix to one of them goes to both.
// Different from step_kernel_duo on purpose (profiles/step_seq_rows/README.md): there the pose wave
// turns action into thrust, makes the row's state columns (Euler angles, float conversions, the
// terminal and the template's row) and stores them with reward and flags; here the rate chains
// publish the thrust with their rows and the io wave makes and stores the row from what the pose
// wave publishes (seq_obs_euler_f32 restates obs_euler_f32 on published arguments, seq_rate_weights
// restates rate_weights with |w|^2 spelled out).  last_clipped_action is formed once, at the end.
// Needs what gpd_step_duo.h includes.
#pragma once
#include "gpd_step_duo.h"

namespace gpd {

// ---------------------------------------------------------------------------------------
// Arguments: step_kernel_duo's, with actions_p the base of the action slots [n_slots][N][A];
// step t of the launch reads slot (slot0 + t) % n_slots.  All of them are fixed per launch (the
// ring head and the step counters live in device memory), so a hipGraph can replay it.
//   pose wave  the drone, the step counter and the ring head in registers; per step the thrust from
//              the chain it follows, the substeps' pose halves, the final readback, the tilt and
//              hover decisions and the reset of an env that finishes.  It publishes what the row is
//              made of (kSeqRowVals reals per lane, 16-byte LDS writes) and four masks: terminal
//              rows wanted, reset, terminated, truncated.  The state, last_clipped_action (from the
//              launch's last action row, loaded at entry), the ring mark and {step_counter, head}
//              once, at the end
//   rate waves the body rates in registers; the substeps' rate halves and the thrust of the NEXT
//              step, from the true rates (chain a) and from the template's zero rates (chain b)
//   io wave   the action history: the ring's slots are DMA'd into the tile once, tile slot s
//              being ring slot s.  Each step writes its action into slot `head` (and into the HBM
//              ring, a plain store nothing waits for); history column j of a row is then tile slot
//              (head + 1 + j) mod L, so an element's LDS address advances by one slot per step
//              and wraps, while its place in the row stays the same.  Behind the barrier of step
//              t lane i makes row i of step t from the pose wave's entry: the float32 Euler angles
//              (gimbal branches as a wave-uniform fix-up), the twelve state columns, for a reset
//              lane the terminal row and then the template's row, reward and flags.  The pose wave
//              is in step t+1 meanwhile; the row buffer and the masks are double-buffered by step
//              parity like the hand-off rows.  After the last barrier the io wave finishes the last
//              row and returns.
//
// The rate chain a step ahead.  The body-rate chain of a step needs the step's action and the
// rates at its start, nothing of the pose (gpd_device.h, above rate_recur), and an open-loop
// sequence has every action in memory.  So while the pose wave runs step t, the rate work of step
// t+1 is done in full under both outcomes of step t's reset decision, by two rate waves:
//   chain a (wave 1)  from the true rates at the end of step t.  Those are known behind the barrier
//                     of step t-1: the lanes reset in step t-1 (sreset) ran step t on chain b's
//                     rates, the others on chain a's own
//   chain b (wave 3)  from the template's rates, zero (drone_from_template): a lane reset in step t
// Each writes the substeps' weights h[5] and its end rates to the hand-off buffer, which lies in
// dynamic LDS behind the tile: [step parity][chain][lane < tpb][seq_rows(nsub)] reals.  Behind the
// barrier of step t the pose wave holds sreset(t) in a register, reads step t+1's rows per lane
// from chain b where the lane was reset and from chain a otherwise, and runs its nsub pose halves
// with no barrier between them.
// ONE barrier per step for all four waves.  In front of the barrier of step t the pose wave
// publishes sdone / sreset of step t and the rate waves the rows of step t+1; behind it the rate
// waves write the rows of step t+2 where step t's were, which the pose wave has read.  sdone /
// sreset are double-buffered by step parity: the readers of step t's (io wave, chain a) read them
// between the barriers of steps t and t+1, the pose wave writes step t+1's in the same interval
// and step t+2's behind the next barrier.  The first step of a launch has chain a alone, computed
// from the stored rates in front of an entry barrier; in the last step the rate waves compute
// nothing.  Every wave meets n_steps + 1 barriers.
// Each wave loads its next action row while it works on the current one.

// rows of a lane in one chain's hand-off buffer: 5 weights per substep, the 3 end rates and the
// step's thrust fz, made odd so that the lanes' rows start in different LDS banks
__host__ __device__ inline int seq_rows(int nsub) { return (5 * nsub + 4) | 1; }
// what the pose wave publishes of a lane's row, in reals: pos(3) vel(3) ang_v(3), getEulerZYX's
// arguments sarg a b, yaw's two arguments, the readback's x y (the gimbal branches), the reward;
// one pad, so that a lane's entry is 9 16-byte pairs (f64).  Lanes are 36 dwords apart: 16 lanes'
// pairs fall into 64 different banks.
constexpr int kSeqRowVals = 18;
// the hand-off buffers' place behind the tile, the row buffer [step parity][lane < tpb][kSeqRowVals]
// behind them (in reals from the hand-off buffers' start), and the kernel's dynamic LDS
__host__ __device__ inline int seq_hand_off_at(int tile_bytes) { return (tile_bytes + 15) & ~15; }
__host__ __device__ inline int seq_row_buf_at(int nsub, int tpb) { return 2 * 2 * seq_rows(nsub) * tpb; }
inline size_t seq_lds_bytes(int tile_bytes, int nsub, int tpb, size_t real_bytes) {
  return (size_t)seq_hand_off_at(tile_bytes) +
         ((size_t)seq_row_buf_at(nsub, tpb) + (size_t)2 * kSeqRowVals * tpb) * real_bytes;
}

// rate_weights (gpd_device.h) with |w|^2 in the very operations of step_kernel_duo's rate wave: wx wx
// the plain product, wy wy and then wz wz fused onto it.  Left to hipcc the choice of the plain
// product moves with the code around it; one ulp of |w|^2 shows in cos / sinc at large rotation
// angles (tests/test_gpu_step_seq_ahead.py::test_large_angle_weights_on_chain_a).  A change to
// rate_weights goes here too.  f64 only, like the kernel.
__device__ __forceinline__ double seq_rate_n2(double wx, double wy, double wz) {
#pragma clang fp contract(off)
  return __builtin_fma(wz, wz, __builtin_fma(wy, wy, wx * wx));
}
// yaw's arguments 2(xy + wz) and ww + xx - yy - zz of obs_euler_f32, in the very operations
// step_kernel_duo's pose wave compiles them to: xy fused onto the plain product wz, and four plain
// squares summed in the order written.
__device__ __forceinline__ void seq_yaw_args(const double q[4], double& yn, double& yd) {
#pragma clang fp contract(off)
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  yn = 2.0 * __builtin_fma(x, y, w * z);
  yd = ((w * w + x * x) - y * y) - z * z;
}
template <typename R>
__device__ __forceinline__ bool seq_rate_weights(R wx, R wy, R wz, const DynK<R>& k, R h[5], R& n2) {
  n2 = seq_rate_n2(wx, wy, wz);
  const bool rot = n2 > R(1e-16);
  const R t2 = n2 * k.hdt2;
  R co, sc;
  cos_sinc(t2, co, sc);
  h[0] = co; h[1] = k.hdt * sc;
  h[2] = rot ? wx : R(0); h[3] = rot ? wy : R(0); h[4] = rot ? wz : R(0);
  return t2 >= R(0.25);
}

// obs_euler_f32 (gpd_device.h) from the published arguments: sarg a b as attitude_decide left them,
// yn = 2(xy + wz) and yd = ww + xx - yy - zz formed by the pose wave (another wave's contraction of
// them could differ in the last bit), x y of the readback for the gimbal branches.  The gimbal
// flag is attitude_args' / attitude_literal's predicate of sarg.
template <typename R>
__device__ __forceinline__ void seq_obs_euler_f32(R sarg, R a, R b, R yn, R yd, R x, R y, float& roll, float& pitch,
                                                  float& yaw) {
  const bool gimbal = sarg <= R(-0.99999) || sarg >= R(0.99999);
  const R sa = sarg < R(-1) ? R(-1) : (sarg > R(1) ? R(1) : sarg);
  pitch = asinf((float)sa);
  roll = atan2f((float)a, (float)b);
  yaw = atan2f((float)yn, (float)yd);
  if (GPD_RARE(__ballot(gimbal) != 0ull)) {
    if (sarg <= R(-0.99999)) {
      pitch = -1.57079632679489661923f; roll = 0.0f; yaw = (float)(R(2) * g_atan2(x, -y));
    } else if (sarg >= R(0.99999)) {
      pitch = 1.57079632679489661923f; roll = 0.0f; yaw = (float)(R(2) * g_atan2(-x, y));
    }
  }
}

template <typename R, int ACT>
__global__ __launch_bounds__(4 * kWave) void step_seq_kernel(R* __restrict__ state_p, const float* __restrict__ actions_p,
                                                             int2* __restrict__ ctr_p, const Consts<R>* __restrict__ cp,
                                                             long long npad_p, int n_p, int tpb_p, SimView<R> v,
                                                             StepIO<R> io, int n_slots, int slot0, int n_steps,
                                                             int hand_off_at) {
  static_assert(!act_is_pid(ACT), "the fused sequence kernel serves the RPM action types");
  static_assert(sizeof(R) == 8, "the fused sequence kernel is built for f64 sims only (gpd.hip, step_seq_fn)");
  v.state = state_p; v.ctr = ctr_p; v.npad = npad_p; v.N = n_p; v.tpb = tpb_p;
  constexpr int A = act_width(ACT);
  extern __shared__ float4 tile4[];
  float* tilef = reinterpret_cast<float*>(tile4);
  __shared__ unsigned long long sdone[2];    // rows whose terminal observation is wanted (tile rows), by step parity
  __shared__ unsigned long long sreset[2];   // lanes whose env was reset in the step, by step parity
  __shared__ unsigned long long sterm[2];    // lanes whose env is `terminated` / `truncated` in the step,
  __shared__ unsigned long long strunc[2];   // by step parity (the io wave stores the flags)
  __shared__ int shead[kWave];               // ring head of every lane's env at entry (io wave)
  const Consts<R>& c = *cp;
  const int tid = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x) / kWave;   // wave-uniform
  const long long n0 = (long long)blockIdx.x * v.tpb;
  const long long n = n0 + tid;
  const int nact = (int)((v.N - n0) < v.tpb ? (v.N - n0) : v.tpb);
  const bool active = tid < nact;
  const long long nn = active ? n : n0;  // inactive lanes compute on the block's first drone, store nothing
  // the action row of this lane in the slot a step reads; the slot advances and wraps per step
  const long long slot_stride = (long long)v.N * A;
  int slot = slot0;
  auto next_slot = [&]() { slot = slot + 1 == n_slots ? 0 : slot + 1; };
  float nxt[A];
  // the hand-off buffers [parity][chain][lane][rows]; the lanes past the block's drones compute
  // on its first drone (nn), read lane 0's rows and write none
  R* const hbuf = reinterpret_cast<R*>(reinterpret_cast<char*>(tile4) + hand_off_at);
  const int rows = seq_rows(c.nsub);
  const int cstride = v.tpb * rows;        // chain a -> chain b
  const int pstride = 2 * cstride;         // even step -> odd step
  const bool own = tid < v.tpb;
  const int lrow = (own ? tid : 0) * rows;
  // the row buffer [parity][lane][kSeqRowVals], as 16-byte pairs
  typedef R R2 __attribute__((ext_vector_type(2)));
  constexpr int kRowPairs = kSeqRowVals / 2;
  R2* const rbuf = reinterpret_cast<R2*>(hbuf + seq_row_buf_at(c.nsub, v.tpb)) + (own ? tid : 0) * kRowPairs;
  const int rpar = v.tpb * kRowPairs;      // even step -> odd step

  if (wave == 2) {
    // ------------------------------------------------------------ wave 2: history columns
    const int L = v.ring_len;
    // the whole ring of the block's drones -> tile, slot s to tile slot s, once per launch
    {
      const float* rb = v.ring + ridx(nn, 0, L, A);
      for (int s = 0; s < L; ++s) {
        const float* src = rb + (long long)s * (64 * A);
        if (A == 4) __builtin_amdgcn_global_load_lds((gbl_void_ptr)src, (lds_void_ptr)(tile4 + s * kPad), 16, 0, 0);
        else __builtin_amdgcn_global_load_lds((gbl_void_ptr)src, (lds_void_ptr)(tilef + s * kPad), 4, 0, 0);
      }
    }
    int hd = v.ctr[nn].y;                         // ring slot receiving the step's action
    action_load<A>(actions_p + slot * slot_stride, nn, nxt);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the ring is in the tile (before any step writes its slot)
    shead[tid] = hd;
    wave_lds_sync();
    // An element of the block's history columns: row i = g / L, column k = g - i * L, g < nact * L.
    // Blocks whose elements fit one pass of U per lane (`fits`) form each element's row offset
    // once and step its tile index; longer histories form both per pass.
    constexpr int U = 4;                          // elements per lane in flight per pass
    constexpr int EB = A == 4 ? 16 : 4;           // bytes of a tile element
    const int total = nact * L;
    const int NC = A == 4 ? 3 + L : v.W;          // row stride in elements
    const int c0 = A == 4 ? 3 : 12;               // first history column
    const float rL = 1.0f / (float)L;             // (g + 0.5) / L: exact row index for g < 2^12
    const bool fits = total <= U * kWave;
    const bool wt_rows = (v.wt & 1) != 0;
    const int span = L * kPad;                    // tile elements of the L slots
    float* const dst0 = uniform_ptr(io.obs + n0 * v.W);
    const int nrec = __builtin_amdgcn_readfirstlane(nact * v.W * 4);
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(dst0, 0, nrec, 0x00020000);
    int off[U], row[U], idx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // an element past the end gets an offset past num_records, so the buffer unit drops its store
      const int g = tid + u * kWave;
      const bool ok = g < total;
      const int gg = ok ? g : total - 1;
      const int i = (int)(((float)gg + 0.5f) * rL), k = gg - i * L;
      int s = shead[i] + 1 + k;
      s -= s >= L ? L : 0;
      s -= s >= L ? L : 0;
      row[u] = i;
      off[u] = ok ? (i * NC + c0 + k) * EB : nrec;
      idx[u] = s * kPad + i;
    }
    float tmpl12[12];                             // the template's row, for the lanes reset in a step
    row12_from_template(c.init0, tmpl12);
    int tmod = 0;                                 // steps of this launch so far, mod L
    asm volatile("s_barrier" ::: "memory");       // entry (this wave publishes nothing to the others there)
    for (int t = 0; t < n_steps; ++t) {
      float a[A];
#pragma unroll
      for (int j = 0; j < A; ++j) a[j] = nxt[j];
      next_slot();
      // the next step's row is in flight while this step's substeps run
      if (t + 1 < n_steps) action_load<A>(actions_p + slot * slot_stride, nn, nxt);
      if (A == 4) tile4[hd * kPad + tid] = make_float4(a[0], a[1], a[2], a[3]);
      else tilef[hd * kPad + tid] = a[0];
      if (active) ring_append<A>(v.ring, n, hd, L, a);   // deque.append
      wave_lds_sync();
      float4 v4[U];
      float v1[U];
      if (fits) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (A == 4) v4[u] = tile4[idx[u]];
          else v1[u] = tilef[idx[u]];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (wt_rows) {
            if (A == 4) store_wt(rsrc, off[u], v4[u]);
            else store_wt(rsrc, off[u], v1[u]);
          } else {
            if (A == 4) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gpd_v4i, v4[u]), rsrc, off[u], 0, 0);
            else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v1[u]), rsrc, off[u], 0, 0);
          }
        }
      }
      // longer histories: one element per lane per pass
      for (int g = fits ? total : tid; g < total; g += kWave) {
        const int i = (int)(((float)g + 0.5f) * rL), k = g - i * L;
        int s = shead[i] + tmod + 1 + k;
        s -= s >= L ? L : 0;
        s -= s >= L ? L : 0;
        const int o = (i * NC + c0 + k) * EB;
        if (A == 4) {
          const float4 p = tile4[s * kPad + i];
          if (wt_rows) store_wt(rsrc, o, p);
          else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gpd_v4i, p), rsrc, o, 0, 0);
        } else {
          const float p = tilef[s * kPad + i];
          if (wt_rows) store_wt(rsrc, o, p);
          else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, p), rsrc, o, 0, 0);
        }
      }
      lds_barrier();     // the step's barrier: sdone published by the pose wave
      const unsigned long long dr = sdone[t & 1];
      if (dr) {          // the history columns of the terminal rows (the tile is unchanged until the next step's write)
        float* const tdst = io.terminal_obs + n0 * v.W;
        if (fits) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (tid + u * kWave < total && ((dr >> row[u]) & 1ull)) {
              char* const tp = reinterpret_cast<char*>(tdst) + off[u];
              if (A == 4) *reinterpret_cast<float4*>(tp) = v4[u];
              else *reinterpret_cast<float*>(tp) = v1[u];
            }
          }
        }
        for (int g = fits ? total : tid; g < total; g += kWave) {
          const int i = (int)(((float)g + 0.5f) * rL), k = g - i * L;
          if ((dr >> i) & 1ull) {
            int s = shead[i] + tmod + 1 + k;
            s -= s >= L ? L : 0;
            s -= s >= L ? L : 0;
            const int e = i * NC + c0 + k;
            if (A == 4) reinterpret_cast<float4*>(tdst)[e] = tile4[s * kPad + i];
            else tdst[e] = tilef[s * kPad + i];
          }
        }
      }
      // the step's row: state columns from what the pose wave published, reward and flags.  Lane
      // i makes row i in every step, so the last step's values stay.  Nothing waits for these
      // stores before the launch ends.
      {
        const unsigned long long rs = sreset[t & 1], tm = sterm[t & 1], tr = strunc[t & 1];
        if (active) {
          const R2* const rp = rbuf + (t & 1) * rpar;
          R2 e[kRowPairs];
#pragma unroll
          for (int k = 0; k < kRowPairs; ++k) e[k] = rp[k];
          float roll, pitch, yaw;
          seq_obs_euler_f32<R>(e[4].y, e[5].x, e[5].y, e[6].x, e[6].y, e[7].x, e[7].y, roll, pitch, yaw);
          float row12[12] = {(float)e[0].x, (float)e[0].y, (float)e[1].x, roll, pitch, yaw,
                             (float)e[1].y, (float)e[2].x, (float)e[2].y, (float)e[3].x, (float)e[3].y, (float)e[4].x};
          const float reward = v.task != TASK_NONE ? (float)e[8].x : -1.0f;
          if ((rs >> tid) & 1ull) {
            if ((dr >> tid) & 1ull) row12_store<A>(io.terminal_obs + n * v.W, row12);
#pragma unroll
            for (int k = 0; k < 12; ++k) row12[k] = tmpl12[k];
          }
          if (A == 4) {
            const float4 r0 = make_float4(row12[0], row12[1], row12[2], row12[3]);
            const float4 r1 = make_float4(row12[4], row12[5], row12[6], row12[7]);
            const float4 r2 = make_float4(row12[8], row12[9], row12[10], row12[11]);
            if (wt_rows) {
              const int o = tid * v.W * 4;
              store_wt(rsrc, o, r0); store_wt(rsrc, o + 16, r1); store_wt(rsrc, o + 32, r2);
            } else {
              float4* o4 = reinterpret_cast<float4*>(io.obs + n * v.W);
              o4[0] = r0; o4[1] = r1; o4[2] = r2;
            }
          } else {
            float* orow = io.obs + n * v.W;
#pragma unroll
            for (int k = 0; k < 12; ++k) orow[k] = row12[k];
          }
          io.reward[n] = reward;
          io.term[n] = (uint8_t)((tm >> tid) & 1ull);
          io.trunc[n] = (uint8_t)((tr >> tid) & 1ull);
        }
      }
      // one slot on: the head, every element's tile index, the step count mod L
      hd = hd + 1 == L ? 0 : hd + 1;
      tmod = tmod + 1 == L ? 0 : tmod + 1;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        idx[u] += kPad;
        idx[u] -= idx[u] >= span ? span : 0;
      }
    }
    return;
  }

  const R* st = v.state + tidx(nn, 0, kStateComps);

  if (wave != 0) {
    // ------------------------------------------------------------ waves 1 and 3: body rates
    const bool from_zero = wave == 3;      // chain b
    R* const hw = hbuf + (from_zero ? cstride : 0) + lrow;
    // chain a starts with step 0, from the stored rates; chain b with step 1, from zero
    if (from_zero) next_slot();
    if (!from_zero || n_steps > 1) action_load<A>(actions_p + slot * slot_stride, nn, nxt);
    R wx = R(0), wy = R(0), wz = R(0);
    if (!from_zero) { wx = st[10 * 64]; wy = st[11 * 64]; wz = st[12 * 64]; }
    DynK<R> dk = dyn_consts(c);
    const int nsub = dk.nsub;
    // the entry loads have landed before the first step: a wait for them left inside the loop
    // would, from the second step on, wait for the action row just requested
    asm volatile("" : "+v"(wx), "+v"(wy), "+v"(wz));
    // the rate work of step u, whose action row is in nxt: the substeps' weights and the end
    // rates into `out`.  The recurrence is written one substep ahead of its weights as in
    // step_kernel_duo.  There it hid the recurrence behind a hand-off barrier; here no barrier is
    // left to hide it behind, and the order is kept because it is the text whose contractions give
    // step_kernel_duo's bits (the tests compare them).  Per lane the operations are the same.
    // (The other copy is step_kernel_duo's kAhead loop; one helper with the publishing step a
    // functor made its f64 instantiations 4 to 8 bytes shorter.)
    auto chain = [&](int u, R* out) {
      float a[A];
#pragma unroll
      for (int j = 0; j < A; ++j) a[j] = nxt[j];
      next_slot();
      if (u + 1 < n_steps) action_load<A>(actions_p + slot * slot_stride, nn, nxt);
      R rpm[4], W[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) rpm[k] = (R)action_to_rpm(dk.hover_f32, a[A == 4 ? k : 0]);
      rpm_wrench<R, 0>(rpm, dk, c, W);
      if (own) out[5 * nsub + 3] = W[0];   // the step's thrust, for the pose wave
      rate_recur(wx, wy, wz, W, dk);   // ω_1
      for (int k = 0; k < nsub - 1; ++k) {
        R h[5], n2;
        const R cx = wx, cy = wy, cz = wz;   // ω_{k+1}
        const bool big = seq_rate_weights(cx, cy, cz, dk, h, n2);
        rate_weights_big(big, n2, dk, h);
        if (own) {
#pragma unroll
          for (int j = 0; j < 5; ++j) out[5 * k + j] = h[j];
        }
        rate_recur(wx, wy, wz, W, dk);       // ω_{k+2}
      }
      {
        R h[5], n2;
        const bool big = seq_rate_weights(wx, wy, wz, dk, h, n2);
        rate_weights_big(big, n2, dk, h);
        if (own) {
          R* const o = out + 5 * (nsub - 1);
#pragma unroll
          for (int j = 0; j < 5; ++j) o[j] = h[j];
          o[5] = wx; o[6] = wy; o[7] = wz;
        }
      }
    };
    // t = -1 is the part in front of the entry barrier: step 0's rows, by chain a alone
    for (int t = -1; t < n_steps; ++t) {
      // behind the barrier of step t-1, the pose wave in step t: the rows of step t+1
      if (t + 1 < n_steps && (t >= 0 || !from_zero)) {
        if (from_zero) {
          wx = wy = wz = R(0);
          asm volatile("" : "+v"(wx), "+v"(wy), "+v"(wz));
        } else if (t > 0) {
          // the rates at the end of step t: chain b's for the lanes reset in step t-1
          if ((sreset[(t - 1) & 1] >> tid) & 1ull) {
            const R* e = hbuf + (t & 1) * pstride + cstride + lrow + 5 * nsub;
            wx = e[0]; wy = e[1]; wz = e[2];
          }
        }
        chain(t + 1, hw + ((t + 1) & 1) * pstride);
      }
      lds_barrier();     // the step's barrier: the rows of step t+1 published
    }
    return;
  }

  // -------------------------------------------------------------- wave 0: pose
  // the launch's last action row: last_clipped_action is needed for the state store alone
  float alast[A];
  action_load<A>(actions_p + ((slot0 + n_steps - 1) % n_slots) * slot_stride, nn, alast);
  Drone<R> s;
  R last[4];
  load_drone(v, nn, s, last, false);
  const int2 cv = v.ctr[nn];
  int sc = cv.x;          // step_counter
  int head = cv.y;        // ring slot receiving the step's action
  DynK<R> dk = dyn_consts(c, v.task, io.trunc);
  const TailK<R> tk = tail_consts(c, v.bound_xy);
  const int nsub = dk.nsub;
  // where the lane's results go, formed once (global-address-space pointers, as step_kernel_duo)
  gpd_global R* st_out = (gpd_global R*)(v.state + tidx(nn, 0, kStateComps));
  int st_off = (int)(tidx(nn, 0, kStateComps) * sizeof(R));
  gpd_global gpd_v2i* ctr_out = (gpd_global gpd_v2i*)(v.ctr + nn);
  asm volatile("" : "+v"(st_out), "+v"(st_off), "+v"(ctr_out));
  // the entry loads have landed before the first step: a wait for them left inside the loop would,
  // from the second step on, wait for the previous step's stores
  asm volatile("" : "+v"(s.px), "+v"(s.py), "+v"(s.pz), "+v"(s.qx), "+v"(s.qy), "+v"(s.qz), "+v"(s.qw), "+v"(s.vx),
               "+v"(s.vy), "+v"(s.vz), "+v"(sc), "+v"(head));
#pragma unroll
  for (int j = 0; j < A; ++j) asm volatile("" : "+v"(alast[j]));
  const R wnone[3] = {R(0), R(0), R(0)};
  auto hand_off = [&](const R* hp, int k, R h[5]) {
#pragma unroll
    for (int j = 0; j < 5; ++j) h[j] = hp[5 * k + j];
  };
  bool was_reset = false;   // this lane's env was reset in the previous step: its rates are chain b's
  lds_barrier();            // entry: step 0's rows are there
  for (int t = 0; t < n_steps; ++t) {
    // the step's rows: the weights of substep k + 1 are read ahead of substep k's arithmetic
    const R* const hp = hbuf + (t & 1) * pstride + (was_reset ? cstride : 0) + lrow;
    // rpm_wrench's W[0] of the step's action, by the chain the lane follows
    const R fz = hp[5 * nsub + 3];
    R h[5];
    hand_off(hp, 0, h);
    if (nsub > 1) {
      R hn[5];
      hand_off(hp, 1, hn);
      pose_half<R, false, true>(s, fz, h, wnone, dk);
      for (int k = 1; k < nsub - 1; ++k) {
#pragma unroll
        for (int j = 0; j < 5; ++j) h[j] = hn[j];
        hand_off(hp, k + 1, hn);
        pose_half<R, false, false>(s, fz, h, wnone, dk);
      }
#pragma unroll
      for (int j = 0; j < 5; ++j) h[j] = hn[j];
    }
    {
      const R* const e = hp + 5 * nsub;   // the rates after the last substep
      s.wx = e[0]; s.wy = e[1]; s.wz = e[2];
      const R w[3] = {s.wx, s.wy, s.wz};
      if (nsub > 1) pose_half<R, true, false, true>(s, fz, h, w, dk);
      else pose_half<R, true, true>(s, fz, h, w, dk);
    }
    // final readback (:374) -> obs / reward / done
    R qn[4], Rm[9];
    if constexpr (sizeof(R) == 8) readback_fused_rare(s.qx, s.qy, s.qz, s.qw, qn, Rm);
    else readback_fused(s.qx, s.qy, s.qz, s.qw, qn, Rm);
    AttitudeArgs<R> att = attitude_args(qn);
    bool tilted, up_unused;   // |roll| or |pitch| > 0.4, decided exactly near the limit (attitude_decide)
    attitude_decide<R, true, false>(s.qx, s.qy, s.qz, s.qw, att, tilted, up_unused);
    R rew = R(0);   // the reward in f64; the io wave rounds it (and stores -1 without a task)
    bool term = false, trunc = false;
    if (v.task != TASK_NONE) {
      const R tx = tk.tg[0] - s.px, ty = tk.tg[1] - s.py, tz = tk.tg[2] - s.pz;
      const R d2 = hover_d2(tx, ty, tz);
      R r = R(2) - d2 * d2;
      r = r > R(0) ? r : R(0);
      const bool oob = g_abs(s.px) > tk.bound_xy || g_abs(s.py) > tk.bound_xy || s.pz > R(2) || tilted;
      rew = r;
      // np.linalg.norm(...) < .0001 (HoverAviary.py:92) with the root taken only inside the band
      // where it decides (step_kernel_duo)
      term = d2 < R(0.99e-8);
      const bool band = !(d2 < R(0.99e-8)) && !(d2 > R(1.01e-8));   // a NaN goes the root's way, too
      if (GPD_RARE(__ballot(band) != 0ull)) term = g_sqrt(d2) < R(1e-4);
      trunc = oob || sc >= v.trunc_sc;
    }
    const bool done = term || trunc;
    const bool do_reset = done && v.autoreset;
    // what the step's row is made of, for the io wave (kSeqRowVals): the live values, before a reset
    R yn, yd;
    seq_yaw_args(qn, yn, yd);
    if (own) {
      R2* const rp = rbuf + (t & 1) * rpar;
      rp[0] = R2{s.px, s.py}; rp[1] = R2{s.pz, s.vx}; rp[2] = R2{s.vy, s.vz};
      rp[3] = R2{s.ax, s.ay}; rp[4] = R2{s.az, att.sarg}; rp[5] = R2{att.a, att.b};
      rp[6] = R2{yn, yd};
      rp[7] = R2{qn[0], qn[1]}; rp[8] = R2{rew, R(0)};
    }
    if (do_reset) drone_from_template(tk.ini, s);
    const unsigned long long done_rows = __ballot(do_reset && active && io.terminal_obs != nullptr);
    const unsigned long long reset_rows = __ballot(do_reset);
    const unsigned long long term_rows = __ballot(term), trunc_rows = __ballot(trunc);
    if (tid == 0) { sterm[t & 1] = term_rows; strunc[t & 1] = trunc_rows; }
    if (tid == 0) { sdone[t & 1] = done_rows; sreset[t & 1] = reset_rows; }
    was_reset = do_reset;
    lds_barrier();   // the step's barrier: the masks and the row published, the next step's rows are there
    sc = do_reset ? 0 : sc + nsub;
    head = head + 1 == v.ring_len ? 0 : head + 1;
  }
  if (!active) return;
  // self.last_clipped_action = clipped_action (:372) of the last step; zero in a lane reset in it
#pragma unroll
  for (int k = 0; k < 4; ++k) last[k] = was_reset ? R(0) : (R)action_to_rpm(dk.hover_f32, alast[A == 4 ? k : 0]);
  store_drone_step_at<R, kAuxWt>(v, st_out, st_off, s, last);
  mark_last_in_ring_single(v, n);
  *ctr_out = gpd_v2i{sc, head};
}

}  // namespace gpd
