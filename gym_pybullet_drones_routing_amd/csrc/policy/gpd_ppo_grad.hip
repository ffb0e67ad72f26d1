// gpd_ppo_grad.hip — the PPO minibatch gradient (include/gpd_policy.h: gpd_policy_ppo_grad) for gfx950.
//
// examples/learn.py's minibatch step is: gather five buffers by idx, actor + critic forward, the
// clipped surrogate + value loss, autograd's backward, clip_grad_norm_, Adam: ~100 library kernels.
// Everything up to the clipped gradient is four launches here (Adam stays torch's):
//   1. adv_stats_kernel   mean and unbiased std of adv[idx]            (one block, fixed order)
//   2. grad_kernel        blocks of four waves over 16-row groups: the gather, the forward pass as
//                         gpd_policy.hip's forward<> computes it (K order and output sums from
//                         gpd_policy_mlp.h: the same bits for mu and V),
//                         the per-row dL/dmu, dL/dlog_std, dL/dv, and the backward pass of both MLPs
//                         on v_mfma_f32_16x16x4_f32; a block keeps its weight gradients in registers
//                         over all of its groups and stores them once, as one slab of the workspace
//   3. reduce_kernel      sums the slabs in block order (one thread per parameter) and a partial
//                         squared norm per block, in a fixed tree
//   4. finish_kernel      the norm from the partials by a fixed tree, the clip scale, grad *= scale,
//                         stats
// No float atomics and no in-launch "last arriver": every sum has one order, fixed by the shapes and
// max_blocks, so the gradient is bit-reproducible.  (3 and 4 are two launches because the clip
// scale needs the whole norm and 3 is spread over many blocks; 4 is one block over <= 34k floats.)
//
// The MFMA maps (lane l: i = l & 15, g = l >> 4; A[row i][k slot g], B[k slot g][col i],
// D[row 4g + r][col i]).  Wave w owns neurons 16w .. 16w + 15 as in the forward pass, so h1, h2 of
// (row 4g + r, neuron 16w + i) are in this lane's accumulators.  A product that sums over ROWS
// takes such an accumulator as its A operand directly (step s, slot g <-> row 4g + s):
//   dW3^T[neuron][o]  = sum_row h2[row][neuron] dOut[row][o]      A = h2 regs,  B = dOut (LDS)
//   dW2[neuron][k]    = sum_row dz2[row][neuron] h1[row][k]       A = dz2 regs, B = h1 (LDS), 4 column tiles
//   dW1[neuron][k]    = sum_row dz1[row][neuron] x[row][k]        A = dz1 regs, B = x (LDS), ceil(n_obs/16) tiles
// each with D[row 4g + r -> neuron 16w + 4g + r][col i -> k = 16 tile + i], accumulated over groups.
// The one product that sums over NEURONS goes through LDS:
//   dh1[row][k]       = sum_j dz2[row][j] W2[j][k]                A = dz2 (LDS), B = W2[16g + s][16w + i] regs
// and lands as D[row 4g + r][neuron 16w + i]: where h1 is.  dh2 = dOut W3 has K = n_act (1 for the
// critic): VALU.
#include <hip/hip_runtime.h>

#include <cmath>

#include "gpd_policy.h"
#include "gpd_policy_mlp.h"

using namespace gpd_policy;

namespace {

constexpr int kMaxAct = GPD_POLICY_MAX_ACT;
constexpr int kV = kMaxAct;                    // column of the value / dL/dv beside the actions' 0 .. 7
constexpr int kRv = 33;                        // row stride of Lds::rowv
constexpr int kMaxKc = GPD_POLICY_MAX_OBS / 16;
constexpr int kDefaultBlocks = 256;            // one block per CU
constexpr int kHead = 16;                      // workspace floats: adv mean, std + 1e-8, ...
constexpr int kNormParts = 256;                // ... then reduce_kernel's partial squared norms, then the slabs
constexpr int kStatsThreads = 1024, kStatsBatch = 8;

struct Args {
  Net pi, vf;
  const float* log_std;
  int n_obs, n_act, n_rows;
  const int64_t* idx;
  const float *obs, *act, *old_logp, *adv, *ret;
  float lo, hi, clip, vf_coef, inv_n;
  const float* head;     // adv mean, std + 1e-8
  float* slabs;
  int stride;            // floats per slab: n_params + 3 (policy loss, value loss, clipped rows), padded to 4
};

// offsets of the 13 tensors in the flat gradient (gpd_mlp_policy's field order)
struct Offsets {
  int pw1, pb1, pw2, pb2, pw3, pb3, vw1, vb1, vw2, vb2, vw3, vb3, ls, n;
};
__host__ __device__ inline Offsets offsets(int n_obs, int n_act) {
  Offsets o;
  int p = 0;
  o.pw1 = p; p += H * n_obs;
  o.pb1 = p; p += H;
  o.pw2 = p; p += H * H;
  o.pb2 = p; p += H;
  o.pw3 = p; p += n_act * H;
  o.pb3 = p; p += n_act;
  o.vw1 = p; p += H * n_obs;
  o.vb1 = p; p += H;
  o.vw2 = p; p += H * H;
  o.vb2 = p; p += H;
  o.vw3 = p; p += H;
  o.vb3 = p; p += 1;
  o.ls = p; p += n_act;
  o.n = p;
  return o;
}

struct Lds {
  float xt[kMaxKc * 16 * kXs];          // the group's input rows, k-major: xt[k * kXs + row], 0 past n_obs
  float h1v[H * kXs], h1p[H * kXs];     // layer-1 activations, neuron-major
  float dzv[H * kXs], dzp[H * kXs];     // dL/dz2, neuron-major
  Part part;                            // per wave: its 16 neurons' share of the output sums
  float rowv[kM][kRv];                  // per row: dL/dmu 0..7, dL/dv 8, (9..15 zero), dL/dlog_std 16..23,
                                        // policy loss 24, value loss 25, clipped 26
  float red[4][4][H];                   // the bias gradients' partial sums per lane group
};

// one network's registers of a lane: the forward B operands, W2 transposed for dh1, the accumulators
template <int KQ>
struct NetRegs {
  static constexpr int KC = (KQ + 3) / 4;
  float w1[KQ], w2[16], w2t[16], b1, b2;
  f4 dw1[KC], dw2[4], dw3;
  float db1, db2;
};

template <int KQ>
__device__ inline void load_net(NetRegs<KQ>& R, const Net& N, int n_obs, int j, int g, int col) {
  load_slice<KQ>(R.w1, N.w1 + (size_t)j * n_obs, k_of<KQ>(g, 0), n_obs);
  load_slice<16>(R.w2, N.w2 + (size_t)j * H, k_of<16>(g, 0), H);
#pragma unroll
  for (int s = 0; s < 16; ++s) R.w2t[s] = N.w2[k_of<16>(g, s) * H + col];
  R.b1 = N.b1[j]; R.b2 = N.b2[j];
  const f4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NetRegs<KQ>::KC; ++c) R.dw1[c] = z;
#pragma unroll
  for (int c = 0; c < 4; ++c) R.dw2[c] = z;
  R.dw3 = z;
  R.db1 = 0.0f; R.db2 = 0.0f;
}

// a group's loads of one thread: row i = t >> 4 of the group, columns (t & 15) + 16 u
template <int KQ>
struct Group {
  float x[NetRegs<KQ>::KC];
  float act, old_logp, adv, ret;
};

__device__ inline int64_t source_row(const Args& A, int row) {
  if (row >= A.n_rows) return 0;
  return A.idx ? A.idx[row] : (int64_t)row;
}

template <int KQ>
__device__ inline void load_group(Group<KQ>& G, const Args& A, int64_t src, int row, int c) {
  const bool on = row < A.n_rows;
  const float* __restrict__ xr = A.obs + (size_t)src * A.n_obs;
#pragma unroll
  for (int u = 0; u < NetRegs<KQ>::KC; ++u) G.x[u] = on && c + 16 * u < A.n_obs ? xr[c + 16 * u] : 0.0f;
  G.act = on && c < A.n_act ? A.act[(size_t)src * A.n_act + c] : 0.0f;
  G.old_logp = on ? A.old_logp[src] : 0.0f;
  G.adv = on ? A.adv[src] : 0.0f;
  G.ret = on ? A.ret[src] : 0.0f;
}

// the row-sum products of one network for one group (see the head of the file)
template <int KQ>
__device__ inline void backward(Lds& L, NetRegs<KQ>& R, const float* h1l, float* dzl, const float (&h1)[4],
                                const f4& h2, const float (&dh2)[4], int j, int g, int i) {
  f4 dz2;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    dz2[r] = dh2[r] * (1.0f - h2[r] * h2[r]);
    dzl[j * kXs + 4 * g + r] = dz2[r];
  }
  R.db2 += (dz2[0] + dz2[1]) + (dz2[2] + dz2[3]);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    R.dw3 = __builtin_amdgcn_mfma_f32_16x16x4f32(h2[s], L.rowv[4 * g + s][i], R.dw3, 0, 0, 0);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      R.dw2[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(dz2[s], h1l[(16 * c + i) * kXs + 4 * g + s], R.dw2[c], 0, 0, 0);
  }
  __syncthreads();   // dz of all four waves
  f4 dh1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 16; ++s)
    dh1 = __builtin_amdgcn_mfma_f32_16x16x4f32(dzl[k_of<16>(g, s) * kXs + i], R.w2t[s], dh1, 0, 0, 0);
  f4 dz1;
#pragma unroll
  for (int r = 0; r < 4; ++r) dz1[r] = dh1[r] * (1.0f - h1[r] * h1[r]);
  R.db1 += (dz1[0] + dz1[1]) + (dz1[2] + dz1[3]);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int c = 0; c < NetRegs<KQ>::KC; ++c)
      R.dw1[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(dz1[s], L.xt[(16 * c + i) * kXs + 4 * g + s], R.dw1[c], 0, 0, 0);
  }
}

// a block's accumulators of one network -> its slab (neuron of D row 4g + r: 16w + 4g + r; column i)
template <int KQ>
__device__ inline void store_net(float* __restrict__ slab, const NetRegs<KQ>& R, int n_obs, int ow1, int ow2, int w,
                                 int g, int i) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int jj = 16 * w + 4 * g + r;
#pragma unroll
    for (int c = 0; c < NetRegs<KQ>::KC; ++c)
      if (16 * c + i < n_obs) slab[ow1 + jj * n_obs + 16 * c + i] = R.dw1[c][r];
#pragma unroll
    for (int c = 0; c < 4; ++c) slab[ow2 + jj * H + 16 * c + i] = R.dw2[c][r];
  }
}

template <int KQ>
__global__ void __launch_bounds__(kBlock) gpd_ppo_grad_kernel(Args A) {
  __shared__ Lds L;
  constexpr int KC = NetRegs<KQ>::KC;
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int g = l >> 4, i = l & 15, j = 16 * w + i;
  const int ri = t >> 4, c = t & 15;       // per-row phases: row ri of the group, column c
  const int na = A.n_act;
  int row0 = blockIdx.x * kM;
  const int stride = gridDim.x * kM;
  // every group's loads are issued a group ahead, its source row (idx) two groups ahead
  int64_t src = source_row(A, row0 + ri);
  int64_t src_next = source_row(A, row0 + stride + ri);
  Group<KQ> G;
  load_group(G, A, src, row0 + ri, c);
  NetRegs<KQ> P, V;
  load_net(P, A.pi, A.n_obs, j, g, j);
  load_net(V, A.vf, A.n_obs, j, g, j);
  float w3p[kMaxAct];
#pragma unroll
  for (int a = 0; a < kMaxAct; ++a) w3p[a] = a < na ? A.pi.w3[a * H + j] : 0.0f;
  const float w3v = A.vf.w3[j];
  const float b3c = c < na ? A.pi.b3[c] : (c == kV ? A.vf.b3[0] : 0.0f);
  const float ls = c < na ? A.log_std[c] : 0.0f;
  const float sc = expf(ls), var = sc * sc;
  const float mean = A.head[0], den = A.head[1];
  float racc = 0.0f;                       // thread t < 27: the sum over rows of rowv's column t
  for (; row0 < A.n_rows; row0 += stride) {
#pragma unroll
    for (int u = 0; u < KC; ++u) L.xt[(c + 16 * u) * kXs + ri] = G.x[u];
    const float act = G.act, old_logp = G.old_logp, adv = G.adv, ret = G.ret;
    const bool valid = row0 + ri < A.n_rows;
    __syncthreads();
    if (row0 + stride < A.n_rows) load_group(G, A, src_next, row0 + stride + ri, c);
    src_next = source_row(A, row0 + 2 * stride + ri);
    // ---- forward, as gpd_policy.hip's forward<>: the K order, tile offsets and output sums are gpd_policy_mlp.h's
    f4 av = {0.f, 0.f, 0.f, 0.f}, ap = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KQ; ++s) {
      const float x = L.xt[a_off<KQ>(g, s, i)];
      av = __builtin_amdgcn_mfma_f32_16x16x4f32(x, V.w1[s], av, 0, 0, 0);
      ap = __builtin_amdgcn_mfma_f32_16x16x4f32(x, P.w1[s], ap, 0, 0, 0);
    }
    float h1v[4], h1p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      h1v[r] = tanhf(av[r] + V.b1);
      h1p[r] = tanhf(ap[r] + P.b1);
      L.h1v[j * kXs + 4 * g + r] = h1v[r];
      L.h1p[j * kXs + 4 * g + r] = h1p[r];
    }
    __syncthreads();
    av = f4{0.f, 0.f, 0.f, 0.f};
    ap = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int o = a_off<16>(g, s, i);
      av = __builtin_amdgcn_mfma_f32_16x16x4f32(L.h1v[o], V.w2[s], av, 0, 0, 0);
      ap = __builtin_amdgcn_mfma_f32_16x16x4f32(L.h1p[o], P.w2[s], ap, 0, 0, 0);
    }
    f4 h2v, h2p;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      h2v[r] = tanhf(av[r] + V.b2);
      h2p[r] = tanhf(ap[r] + P.b2);
      const float sv = out_share(w3v, h2v[r]);
      if (i == 0) L.part[w][4 * g + r][kV] = sv;
#pragma unroll
      for (int a = 0; a < kMaxAct; ++a) {
        if (a < na) {
          const float sp = out_share(w3p[a], h2p[r]);
          if (i == 0) L.part[w][4 * g + r][a] = sp;
        }
      }
    }
    __syncthreads();
    // ---- per row (thread = row ri, column c; the row's 16 threads are one DPP row): c < na holds
    // mu_c, c == 8 the value
    float out = 0.0f;
    if (c < na || c == kV) out = out_sum(L.part, ri, c) + b3c;
    const float d = c < na ? act - out : 0.0f;
    // torch.distributions.Normal.log_prob: -((value - loc) ** 2) / (2 * var) - log(scale) - log(sqrt(2 pi))
    const float lp = c < na ? -(d * d) / (2.0f * var) - ls - 0.91893853320467274f : 0.0f;
    const float logp = row16_sum(lp);
    const float ratio = expf(logp - old_logp);
    const float an = (adv - mean) / den;
    const float s1 = ratio * an, s2 = fminf(fmaxf(ratio, A.lo), A.hi) * an;
    // min(s1, s2): the gradient reaches ratio through s1, and through s2 inside the clip range
    const bool flow = s1 < s2 || (ratio >= A.lo && ratio <= A.hi);
    const float dlogp = valid && flow ? -(an * ratio) * A.inv_n : 0.0f;
    float dout = 0.0f;
    if (c < na) dout = dlogp * (d / var);
    const float verr = out - ret;
    if (c == kV && valid) dout = (A.vf_coef * 2.0f) * verr * A.inv_n;
    L.rowv[ri][c] = dout;
    if (c < kMaxAct) L.rowv[ri][16 + c] = c < na ? dlogp * (d * d / var - 1.0f) : 0.0f;
    if (c == 0) {
      L.rowv[ri][24] = valid ? -fminf(s1, s2) * A.inv_n : 0.0f;
      L.rowv[ri][26] = valid && fabsf(ratio - 1.0f) > A.clip ? 1.0f : 0.0f;
    }
    if (c == kV) L.rowv[ri][25] = valid ? verr * verr * A.inv_n : 0.0f;
    __syncthreads();
    if (t < 27) {
      float s = 0.0f;
#pragma unroll
      for (int r = 0; r < kM; ++r) s += L.rowv[r][t];
      racc += s;
    }
    // ---- backward: dh2 = dOut W3 (VALU: K = n_act, 1 for the critic), then the MFMA products
    float dh2v[4], dh2p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      dh2v[r] = L.rowv[4 * g + r][kV] * w3v;
      float s = 0.0f;
#pragma unroll
      for (int a = 0; a < kMaxAct; ++a)
        if (a < na) s += L.rowv[4 * g + r][a] * w3p[a];
      dh2p[r] = s;
    }
    // (the critic's pass ends with its reads of L.xt and L.h1v; the actor's barrier inside
    // backward() then also orders them before the next group's staging)
    backward<KQ>(L, V, L.h1v, L.dzv, h1v, h2v, dh2v, j, g, i);
    backward<KQ>(L, P, L.h1p, L.dzp, h1p, h2p, dh2p, j, g, i);
    __syncthreads();   // xt, h1, part and rowv are rewritten by the next group
  }
  // ---- the block's slab
  const Offsets O = offsets(A.n_obs, na);
  float* __restrict__ slab = A.slabs + (size_t)blockIdx.x * A.stride;
  store_net<KQ>(slab, P, A.n_obs, O.pw1, O.pw2, w, g, i);
  store_net<KQ>(slab, V, A.n_obs, O.vw1, O.vw2, w, g, i);
#pragma unroll
  for (int r = 0; r < 4; ++r) {   // dW3^T: D[neuron 16w + 4g + r][output i]
    const int jj = 16 * w + 4 * g + r;
    if (i < na) slab[O.pw3 + i * H + jj] = P.dw3[r];
    if (i == kV) slab[O.vw3 + jj] = V.dw3[r];
  }
  // bias gradients: this lane's rows 4g .. 4g + 3 of neuron j; the four lane groups in order
  L.red[0][g][j] = P.db1; L.red[1][g][j] = P.db2; L.red[2][g][j] = V.db1; L.red[3][g][j] = V.db2;
  __syncthreads();
  {
    const int q = t >> 6, n = t & 63;
    const float s = ((L.red[q][0][n] + L.red[q][1][n]) + L.red[q][2][n]) + L.red[q][3][n];
    slab[(q == 0 ? O.pb1 : q == 1 ? O.pb2 : q == 2 ? O.vb1 : O.vb2) + n] = s;
  }
  if (t < na) slab[O.pb3 + t] = racc;
  if (t == kV) slab[O.vb3] = racc;
  if (t >= 16 && t < 16 + na) slab[O.ls + t - 16] = racc;
  if (t >= 24 && t < 27) slab[O.n + t - 24] = racc;
}

// The sum of v over threads 0 .. N - 1 of a block of kThreads, by a fixed halving tree through sh[N], in
// every thread.  A caller that goes on to reuse sh synchronises first.
template <typename T, int N, int kThreads = N>
__device__ inline T block_tree_sum(T v, T* sh) {
  const int t = threadIdx.x;
  if (kThreads == N || t < N) sh[t] = v;
  __syncthreads();
  for (int s = N / 2; s > 0; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  return sh[0];
}

// adv[idx] of rows r0 + u * kStatsThreads (0 past n): eight gathers in flight per thread and trip (a
// thread's rows: t, t + 1024, ...; 16 at 16 384 rows)
__device__ inline void gather_adv(float (&v)[kStatsBatch], int r0, int n, const int64_t* __restrict__ idx,
                                  const float* __restrict__ adv) {
#pragma unroll
  for (int u = 0; u < kStatsBatch; ++u) {
    const int r = r0 + u * kStatsThreads;
    v[u] = r < n ? adv[idx ? idx[r] : (int64_t)r] : 0.0f;
  }
}

// mean and unbiased std (torch .std()) of adv[idx]: two passes, every thread a strided share in
// double, the shares added by a fixed tree: the order depends on n_rows alone
__global__ void __launch_bounds__(kStatsThreads) gpd_ppo_adv_stats_kernel(int n, const int64_t* __restrict__ idx,
                                                                          const float* __restrict__ adv,
                                                                          float* __restrict__ head) {
  __shared__ double sh[kStatsThreads];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int r0 = t; r0 < n; r0 += kStatsBatch * kStatsThreads) {
    float v[kStatsBatch];
    gather_adv(v, r0, n, idx, adv);
#pragma unroll
    for (int u = 0; u < kStatsBatch; ++u) s += (double)v[u];
  }
  const double mean = block_tree_sum<double, kStatsThreads>(s, sh) / (double)n;
  __syncthreads();   // sh is written again below
  double q = 0.0;
  for (int r0 = t; r0 < n; r0 += kStatsBatch * kStatsThreads) {
    float v[kStatsBatch];
    gather_adv(v, r0, n, idx, adv);
#pragma unroll
    for (int u = 0; u < kStatsBatch; ++u) {
      const double d = (double)v[u] - mean;
      if (r0 + u * kStatsThreads < n) q += d * d;
    }
  }
  // (n == 1: 0 / 0 = NaN, as torch)
  const double var = block_tree_sum<double, kStatsThreads>(q, sh) / (double)(n - 1);
  if (t == 0) {
    head[0] = (float)mean;
    head[1] = (float)sqrt(var) + 1e-8f;
  }
}

// grad[e] = the slabs' e in block order; a partial squared norm per block (fixed tree); the three
// loss sums to head[4..6]
__global__ void __launch_bounds__(256) gpd_ppo_reduce_kernel(const float* __restrict__ slabs, int n_slabs, int stride,
                                                             int n_params, float* __restrict__ grad,
                                                             float* __restrict__ head) {
  __shared__ float sh[256];
  const int t = threadIdx.x, e = blockIdx.x * 256 + t;
  float s = 0.0f;
  if (e < stride) {
#pragma unroll 8
    for (int b = 0; b < n_slabs; ++b) s += slabs[(size_t)b * stride + e];
    if (e < n_params) grad[e] = s;
    else if (e < n_params + 3) head[4 + e - n_params] = s;
  }
  const float sq = block_tree_sum<float, 256>(e < n_params ? s * s : 0.0f, sh);
  if (t == 0) head[kHead + blockIdx.x] = sq;
}

__global__ void __launch_bounds__(1024) gpd_ppo_finish_kernel(int n_parts, int n_params, int n_rows, float max_grad_norm,
                                                              float* __restrict__ grad, const float* __restrict__ head,
                                                              float* __restrict__ stats) {
  __shared__ float sh[kNormParts];
  const int t = threadIdx.x;
  // a fixed tree over the blocks' partial norms
  const float sq = block_tree_sum<float, kNormParts, 1024>(t < n_parts ? head[kHead + t] : 0.0f, sh);
  const float norm = sqrtf(sq);
  // torch clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
  const float scale = max_grad_norm > 0.0f ? fminf(1.0f, max_grad_norm / (norm + 1e-6f)) : 1.0f;
  if (scale < 1.0f)
    for (int e = threadIdx.x; e < n_params; e += 1024) grad[e] *= scale;
  if (threadIdx.x == 0) {
    stats[0] = head[4];
    stats[1] = head[5];
    stats[2] = norm;
    stats[3] = head[6] / (float)n_rows;
  }
}

int n_blocks(int n_rows, int max_blocks) {
  const int groups = (n_rows + kM - 1) / kM;
  const int cap = max_blocks > 0 ? max_blocks : kDefaultBlocks;
  return groups < cap ? groups : cap;
}
int slab_stride(int n_params) { return (n_params + 3 + 3) & ~3; }

}  // namespace

extern "C" {

int gpd_policy_n_params(int n_obs, int n_act) {
  if (n_obs < 1 || n_obs > GPD_POLICY_MAX_OBS || n_act < 1 || n_act > GPD_POLICY_MAX_ACT) {
    fail(kEinval, "gpd_policy_n_params: n_obs must be in [1, 192] and n_act in [1, 8]");
    return -1;
  }
  return offsets(n_obs, n_act).n;
}

size_t gpd_policy_ppo_grad_workspace(int n_obs, int n_act, int n_rows, int max_blocks) {
  if (n_obs < 1 || n_obs > GPD_POLICY_MAX_OBS || n_act < 1 || n_act > GPD_POLICY_MAX_ACT || n_rows < 1 ||
      max_blocks < 0) {
    fail(kEinval, "gpd_policy_ppo_grad_workspace: invalid argument");
    return 0;
  }
  const size_t slabs = (size_t)n_blocks(n_rows, max_blocks) * slab_stride(offsets(n_obs, n_act).n);
  return (kHead + kNormParts + slabs) * sizeof(float);
}

int gpd_policy_ppo_grad(const gpd_mlp_policy* p, int n_rows, const int64_t* idx, const float* obs, const float* act,
                        const float* old_logp, const float* adv, const float* ret, float clip_range, float vf_coef,
                        float max_grad_norm, float* grad, float* stats, void* workspace, size_t workspace_bytes,
                        int max_blocks, void* stream) {
  const std::string me = "gpd_policy_ppo_grad: ";
  if (!p) return fail(kEinval, me + "NULL policy");
  if (n_rows < 1) return fail(kEinval, me + "n_rows < 1");
  if (p->n_obs < 1 || p->n_obs > GPD_POLICY_MAX_OBS)
    return fail(kEinval, me + "n_obs must be in [1, " + std::to_string(GPD_POLICY_MAX_OBS) + "]");
  if (p->n_act < 1 || p->n_act > GPD_POLICY_MAX_ACT)
    return fail(kEinval, me + "n_act must be in [1, " + std::to_string(GPD_POLICY_MAX_ACT) + "]");
  if (!p->pi_w1 || !p->pi_b1 || !p->pi_w2 || !p->pi_b2 || !p->pi_w3 || !p->pi_b3 || !p->vf_w1 || !p->vf_b1 ||
      !p->vf_w2 || !p->vf_b2 || !p->vf_w3 || !p->vf_b3 || !p->log_std)
    return fail(kEinval, me + "NULL weight");
  if (!obs || !act || !old_logp || !adv || !ret) return fail(kEinval, me + "NULL rollout buffer");
  if (!grad || !stats || !workspace) return fail(kEinval, me + "NULL grad, stats or workspace");
  if (max_blocks < 0) return fail(kEinval, me + "max_blocks < 0");
  const size_t need = gpd_policy_ppo_grad_workspace(p->n_obs, p->n_act, n_rows, max_blocks);
  if (workspace_bytes < need)
    return fail(kEinval, me + "workspace holds " + std::to_string(workspace_bytes) + " bytes, " +
                                      std::to_string(n_rows) + " rows need " + std::to_string(need));
  // the slabs are read as whole floats at any offset; 16 B keeps every slab on a float4 boundary
  if (((uintptr_t)workspace & 15) || ((uintptr_t)grad & 3) || ((uintptr_t)stats & 3) || ((uintptr_t)obs & 3) ||
      ((uintptr_t)act & 3) || ((uintptr_t)old_logp & 3) || ((uintptr_t)adv & 3) || ((uintptr_t)ret & 3) ||
      ((uintptr_t)idx & 7))
    return fail(kEinval, me + "misaligned pointer (workspace 16 B, idx 8 B, floats 4 B)");
  const Offsets O = offsets(p->n_obs, p->n_act);
  float* head = (float*)workspace;
  Args A = {};
  nets_of(p, A.pi, A.vf);
  A.log_std = p->log_std;
  A.n_obs = p->n_obs; A.n_act = p->n_act; A.n_rows = n_rows;
  A.idx = idx; A.obs = obs; A.act = act; A.old_logp = old_logp; A.adv = adv; A.ret = ret;
  // torch rounds the Python scalars 1 - clip, 1 + clip to f32 once
  A.lo = (float)(1.0 - (double)clip_range); A.hi = (float)(1.0 + (double)clip_range); A.clip = clip_range;
  A.vf_coef = vf_coef;
  A.inv_n = 1.0f / (float)n_rows;
  A.head = head;
  A.slabs = head + kHead + kNormParts;
  A.stride = slab_stride(O.n);
  const int grid = n_blocks(n_rows, max_blocks);
  const int parts = (A.stride + 255) / 256;   // <= 133 < kNormParts at n_obs = 192, n_act = 8
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gpd_ppo_adv_stats_kernel, dim3(1), dim3(kStatsThreads), 0, st, n_rows, idx, adv, head);
  with_kq((p->n_obs + 3) / 4, [&](auto kq) {
    hipLaunchKernelGGL((gpd_ppo_grad_kernel<decltype(kq)::value>), dim3(grid), dim3(kBlock), 0, st, A);
  });
  hipLaunchKernelGGL(gpd_ppo_reduce_kernel, dim3(parts), dim3(256), 0, st, A.slabs, grid, A.stride, O.n, grad, head);
  hipLaunchKernelGGL(gpd_ppo_finish_kernel, dim3(1), dim3(1024), 0, st, parts, O.n, n_rows, max_grad_norm, grad, head,
                     stats);
  HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
