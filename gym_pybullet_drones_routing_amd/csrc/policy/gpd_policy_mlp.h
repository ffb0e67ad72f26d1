// gpd_policy_mlp.h — what libgpd_policy.so's two units (gpd_policy.hip: the rollout step and GAE;
// gpd_ppo_grad.hip: the PPO minibatch gradient) share, each written once.  Nothing is here that only
// one unit uses.
// The gradient kernel lands on the rollout kernel's bits for mu and V (act - mu and V - ret of a
// deterministic rollout are exactly 0: tests/test_gpu_policy_shared_forward.py) because both take from
// here what fixes the order of every sum: the K index of an MFMA step (k_of, a_off: the order in which
// a neuron's products are summed), the LDS tile strides (kXs, Part) and the output sum
// (out_share: row16_sum over a wave's 16 neurons; out_sum: the four waves in wave order, then the bias).
// The accumulator updates themselves stay plain statements in each kernel's one unrolled loop body, so
// that its independent MFMA chains interleave as before: a piece that took the chains as objects
// moved the register allocation of both kernels (profiles/policy_shared/README.md).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <type_traits>

#include "gpd_policy.h"

namespace gpd_policy {

// sets gpd_policy_last_error() and returns `code` (gpd_policy.hip, beside g_err; not exported)
__attribute__((visibility("hidden"))) int fail(int code, const std::string& msg);

constexpr int kOk = 0, kEinval = -1, kEhip = -2, kEunsupported = -4;   // gpd.h GPD_OK / GPD_E*

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) return fail(kEhip, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

constexpr int H = GPD_POLICY_HIDDEN;
constexpr int kWaves = 4;                      // waves per block: neurons 16w .. 16w+15 each
constexpr int kBlock = kWaves * 64;
constexpr int kM = 16;                         // rows per group (MFMA M)
constexpr int kXs = kM + 1;                    // LDS row stride of the k-major tiles (odd: no bank conflicts)
constexpr int kRes = 16;                       // LDS stride of a row's outputs (n_act + 2 <= 10)
constexpr int kMaxKq = GPD_POLICY_MAX_OBS / 4;
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float Part[kWaves][kM][kRes];          // per wave: its 16 neurons' share of a row's output sums

struct Net {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
};

template <int CTRL>
__device__ inline float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// the sum over the 16 lanes of a DPP row (lanes 16r .. 16r+15), in every lane of the row
__device__ inline float row16_sum(float v) {
  v += dpp<0x140>(v);   // row_mirror: i <-> 15 - i
  v += dpp<0x141>(v);   // row_half_mirror: i <-> 7 - i within each half
  v += dpp<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  v += dpp<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  return v;
}

// dst[s] = row[k0 + s] (0 past n or when !on); float4 / float2 loads when the slice is 16- / 8-B aligned
template <int N>
__device__ inline void load_slice(float (&dst)[N], const float* __restrict__ row, int k0, int n, bool on = true) {
  if (N % 4 == 0 && on && (n & 3) == 0 && (k0 & 3) == 0 && ((uintptr_t)row & 15) == 0 && k0 + N <= n) {
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
      const float4 v = reinterpret_cast<const float4*>(row + k0)[q];
      dst[4 * q] = v.x; dst[4 * q + 1] = v.y; dst[4 * q + 2] = v.z; dst[4 * q + 3] = v.w;
    }
  } else if (N % 2 == 0 && on && (n & 1) == 0 && (k0 & 1) == 0 && ((uintptr_t)row & 7) == 0 && k0 + N <= n) {
#pragma unroll
    for (int q = 0; q < N / 2; ++q) {   // float2 (KQ = 18: the slices start 72 B apart)
      const float2 v = reinterpret_cast<const float2*>(row + k0)[q];
      dst[2 * q] = v.x; dst[2 * q + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int s = 0; s < N; ++s) dst[s] = on && k0 + s < n ? row[k0 + s] : 0.0f;
  }
}

// ---- the forward pass (lane l of wave w: g = l >> 4, i = l & 15, neuron j = 16 w + i)
// The K index of MFMA step s and operand slot g of a layer of KQ steps is g KQ + s (not 4 s + g): a
// lane's weights of one layer are then contiguous in the row-major nn.Linear weight, so they arrive
// as float4 loads (a quarter of the load instructions; one scalar load per element took ~2 us of
// address processing per launch).
template <int KQ>
__device__ constexpr int k_of(int g, int s) { return g * KQ + s; }

// LDS offset of A[row i][k = k_of(g, s)] in a k-major tile (the staged rows, or a neuron-major h1
// tile read as the next layer's A operand)
template <int KQ>
__device__ constexpr int a_off(int g, int s, int i) { return k_of<KQ>(g, s) * kXs + i; }

// this wave's 16 neurons' share of one output of a row: w3 * h2 summed over the DPP row (the 16 lanes
// of one g); lane i == 0 stores it to part[w][row][o]
__device__ inline float out_share(float w3, float h2) { return row16_sum(w3 * h2); }

// output o of a row before its bias: the four waves' shares in wave order (the callers add the bias to
// this sum, last)
__device__ inline float out_sum(const Part& part, int row, int o) {
  float acc = part[0][row][o];
#pragma unroll
  for (int ww = 1; ww < kWaves; ++ww) acc += part[ww][row][o];
  return acc;
}

// The weight slices live in VGPRs: the layer-1 slice is sized by the obs width's bucket (18 / 36: the
// KIN observation of one / two RPM drones, 72 / 144 wide, without padding MFMA steps).
// f(std::integral_constant<int, KQ>) for the bucket of kq = n_obs rounded up to 4, / 4.
template <class F>
inline auto with_kq(int kq, F&& f) {
  if (kq <= 8) return f(std::integral_constant<int, 8>{});
  if (kq <= 16) return f(std::integral_constant<int, 16>{});
  if (kq <= 18) return f(std::integral_constant<int, 18>{});
  if (kq <= 24) return f(std::integral_constant<int, 24>{});
  if (kq <= 36) return f(std::integral_constant<int, 36>{});
  return f(std::integral_constant<int, kMaxKq>{});
}

inline void nets_of(const gpd_mlp_policy* p, Net& pi, Net& vf) {
  pi = {p->pi_w1, p->pi_b1, p->pi_w2, p->pi_b2, p->pi_w3, p->pi_b3};
  vf = {p->vf_w1, p->vf_b1, p->vf_w2, p->vf_b2, p->vf_w3, p->vf_b3};
}

}  // namespace gpd_policy
