// What the inference (fmt.hip) and training (fmt_train.hip) Feature Matching Transformer kernels must
// agree on: the model width, the K/V summary layout, the elu feature map and the two epsilons.
#pragma once
#include "common.h"

namespace tmvs {

constexpr int kD = 32;  // d_model: 8 heads x 4 dims
constexpr float kLnEps = 1e-5f;    // nn.LayerNorm
constexpr float kAttnEps = 1e-6f;  // LinearAttention (FMT.py:17)

// One view's K/V summary, TMVS_KV_NFLOATS floats: KV[h][m][d] = sum_s K[s,h,d] V[s,h,m], then Ksum[h][d]
constexpr int kKV = TMVS_KV_NFLOATS;
constexpr int kv_at(int h, int m, int d) { return h * 16 + m * 4 + d; }
constexpr int ksum_at(int h, int d) { return 128 + h * 4 + d; }
static_assert(kv_at(7, 3, 3) + 1 == ksum_at(0, 0) && ksum_at(7, 3) + 1 == TMVS_KV_NFLOATS, "K/V summary layout");

__device__ __forceinline__ float elu1(float x) { return (x > 0.f ? x : expm1f(x)) + 1.f; }  // elu(x) + 1
__device__ __forceinline__ float elu1_grad(float x) { return x > 0.f ? 1.f : expf(x); }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

}  // namespace tmvs
