// DepthNet view aggregation and the stage-1 PixelwiseNet in train mode, forward and backward
// (SURVEY.md 8f rank 2, config C5): models/TransMVSNet.py:10-30 (PixelwiseNet: 1x1x1 Conv3d 1->16
// + BatchNorm3d + ReLU, 16->8 + BatchNorm3d + ReLU, 8->1 + bias, sigmoid, max over D) and :71-93
// (sim = sum_v w_v sim_v / (1e-5 + sum_v w_v), views in order).
//
// A batch of B samples; per-view similarity volumes sims [B][V][D][P] (P = H*W). PixelwiseNet runs per
// view on that view's [B,1,D,h,w] volume (models/TransMVSNet.py:71-77), so its BatchNorm batch statistics
// are joint over the B*D*P elements of the view's B chunks, which lie V*D*P floats apart: every pass walks
// the view's elements in (sample, depth, pixel) order through a BatchWalk, one launch whatever B is. The
// single-sample entry points are the B = 1 case of the same kernels.
// Parameters (device, fp32, "pwp"): w0[16] g0[16] b0[16] W1[8][16] g1[8] b1[8] w2[8] b2 (201).
// Per-view statistics ("st", fp32): mean0[16] var0[16] mean1[8] var1[8] (biased variances).
// Every reduction is fp64 block partials + a fixed-order combine (deterministic, no atomics);
// the backward recomputes the forward chain per element instead of storing 24 channels per voxel.
#include "train_reduce.h"
#include "../../include/transmvs_sync.h"

namespace tmvs {

constexpr int kPwBlock = 256;
constexpr int PW_W0 = 0, PW_G0 = 16, PW_B0 = 32, PW_W1 = 48, PW_G1 = 176, PW_B1 = 184, PW_W2 = 192, PW_B2 = 200;
constexpr int ST_M0 = 0, ST_V0 = 16, ST_M1 = 32, ST_V1 = 40;
constexpr float kPwEps = 1e-5f;

// A thread's walk over the rows [i0, i1) of a view's batch, 256 rows per step: row i is row r = i % n of
// sample b = i / n (n rows per sample: D*P elements or P pixels). One division at the start, then carries.
struct BatchWalk {
  long n, b, r;
  __device__ __forceinline__ BatchWalk(long i, long n_) : n(n_), b(i / n_), r(i - (i / n_) * n_) {}
  __device__ __forceinline__ void step() {
    r += kPwBlock;
    while (r >= n) {
      r -= n;
      ++b;
    }
  }
};

struct PwChain {  // one element's forward chain
  float y0[16], pre1[8], y1[8], xhat1[8];
  float o, sg;
};

__device__ __forceinline__ void bn_coef(float mean, float var, float g, float b, float& a, float& sh, float& rstd) {
  rstd = 1.f / sqrtf(var + kPwEps);
  a = rstd * g;
  sh = fmaf(-mean, a, b);
}

// z0 -> y0 (and, if pre0 given, the pre-ReLU values), z1 = W1 y0
__device__ __forceinline__ void pw_layer0(float s, const float* __restrict__ p, const float* __restrict__ st,
                                          float (&y0)[16], float (&z1)[8], float* pre0 = nullptr) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    float a, sh, rstd;
    bn_coef(st[ST_M0 + j], st[ST_V0 + j], p[PW_G0 + j], p[PW_B0 + j], a, sh, rstd);
    const float pre = fmaf(p[PW_W0 + j] * s, a, sh);
    if (pre0) pre0[j] = pre;
    y0[j] = relu(pre);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc = fmaf(p[PW_W1 + k * 16 + j], y0[j], acc);
    z1[k] = acc;
  }
}

__device__ __forceinline__ void pw_chain(float s, const float* __restrict__ p, const float* __restrict__ st,
                                         PwChain& c) {
  float z1[8];
  pw_layer0(s, p, st, c.y0, z1);
  float o = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float a, sh, rstd;
    bn_coef(st[ST_M1 + k], st[ST_V1 + k], p[PW_G1 + k], p[PW_B1 + k], a, sh, rstd);
    c.pre1[k] = fmaf(z1[k], a, sh);
    c.xhat1[k] = (z1[k] - st[ST_M1 + k]) * rstd;
    c.y1[k] = relu(c.pre1[k]);
    o = fmaf(p[PW_W2 + k], c.y1[k], o);
  }
  c.o = o + p[PW_B2];
  c.sg = 1.f / (1.f + expf(-c.o));
}

// ---------------------------------------------------------------- forward
// stats of s (sum, sum^2) -> layer-0 statistics mean0 = w0*mean_s, var0 = w0^2 * var_s
// (s: the view's chunk of sample 0; sample b's is b * bstride floats on; n = D*P per sample, tot = B*n)
__global__ __launch_bounds__(kPwBlock) void pw_s_partial_kernel(const float* __restrict__ s, long n, long tot,
                                                                long bstride, long vpb,
                                                                double* __restrict__ partial) {
  const long i0 = (long)blockIdx.x * vpb, i1 = i0 + vpb < tot ? i0 + vpb : tot;
  double v[2] = {0.0, 0.0};
  BatchWalk k(i0 + threadIdx.x, n);
  for (long i = i0 + threadIdx.x; i < i1; i += kPwBlock, k.step()) {
    const double x = (double)s[k.b * bstride + k.r];
    v[0] += x;
    v[1] += x * x;
  }
  block_sum_store<false>(v, partial + (size_t)blockIdx.x * 2);
}

__global__ void pw_stats0_kernel(const double* __restrict__ sums, long n, const float* __restrict__ p,
                                 float* __restrict__ st) {
  const int j = threadIdx.x;
  if (j >= 16) return;
  const double m = sums[0] / (double)n;
  double var = sums[1] / (double)n - m * m;
  var = var > 0.0 ? var : 0.0;
  const double w = (double)p[PW_W0 + j];
  st[ST_M0 + j] = (float)(w * m);
  st[ST_V0 + j] = (float)(w * w * var);
}

__global__ __launch_bounds__(kPwBlock) void pw_z1_partial_kernel(const float* __restrict__ s, long n, long tot,
                                                                 long bstride, long vpb,
                                                                 const float* __restrict__ p,
                                                                 const float* __restrict__ st,
                                                                 double* __restrict__ partial) {
  const long i0 = (long)blockIdx.x * vpb, i1 = i0 + vpb < tot ? i0 + vpb : tot;
  double v[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = 0.0;
  BatchWalk wk(i0 + threadIdx.x, n);
  for (long i = i0 + threadIdx.x; i < i1; i += kPwBlock, wk.step()) {
    float y0[16], z1[8];
    pw_layer0(s[wk.b * bstride + wk.r], p, st, y0, z1);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      v[k] += (double)z1[k];
      v[8 + k] += (double)z1[k] * (double)z1[k];
    }
  }
  block_sum_store<true>(v, partial + (size_t)blockIdx.x * 16);
}

__global__ void pw_stats1_kernel(const double* __restrict__ sums, long n, float* __restrict__ st) {
  const int k = threadIdx.x;
  if (k >= 8) return;
  const double m = sums[k] / (double)n;
  const double var = sums[8 + k] / (double)n - m * m;
  st[ST_M1 + k] = (float)m;
  st[ST_V1 + k] = (float)(var > 0.0 ? var : 0.0);
}

// view weight w[p] = max_d sigmoid(PixelwiseNet(s[d][p])) and its (first) argmax, over the B*P pixels of
// the view's batch (sample b's volume b * bstride floats, its maps b * wstride floats on)
__global__ __launch_bounds__(kPwBlock) void pw_weight_kernel(const float* __restrict__ s, int B, int D, int P,
                                                             long bstride, long wstride,
                                                             const float* __restrict__ p, const float* __restrict__ st,
                                                             float* __restrict__ w, int* __restrict__ dstar) {
  const int bq = blockIdx.x * kPwBlock + threadIdx.x;
  if (bq >= B * P) return;
  const int b = bq / P, q = bq - b * P;
  s += (size_t)b * bstride;
  w += (size_t)b * wstride;
  dstar += (size_t)b * wstride;
  float best = 0.f;
  int bi = 0;
  for (int d = 0; d < D; ++d) {
    PwChain c;
    pw_chain(s[(size_t)d * P + q], p, st, c);
    if (d == 0 || c.sg > best) {
      best = c.sg;
      bi = d;
    }
  }
  w[q] = best;
  dstar[q] = bi;
}

// sim[d][p] = (sum_v sims[v][d][p] * w_v) / (1e-5 + sum_v w_v), views in order; w_v read at
// (y >> shift, x >> shift) of a [V][H>>shift][W>>shift] map (nearest x2^shift up-sampling)
__global__ __launch_bounds__(kPwBlock) void aggregate_train_kernel(const float* __restrict__ sims,
                                                                   const float* __restrict__ w, int V, int D, int H,
                                                                   int W, int shift, float* __restrict__ sim,
                                                                   float* __restrict__ wsum) {
  const int P = H * W;
  const int q = blockIdx.x * kPwBlock + threadIdx.x;
  if (q >= P) return;
  const int y = q / W, x = q - y * W;
  const int Ws = W >> shift, Ps = (H >> shift) * Ws;
  const int qs = (y >> shift) * Ws + (x >> shift);
  float ws = 1e-5f;
  for (int v = 0; v < V; ++v) ws = ws + w[(size_t)v * Ps + qs];
  wsum[q] = ws;
  for (int d = 0; d < D; ++d) {
    float acc = 0.f;
    for (int v = 0; v < V; ++v) acc = acc + sims[((size_t)v * D + d) * P + q] * w[(size_t)v * Ps + qs];
    sim[(size_t)d * P + q] = acc / ws;
  }
}

// ---------------------------------------------------------------- backward
// dsims[v][d][p] = dsim[d][p] / wsum[p] * w_v[p]; dw_v[p] = sum_d dsim/wsum * (sims_v - sim)  (dw optional).
// sims_v - sim is formed as (sims_v * W - sum_u w_u sims_u) / W in fp64, W = 1e-5 + sum_u w_u, where every
// product is exact: subtracting the forward's rounded sim loses the difference to rounding wherever one view
// carries nearly all the weight (a single view: sims - sim = 1e-5 sims / W, below sim's last bits).
__global__ __launch_bounds__(kPwBlock) void aggregate_backward_kernel(
    const float* __restrict__ dsim, const float* __restrict__ sims, const float* __restrict__ wsum,
    const float* __restrict__ w, int V, int D, int H, int W, int shift, float* __restrict__ dsims,
    float* __restrict__ dw) {
  const int P = H * W;
  const int q = blockIdx.x * kPwBlock + threadIdx.x;
  if (q >= P) return;
  const int y = q / W, x = q - y * W;
  const int Ws = W >> shift, Ps = (H >> shift) * Ws;
  const int qs = (y >> shift) * Ws + (x >> shift);
  const float ws = wsum[q];
  double wd = (double)1e-5f;
  if (dw)
    for (int v = 0; v < V; ++v) wd += (double)w[(size_t)v * Ps + qs];
  for (int v = 0; v < V; ++v) {
    const float wv = w[(size_t)v * Ps + qs];
    double acc = 0.0;
    for (int d = 0; d < D; ++d) {
      const float g = dsim[(size_t)d * P + q] / ws;
      const size_t e = ((size_t)v * D + d) * P + q;
      dsims[e] = g * wv;
      if (dw) {
        double a = 0.0;
        for (int u = 0; u < V; ++u) a += (double)w[(size_t)u * Ps + qs] * (double)sims[((size_t)u * D + d) * P + q];
        acc += (double)g * ((double)sims[e] * wd - a);
      }
    }
    if (dw) dw[(size_t)v * P + q] = (float)(acc / wd);
  }
}

// pass 1 (per pixel, at the argmax plane): sums of g1 (8), g1*xhat1 (8), g_o*y1 (8), g_o (1)
__global__ __launch_bounds__(kPwBlock) void pw_bwd1_kernel(const float* __restrict__ s, int D, int P,
                                                           const float* __restrict__ p, const float* __restrict__ st,
                                                           const float* __restrict__ w, const int* __restrict__ dstar,
                                                           const float* __restrict__ dw, int B, long bstride,
                                                           long wstride, long ppb,
                                                           double* __restrict__ partial) {
  double v[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) v[i] = 0.0;
  const long tot = (long)B * P;
  const long q0 = (long)blockIdx.x * ppb, q1 = q0 + ppb < tot ? q0 + ppb : tot;
  BatchWalk wk(q0 + threadIdx.x, P);
  for (long bq = q0 + threadIdx.x; bq < q1; bq += kPwBlock, wk.step()) {
    const long q = wk.r, m = wk.b * wstride + q;  // the pixel, and its place in the [B][V][P] maps
    PwChain c;
    pw_chain(s[wk.b * bstride + (size_t)dstar[m] * P + q], p, st, c);
    const float sg = w[m];
    const float go = dw[m] * ((1.f - sg) * sg);  // sigmoid backward at the argmax
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float g1 = c.pre1[k] > 0.f ? go * p[PW_W2 + k] : 0.f;
      v[k] += (double)g1;
      v[8 + k] += (double)g1 * (double)c.xhat1[k];
      v[16 + k] += (double)go * (double)c.y1[k];
    }
    v[24] += (double)go;
  }
  // the __shfl_xor butterfly: with 25 values the DPP moves raised this kernel to 178 VGPRs (train_reduce.h)
  block_sum_store<false>(v, partial + (size_t)blockIdx.x * 25);
}

// the layer-1 gradient of one element: dz1 = a1 (g1 - S1a/N - xhat1 S1b/N), g1 nonzero at the argmax only
__device__ __forceinline__ void pw_dz1(float s, int d, int ds, float go, const float* __restrict__ p,
                                       const float* __restrict__ st, const double* __restrict__ s1, double inv_n,
                                       float (&y0)[16], float (&pre0)[16], float (&dz1)[8]) {
  float z1[8];
  pw_layer0(s, p, st, y0, z1, pre0);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float a, sh, rstd;
    bn_coef(st[ST_M1 + k], st[ST_V1 + k], p[PW_G1 + k], p[PW_B1 + k], a, sh, rstd);
    const float xhat = (z1[k] - st[ST_M1 + k]) * rstd;
    const float g1 = (d == ds && fmaf(z1[k], a, sh) > 0.f) ? go * p[PW_W2 + k] : 0.f;
    dz1[k] = a * ((g1 - (float)(s1[k] * inv_n)) - xhat * (float)(s1[8 + k] * inv_n));
  }
}

// pass 2 (per element): sums of g0 (16), g0*xhat0 (16), dz1_k * y0_j (128)
__global__ __launch_bounds__(kPwBlock) void pw_bwd2_kernel(const float* __restrict__ s, int D, int P,
                                                           const float* __restrict__ p, const float* __restrict__ st,
                                                           const float* __restrict__ w, const int* __restrict__ dstar,
                                                           const float* __restrict__ dw, const double* __restrict__ s1,
                                                           int B, long bstride, long wstride, long epb,
                                                           long n_total, double* __restrict__ partial) {
  const long n = (long)D * P, tot = (long)B * n;
  // the BatchNorm's count behind s1: the view's whole batch (tot), on all ranks when they share statistics
  const double inv_n = 1.0 / (double)n_total;
  float acc[160];  // g0 sums [0,16), g0*xhat0 sums [16,32), dW1 [32,160)
#pragma unroll
  for (int i = 0; i < 160; ++i) acc[i] = 0.f;
  const long e0 = (long)blockIdx.x * epb, e1 = e0 + epb < tot ? e0 + epb : tot;
  BatchWalk wk(e0 + threadIdx.x, n);
  for (long e = e0 + threadIdx.x; e < e1; e += kPwBlock, wk.step()) {
    const int d = (int)(wk.r / P), q = (int)(wk.r - (long)d * P);
    const long m = wk.b * wstride + q;
    const float sg = w[m];
    const float go = dw[m] * ((1.f - sg) * sg);
    float y0[16], pre0[16], dz1[8];
    const float sv = s[wk.b * bstride + wk.r];
    pw_dz1(sv, d, dstar[m], go, p, st, s1, inv_n, y0, pre0, dz1);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      float dy0 = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        dy0 = fmaf(p[PW_W1 + k * 16 + j], dz1[k], dy0);
        acc[32 + k * 16 + j] = fmaf(dz1[k], y0[j], acc[32 + k * 16 + j]);
      }
      const float g0 = pre0[j] > 0.f ? dy0 : 0.f;
      float a, sh, rstd;
      bn_coef(st[ST_M0 + j], st[ST_V0 + j], p[PW_G0 + j], p[PW_B0 + j], a, sh, rstd);
      const float xhat0 = (p[PW_W0 + j] * sv - st[ST_M0 + j]) * rstd;
      acc[j] += g0;
      acc[16 + j] = fmaf(g0, xhat0, acc[16 + j]);
    }
  }
  block_sum_store<true>(acc, partial + (size_t)blockIdx.x * 160);
}

// pass 3 (per element): dz0 = a0 (g0 - S0a/N - xhat0 S0b/N); dsims += sum_j w0_j dz0_j; sums of dz0*s (16)
__global__ __launch_bounds__(kPwBlock) void pw_bwd3_kernel(const float* __restrict__ s, int D, int P,
                                                           const float* __restrict__ p, const float* __restrict__ st,
                                                           const float* __restrict__ w, const int* __restrict__ dstar,
                                                           const float* __restrict__ dw, const double* __restrict__ s1,
                                                           const double* __restrict__ s2, int B, long bstride,
                                                           long wstride, long epb, long n_total,
                                                           float* __restrict__ dsims, double* __restrict__ partial) {
  const long n = (long)D * P, tot = (long)B * n;
  const double inv_n = 1.0 / (double)n_total;
  double v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = 0.0;
  const long e0 = (long)blockIdx.x * epb, e1 = e0 + epb < tot ? e0 + epb : tot;
  BatchWalk wk(e0 + threadIdx.x, n);
  for (long e = e0 + threadIdx.x; e < e1; e += kPwBlock, wk.step()) {
    const int d = (int)(wk.r / P), q = (int)(wk.r - (long)d * P);
    const long m = wk.b * wstride + q, at = wk.b * bstride + wk.r;
    const float sg = w[m];
    const float go = dw[m] * ((1.f - sg) * sg);
    float y0[16], pre0[16], dz1[8];
    const float sv = s[at];
    pw_dz1(sv, d, dstar[m], go, p, st, s1, inv_n, y0, pre0, dz1);
    float ds = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      float dy0 = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) dy0 = fmaf(p[PW_W1 + k * 16 + j], dz1[k], dy0);
      const float g0 = pre0[j] > 0.f ? dy0 : 0.f;
      float a, sh, rstd;
      bn_coef(st[ST_M0 + j], st[ST_V0 + j], p[PW_G0 + j], p[PW_B0 + j], a, sh, rstd);
      const float xhat0 = (p[PW_W0 + j] * sv - st[ST_M0 + j]) * rstd;
      const float dz0 = a * ((g0 - (float)(s2[j] * inv_n)) - xhat0 * (float)(s2[16 + j] * inv_n));
      ds = fmaf(p[PW_W0 + j], dz0, ds);
      v[j] += (double)dz0 * (double)sv;
    }
    dsims[at] = dsims[at] + ds;
  }
  block_sum_store<true>(v, partial + (size_t)blockIdx.x * 16);
}

// parameter gradients of this view, added to grad[201] (pwp layout)
__global__ void pw_grad_finalize_kernel(const double* __restrict__ s1, const double* __restrict__ s2,
                                        const double* __restrict__ s3, float* __restrict__ grad) {
  const int t = threadIdx.x;
  if (t < 16) {
    grad[PW_W0 + t] += (float)s3[t];
    grad[PW_G0 + t] += (float)s2[16 + t];
    grad[PW_B0 + t] += (float)s2[t];
  }
  if (t < 128) grad[PW_W1 + t] += (float)s2[32 + t];
  if (t < 8) {
    grad[PW_G1 + t] += (float)s1[8 + t];
    grad[PW_B1 + t] += (float)s1[t];
    grad[PW_W2 + t] += (float)s1[16 + t];
  }
  if (t == 0) grad[PW_B2] += (float)s1[24];
}

// element / pixel ranges of the partial passes: at most the 1024 blocks the workspace holds
static Chunk pw_chunk(long n) { return chunk_for(n, 1024, 1024); }

// the aggregate kernels read view_w at (y >> shift, x >> shift) of an [H >> shift][W >> shift] map: a
// remainder would put the last column on the next row's weight and the last row past the view's map
constexpr int kMaxVwShift = 4;
static bool vw_map_covers(int height, int width, int shift) {
  return shift <= kMaxVwShift && !(height & ((1 << shift) - 1)) && !(width & ((1 << shift) - 1));
}

}  // namespace tmvs

using namespace tmvs;

// workspace: partials (<= 1024 blocks x 160 doubles) + sums (2 + 16 + 25 + 160 + 16 doubles)
extern "C" size_t tmvs_pixelwise_train_workspace(void) { return (1024 * 160 + 256) * sizeof(double) + 256; }

// A batch's counts as the kernels index them: B*P pixels and the [B][V][D][P] volume's floats in int / long
static bool pw_batch_fits(int batch, int n_views, int ndepth, int height, int width) {
  const long P = (long)height * width;
  return batch * P < (1L << 31) - kPwBlock && (double)batch * n_views * ndepth * (double)P < 9e18;
}

// One call's geometry and the launch of each stage of a view's passes. The fused entries run a view's stages
// back to back on sums in the workspace; the staged ones (include/transmvs_sync.h) run one stage over all
// views, so that the fp64 sums between two stages can be added over ranks. Same kernels, same arguments.
struct PwGeo {
  int B, V, D, P;
  long n, tot, bstride, wstride;
  Chunk ce, cp;  // element and pixel ranges of the partial passes
  PwGeo(int batch, int n_views, int ndepth, int height, int width)
      : B(batch), V(n_views), D(ndepth), P(height * width), n((long)ndepth * P), tot((long)batch * n),
        bstride((long)n_views * n), wstride((long)n_views * P), ce(pw_chunk(tot)), cp(pw_chunk((long)batch * P)) {}
};

static bool pw_dims_ok(int batch, int n_views, int ndepth, int height, int width) {
  return batch > 0 && n_views > 0 && ndepth > 0 && height > 0 && width > 0;
}

// stage 1: sums[2] = (sum s, sum s^2) of view v
static void pw_fwd_s_sums(const PwGeo& g, const float* sims, int v, double* part, double* sums, hipStream_t st) {
  hipLaunchKernelGGL(pw_s_partial_kernel, dim3(g.ce.blocks), dim3(kPwBlock), 0, st, sims + (size_t)v * g.n, g.n, g.tot,
                     g.bstride, g.ce.rows, part);
  hipLaunchKernelGGL(sum_partials_f64_kernel<>, dim3(2), dim3(kPwBlock), 0, st, (const double*)part, g.ce.blocks, 2,
                     sums);
}

// stage 2: layer-0 statistics from the sums over n_total elements, then sums[16] = (sum z1, sum z1^2)
static void pw_fwd_z1_sums(const PwGeo& g, const float* sims, int v, const float* pwp, const double* s_sums,
                           long n_total, float* sv, double* part, double* sums, hipStream_t st) {
  hipLaunchKernelGGL(pw_stats0_kernel, dim3(1), dim3(64), 0, st, s_sums, n_total, pwp, sv);
  hipLaunchKernelGGL(pw_z1_partial_kernel, dim3(g.ce.blocks), dim3(kPwBlock), 0, st, sims + (size_t)v * g.n, g.n, g.tot,
                     g.bstride, g.ce.rows, pwp, (const float*)sv, part);
  hipLaunchKernelGGL(sum_partials_f64_kernel<>, dim3(16), dim3(kPwBlock), 0, st, (const double*)part, g.ce.blocks, 16,
                     sums);
}

// stage 3: layer-1 statistics, then the view's weights and argmax
static void pw_fwd_weights(const PwGeo& g, const float* sims, int v, const float* pwp, const double* z1_sums,
                           long n_total, float* sv, float* view_w, int* dstar, hipStream_t st) {
  hipLaunchKernelGGL(pw_stats1_kernel, dim3(1), dim3(64), 0, st, z1_sums, n_total, sv);
  hipLaunchKernelGGL(pw_weight_kernel, dim3((g.B * g.P + kPwBlock - 1) / kPwBlock), dim3(kPwBlock), 0, st,
                     sims + (size_t)v * g.n, g.B, g.D, g.P, g.bstride, g.wstride, pwp, (const float*)sv,
                     view_w + (size_t)v * g.P, dstar + (size_t)v * g.P);
}

static int pw_forward(const float* sims, int batch, int n_views, int ndepth, int height, int width, const float* pwp,
                      void* workspace, size_t workspace_bytes, float* stats, float* view_w, int* dstar, void* stream) {
  if (!sims || !pwp || !workspace || !stats || !view_w || !dstar || !pw_dims_ok(batch, n_views, ndepth, height, width))
    return TMVS_ERR_ARG;
  if (workspace_bytes < tmvs_pixelwise_train_workspace()) return TMVS_ERR_ARG;
  if (!pw_batch_fits(batch, n_views, ndepth, height, width)) return TMVS_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const PwGeo g(batch, n_views, ndepth, height, width);
  double* part = (double*)workspace;
  double* sums = part + 1024 * 160;
  for (int v = 0; v < n_views; ++v) {
    float* sv = stats + (size_t)v * 48;
    pw_fwd_s_sums(g, sims, v, part, sums, st);
    pw_fwd_z1_sums(g, sims, v, pwp, sums, g.tot, sv, part, sums, st);
    pw_fwd_weights(g, sims, v, pwp, sums, g.tot, sv, view_w, dstar, st);
    TMVS_CHECK_LAUNCH();
  }
  return TMVS_OK;
}

extern "C" int tmvs_pixelwise_train_forward(const float* sims, int n_views, int ndepth, int height, int width,
                                            const float* pwp, void* workspace, size_t workspace_bytes, float* stats,
                                            float* view_w, int* dstar, void* stream) {
  return pw_forward(sims, 1, n_views, ndepth, height, width, pwp, workspace, workspace_bytes, stats, view_w, dstar,
                    stream);
}

extern "C" int tmvs_pixelwise_train_forward_batched(const float* sims, int batch, int n_views, int ndepth, int height,
                                                    int width, const float* pwp, void* workspace,
                                                    size_t workspace_bytes, float* stats, float* view_w, int* dstar,
                                                    void* stream) {
  return pw_forward(sims, batch, n_views, ndepth, height, width, pwp, workspace, workspace_bytes, stats, view_w, dstar,
                    stream);
}

extern "C" int tmvs_aggregate_train(const float* sims, const float* view_w, int n_views, int ndepth, int height,
                                    int width, int vw_shift, float* sim, float* wsum, void* stream) {
  if (!sims || !view_w || !sim || !wsum || n_views <= 0 || ndepth <= 0 || height <= 0 || width <= 0 || vw_shift < 0)
    return TMVS_ERR_ARG;
  if (!vw_map_covers(height, width, vw_shift)) return TMVS_ERR_SHAPE;
  const int P = height * width;
  hipLaunchKernelGGL(aggregate_train_kernel, dim3((P + kPwBlock - 1) / kPwBlock), dim3(kPwBlock), 0,
                     (hipStream_t)stream, sims, view_w, n_views, ndepth, height, width, vw_shift, sim, wsum);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_aggregate_train_backward(const float* dsim, const float* sims, const float* sim, const float* wsum,
                                             const float* view_w, int n_views, int ndepth, int height, int width,
                                             int vw_shift, float* dsims, float* dview_w, void* stream) {
  if (!dsim || !sims || !sim || !wsum || !view_w || !dsims || n_views <= 0 || ndepth <= 0 || height <= 0 ||
      width <= 0 || vw_shift < 0)
    return TMVS_ERR_ARG;
  if (!vw_map_covers(height, width, vw_shift)) return TMVS_ERR_SHAPE;
  const int P = height * width;
  hipLaunchKernelGGL(aggregate_backward_kernel, dim3((P + kPwBlock - 1) / kPwBlock), dim3(kPwBlock), 0,
                     (hipStream_t)stream, dsim, sims, wsum, view_w, n_views, ndepth, height, width, vw_shift, dsims,
                     dview_w);  // sim: required by the ABI, no longer read
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

struct PwSaved {  // what the backward reads of the forward, per call
  const float *sims, *pwp, *stats, *view_w, *dview_w;
  const int* dstar;
};

// backward stage 1: s1[25] of view v
static void pw_bwd_s1(const PwGeo& g, const PwSaved& f, int v, double* part, double* s1, hipStream_t st) {
  hipLaunchKernelGGL(pw_bwd1_kernel, dim3(g.cp.blocks), dim3(kPwBlock), 0, st, f.sims + (size_t)v * g.n, g.D, g.P,
                     f.pwp, f.stats + (size_t)v * 48, f.view_w + (size_t)v * g.P, f.dstar + (size_t)v * g.P,
                     f.dview_w + (size_t)v * g.P, g.B, g.bstride, g.wstride, g.cp.rows, part);
  hipLaunchKernelGGL(sum_partials_f64_kernel<>, dim3(25), dim3(kPwBlock), 0, st, (const double*)part, g.cp.blocks, 25,
                     s1);
}

// backward stage 2: s2[160] of view v from the BatchNorm sums of s1 over n_total elements
static void pw_bwd_s2(const PwGeo& g, const PwSaved& f, int v, const double* s1, long n_total, double* part,
                      double* s2, hipStream_t st) {
  hipLaunchKernelGGL(pw_bwd2_kernel, dim3(g.ce.blocks), dim3(kPwBlock), 0, st, f.sims + (size_t)v * g.n, g.D, g.P,
                     f.pwp, f.stats + (size_t)v * 48, f.view_w + (size_t)v * g.P, f.dstar + (size_t)v * g.P,
                     f.dview_w + (size_t)v * g.P, s1, g.B, g.bstride, g.wstride, g.ce.rows, n_total, part);
  hipLaunchKernelGGL(sum_partials_f64_kernel<>, dim3(160), dim3(kPwBlock), 0, st, (const double*)part, g.ce.blocks,
                     160, s2);
}

// backward stage 3: dsims and s3[16] of view v from the BatchNorm sums of s1 and s2 over n_total elements
static void pw_bwd_s3(const PwGeo& g, const PwSaved& f, int v, const double* s1, const double* s2, long n_total,
                      float* dsims, double* part, double* s3, hipStream_t st) {
  hipLaunchKernelGGL(pw_bwd3_kernel, dim3(g.ce.blocks), dim3(kPwBlock), 0, st, f.sims + (size_t)v * g.n, g.D, g.P,
                     f.pwp, f.stats + (size_t)v * 48, f.view_w + (size_t)v * g.P, f.dstar + (size_t)v * g.P,
                     f.dview_w + (size_t)v * g.P, s1, s2, g.B, g.bstride, g.wstride, g.ce.rows, n_total,
                     dsims + (size_t)v * g.n, part);
  hipLaunchKernelGGL(sum_partials_f64_kernel<>, dim3(16), dim3(kPwBlock), 0, st, (const double*)part, g.ce.blocks, 16,
                     s3);
}

static int pw_backward(const float* sims, int batch, int n_views, int ndepth, int height, int width, const float* pwp,
                       const float* stats, const float* view_w, const int* dstar, const float* dview_w,
                       void* workspace, size_t workspace_bytes, float* dsims, float* dpwp, void* stream) {
  if (!sims || !pwp || !stats || !view_w || !dstar || !dview_w || !workspace || !dsims || !dpwp ||
      !pw_dims_ok(batch, n_views, ndepth, height, width))
    return TMVS_ERR_ARG;
  if (workspace_bytes < tmvs_pixelwise_train_workspace()) return TMVS_ERR_ARG;
  if (!pw_batch_fits(batch, n_views, ndepth, height, width)) return TMVS_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const PwGeo g(batch, n_views, ndepth, height, width);
  const PwSaved f{sims, pwp, stats, view_w, dview_w, dstar};
  double* part = (double*)workspace;
  double* s1 = part + 1024 * 160;
  double* s2 = s1 + 32;
  double* s3 = s2 + 160;
  for (int v = 0; v < n_views; ++v) {
    pw_bwd_s1(g, f, v, part, s1, st);
    pw_bwd_s2(g, f, v, s1, g.tot, part, s2, st);
    pw_bwd_s3(g, f, v, s1, s2, g.tot, dsims, part, s3, st);
    hipLaunchKernelGGL(pw_grad_finalize_kernel, dim3(1), dim3(128), 0, st, (const double*)s1, (const double*)s2,
                       (const double*)s3, dpwp);
    TMVS_CHECK_LAUNCH();
  }
  return TMVS_OK;
}

extern "C" int tmvs_pixelwise_train_backward(const float* sims, int n_views, int ndepth, int height, int width,
                                             const float* pwp, const float* stats, const float* view_w,
                                             const int* dstar, const float* dview_w, void* workspace,
                                             size_t workspace_bytes, float* dsims, float* dpwp, void* stream) {
  return pw_backward(sims, 1, n_views, ndepth, height, width, pwp, stats, view_w, dstar, dview_w, workspace,
                     workspace_bytes, dsims, dpwp, stream);
}

extern "C" int tmvs_pixelwise_train_backward_batched(const float* sims, int batch, int n_views, int ndepth, int height,
                                                     int width, const float* pwp, const float* stats,
                                                     const float* view_w, const int* dstar, const float* dview_w,
                                                     void* workspace, size_t workspace_bytes, float* dsims,
                                                     float* dpwp, void* stream) {
  return pw_backward(sims, batch, n_views, ndepth, height, width, pwp, stats, view_w, dstar, dview_w, workspace,
                     workspace_bytes, dsims, dpwp, stream);
}

// ---------------------------------------------------------------- statistics synchronised across ranks
// (include/transmvs_sync.h) The passes above stage-major over the views: each entry runs one stage for all V
// views and returns (or takes) that stage's fp64 sums [V][K], so one collective per stage serves every view.
// Fed the local sums and n_total = B*D*P, the six entries are tmvs_pixelwise_train_*_batched bit for bit.
static int pw_sync_check(const void* const* ptrs, int nptrs, int batch, int n_views, int ndepth, int height, int width,
                         long n_total, bool has_ws, size_t workspace_bytes) {
  for (int i = 0; i < nptrs; ++i)
    if (!ptrs[i]) return TMVS_ERR_ARG;
  if (!pw_dims_ok(batch, n_views, ndepth, height, width)) return TMVS_ERR_ARG;
  if (has_ws && workspace_bytes < tmvs_pixelwise_train_workspace()) return TMVS_ERR_ARG;
  if (!pw_batch_fits(batch, n_views, ndepth, height, width)) return TMVS_ERR_SHAPE;
  if (n_total < (long)batch * ndepth * height * width) return TMVS_ERR_ARG;  // fewer elements than this rank's own
  return TMVS_OK;
}

extern "C" int tmvs_pw_sync_forward_sums(const float* sims, int batch, int n_views, int ndepth, int height, int width,
                                         void* workspace, size_t workspace_bytes, double* s_sums, void* stream) {
  const void* ptrs[] = {sims, workspace, s_sums};
  if (int e = pw_sync_check(ptrs, 3, batch, n_views, ndepth, height, width, 1L << 62, true, workspace_bytes)) return e;
  const PwGeo g(batch, n_views, ndepth, height, width);
  for (int v = 0; v < n_views; ++v) pw_fwd_s_sums(g, sims, v, (double*)workspace, s_sums + 2 * v, (hipStream_t)stream);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_pw_sync_forward_z1(const float* sims, int batch, int n_views, int ndepth, int height, int width,
                                       const float* pwp, const double* s_sums, long n_total, void* workspace,
                                       size_t workspace_bytes, float* stats, double* z1_sums, void* stream) {
  const void* ptrs[] = {sims, pwp, s_sums, workspace, stats, z1_sums};
  if (int e = pw_sync_check(ptrs, 6, batch, n_views, ndepth, height, width, n_total, true, workspace_bytes)) return e;
  const PwGeo g(batch, n_views, ndepth, height, width);
  for (int v = 0; v < n_views; ++v)
    pw_fwd_z1_sums(g, sims, v, pwp, s_sums + 2 * v, n_total, stats + (size_t)v * 48, (double*)workspace,
                   z1_sums + 16 * v, (hipStream_t)stream);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_pw_sync_forward_weights(const float* sims, int batch, int n_views, int ndepth, int height,
                                            int width, const float* pwp, const double* z1_sums, long n_total,
                                            float* stats, float* view_w, int* dstar, void* stream) {
  const void* ptrs[] = {sims, pwp, z1_sums, stats, view_w, dstar};
  if (int e = pw_sync_check(ptrs, 6, batch, n_views, ndepth, height, width, n_total, false, 0)) return e;
  const PwGeo g(batch, n_views, ndepth, height, width);
  for (int v = 0; v < n_views; ++v)
    pw_fwd_weights(g, sims, v, pwp, z1_sums + 16 * v, n_total, stats + (size_t)v * 48, view_w, dstar,
                   (hipStream_t)stream);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_pw_sync_backward_s1(const float* sims, int batch, int n_views, int ndepth, int height, int width,
                                        const float* pwp, const float* stats, const float* view_w, const int* dstar,
                                        const float* dview_w, void* workspace, size_t workspace_bytes, double* s1,
                                        void* stream) {
  const void* ptrs[] = {sims, pwp, stats, view_w, dstar, dview_w, workspace, s1};
  if (int e = pw_sync_check(ptrs, 8, batch, n_views, ndepth, height, width, 1L << 62, true, workspace_bytes)) return e;
  const PwGeo g(batch, n_views, ndepth, height, width);
  const PwSaved f{sims, pwp, stats, view_w, dview_w, dstar};
  for (int v = 0; v < n_views; ++v) pw_bwd_s1(g, f, v, (double*)workspace, s1 + 25 * v, (hipStream_t)stream);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_pw_sync_backward_s2(const float* sims, int batch, int n_views, int ndepth, int height, int width,
                                        const float* pwp, const float* stats, const float* view_w, const int* dstar,
                                        const float* dview_w, const double* global_s1, long n_total, void* workspace,
                                        size_t workspace_bytes, double* s2, void* stream) {
  const void* ptrs[] = {sims, pwp, stats, view_w, dstar, dview_w, global_s1, workspace, s2};
  if (int e = pw_sync_check(ptrs, 9, batch, n_views, ndepth, height, width, n_total, true, workspace_bytes)) return e;
  const PwGeo g(batch, n_views, ndepth, height, width);
  const PwSaved f{sims, pwp, stats, view_w, dview_w, dstar};
  for (int v = 0; v < n_views; ++v)
    pw_bwd_s2(g, f, v, global_s1 + 25 * v, n_total, (double*)workspace, s2 + 160 * v, (hipStream_t)stream);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_pw_sync_backward_apply(const float* sims, int batch, int n_views, int ndepth, int height,
                                           int width, const float* pwp, const float* stats, const float* view_w,
                                           const int* dstar, const float* dview_w, const double* global_s1,
                                           const double* global_s2, long n_total, const double* local_s1,
                                           const double* local_s2, void* workspace, size_t workspace_bytes,
                                           float* dsims, float* dpwp, void* stream) {
  const void* ptrs[] = {sims, pwp, stats, view_w, dstar, dview_w, global_s1, global_s2, local_s1, local_s2, workspace,
                        dsims, dpwp};
  if (int e = pw_sync_check(ptrs, 13, batch, n_views, ndepth, height, width, n_total, true, workspace_bytes)) return e;
  hipStream_t st = (hipStream_t)stream;
  const PwGeo g(batch, n_views, ndepth, height, width);
  const PwSaved f{sims, pwp, stats, view_w, dview_w, dstar};
  double* part = (double*)workspace;
  double* s3 = part + 1024 * 160;
  for (int v = 0; v < n_views; ++v) {  // the parameter gradients are this rank's: its own s1 / s2 / s3
    pw_bwd_s3(g, f, v, global_s1 + 25 * v, global_s2 + 160 * v, n_total, dsims, part, s3, st);
    hipLaunchKernelGGL(pw_grad_finalize_kernel, dim3(1), dim3(128), 0, st, local_s1 + 25 * v, local_s2 + 160 * v,
                       (const double*)s3, dpwp);
  }
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}
