// CostRegNet training: the train-mode forward and the backward of
// models/module.py:425-456 (Conv3d :108-147, Deconv3d :150-191, nn.BatchNorm3d in train mode).
//
// Every convolution of the network and of its backward is one of two gathers over NDHWC
// activations with weights packed [27][Cout][Cin] (tap = kd*9 + kh*3 + kw):
//   strided    : y[o] = sum_{k,ci} W[k][co][ci] x[o*s - 1 + k]          (Conv3d k3 p1; dgrad of a
//                                                                        ConvTranspose3d)
//   transposed : y[o] = sum_{k,ci} W[k][co][ci] x[(o + 1 - k)/s]  if s | (o + 1 - k)
//                                                                       (ConvTranspose3d k3 s2 p1 op1;
//                                                                        dgrad of a Conv3d, s = 1 or 2)
// and every weight gradient is one reduction
//   dW[k][a][b] = sum_p direct[p][a] * gathered[p*s - 1 + k][b]         (conv: direct = dz, gathered
//                                                                        = x; deconv: direct = x,
//                                                                        gathered = dz)
// The host packs the weights for each use (transposes / flips are index permutations of the
// [27][Cout][Cin] block). BatchNorm3d in train mode: batch mean and biased variance per channel
// over all B*D*H*W voxels (fp64 partial sums, combined in a fixed order: bitwise reproducible),
// y = relu(fmaf(z, alpha, shift)) [+ skip] with alpha = gamma/sqrt(var+eps), shift = beta -
// mean*alpha (the CPU kernel's form); backward dz = alpha/N * (N*g - sum g - xhat * sum g*xhat),
// g = dy * [fmaf(z, alpha, shift) > 0]. No atomics anywhere: every reduction is block partials
// plus a fixed-order combine.
//
// Bounds: the convolutions are fp32 FMA work (VALU; 3 x 3,456 MAC per voxel for forward + both
// gradients), the BN passes HBM (2-3 reads of z per pass).
#include "train_reduce.h"
#include "../../include/transmvs_sync.h"

namespace tmvs {

constexpr int kTrainBlock = 256;

// ---------------------------------------------------------------- generic direct conv (VALU)
// One thread = one output voxel x COB output channels; the co-block's weights [27][COB][CIN] are
// wave-uniform (scalar loads feeding v_fma_f32 as SGPR operands: no LDS staging per block). Each
// tap's CIN input channels are one contiguous NDHWC row (float4 loads).
template <int CIN, int COB>
__global__ __launch_bounds__(kTrainBlock) void conv3d_generic_kernel(
    const float* __restrict__ x, const float* __restrict__ w, int cout, int B, int Di, int Hi, int Wi, int Do, int Ho,
    int Wo, int stride, int transposed, int accumulate, float* __restrict__ y) {
  const int cob = blockIdx.y;
  const long nvox = (long)B * Do * Ho * Wo;
  const long vl = (long)blockIdx.x * kTrainBlock + threadIdx.x;
  if (vl >= nvox) return;
  int ow = (int)(vl % Wo);
  if (transposed && stride == 2) {  // even columns first, then odd: a wave's lanes share the kw tap set
    const int ne = (Wo + 1) / 2;
    ow = ow < ne ? 2 * ow : 2 * (ow - ne) + 1;
  }
  const long v = vl - (long)(vl % Wo) + ow;
  long t = vl / Wo;
  const int oh = (int)(t % Ho);
  t /= Ho;
  const int od = (int)(t % Do);
  const int b = (int)(t / Do);
  float acc[COB];
#pragma unroll
  for (int c = 0; c < COB; ++c) acc[c] = 0.f;
  const float* xb = x + (size_t)b * Di * Hi * Wi * CIN;
#pragma unroll 1
  for (int k = 0; k < 27; ++k) {
    const int kd = k / 9, kh = (k / 3) % 3, kw = k % 3;
    int id, ih, iw;
    if (transposed) {
      const int td = od + 1 - kd, th = oh + 1 - kh, tw = ow + 1 - kw;
      if (td < 0 || th < 0 || tw < 0 || td % stride || th % stride || tw % stride) continue;
      id = td / stride;
      ih = th / stride;
      iw = tw / stride;
    } else {
      id = od * stride - 1 + kd;
      ih = oh * stride - 1 + kh;
      iw = ow * stride - 1 + kw;
      if (id < 0 || ih < 0 || iw < 0) continue;
    }
    if (id >= Di || ih >= Hi || iw >= Wi) continue;
    const float* xp = xb + (((size_t)id * Hi + ih) * Wi + iw) * CIN;
    const float* wk = w + ((size_t)k * cout + cob * COB) * CIN;  // wave-uniform: scalar loads, SGPR operands
    if constexpr (CIN % 4 == 0) {
#pragma unroll 4
      for (int c4 = 0; c4 < CIN / 4; ++c4) {
        const float4 xv = *reinterpret_cast<const float4*>(xp + 4 * c4);
#pragma unroll
        for (int co = 0; co < COB; ++co) {
          const float4 wv = *reinterpret_cast<const float4*>(wk + co * CIN + 4 * c4);
          acc[co] = fmaf(wv.x, xv.x, acc[co]);
          acc[co] = fmaf(wv.y, xv.y, acc[co]);
          acc[co] = fmaf(wv.z, xv.z, acc[co]);
          acc[co] = fmaf(wv.w, xv.w, acc[co]);
        }
      }
    } else {
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) {
        const float xv = xp[ci];
#pragma unroll
        for (int co = 0; co < COB; ++co) acc[co] = fmaf(wk[co * CIN + ci], xv, acc[co]);
      }
    }
  }
  float* yp = y + (size_t)v * cout + cob * COB;
  if (accumulate) {  // y += conv (a gradient reaching a tensor along two paths)
#pragma unroll
    for (int c = 0; c < COB; ++c) acc[c] = yp[c] + acc[c];
  }
  if constexpr (COB % 4 == 0) {
#pragma unroll
    for (int c4 = 0; c4 < COB / 4; ++c4)
      *reinterpret_cast<float4*>(yp + 4 * c4) = make_float4(acc[4 * c4], acc[4 * c4 + 1], acc[4 * c4 + 2], acc[4 * c4 + 3]);
  } else {
#pragma unroll
    for (int c = 0; c < COB; ++c) yp[c] = acc[c];
  }
}

// ---------------------------------------------------------------- weight gradient
// Both channel counts multiples of 8 (the CostRegNet / pathway layers): on the matrix cores. Block
// (rb, k) of the 1-D grid reduces voxels [rb*vpb, (rb+1)*vpb) of `direct` for tap k into
// partial[rb][k][A][BC] (tile_reduce_mfma, reduce_mfma.h: 64-row chunks staged in LDS, fp32 within a
// chunk, fp64 across chunks, the waves combined in a fixed order); a gathered row whose tap falls
// outside reads as zeros.
template <int A, int BC>
__global__ __launch_bounds__(kTrainBlock) void conv3d_wgrad_tile_kernel(
    const float* __restrict__ direct, const float* __restrict__ gath, int B, int Pd, int Ph, int Pw, int Gd, int Gh,
    int Gw, int stride, long vpb, int nblk, double* __restrict__ partial) {
  static_assert(A % 8 == 0 && BC % 8 == 0, "the matrix-core tile takes multiples of 8");
  int rb, k;  // the 27 taps of a voxel range on one XCD (common.h)
  if (!xcd_range_tap(27, nblk, rb, k)) return;
  const int kd = k / 9, kh = (k / 3) % 3, kw = k % 3;
  const long nv = (long)B * Pd * Ph * Pw;
  const long u0 = (long)rb * vpb, u1 = u0 + vpb < nv ? u0 + vpb : nv;
  auto la = [&](long v, int q) { return *reinterpret_cast<const float4*>(direct + v * A + 4 * q); };
  auto lb = [&](long v, int q) {
    int b, pd, ph, pw;
    chunk_row_coords3(v, Pd, Ph, Pw, b, pd, ph, pw);  // rows of 64-aligned chunks (wgrad_chunk: multiples of 2048)
    const int gd = pd * stride - 1 + kd, gh = ph * stride - 1 + kh, gw = pw * stride - 1 + kw;
    if (gd < 0 || gh < 0 || gw < 0 || gd >= Gd || gh >= Gh || gw >= Gw) return make_float4(0.f, 0.f, 0.f, 0.f);
    return *reinterpret_cast<const float4*>(gath + ((((size_t)b * Gd + gd) * Gh + gh) * Gw + gw) * BC + 4 * q);
  };
  tile_reduce_mfma<A, BC>(u0, u1, la, lb, partial + ((size_t)rb * 27 + k) * A * BC);
}

// Few (a, b) pairs, one kd plane of taps per block row (grid.y = 3): a thread reads its voxel's
// `direct` row once per kd and the 9 neighbours' `gathered` rows (L1/L2 hits), keeping 9 x A x BC fp32
// sums over its voxels; then block_sum_store (train_reduce.h) per value.
// Replaces 27 passes over `direct` with 3.
template <int A, int BC>
__global__ __launch_bounds__(kTrainBlock) void conv3d_wgrad_taps_kernel(
    const float* __restrict__ direct, const float* __restrict__ gath, int B, int Pd, int Ph, int Pw, int Gd, int Gh,
    int Gw, int stride, long vpb, double* __restrict__ partial) {
  constexpr int NPR = A * BC;
  const int kd = blockIdx.y;
  const long nvox = (long)B * Pd * Ph * Pw;
  const long v0 = (long)blockIdx.x * vpb, v1 = v0 + vpb < nvox ? v0 + vpb : nvox;
  float acc[9 * NPR];  // [tap of the plane][a][b]
#pragma unroll
  for (int i = 0; i < 9 * NPR; ++i) acc[i] = 0.f;
  long v = v0 + threadIdx.x;
  int pw = (int)(v % Pw), ph, pd, b;
  {
    const long t = v / Pw;
    ph = (int)(t % Ph);
    pd = (int)((t / Ph) % Pd);
    b = (int)(t / ((long)Ph * Pd));
  }
  for (; v < v1; v += kTrainBlock) {
    float dv[A];
    if constexpr (A % 4 == 0) {
#pragma unroll
      for (int a = 0; a < A; a += 4) {
        const float4 t4 = *reinterpret_cast<const float4*>(direct + v * A + a);
        dv[a] = t4.x;
        dv[a + 1] = t4.y;
        dv[a + 2] = t4.z;
        dv[a + 3] = t4.w;
      }
    } else {
#pragma unroll
      for (int a = 0; a < A; ++a) dv[a] = direct[v * A + a];
    }
    const float* gb = gath + (size_t)b * Gd * Gh * Gw * BC;
    const int gd = pd * stride - 1 + kd;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int gh = ph * stride - 1 + k / 3, gw = pw * stride - 1 + k % 3;
      const bool ok = gd >= 0 && gh >= 0 && gw >= 0 && gd < Gd && gh < Gh && gw < Gw;
      const float* gp = gb + (ok ? (((size_t)gd * Gh + gh) * Gw + gw) * BC : 0);  // always a valid address
      float gv[BC];  // unconditional loads, zeroed after: no branch per load
      if constexpr (BC % 4 == 0) {
#pragma unroll
        for (int c = 0; c < BC; c += 4) {
          const float4 t4 = *reinterpret_cast<const float4*>(gp + c);
          gv[c] = ok ? t4.x : 0.f;
          gv[c + 1] = ok ? t4.y : 0.f;
          gv[c + 2] = ok ? t4.z : 0.f;
          gv[c + 3] = ok ? t4.w : 0.f;
        }
      } else {
#pragma unroll
        for (int c = 0; c < BC; ++c) {
          const float t1 = gp[c];
          gv[c] = ok ? t1 : 0.f;
        }
      }
#pragma unroll
      for (int a = 0; a < A; ++a)
#pragma unroll
        for (int c = 0; c < BC; ++c) acc[(k * A + a) * BC + c] = fmaf(dv[a], gv[c], acc[(k * A + a) * BC + c]);
    }
    pw += kTrainBlock;
    while (pw >= Pw) {
      pw -= Pw;
      if (++ph == Ph) {
        ph = 0;
        if (++pd == Pd) {
          pd = 0;
          ++b;
        }
      }
    }
  }
  block_sum_store<true>(acc, partial + ((size_t)blockIdx.x * 27 + kd * 9) * NPR);
}

// ---------------------------------------------------------------- BatchNorm3d, train mode
// The two BatchNorm partial passes share one walk: thread t handles channel t % C of the block's rows
// v = v0 + t / C, + rs, + 2 rs, ... (rs = 256 / C; C divides 256) and keeps two sums in 4 chains each.
// Rows go in groups of 4 (row j of a group into chain j), two groups in flight: group g+1's loads are
// issued before group g is accumulated (a block walks up to thousands of rows; one group at a time left
// each load's latency exposed); the groups are accumulated in order, the rows left over one by one into
// chain 0. Two named register sets, written out: a generic ring of 2-4 groups under a rolled loop
// measured slower than this hand-unrolled pair (r14t).
// load4(v, regs): rows v, v + rs, v + 2 rs, v + 3 rs into regs; add4(regs); tail(v): one row.
template <typename Regs, typename Load4, typename Add4, typename Tail>
__device__ __forceinline__ void walk_rows_two_groups(long v, long v1, int rs, Load4 load4, Add4 add4, Tail tail) {
  Regs ra, rb;
  if (v + 3L * rs < v1) load4(v, ra);
  while (v + 3L * rs < v1) {
    const long vb = v + 4L * rs;
    const bool hb = vb + 3L * rs < v1;
    if (hb) load4(vb, rb);
    add4(ra);
    v = vb;
    if (!hb) break;
    const long va = v + 4L * rs;
    const bool ha = va + 3L * rs < v1;
    if (ha) load4(va, ra);
    add4(rb);
    v = va;
    if (!ha) break;
  }
  for (; v < v1; v += rs) tail(v);
}

// ... and one end: each thread's chains as (c0 + c1) + (c2 + c3), then thread c < C adds its channel's
// rs thread sums in thread order; partial[blockIdx.x][2][C] = (sum of a, sum of b)
__device__ __forceinline__ void channel_pair_store(const double (&a)[4], const double (&b)[4], int C,
                                                   double* __restrict__ partial) {
  __shared__ double red[2][kTrainBlock];
  red[0][threadIdx.x] = (a[0] + a[1]) + (a[2] + a[3]);
  red[1][threadIdx.x] = (b[0] + b[1]) + (b[2] + b[3]);
  __syncthreads();
  if (threadIdx.x < C) {
    double ta = 0.0, tb = 0.0;
    for (int r = 0; r < kTrainBlock / C; ++r) {
      ta += red[0][r * C + threadIdx.x];
      tb += red[1][r * C + threadIdx.x];
    }
    partial[((size_t)blockIdx.x * 2 + 0) * C + threadIdx.x] = ta;
    partial[((size_t)blockIdx.x * 2 + 1) * C + threadIdx.x] = tb;
  }
}

// Per-block fp64 partials of (sum z, sum z^2) per channel
// (grid.y = group: independent statistics of `groups` consecutive [nvox][C] slabs)
__global__ __launch_bounds__(kTrainBlock) void bn_stats_partial_kernel(const float* __restrict__ z, long nvox, int C,
                                                                       long vpb, double* __restrict__ partial) {
  z += (size_t)blockIdx.y * nvox * C;
  partial += (size_t)blockIdx.y * gridDim.x * 2 * C;
  const int c = threadIdx.x % C, r0 = threadIdx.x / C, rs = kTrainBlock / C;
  const long v0 = (long)blockIdx.x * vpb, v1 = v0 + vpb < nvox ? v0 + vpb : nvox;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
  struct Regs {
    float x[4];
  };
  walk_rows_two_groups<Regs>(
      v0 + r0, v1, rs,
      [&](long vv, Regs& r) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r.x[j] = z[(vv + (long)j * rs) * C + c];
      },
      [&](const Regs& r) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s[j] += (double)r.x[j];
          q[j] += (double)r.x[j] * (double)r.x[j];
        }
      },
      [&](long v) {
        const double x = (double)z[v * C + c];
        s[0] += x;
        q[0] += x * x;
      });
  channel_pair_store(s, q, C, partial);
}

// mean, biased var (fp32) from the summed (sum z, sum z^2)
__device__ __forceinline__ void bn_stats_from_sums(double s, double s2, long nvox, float& mean, float& var) {
  const double m = s / (double)nvox;
  const double v = s2 / (double)nvox - m * m;
  mean = (float)m;
  var = (float)(v > 0.0 ? v : 0.0);
}

// sum_partials_f64_kernel's two sums of channel c (sum z, sum z^2: tree_sum_256, train_reduce.h) and
// bn_stats_from_sums in one launch: grid (C, groups)
__global__ __launch_bounds__(kTrainBlock) void bn_sums_stats_kernel(const double* __restrict__ partial, int nblk, int C,
                                                                    long nvox, float* __restrict__ mean,
                                                                    float* __restrict__ var) {
  __shared__ double tot[2];
  const int c = blockIdx.x, K = 2 * C;
  partial += (size_t)blockIdx.y * nblk * K;
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {
    const double t = tree_sum_256(partial + h * C + c, nblk, (size_t)K);
    if (threadIdx.x == 0) tot[h] = t;
    __syncthreads();
  }
  if (threadIdx.x == 0)
    bn_stats_from_sums(tot[0], tot[1], nvox, mean[(size_t)blockIdx.y * C + c], var[(size_t)blockIdx.y * C + c]);
}

__device__ __forceinline__ void bn_affine(float mean, float var, float g, float bt, float eps, float& al, float& sh) {
  al = (1.f / sqrtf(var + eps)) * g;
  sh = fmaf(-mean, al, bt);
}

// VEC consecutive floats as one load / store: VEC = 4 moves a 16-byte-aligned quad
template <int VEC>
__device__ __forceinline__ void load_vec(const float* __restrict__ p, float (&v)[VEC]) {
  static_assert(VEC == 1 || VEC == 4, "scalar or float4");
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x;
    v[1] = t.y;
    v[2] = t.z;
    v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void store_vec(float* __restrict__ p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// out = relu(fmaf(z, alpha, shift)) [+ skip]; group i / per uses statistics [group][C]. A thread takes
// VEC consecutive elements (nv = n / VEC threads). VEC = 4 (C % 4 == 0, 16-byte aligned tensors): the
// channel / group indices once per 4 elements instead of a 64-bit divide per element; one body per
// element for both, so the same bits.
template <int VEC>
__global__ __launch_bounds__(kTrainBlock) void bn_relu_apply_kernel(const float* __restrict__ z, long nv, long per,
                                                                    int C, const float* __restrict__ mean,
                                                                    const float* __restrict__ var,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float eps,
                                                                    const float* __restrict__ skip,
                                                                    float* __restrict__ out) {
  const long iv = (long)blockIdx.x * kTrainBlock + threadIdx.x;
  if (iv >= nv) return;
  const long i = VEC * iv;
  const int c0 = (int)(i % C);
  const long g0 = (i / per) * C + c0;
  float zz[VEC], y[VEC];
  load_vec<VEC>(z + i, zz);
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    float al, sh;
    bn_affine(mean[g0 + j], var[g0 + j], gamma[c0 + j], beta[c0 + j], eps, al, sh);
    y[j] = relu(fmaf(zz[j], al, sh));
  }
  if (skip) {
    float sv[VEC];
    load_vec<VEC>(skip + i, sv);
#pragma unroll
    for (int j = 0; j < VEC; ++j) y[j] = sv[j] + y[j];
  }
  store_vec<VEC>(out + i, y);
}

// backward pass 1: per-block fp64 partials of (sum g, sum g*xhat), g = dy * [fmaf(z, alpha, shift) > 0]
__global__ __launch_bounds__(kTrainBlock) void bn_relu_bwd_partial_kernel(
    const float* __restrict__ dy, const float* __restrict__ z, long nvox, int C, const float* __restrict__ mean,
    const float* __restrict__ var, const float* __restrict__ gamma, const float* __restrict__ beta, float eps, long vpb,
    double* __restrict__ partial) {
  const int c = threadIdx.x % C, r0 = threadIdx.x / C, rs = kTrainBlock / C;
  dy += (size_t)blockIdx.y * nvox * C;  // grid.y = group
  z += (size_t)blockIdx.y * nvox * C;
  partial += (size_t)blockIdx.y * gridDim.x * 2 * C;
  mean += (size_t)blockIdx.y * C;
  var += (size_t)blockIdx.y * C;
  float al, sh;
  bn_affine(mean[c], var[c], gamma[c], beta[c], eps, al, sh);
  const float m = mean[c], rstd = 1.f / sqrtf(var[c] + eps);
  const long v0 = (long)blockIdx.x * vpb, v1 = v0 + vpb < nvox ? v0 + vpb : nvox;
  double sg[4] = {0.0, 0.0, 0.0, 0.0}, sgx[4] = {0.0, 0.0, 0.0, 0.0};
  auto add1 = [&](float zz, float gg, int j) {
    const float g = fmaf(zz, al, sh) > 0.f ? gg : 0.f;
    sg[j] += (double)g;
    sgx[j] += (double)g * (double)((zz - m) * rstd);
  };
  struct Regs {
    float z[4], g[4];
  };
  walk_rows_two_groups<Regs>(
      v0 + r0, v1, rs,
      [&](long vv, Regs& r) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          r.z[j] = z[(vv + (long)j * rs) * C + c];
          r.g[j] = dy[(vv + (long)j * rs) * C + c];
        }
      },
      [&](const Regs& r) {
#pragma unroll
        for (int j = 0; j < 4; ++j) add1(r.z[j], r.g[j], j);
      },
      [&](long v) { add1(z[v * C + c], dy[v * C + c], 0); });
  channel_pair_store(sg, sgx, C, partial);
}

// dbeta = sum g, dgamma = sum g*xhat from the summed partials: per group in fp32, then added over the
// groups in order (as autograd accumulates the per-view gradients of a module called per view)
// (run by the first block of the backward apply kernels, thread c < C: one launch less per BatchNorm)
__device__ __forceinline__ void bn_relu_bwd_finalize(const double* __restrict__ sums, int C, int groups,
                                                     float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = threadIdx.x;
  if (!dgamma || blockIdx.x != 0 || c >= C) return;  // (no dgamma: the split entries finalize on their own sums)
  float b = (float)sums[c], g = (float)sums[C + c];
  for (int k = 1; k < groups; ++k) {
    b = b + (float)sums[(size_t)k * 2 * C + c];
    g = g + (float)sums[(size_t)k * 2 * C + C + c];
  }
  dbeta[c] = b;
  dgamma[c] = g;
}

// pass 2: dz = gamma*rstd/N * (N*g - sum g - xhat * sum g*xhat); VEC elements per thread as
// bn_relu_apply_kernel (one body per element, the same bits). N = n_total, the count behind `sums`: the
// group's nvox, or with statistics synchronised across ranks the count of all ranks' elements
template <int VEC>
__global__ __launch_bounds__(kTrainBlock) void bn_relu_bwd_apply_kernel(
    const float* __restrict__ dy, const float* __restrict__ z, long nv, int C, long nvox, long n_total,
    const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, const double* __restrict__ sums, int groups,
    float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dz) {
  bn_relu_bwd_finalize(sums, C, groups, dgamma, dbeta);
  const long iv = (long)blockIdx.x * kTrainBlock + threadIdx.x;
  if (iv >= nv) return;
  const long i = VEC * iv;
  const int c0 = (int)(i % C);
  const long grp = i / (nvox * C);  // statistics and sums of element i's group
  const long g0 = grp * C + c0;
  const double* sg = sums + (size_t)grp * 2 * C;
  float zz[VEC], dd[VEC], o[VEC];
  load_vec<VEC>(z + i, zz);
  load_vec<VEC>(dy + i, dd);
  const double inv_n = 1.0 / (double)n_total;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int c = c0 + j;
    const long gc = g0 + j;
    float al, sh;
    bn_affine(mean[gc], var[gc], gamma[c], beta[c], eps, al, sh);
    const float rstd = 1.f / sqrtf(var[gc] + eps);
    const float xhat = (zz[j] - mean[gc]) * rstd;
    const float g = fmaf(zz[j], al, sh) > 0.f ? dd[j] : 0.f;
    const float mg = (float)(sg[c] * inv_n), mgx = (float)(sg[C + c] * inv_n);
    o[j] = (gamma[c] * rstd) * ((g - mg) - xhat * mgx);
  }
  store_vec<VEC>(dz + i, o);
}

// ---------------------------------------------------------------- dispatch helpers
template <int CIN, int COB>
static int launch_generic(const float* x, const float* w, int cout, int B, int Di, int Hi, int Wi, int Do, int Ho,
                          int Wo, int stride, int transposed, int accumulate, float* y, hipStream_t st) {
  const long nvox = (long)B * Do * Ho * Wo;
  hipLaunchKernelGGL((conv3d_generic_kernel<CIN, COB>), dim3((unsigned)((nvox + kTrainBlock - 1) / kTrainBlock),
                                                             cout / COB),
                     dim3(kTrainBlock), 0, st, x, w, cout, B, Di, Hi, Wi, Do, Ho, Wo, stride, transposed, accumulate, y);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

// voxel ranges of the partial passes (chunk_for, train_reduce.h)
static Chunk wgrad_chunk(long nvox) { return chunk_for(nvox, 2048, 512); }
static Chunk bn_chunk(long nvox) { return chunk_for(nvox, 1024, 4096); }

template <int A, int BC>
static int launch_wgrad(const float* direct, const float* gath, int B, int Pd, int Ph, int Pw, int Gd, int Gh, int Gw,
                        int stride, double* ws, float* dw, hipStream_t st) {
  const long nvox = (long)B * Pd * Ph * Pw;
  const auto [vpb, nblk] = wgrad_chunk(nvox);
  // the taps kernel for the few-pair layers (conv0: 8 x 1, prob: 1 x 8), the matrix-core tile otherwise
  static_assert(A * BC <= 8 || (A % 8 == 0 && BC % 8 == 0), "no weight-gradient kernel for this channel pair");
  if constexpr (A * BC <= 8)
    hipLaunchKernelGGL((conv3d_wgrad_taps_kernel<A, BC>), dim3(nblk, 3), dim3(kTrainBlock), 0, st, direct, gath, B,
                       Pd, Ph, Pw, Gd, Gh, Gw, stride, vpb, ws);
  else
    hipLaunchKernelGGL((conv3d_wgrad_tile_kernel<A, BC>), xcd_range_tap_grid(27, nblk), dim3(kTrainBlock), 0, st, direct,
                       gath, B, Pd, Ph, Pw, Gd, Gh, Gw, stride, vpb, nblk, ws);
  TMVS_CHECK_LAUNCH();
  sum_partials_f32(ws, nblk, 27L * A * BC, dw, st);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

static bool valid_ch(int c) { return c == 1 || c == 8 || c == 16 || c == 32 || c == 64; }

}  // namespace tmvs

using namespace tmvs;

extern "C" int tmvs_conv3d_generic(const float* x, int batch, int cin, int d_in, int h_in, int w_in, const float* w,
                                   int cout, int d_out, int h_out, int w_out, int stride, int flags, float* y,
                                   void* stream) {
  const int transposed = (flags & TMVS_CONV_TRANSPOSED) ? 1 : 0, accumulate = (flags & TMVS_CONV_ACCUMULATE) ? 1 : 0;
  if (!x || !w || !y || batch <= 0 || d_in <= 0 || h_in <= 0 || w_in <= 0 || d_out <= 0 || h_out <= 0 || w_out <= 0)
    return TMVS_ERR_ARG;
  if (!valid_ch(cin) || !valid_ch(cout) || (stride != 1 && stride != 2)) return TMVS_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
#define TMVS_GEN(CI, CB) \
  return launch_generic<CI, CB>(x, w, cout, batch, d_in, h_in, w_in, d_out, h_out, w_out, stride, transposed, \
                                accumulate, y, st)
  if (cout == 1) {
    switch (cin) {
      case 1: TMVS_GEN(1, 1);
      case 8: TMVS_GEN(8, 1);
      case 16: TMVS_GEN(16, 1);
      case 32: TMVS_GEN(32, 1);
      case 64: TMVS_GEN(64, 1);
    }
  } else if (cin == 64) {
    TMVS_GEN(64, 4);
  } else {
    switch (cin) {
      case 1: TMVS_GEN(1, 8);
      case 8: TMVS_GEN(8, 8);
      case 16: TMVS_GEN(16, 8);
      case 32: TMVS_GEN(32, 8);
    }
  }
#undef TMVS_GEN
  return TMVS_ERR_SHAPE;
}

extern "C" size_t tmvs_conv3d_wgrad_workspace(int batch, int d, int h, int w, int a_ch, int b_ch) {
  const long nvox = (long)batch * d * h * w;
  return (size_t)wgrad_chunk(nvox).blocks * 27 * a_ch * b_ch * sizeof(double);
}

extern "C" int tmvs_conv3d_wgrad(const float* direct, int a_ch, int batch, int pd, int ph, int pw, const float* gathered,
                                 int b_ch, int gd, int gh, int gw, int stride, void* workspace, size_t workspace_bytes,
                                 float* dw, void* stream) {
  if (!direct || !gathered || !workspace || !dw || batch <= 0 || pd <= 0 || ph <= 0 || pw <= 0 || gd <= 0 ||
      gh <= 0 || gw <= 0)
    return TMVS_ERR_ARG;
  if (stride != 1 && stride != 2) return TMVS_ERR_SHAPE;
  if (workspace_bytes < tmvs_conv3d_wgrad_workspace(batch, pd, ph, pw, a_ch, b_ch)) return TMVS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  double* ws = (double*)workspace;
#define TMVS_WG(AA, BB)                                                                                             \
  if (a_ch == AA && b_ch == BB)                                                                                     \
    return launch_wgrad<AA, BB>(direct, gathered, batch, pd, ph, pw, gd, gh, gw, stride, ws, dw, st);
  // (direct, gathered) channel pairs of CostRegNet's layers: conv (dz, x) and deconv (x, dz)
  TMVS_WG(8, 1) TMVS_WG(16, 8) TMVS_WG(16, 16) TMVS_WG(32, 16) TMVS_WG(32, 32) TMVS_WG(64, 32) TMVS_WG(64, 64)
  TMVS_WG(1, 8) TMVS_WG(8, 16) TMVS_WG(16, 32) TMVS_WG(32, 64) TMVS_WG(8, 8)
#undef TMVS_WG
  return TMVS_ERR_SHAPE;
}

static size_t bn_group_ws(long nvox, int channels) {
  return (size_t)bn_chunk(nvox).blocks * 2 * channels * sizeof(double) + 2 * channels * sizeof(double);
}

extern "C" size_t tmvs_bn_train_workspace(long nvox, int channels) { return bn_group_ws(nvox, channels); }
extern "C" size_t tmvs_bn_train_workspace_grouped(int groups, long nvox, int channels) {
  return groups > 0 ? (size_t)groups * bn_group_ws(nvox, channels) : 0;
}

// workspace: [groups][nblk][2][C] partials, then [groups][2][C] sums
extern "C" int tmvs_bn_stats_grouped(const float* z, int groups, long nvox, int channels, void* workspace,
                                     size_t workspace_bytes, float* mean, float* var, void* stream) {
  if (!z || !workspace || !mean || !var || nvox <= 0 || groups <= 0) return TMVS_ERR_ARG;
  if (channels <= 0 || kTrainBlock % channels) return TMVS_ERR_SHAPE;
  if (workspace_bytes < tmvs_bn_train_workspace_grouped(groups, nvox, channels)) return TMVS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const auto [vpb, nblk] = bn_chunk(nvox);
  double* part = (double*)workspace;
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(nblk, groups), dim3(kTrainBlock), 0, st, z, nvox, channels, vpb,
                     part);
  TMVS_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_sums_stats_kernel, dim3(channels, groups), dim3(kTrainBlock), 0, st, (const double*)part,
                     nblk, channels, nvox, mean, var);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_bn_stats(const float* z, long nvox, int channels, void* workspace, size_t workspace_bytes,
                             float* mean, float* var, void* stream) {
  return tmvs_bn_stats_grouped(z, 1, nvox, channels, workspace, workspace_bytes, mean, var, stream);
}

extern "C" int tmvs_bn_relu_train_grouped(const float* z, int groups, long nvox, int channels, const float* mean,
                                          const float* var, const float* gamma, const float* beta, float eps,
                                          const float* skip, float* out, void* stream) {
  if (!z || !mean || !var || !gamma || !beta || !out || nvox <= 0 || channels <= 0 || groups <= 0)
    return TMVS_ERR_ARG;
  if (kTrainBlock % channels) return TMVS_ERR_SHAPE;  // as the statistics and the backward: C divides 256
  const long per = nvox * channels, n = per * groups;
  if (channels % 4 == 0 && aligned16(z) && aligned16(out) && (!skip || aligned16(skip))) {
    hipLaunchKernelGGL(bn_relu_apply_kernel<4>, dim3((unsigned)((n / 4 + kTrainBlock - 1) / kTrainBlock)),
                       dim3(kTrainBlock), 0, (hipStream_t)stream, z, n / 4, per, channels, mean, var, gamma, beta, eps,
                       skip, out);
  } else {
    hipLaunchKernelGGL(bn_relu_apply_kernel<1>, dim3((unsigned)((n + kTrainBlock - 1) / kTrainBlock)),
                       dim3(kTrainBlock), 0, (hipStream_t)stream, z, n, per, channels, mean, var, gamma, beta, eps, skip,
                       out);
  }
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_bn_relu_train(const float* z, long nvox, int channels, const float* mean, const float* var,
                                  const float* gamma, const float* beta, float eps, const float* skip, float* out,
                                  void* stream) {
  return tmvs_bn_relu_train_grouped(z, 1, nvox, channels, mean, var, gamma, beta, eps, skip, out, stream);
}

// the backward's two halves, the sums and the apply: tmvs_bn_relu_backward_grouped runs one after the other, the
// split entries (include/transmvs_sync.h) one each, with the sums of all ranks in between
static int bn_launch_bwd_sums(const float* dy, const float* z, int groups, long nvox, int channels, const float* mean,
                              const float* var, const float* gamma, const float* beta, float eps, double* part,
                              double* sums, hipStream_t st) {
  const auto [vpb, nblk] = bn_chunk(nvox);
  hipLaunchKernelGGL(bn_relu_bwd_partial_kernel, dim3(nblk, groups), dim3(kTrainBlock), 0, st, dy, z, nvox, channels,
                     mean, var, gamma, beta, eps, vpb, part);
  TMVS_CHECK_LAUNCH();
  hipLaunchKernelGGL(sum_partials_f64_kernel<>, dim3(2 * channels, groups), dim3(kTrainBlock), 0, st,
                     (const double*)part, nblk, 2 * channels, sums);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

static int bn_launch_bwd_apply(const float* dy, const float* z, int groups, long nvox, int channels, long n_total,
                               const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                               const double* sums, float* dz, float* dgamma, float* dbeta, hipStream_t st) {
  const long n = nvox * channels * groups;
  if (channels % 4 == 0 && aligned16(dy) && aligned16(z) && aligned16(dz)) {
    hipLaunchKernelGGL(bn_relu_bwd_apply_kernel<4>, dim3((unsigned)((n / 4 + kTrainBlock - 1) / kTrainBlock)),
                       dim3(kTrainBlock), 0, st, dy, z, n / 4, channels, nvox, n_total, mean, var, gamma, beta, eps,
                       sums, groups, dgamma, dbeta, dz);
  } else {
    hipLaunchKernelGGL(bn_relu_bwd_apply_kernel<1>, dim3((unsigned)((n + kTrainBlock - 1) / kTrainBlock)),
                       dim3(kTrainBlock), 0, st, dy, z, n, channels, nvox, n_total, mean, var, gamma, beta, eps, sums,
                       groups, dgamma, dbeta, dz);
  }
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_bn_relu_backward_grouped(const float* dy, const float* z, int groups, long nvox, int channels,
                                             const float* mean, const float* var, const float* gamma,
                                             const float* beta, float eps, void* workspace, size_t workspace_bytes,
                                             float* dz, float* dgamma, float* dbeta, void* stream) {
  if (!dy || !z || !mean || !var || !gamma || !beta || !workspace || !dz || !dgamma || !dbeta || nvox <= 0 ||
      groups <= 0)
    return TMVS_ERR_ARG;
  if (channels <= 0 || kTrainBlock % channels) return TMVS_ERR_SHAPE;
  if (workspace_bytes < tmvs_bn_train_workspace_grouped(groups, nvox, channels)) return TMVS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  double* sums = part + (size_t)groups * bn_chunk(nvox).blocks * 2 * channels;
  if (int e = bn_launch_bwd_sums(dy, z, groups, nvox, channels, mean, var, gamma, beta, eps, part, sums, st)) return e;
  return bn_launch_bwd_apply(dy, z, groups, nvox, channels, nvox, mean, var, gamma, beta, eps, sums, dz, dgamma, dbeta,
                             st);
}

extern "C" int tmvs_bn_relu_backward(const float* dy, const float* z, long nvox, int channels, const float* mean,
                                     const float* var, const float* gamma, const float* beta, float eps,
                                     void* workspace, size_t workspace_bytes, float* dz, float* dgamma, float* dbeta,
                                     void* stream) {
  return tmvs_bn_relu_backward_grouped(dy, z, 1, nvox, channels, mean, var, gamma, beta, eps, workspace,
                                       workspace_bytes, dz, dgamma, dbeta, stream);
}

// ---------------------------------------------------------------- statistics synchronised across ranks
// (include/transmvs_sync.h) The same passes, cut where the sums cross ranks: the fp64 [groups][2][C] sums come
// out before any finalize and go back in as the sums of all ranks with their count n_total. With the local sums
// and n_total = nvox every output is bitwise the fused entries'.
__global__ void bn_stats_from_sums_kernel(const double* __restrict__ sums, int n, int C, long n_total,
                                          float* __restrict__ mean, float* __restrict__ var) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // (group, channel)
  if (i >= n) return;
  const int g = i / C, c = i - g * C;
  bn_stats_from_sums(sums[(size_t)g * 2 * C + c], sums[(size_t)g * 2 * C + C + c], n_total, mean[i], var[i]);
}

__global__ __launch_bounds__(kTrainBlock) void bn_relu_bwd_finalize_kernel(const double* __restrict__ sums, int C,
                                                                           int groups, float* __restrict__ dgamma,
                                                                           float* __restrict__ dbeta) {
  bn_relu_bwd_finalize(sums, C, groups, dgamma, dbeta);
}

extern "C" int tmvs_bn_moments_grouped(const float* z, int groups, long nvox, int channels, void* workspace,
                                       size_t workspace_bytes, double* sums, void* stream) {
  if (!z || !workspace || !sums || nvox <= 0 || groups <= 0) return TMVS_ERR_ARG;
  if (channels <= 0 || kTrainBlock % channels) return TMVS_ERR_SHAPE;
  if (workspace_bytes < tmvs_bn_train_workspace_grouped(groups, nvox, channels)) return TMVS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const auto [vpb, nblk] = bn_chunk(nvox);
  double* part = (double*)workspace;
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(nblk, groups), dim3(kTrainBlock), 0, st, z, nvox, channels, vpb,
                     part);
  TMVS_CHECK_LAUNCH();
  hipLaunchKernelGGL(sum_partials_f64_kernel<>, dim3(2 * channels, groups), dim3(kTrainBlock), 0, st,
                     (const double*)part, nblk, 2 * channels, sums);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_bn_stats_from_sums(const double* sums, int groups, int channels, long n_total, float* mean,
                                       float* var, void* stream) {
  if (!sums || !mean || !var || groups <= 0 || n_total <= 0) return TMVS_ERR_ARG;
  if (channels <= 0 || kTrainBlock % channels) return TMVS_ERR_SHAPE;
  const int n = groups * channels;
  hipLaunchKernelGGL(bn_stats_from_sums_kernel, dim3((n + kTrainBlock - 1) / kTrainBlock), dim3(kTrainBlock), 0,
                     (hipStream_t)stream, sums, n, channels, n_total, mean, var);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_bn_relu_backward_sums_grouped(const float* dy, const float* z, int groups, long nvox, int channels,
                                                  const float* mean, const float* var, const float* gamma,
                                                  const float* beta, float eps, void* workspace,
                                                  size_t workspace_bytes, double* sums, float* dgamma, float* dbeta,
                                                  void* stream) {
  if (!dy || !z || !mean || !var || !gamma || !beta || !workspace || !sums || !dgamma || !dbeta || nvox <= 0 ||
      groups <= 0)
    return TMVS_ERR_ARG;
  if (channels <= 0 || kTrainBlock % channels) return TMVS_ERR_SHAPE;
  if (workspace_bytes < tmvs_bn_train_workspace_grouped(groups, nvox, channels)) return TMVS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (int e = bn_launch_bwd_sums(dy, z, groups, nvox, channels, mean, var, gamma, beta, eps, (double*)workspace, sums,
                                 st))
    return e;
  hipLaunchKernelGGL(bn_relu_bwd_finalize_kernel, dim3(1), dim3(kTrainBlock), 0, st, (const double*)sums, channels,
                     groups, dgamma, dbeta);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_bn_relu_backward_apply_grouped(const float* dy, const float* z, int groups, long nvox,
                                                   int channels, const float* mean, const float* var,
                                                   const float* gamma, const float* beta, float eps,
                                                   const double* global_sums, long n_total, float* dz, void* stream) {
  if (!dy || !z || !mean || !var || !gamma || !beta || !global_sums || !dz || nvox <= 0 || groups <= 0 ||
      n_total < nvox)
    return TMVS_ERR_ARG;
  if (channels <= 0 || kTrainBlock % channels) return TMVS_ERR_SHAPE;
  return bn_launch_bwd_apply(dy, z, groups, nvox, channels, n_total, mean, var, gamma, beta, eps, global_sums, dz,
                             nullptr, nullptr, (hipStream_t)stream);
}
