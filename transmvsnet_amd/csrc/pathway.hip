// FMT_with_pathway lateral step (models/FMT.py:195-228), fused:
//   out = smooth(bilinear_up2(reduce(coarse)) + lateral)
// reduce = 1x1 conv (no bias), bilinear align_corners=False (F.interpolate default, :209),
// smooth = 3x3 conv pad 1 (no bias). Weights arrive re-laid-out ([ci][co] and [ci][tap][co]) so
// every input value meets CF consecutive weights (one scalar load). A workgroup owns a 16x16 output tile: it reduces the
// 10x10 coarse pixels the tile's 18x18 halo interpolates from into LDS, builds the up-sampled
// + lateral halo in LDS, then each thread convolves one output pixel for all channels and
// writes it channels-last -- the layout the cost-volume kernel gathers from.
#include "common.h"

namespace tmvs {

constexpr int kTile = 16;
constexpr int kHalo = kTile + 2;
constexpr int kCoarse = kTile / 2 + 2;

// The two kernels below share the tile decode, the lateral prefetch and phase 1. A tile is kTile wide and TH
// high (16 for the 16-channel kernel, 16R for the rows kernel); its halo is HH = TH + 2 rows of kHalo, its coarse
// patch CH = TH / 2 + 2 rows of kCoarse. Phase 2 (bilinear x2 + lateral into the halo) is spelled out in each
// kernel: as a shared function with a store functor it cost the 16-channel kernel 12 VGPRs and a wave per SIMD
// (profiles/fmt_pathway_scaffold_resources.md).
constexpr int halo_iters(int HH) { return (HH * kHalo + 255) / 256; }  // halo pixels per thread

// Tiles are dealt out XCD-contiguously over a 1-D grid (x fastest, then y, then view): consecutive
// block ids go to different XCDs, so with the plain 3-D grid a tile's x/y neighbours -- which read
// the same 128-B lines of the halo rows (an 18-float NCHW row spans 2-3 lines) -- sat behind
// different L2s and each re-fetched them.
template <int TH>
__device__ __forceinline__ void pathway_tile(int W, int H, int& v, int& y0, int& x0) {
  const int nbx = (W + kTile - 1) / kTile, nby = (H + TH - 1) / TH;
  int lb = xcd_remap(blockIdx.x, gridDim.x);
  x0 = (lb % nbx) * kTile;
  lb /= nbx;
  y0 = (lb % nby) * TH;
  v = lb / nby;
}

// The lateral halo values (NCHW, the FeatureNet output) do not depend on the coarse reduction:
// every thread requests its halo pixels' CF channels before phase 1, so their HBM latency
// overlaps the reduction instead of sitting after the first barrier. Out-of-image pixels read 0.
template <int CF, int HH>
__device__ __forceinline__ void load_lateral(const float* __restrict__ lv, int y0, int x0, int H, int W,
                                             float (&lat)[halo_iters(HH)][CF]) {
#pragma unroll
  for (int it = 0; it < halo_iters(HH); ++it) {
    const int idx = threadIdx.x + 256 * it;
    const int r = idx / kHalo, c = idx - r * kHalo;
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    const bool ok = idx < HH * kHalo && y >= 0 && y < H && x >= 0 && x < W;
#pragma unroll
    for (int o = 0; o < CF; ++o) lat[it][o] = ok ? lv[((size_t)o * H + y) * W + x] : 0.f;
  }
}

// Phase 1: the 1x1 reduction of the CH x kCoarse coarse patch at (cy0, cx0) into LDS (pixels outside the
// coarse map are left unwritten: phase 2 never reads them)
template <int CC, int CF, int CH>
__device__ __forceinline__ void reduce_coarse(const float* __restrict__ cv, const float* __restrict__ wred, int cy0,
                                              int cx0, int h, int w, float (&red)[CF][CH][kCoarse + 1]) {
  for (int idx = threadIdx.x; idx < CH * kCoarse; idx += 256) {
    const int r = idx / kCoarse, c = idx - r * kCoarse;
    const int cy = cy0 + r, cx = cx0 + c;
    if (cy < 0 || cy >= h || cx < 0 || cx >= w) continue;
    float xin[CC];
    const float* p = cv + ((size_t)cy * w + cx) * CC;
#pragma unroll
    for (int i4 = 0; i4 < CC / 4; ++i4) {
      const float4 t = *reinterpret_cast<const float4*>(p + 4 * i4);
      xin[4 * i4] = t.x;
      xin[4 * i4 + 1] = t.y;
      xin[4 * i4 + 2] = t.z;
      xin[4 * i4 + 3] = t.w;
    }
    float acc[CF];
#pragma unroll
    for (int o = 0; o < CF; ++o) acc[o] = 0.f;
#pragma unroll 2
    for (int i = 0; i < CC; ++i)
#pragma unroll
      for (int o = 0; o < CF; ++o) acc[o] = fmaf(wred[i * CF + o], xin[i], acc[o]);
#pragma unroll
    for (int o = 0; o < CF; ++o) red[o][r][c] = acc[o];
  }
}

// Stage-3 form with R output rows per thread: a workgroup owns a 16 x 16R tile, so the two
// barriers, the coarse/halo staging and every scalar weight load are shared by R pixels. Tap
// (i, k) feeds the R accumulator sets back to back; each output's chain runs in (i, k, o) order
// whatever R is, so the results do not depend on it.
constexpr int kPathwayRows = 2;
template <int CC, int CF, int R>
__global__ __launch_bounds__(256) void pathway_rows_kernel(const float* __restrict__ coarse,
                                                           const float* __restrict__ lateral, long lat_stride,
                                                           const float* __restrict__ wred,
                                                           const float* __restrict__ wsm, int h, int w,
                                                           float* __restrict__ out) {
  constexpr int TH = kTile * R, HH = TH + 2, CH = TH / 2 + 2;
  __shared__ float red[CF][CH][kCoarse + 1];
  __shared__ float inb[CF][HH][kHalo + 1];
  const int H = 2 * h, W = 2 * w;
  int v, y0, x0;
  pathway_tile<TH>(W, H, v, y0, x0);
  const int cy0 = y0 / 2 - 1, cx0 = x0 / 2 - 1;
  float lat[halo_iters(HH)][CF];
  load_lateral<CF, HH>(lateral + (size_t)v * lat_stride, y0, x0, H, W, lat);
  reduce_coarse<CC, CF, CH>(coarse + (size_t)v * h * w * CC, wred, cy0, cx0, h, w, red);  // 1)
  __syncthreads();
  // 2) bilinear x2 up-sampling + lateral over the (16R+2) x 18 halo (zero outside the image)
#pragma unroll
  for (int it = 0; it < halo_iters(HH); ++it) {
    const int idx = threadIdx.x + 256 * it;
    if (idx >= HH * kHalo) break;
    const int r = idx / kHalo, c = idx - r * kHalo;
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    if (y < 0 || y >= H || x < 0 || x >= W) {
#pragma unroll
      for (int o = 0; o < CF; ++o) inb[o][r][c] = 0.f;
      continue;
    }
    const LinAxis ay = lin_axis(y, h, H), ax = lin_axis(x, w, W);
    const int r0 = ay.i0 - cy0, r1 = ay.i1 - cy0, c0 = ax.i0 - cx0, c1 = ax.i1 - cx0;
#pragma unroll
    for (int o = 0; o < CF; ++o) {
      const float t0 = fmaf(red[o][r0][c0], ax.l0, red[o][r0][c1] * ax.l1);
      const float t1 = fmaf(red[o][r1][c0], ax.l0, red[o][r1][c1] * ax.l1);
      const float up = fmaf(t0, ay.l0, t1 * ay.l1);
      inb[o][r][c] = up + lat[it][o];
    }
  }
  __syncthreads();
  // 3) 3x3 smoothing conv, R vertically adjacent output pixels per thread (rows R*ty .. R*ty+R-1)
  const int ty = threadIdx.x / kTile, tx = threadIdx.x - ty * kTile;
  const int x = x0 + tx;
  if (x >= W || y0 + R * ty >= H) return;
  float acc[R][CF];
#pragma unroll
  for (int q = 0; q < R; ++q)
#pragma unroll
    for (int o = 0; o < CF; ++o) acc[q][o] = 0.f;
#pragma unroll 1
  for (int i = 0; i < CF; ++i) {
#pragma unroll 3
    for (int k = 0; k < 9; ++k) {
      const float* __restrict__ wk = wsm + (i * 9 + k) * CF;
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const float xv = inb[i][R * ty + q + k / 3][tx + k % 3];
#pragma unroll
        for (int o = 0; o < CF; ++o) acc[q][o] = fmaf(wk[o], xv, acc[q][o]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const int y = y0 + R * ty + q;
    if (y >= H) break;
    float4* op = reinterpret_cast<float4*>(out + (((size_t)v * H + y) * W + x) * CF);
#pragma unroll
    for (int o4 = 0; o4 < CF / 4; ++o4)
      op[o4] = make_float4(acc[q][4 * o4], acc[q][4 * o4 + 1], acc[q][4 * o4 + 2], acc[q][4 * o4 + 3]);
  }
}

// 16-channel variant (stage-2 pathway, the larger one): the 3x3 smoothing conv runs on fp32
// MFMA as an implicit GEMM -- M = 16 output channels, N = 16 pixels of a tile row,
// K = 16 channels x 9 taps -- with B fragments from the LDS halo and A fragments (weights) in
// VGPRs. The halo is stored [pixel][16 ch] with channels interleaved so a lane's 4 k-values
// (channels kgrp, 4+kgrp, 8+kgrp, 12+kgrp) are one ds_read_b128, quad-swizzled by pixel
// (bank-conflict free for 16 consecutive pixels, as in costreg.hip).
__device__ __forceinline__ int halo16_index(int vox, int o) {
  const int q = (o & 3) ^ ((vox >> 1) & 3);
  return vox * 16 + q * 4 + (o >> 2);
}

template <int CC>
__global__ __launch_bounds__(256) void pathway16_mfma_kernel(const float* __restrict__ coarse,
                                                             const float* __restrict__ lateral, long lat_stride,
                                                             const float* __restrict__ wred,
                                                             const float* __restrict__ wsm, int h, int w,
                                                             float* __restrict__ out) {
  constexpr int CF = 16;
  __shared__ float red[CF][kCoarse][kCoarse + 1];
  __shared__ __attribute__((aligned(16))) float inb[kHalo * kHalo * CF];
  const int H = 2 * h, W = 2 * w;
  int v, y0, x0;
  pathway_tile<kTile>(W, H, v, y0, x0);
  const int cy0 = y0 / 2 - 1, cx0 = x0 / 2 - 1;
  float lat[halo_iters(kHalo)][CF];
  load_lateral<CF, kHalo>(lateral + (size_t)v * lat_stride, y0, x0, H, W, lat);
  reduce_coarse<CC, CF, kCoarse>(coarse + (size_t)v * h * w * CC, wred, cy0, cx0, h, w, red);  // 1)
  // A fragments meanwhile: lane (co = col, kgrp), tap t, k-step j -> W[co][ci = 4j + kgrp][t]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int col = lane & 15, kgrp = lane >> 4;
  float wa[9][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) wa[t][j] = wsm[((4 * j + kgrp) * 9 + t) * CF + col];
  __syncthreads();
  // 2) bilinear x2 up-sampling + lateral over the 18x18 halo (zero outside the image)
#pragma unroll
  for (int it = 0; it < halo_iters(kHalo); ++it) {
    const int idx = threadIdx.x + 256 * it;
    if (idx >= kHalo * kHalo) break;
    const int r = idx / kHalo, c = idx - r * kHalo;
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    if (y < 0 || y >= H || x < 0 || x >= W) {
#pragma unroll
      for (int o = 0; o < CF; ++o) inb[halo16_index(idx, o)] = 0.f;
      continue;
    }
    const LinAxis ay = lin_axis(y, h, H), ax = lin_axis(x, w, W);
    const int r0 = ay.i0 - cy0, r1 = ay.i1 - cy0, c0 = ax.i0 - cx0, c1 = ax.i1 - cx0;
#pragma unroll
    for (int o = 0; o < CF; ++o) {
      const float t0 = fmaf(red[o][r0][c0], ax.l0, red[o][r0][c1] * ax.l1);
      const float t1 = fmaf(red[o][r1][c0], ax.l0, red[o][r1][c1] * ax.l1);
      const float up = fmaf(t0, ay.l0, t1 * ay.l1);
      inb[halo16_index(idx, o)] = up + lat[it][o];
    }
  }
  __syncthreads();
  // 3) 3x3 conv on MFMA: wave wv owns tile rows 4wv .. 4wv+3
  floatx4_t acc[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) acc[rr] = floatx4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int kh = t / 3, kw = t % 3;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int vox = (4 * wv + rr + kh) * kHalo + col + kw;
      const float4 b = *reinterpret_cast<const float4*>(inb + halo16_index(vox, kgrp));  // channels 4j + kgrp, j < 4
      acc[rr] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t][0], b.x, acc[rr], 0, 0, 0);
      acc[rr] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t][1], b.y, acc[rr], 0, 0, 0);
      acc[rr] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t][2], b.z, acc[rr], 0, 0, 0);
      acc[rr] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t][3], b.w, acc[rr], 0, 0, 0);
    }
  }
  // D: lane (col, kgrp) holds output channels 4kgrp .. 4kgrp+3 of pixel (row, col)
  const int x = x0 + col;
  if (x >= W) return;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int y = y0 + 4 * wv + rr;
    if (y >= H) continue;
    *reinterpret_cast<float4*>(out + (((size_t)v * H + y) * W + x) * CF + 4 * kgrp) =
        make_float4(acc[rr][0], acc[rr][1], acc[rr][2], acc[rr][3]);
  }
}

}  // namespace tmvs

using namespace tmvs;

extern "C" int tmvs_fmt_pathway(const float* coarse, const float* lateral, long lat_view_stride,
                                const float* w_reduce, const float* w_smooth, int nv, int cc, int cf, int h, int w,
                                float* out, void* stream) {
  if (!coarse || !lateral || !w_reduce || !w_smooth || !out || nv <= 0 || h <= 0 || w <= 0) return TMVS_ERR_ARG;
  const long nblk = (long)((2 * w + kTile - 1) / kTile) * ((2 * h + kTile - 1) / kTile) * nv;
  if (nblk > 0x7fffffffL) return TMVS_ERR_SHAPE;
  const dim3 grid((unsigned)nblk);
  hipStream_t st = (hipStream_t)stream;
  if (cc == 32 && cf == 16)
    hipLaunchKernelGGL((pathway16_mfma_kernel<32>), grid, dim3(256), 0, st, coarse, lateral, lat_view_stride,
                       w_reduce, w_smooth, h, w, out);
  else if (cc == 16 && cf == 8) {
    constexpr int R = kPathwayRows;
    const long nrb = (long)((2 * w + kTile - 1) / kTile) * ((2 * h + kTile * R - 1) / (kTile * R)) * nv;
    hipLaunchKernelGGL((pathway_rows_kernel<16, 8, R>), dim3((unsigned)nrb), dim3(256), 0, st, coarse, lateral,
                       lat_view_stride, w_reduce, w_smooth, h, w, out);
  } else
    return TMVS_ERR_SHAPE;
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}
