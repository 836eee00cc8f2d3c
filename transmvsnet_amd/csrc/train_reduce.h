// The fixed-order reductions of the training kernels (costreg_train.hip, featurenet_train.hip, fmt_train.hip,
// pw_train.hip), each written once. The training backward is deterministic by construction: every reduction
// over pixels, voxels or tokens is per-block fp64 partials followed by a fixed-order combine, no atomics --
// so the summation orders below are the determinism contract, and changing one changes bits.
// All blocks are 256 threads (4 waves). The matrix-core tile reduction is reduce_mfma.h, included from here.
#pragma once
#include "common.h"
#include "reduce_mfma.h"

namespace tmvs {

constexpr int kRedBlock = 256;

// ---------------------------------------------------------------- inside a block
// out[i] = the block's sum of v[i] over its 256 threads, i < NV, in fp64: inside each wave the xor
// butterfly x += xor_lane(x, off), off = 32, 16, ..., 1, then the 4 wave sums as (w0 + w1) + (w2 + w3).
// DPP: the butterfly by common.h's wave_xor_sum_dpp (the same pairs and operand order, so the same bits, in
// 4 instead of 12 LDS-unit operations per value), otherwise by __shfl_xor. The choice is register pressure
// only -- with the 25 values of pw_bwd1_kernel the DPP moves raised it to 178 VGPRs (r15a) -- so each call
// site names its form. v is a plain register array (a getter lambda in its place cost pw_bwd1_kernel the
// same 14 VGPRs).
template <bool DPP, typename T, int NV>
__device__ __forceinline__ void block_sum_store(const T (&v)[NV], double* __restrict__ out) {
  __shared__ double red[NV][kRedBlock / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double x = (double)v[i];
    if constexpr (DPP) {
      x = wave_xor_sum_dpp(x);
    } else {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    }
    if (lane == 0) red[i][wv] = x;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NV; i += kRedBlock) out[i] = (red[i][0] + red[i][1]) + (red[i][2] + red[i][3]);
}

// ---------------------------------------------------------------- across blocks
// Interleaved-chain sum of the rows p[j * stride], j < n (block partials, or a block's input rows), for
// 256 / N values per block: thread (g, q) = (t / (256 / N), t % (256 / N)) adds the rows j = g, g + N, ...
// of value q in that order in fp64 (chain g; N times the loads in flight of one serial chain), then chain
// 0's thread adds the chains in order 0, 1, ..., N - 1. All 256 threads call it with their value's p
// (live: value q exists); true, with the sum in t, for the thread that holds a live value's result.
template <int N, typename T>
__device__ __forceinline__ bool chain_sum(const T* __restrict__ p, bool live, long n, size_t stride, double& t) {
  constexpr int W = kRedBlock / N;
  __shared__ double red[N][W];
  const int g = threadIdx.x / W, q = threadIdx.x % W;
  double s = 0.0;
  if (live) s = strided_sum(p, g, n, N, stride, s);
  red[g][q] = s;
  __syncthreads();
  if (g != 0 || !live) return false;
  t = red[0][q];
#pragma unroll
  for (int c = 1; c < N; ++c) t += red[c][q];
  return true;
}

// out[i] = (float) sum_j partial[j][i], i < n: 8 chains x 32 values per block, grid (n + 31) / 32.
// ROWS: the partials are [nblk][taps][ap][bc] with the a rows of out [taps][a][bc] padded to ap.
template <bool ROWS>
__global__ __launch_bounds__(kRedBlock) void sum_partials_f32_kernel(const double* __restrict__ partial, int nblk,
                                                                     int ap, int a, int bc, long n,
                                                                     float* __restrict__ out) {
  const long per = ROWS ? (long)a * bc : 1;
  const long np = ROWS ? n / per * ap * bc : n;  // values per partial
  const long i = (long)blockIdx.x * 32 + (threadIdx.x & 31);
  const long src = !ROWS ? i : i < n ? ((i / per) * ap + (i % per) / bc) * bc + i % bc : 0;
  double t;
  if (chain_sum<8>(partial + src, i < n, nblk, (size_t)np, t)) out[i] = (float)t;
}

// The sum of p[j * stride], j < n, in fp64: thread t adds j = t, t + 256, ... in that order, then the LDS
// tree red[t] += red[t + st], st = 128, 64, ..., 1 -- deterministic, and parallel over the (up to 4096)
// partial rows. Every thread returns the sum; __syncthreads() before the block calls it again.
__device__ __forceinline__ double tree_sum_256(const double* __restrict__ p, int n, size_t stride) {
  __shared__ double red[kRedBlock];
  red[threadIdx.x] = strided_sum(p, threadIdx.x, n, kRedBlock, stride, 0.0);
  __syncthreads();
  for (int st = kRedBlock / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  return red[0];
}

// out[group][k] = sum_j partial[group][j][k], fp64: grid (K, groups), one tree_sum_256 per block.
// (A template so that only the translation units that launch it, as sum_partials_f64_kernel<>, emit it.)
template <int BLOCK = kRedBlock>
__global__ __launch_bounds__(BLOCK) void sum_partials_f64_kernel(const double* __restrict__ partial, int nblk, int K,
                                                                 double* __restrict__ out) {
  static_assert(BLOCK == kRedBlock, "tree_sum_256");
  const double s = tree_sum_256(partial + (size_t)blockIdx.y * nblk * K + blockIdx.x, nblk, (size_t)K);
  if (threadIdx.x == 0) out[(size_t)blockIdx.y * K + blockIdx.x] = s;
}

// ---------------------------------------------------------------- host
// Rows per block of a partial-sum pass and the block count: start at `first` rows, double until at most
// max_blocks blocks. A *_workspace entry point and its launcher size through the same call.
struct Chunk {
  long rows;
  int blocks;
};
static inline Chunk chunk_for(long n, long first, long max_blocks) {
  long c = first;
  while ((n + c - 1) / c > max_blocks) c *= 2;
  return {c, (int)((n + c - 1) / c)};
}

// Launches sum_partials_f32_kernel: out[i] = (float) sum_j partial[j][i], i < n; ROWS with the row padding
// (ap, a, bc), n = taps * a * bc. The caller checks the launch.
template <bool ROWS = false>
static inline void sum_partials_f32(const double* partial, int nblk, long n, float* out, hipStream_t st, int ap = 0,
                                    int a = 0, int bc = 0) {
  hipLaunchKernelGGL(sum_partials_f32_kernel<ROWS>, dim3((unsigned)((n + 31) / 32)), dim3(kRedBlock), 0, st, partial,
                     nblk, ap, a, bc, n, out);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace tmvs
