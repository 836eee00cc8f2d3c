// View selection for a COLMAP sparse model (include/transmvs_view_select.h): MVSNet's score of every pair of
// views, summed over the 3-D points both see.
//
//   visibility   one bit per (view, point): bits [V][W] uint64, W = ceil(P / 64), bit p % 64 of word p / 64.
//                vs_set_bits_kernel ORs the observations in with 64-bit vector atomics (idempotent, so the
//                matrix does not depend on their order or on duplicates).
//   pair scores  a view sees a few percent of the points, so the points two views share are sparse: the
//                kernel streams the two rows, ANDs them word by word, counts with popcount, and does the
//                transcendental work (one atan2, one exp, fp64) on the rare set bits only. One 256-thread
//                block per pair on a grid capped at TMVS_VS_MAX_BLOCKS, walking pairs b, b + grid, ...;
//                consecutive pairs share row i, so its words come from L2.
//   summation    thread t owns the word couples q = t, t + 256, ... (words 2q, 2q + 1), loaded as one 16-byte
//                load per row when the rows are 16-byte aligned (W even) and as two 8-byte loads otherwise --
//                the same words either way -- and adds its points' terms in ascending point order into one
//                fp64 partial; block_sum_store (train_reduce.h) adds the 256 partials: xor butterfly inside
//                each wave, off = 32 ... 1, then (w0 + w1) + (w2 + w3). No floating-point atomics: the
//                scores repeat bit for bit. The count rides the same reduction as an fp64 (exact below 2^53).
//
// All arithmetic is fp64 and unfused, in the order the header states (the build passes -ffp-contract=off).
#include <math.h>

#include "../../include/transmvs_view_select.h"
#include "train_reduce.h"

namespace tmvs {

namespace vs {
constexpr double kDegrees = 57.295779513082320876798154814105;  // 180 / pi

// the first pair index of row i of the strict upper triangle of a V x V matrix, rows in order
__device__ __forceinline__ long row_start(long i, long V) { return i * (2 * V - i - 1) / 2; }

// pair index -> (i, j), i < j: the root of row_start(i) = p in fp64, then stepped onto the exact row
__device__ __forceinline__ void pair_of(long p, int V, int& i, int& j) {
  const double b = 2.0 * (double)V - 1.0;
  long r = (long)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
  r = r < 0 ? 0 : (r > V - 2 ? V - 2 : r);
  while (r < V - 2 && row_start(r + 1, V) <= p) ++r;
  while (r > 0 && row_start(r, V) > p) --r;
  i = (int)r;
  j = (int)(p - row_start(r, V)) + i + 1;
}

struct Vec3 {
  double x, y, z;
};

// the term of point X for centres ci, cj
__device__ __forceinline__ double term(const Vec3& ci, const Vec3& cj, const double* __restrict__ X, double theta0,
                                       double sigma1, double sigma2) {
  const double px = X[0], py = X[1], pz = X[2];
  const double ax = ci.x - px, ay = ci.y - py, az = ci.z - pz;
  const double bx = cj.x - px, by = cj.y - py, bz = cj.z - pz;
  const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  const double n = sqrt((cx * cx + cy * cy) + cz * cz);
  const double d = (ax * bx + ay * by) + az * bz;
  const double theta = atan2(n, d) * kDegrees;
  const double sigma = theta <= theta0 ? sigma1 : sigma2;
  const double diff = theta - theta0;
  return exp(-(diff * diff) / ((2.0 * sigma) * sigma));
}
}  // namespace vs

__global__ __launch_bounds__(256) void vs_set_bits_kernel(const int* __restrict__ obs_view,
                                                          const int* __restrict__ obs_point, long M, int V, long P,
                                                          long W, unsigned long long* __restrict__ bits,
                                                          int* __restrict__ errors) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const long v = obs_view[m], p = obs_point[m];
  if (v < 0 || v >= V || p < 0 || p >= P) {
    atomicAdd(errors, 1);
    return;
  }
  atomicOr(bits + (size_t)v * W + (p >> 6), 1ULL << (p & 63));
}

__global__ __launch_bounds__(256) void vs_obs_depth_kernel(const int* __restrict__ obs_view,
                                                           const int* __restrict__ obs_point, long M, int V, long P,
                                                           const double* __restrict__ r3, const double* __restrict__ tz,
                                                           const double* __restrict__ xyz, double* __restrict__ z,
                                                           int* __restrict__ errors) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const long v = obs_view[m], p = obs_point[m];
  if (v < 0 || v >= V || p < 0 || p >= P) {
    atomicAdd(errors, 1);
    z[m] = NAN;
    return;
  }
  const double* r = r3 + 3 * v;
  const double* X = xyz + 3 * p;
  z[m] = ((r[0] * X[0] + r[1] * X[1]) + r[2] * X[2]) + tz[v];
}

// VEC: the rows are 16-byte aligned (W even), one 16-byte load per row and couple
template <bool VEC>
__global__ __launch_bounds__(256) void vs_pair_scores_kernel(const unsigned long long* __restrict__ bits, int V, long P,
                                                             long W, long npairs, const double* __restrict__ centres,
                                                             const double* __restrict__ xyz, double theta0,
                                                             double sigma1, double sigma2, double* __restrict__ scores,
                                                             int* __restrict__ counts) {
  __shared__ double sums[2];
  const long couples = (W + 1) / 2;
  const unsigned long long tail = (P & 63) ? (1ULL << (P & 63)) - 1 : ~0ULL;  // the last word's points
  for (long pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    int i, j;
    vs::pair_of(pair, V, i, j);
    const unsigned long long* __restrict__ ri = bits + (size_t)i * W;
    const unsigned long long* __restrict__ rj = bits + (size_t)j * W;
    const vs::Vec3 ci = {centres[3 * i], centres[3 * i + 1], centres[3 * i + 2]};
    const vs::Vec3 cj = {centres[3 * j], centres[3 * j + 1], centres[3 * j + 2]};
    double v[2] = {0.0, 0.0};  // score, count
    long n = 0;
    for (long q = threadIdx.x; q < couples; q += 256) {
      const long w0 = 2 * q;
      unsigned long long both[2];
      if constexpr (VEC) {
        const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(ri + w0);
        const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(rj + w0);
        both[0] = a.x & b.x;
        both[1] = a.y & b.y;
      } else {
        both[0] = ri[w0] & rj[w0];
        both[1] = w0 + 1 < W ? ri[w0 + 1] & rj[w0 + 1] : 0ULL;
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        unsigned long long word = both[h];
        if (w0 + h == W - 1) word &= tail;
        n += __popcll(word);
        while (word) {  // ascending point order
          const int bit = __ffsll((long long)word) - 1;
          word &= word - 1;
          v[0] += vs::term(ci, cj, xyz + 3 * (((w0 + h) << 6) + bit), theta0, sigma1, sigma2);
        }
      }
    }
    v[1] = (double)n;
    block_sum_store<false>(v, sums);
    __syncthreads();
    if (threadIdx.x == 0) {
      const double s = sums[0];
      const int c = (int)sums[1];
      scores[(size_t)i * V + j] = s;
      scores[(size_t)j * V + i] = s;
      counts[(size_t)i * V + j] = c;
      counts[(size_t)j * V + i] = c;
    }
    __syncthreads();  // sums and block_sum_store's LDS are free for the next pair
  }
  // the diagonals: V entries over the grid
  for (long d = (long)blockIdx.x * 256 + threadIdx.x; d < V; d += (long)gridDim.x * 256) {
    scores[(size_t)d * V + d] = 0.0;
    counts[(size_t)d * V + d] = 0;
  }
}

}  // namespace tmvs

using namespace tmvs;

namespace {
constexpr long kMaxPoints = 2147483647L - 64;  // int32 point indices, and (word << 6) + bit stays below 2^31
constexpr long kMaxObs = 2147483647L - 256;    // 1-D grids of 256-thread blocks
inline int good_sizes(int V, long P) {
  if (V < 2 || P < 1 || P >= kMaxPoints) return TMVS_ERR_SHAPE;
  if ((size_t)V * (size_t)((P + 63) / 64) * 8 > (size_t)TMVS_VS_MAX_BITS_BYTES) return TMVS_ERR_SHAPE;
  return TMVS_OK;
}
inline unsigned blocks(long n) { return (unsigned)((n + 255) / 256); }
}  // namespace

extern "C" int tmvs_vs_set_bits(const int* obs_view, const int* obs_point, long n_obs, int n_views, long n_points,
                                unsigned long long* bits, int* errors, void* stream) {
  if (!obs_view || !obs_point || !bits || !errors || (uintptr_t)bits % 8) return TMVS_ERR_ARG;
  if (n_obs < 1 || n_obs >= kMaxObs) return TMVS_ERR_SHAPE;
  if (const int e = good_sizes(n_views, n_points)) return e;
  hipLaunchKernelGGL(vs_set_bits_kernel, dim3(blocks(n_obs)), dim3(256), 0, (hipStream_t)stream, obs_view, obs_point,
                     n_obs, n_views, n_points, (n_points + 63) / 64, bits, errors);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_vs_obs_depth(const int* obs_view, const int* obs_point, long n_obs, int n_views, long n_points,
                                 const double* r3, const double* tz, const double* xyz, double* z, int* errors,
                                 void* stream) {
  if (!obs_view || !obs_point || !r3 || !tz || !xyz || !z || !errors) return TMVS_ERR_ARG;
  if (n_obs < 1 || n_obs >= kMaxObs) return TMVS_ERR_SHAPE;
  if (const int e = good_sizes(n_views, n_points)) return e;
  hipLaunchKernelGGL(vs_obs_depth_kernel, dim3(blocks(n_obs)), dim3(256), 0, (hipStream_t)stream, obs_view, obs_point,
                     n_obs, n_views, n_points, r3, tz, xyz, z, errors);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_vs_pair_scores(const unsigned long long* bits, int n_views, long n_points, const double* centres,
                                   const double* xyz, double theta0, double sigma1, double sigma2, double* scores,
                                   int* counts, void* stream) {
  if (!bits || !centres || !xyz || !scores || !counts || (uintptr_t)bits % 8) return TMVS_ERR_ARG;
  if (!isfinite(theta0) || !isfinite(sigma1) || !isfinite(sigma2) || !(sigma1 > 0.0) || !(sigma2 > 0.0))
    return TMVS_ERR_ARG;
  if (const int e = good_sizes(n_views, n_points)) return e;
  const long W = (n_points + 63) / 64;
  const long npairs = (long)n_views * (n_views - 1) / 2;
  const unsigned grid = (unsigned)(npairs < TMVS_VS_MAX_BLOCKS ? npairs : TMVS_VS_MAX_BLOCKS);
  const bool vec = W % 2 == 0 && (uintptr_t)bits % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(vs_pair_scores_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, bits, n_views,
                       n_points, W, npairs, centres, xyz, theta0, sigma1, sigma2, scores, counts);
  else
    hipLaunchKernelGGL(vs_pair_scores_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, bits, n_views,
                       n_points, W, npairs, centres, xyz, theta0, sigma1, sigma2, scores, counts);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}
