// The device side of the training driver's data path (transmvsnet_amd/finetune.py).
//
// tmvs_gt_pyramid: the ground truth of one training sample -- the depth and the mask at the three stage
// sizes, six maps -- from the reference view's raw depth map (and, for DTU, its raw depth_visual PNG) in one
// launch. It restates bld_train.MVSDataset.__getitem__ (datasets/bld_train.py:134-148) and
// dtu_yao.MVSDataset.prepare_img / read_mask_hr / read_depth_hr (datasets/dtu_yao.py:75-122). Every resize
// there is cv2.resize(INTER_NEAREST), a pure gather whose source index per output row / column the host
// composes through the whole chain (halving, centre crop, stage scale) in float64
// (transmvsnet_amd.data.nearest_axis) and uploads once per size: rows [H3 + H2 + H1] and cols
// [W3 + W2 + W1] int32, stage 3 first. One thread per output pixel, 256-thread blocks of 64 x 4 pixels, so a
// wave stores 64 consecutive floats of one row (256 bytes) per map; the loads are strided gathers of a map
// that is read once. The blocks of the three stages are laid end to end on grid.x.
//
// tmvs_depth_eval_metrics: the twelve validation scalars of train.py:216-228 on the stage-3 depth
// (utils.AbsDepthError_metrics / Thres_metrics, utils.py:155-175), as tmvs_depth_metrics (loss.hip) does
// the three BlendedMVS ones: per-thread fp32 sums and integer counts, per-block sums in the fixed order of
// train_reduce.h's block_sum_store (fp64), one finalize block that adds the block partials in a fixed order.
// No atomics: two calls on the same input give the same bits.
#include "train_reduce.h"

namespace tmvs {

namespace td {

struct Stage {
  int h, w;           // output size
  int row0, col0;     // where this stage's entries start in rows / cols
  int bx, first;      // blocks along x; first block of this stage on grid.x
};

struct PyramidArgs {
  Stage st[3];  // [0] = stage 3 (full size), [1] = stage 2, [2] = stage 1
  float* depth[3];
  float* mask[3];
};

template <bool DTU>
__global__ __launch_bounds__(256) void gt_pyramid_kernel(const float* __restrict__ depth,
                                                         const unsigned char* __restrict__ png, int src_h, int src_w,
                                                         const int* __restrict__ rows, const int* __restrict__ cols,
                                                         float depth_min, float depth_end, PyramidArgs a) {
  const int blk = blockIdx.x;
  const int s = blk >= a.st[2].first ? 2 : blk >= a.st[1].first ? 1 : 0;  // block-uniform
  const Stage st = a.st[s];
  const int b = blk - st.first;
  const int x = (b % st.bx) * 64 + (threadIdx.x & 63), y = (b / st.bx) * 4 + (threadIdx.x >> 6);
  if (x >= st.w || y >= st.h) return;
  // the tables are the caller's: clamp so that no table can make the gather leave the source
  const int sy = min(max(rows[st.row0 + y], 0), src_h - 1);
  const int sx = min(max(cols[st.col0 + x], 0), src_w - 1);
  const size_t src = (size_t)sy * src_w + sx, dst = (size_t)y * st.w + x;
  const float d = depth[src];
  a.depth[s][dst] = d;
  if (DTU)
    a.mask[s][dst] = png[src] > 10 ? 1.f : 0.f;  // dtu_yao.py:94
  else
    a.mask[s][dst] = (d >= depth_min && d <= depth_end) ? 1.f : 0.f;  // bld_train.py:137 (NaN: 0)
}

// ---------------------------------------------------------------- validation metrics
constexpr int kEvalBlocks = 1024;
constexpr int kEvalSums = 7;     // |err| over the mask, then over each of the 6 bins
constexpr int kEvalCounts = 12;  // masked pixels, err > {2, 4, 8, 14, 20}, pixels in each of the 6 bins

// the block's sum of v[i] over its 256 threads, exact in integers: the xor butterfly inside each wave,
// then the 4 wave sums
template <int NV>
__device__ __forceinline__ void block_count_store(const unsigned (&v)[NV], unsigned* __restrict__ out) {
  __shared__ unsigned red[NV][kRedBlock / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    unsigned x = v[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    if (lane == 0) red[i][wv] = x;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NV; i += kRedBlock) out[i] = (red[i][0] + red[i][1]) + (red[i][2] + red[i][3]);
}

__global__ __launch_bounds__(kRedBlock) void depth_eval_partial_kernel(const float* __restrict__ est,
                                                                       const float* __restrict__ gt,
                                                                       const float* __restrict__ mask, int n,
                                                                       double* __restrict__ psum,
                                                                       unsigned* __restrict__ pcnt) {
  const float thr[5] = {2.f, 4.f, 8.f, 14.f, 20.f};
  const float lo[6] = {0.f, 2.f, 4.f, 8.f, 14.f, 20.f}, hi[6] = {2.f, 4.f, 8.f, 14.f, 20.f, 1e5f};
  float sum[kEvalSums];
  unsigned cnt[kEvalCounts];
#pragma unroll
  for (int i = 0; i < kEvalSums; ++i) sum[i] = 0.f;
#pragma unroll
  for (int i = 0; i < kEvalCounts; ++i) cnt[i] = 0u;
  for (long i = (long)blockIdx.x * kRedBlock + threadIdx.x; i < n; i += (long)gridDim.x * kRedBlock) {
    if (!(mask[i] > 0.5f)) continue;
    const float e = fabsf(est[i] - gt[i]);  // utils.py:160 / :170, fp32 as torch
    sum[0] += e;
    cnt[0] += 1u;
#pragma unroll
    for (int t = 0; t < 5; ++t) cnt[1 + t] += e > thr[t] ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const bool in = e >= lo[k] && e <= hi[k];  // both ends inclusive (utils.py:172)
      sum[1 + k] += in ? e : 0.f;
      cnt[6 + k] += in ? 1u : 0u;
    }
  }
  block_sum_store<false>(sum, psum + (size_t)blockIdx.x * kEvalSums);
  block_count_store(cnt, pcnt + (size_t)blockIdx.x * kEvalCounts);
}

// out[0] = abs_depth_error, out[1..5] = thres{2,4,8,14,20}mm_error, out[6..11] = the binned abs errors.
// Thread t adds the partials t, t + 256, ... in that order, then an LDS tree (tree_sum_256's order).
__global__ __launch_bounds__(kRedBlock) void depth_eval_finalize_kernel(const double* __restrict__ psum,
                                                                        const unsigned* __restrict__ pcnt, int nblk,
                                                                        float* __restrict__ out) {
  __shared__ unsigned long long cred[kRedBlock];
  __shared__ double sums[kEvalSums];
  __shared__ unsigned long long counts[kEvalCounts];
  for (int v = 0; v < kEvalSums; ++v) {
    const double s = tree_sum_256(psum + v, nblk, (size_t)kEvalSums);
    if (threadIdx.x == 0) sums[v] = s;
    __syncthreads();
  }
  for (int v = 0; v < kEvalCounts; ++v) {
    unsigned long long c = 0;
    for (int k = threadIdx.x; k < nblk; k += kRedBlock) c += pcnt[(size_t)k * kEvalCounts + v];
    cred[threadIdx.x] = c;
    __syncthreads();
    for (int st = kRedBlock / 2; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) cred[threadIdx.x] += cred[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) counts[v] = cred[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double n = (double)counts[0];
    out[0] = (float)(sums[0] / n);  // 0 / 0 = NaN: torch's mean of an empty tensor
    for (int t = 0; t < 5; ++t) out[1 + t] = (float)((double)counts[1 + t] / n);
    for (int k = 0; k < 6; ++k)
      out[6 + k] = counts[6 + k] ? (float)(sums[1 + k] / (double)counts[6 + k]) : 0.f;  // utils.py:173-174
  }
}

static size_t eval_sum_bytes() { return (size_t)kEvalBlocks * kEvalSums * sizeof(double); }

}  // namespace td

}  // namespace tmvs

using namespace tmvs;

extern "C" int tmvs_gt_pyramid(int mode, const float* depth, const unsigned char* mask_png, int src_h, int src_w,
                               int target_h, int target_w, float depth_min, float depth_end, const int* rows,
                               const int* cols, float* depth3, float* depth2, float* depth1, float* mask3,
                               float* mask2, float* mask1, void* stream) {
  if (mode != TMVS_GT_BLD && mode != TMVS_GT_DTU) return TMVS_ERR_ARG;
  if (!depth || !rows || !cols || !depth3 || !depth2 || !depth1 || !mask3 || !mask2 || !mask1) return TMVS_ERR_ARG;
  if (mode == TMVS_GT_DTU && !mask_png) return TMVS_ERR_ARG;
  if (src_h <= 0 || src_w <= 0 || src_h > (1 << 20) || src_w > (1 << 20)) return TMVS_ERR_SHAPE;
  int h3 = src_h, w3 = src_w;
  if (mode == TMVS_GT_DTU) {
    if (target_h <= 0 || target_w <= 0) return TMVS_ERR_SHAPE;
    if (target_h > src_h / 2 || target_w > src_w / 2) return TMVS_ERR_SHAPE;  // the crop leaves the halved image
    h3 = target_h;
    w3 = target_w;
  }
  if (h3 / 4 <= 0 || w3 / 4 <= 0) return TMVS_ERR_SHAPE;  // an empty stage 1
  td::PyramidArgs a;
  float* dp[3] = {depth3, depth2, depth1};
  float* mp[3] = {mask3, mask2, mask1};
  int row0 = 0, col0 = 0, first = 0;
  for (int s = 0; s < 3; ++s) {
    td::Stage& st = a.st[s];
    st.h = h3 >> s;
    st.w = w3 >> s;
    st.row0 = row0;
    st.col0 = col0;
    st.bx = (st.w + 63) / 64;
    st.first = first;
    row0 += st.h;
    col0 += st.w;
    first += st.bx * ((st.h + 3) / 4);
    a.depth[s] = dp[s];
    a.mask[s] = mp[s];
  }
  if (mode == TMVS_GT_DTU)
    hipLaunchKernelGGL(td::gt_pyramid_kernel<true>, dim3(first), dim3(256), 0, (hipStream_t)stream, depth, mask_png,
                       src_h, src_w, rows, cols, depth_min, depth_end, a);
  else
    hipLaunchKernelGGL(td::gt_pyramid_kernel<false>, dim3(first), dim3(256), 0, (hipStream_t)stream, depth, mask_png,
                       src_h, src_w, rows, cols, depth_min, depth_end, a);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" size_t tmvs_depth_eval_metrics_workspace(int n) {
  (void)n;
  return td::eval_sum_bytes() + (size_t)td::kEvalBlocks * td::kEvalCounts * sizeof(unsigned);
}

extern "C" int tmvs_depth_eval_metrics(const float* depth_est, const float* depth_gt, const float* mask, int n,
                                       void* workspace, size_t workspace_bytes, float* out, void* stream) {
  if (!depth_est || !depth_gt || !mask || !workspace || !out || n <= 0) return TMVS_ERR_ARG;
  if (((uintptr_t)workspace & 7) || workspace_bytes < tmvs_depth_eval_metrics_workspace(n)) return TMVS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int nblk0 = (n + kRedBlock - 1) / kRedBlock;
  const int nblk = nblk0 < td::kEvalBlocks ? nblk0 : td::kEvalBlocks;
  double* psum = (double*)workspace;
  unsigned* pcnt = (unsigned*)((char*)workspace + td::eval_sum_bytes());
  hipLaunchKernelGGL(td::depth_eval_partial_kernel, dim3(nblk), dim3(kRedBlock), 0, st, depth_est, depth_gt, mask, n,
                     psum, pcnt);
  TMVS_CHECK_LAUNCH();
  hipLaunchKernelGGL(td::depth_eval_finalize_kernel, dim3(1), dim3(kRedBlock), 0, st, (const double*)psum,
                     (const unsigned*)pcnt, nblk, out);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}
