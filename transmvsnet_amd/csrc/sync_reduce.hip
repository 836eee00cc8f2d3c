// The cross-rank combine of synchronised BatchNorm statistics (include/transmvs_sync.h): every rank holds the
// same [world][count] fp64 slots after the all-reduce that acts as a gather, and adds them in rank order, so
// the result is the same bits on every rank whatever algorithm the backend reduced with.
#include "common.h"
#include "../../include/transmvs_sync.h"

namespace tmvs {

constexpr int kRankSumBlock = 256;

__global__ __launch_bounds__(kRankSumBlock) void rank_sum_kernel(const double* __restrict__ slots, int world,
                                                                 long count, double* __restrict__ out) {
  const long i = (long)blockIdx.x * kRankSumBlock + threadIdx.x;
  if (i >= count) return;
  double t = slots[i];
  for (int r = 1; r < world; ++r) t += slots[(size_t)r * count + i];
  out[i] = t;
}

}  // namespace tmvs

using namespace tmvs;

extern "C" int tmvs_rank_sum(const double* slots, int world, long count, double* out, void* stream) {
  if (!slots || !out || world <= 0 || count <= 0) return TMVS_ERR_ARG;
  if ((count + kRankSumBlock - 1) / kRankSumBlock >= (1L << 31)) return TMVS_ERR_SHAPE;
  hipLaunchKernelGGL(rank_sum_kernel, dim3((unsigned)((count + kRankSumBlock - 1) / kRankSumBlock)),
                     dim3(kRankSumBlock), 0, (hipStream_t)stream, slots, world, count, out);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}
