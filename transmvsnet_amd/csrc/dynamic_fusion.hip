// Dynamic geometric-consistency filter of the Tanks & Temples output path (dynamic_fusion.py:78-280,
// run by scripts/test_tnt.sh) for one reference view: for every reference pixel and every source view,
// project the pixel with its depth into the source view, sample the source depth there, project that
// point back, and grade the round trip against nine nested tolerance levels i = 2..10 (pixel distance
// < i/4 and relative depth difference < i/1300). A pixel is geometrically consistent when at least
// thres_view sources pass the loosest level OR at least i sources pass level i for some i in 2..S; the
// depths reprojected from the sources that pass the loosest level are averaged with the pixel's own and
// the average is back-projected to the world point.
//
// Arithmetic follows the reference's numpy dtypes (DESIGN.md "Dynamic fusion" has the table): matrices
// are float32 (composed on the host with numpy, exactly as the reference composes them), every
// per-pixel product with them is float64 (int64 pixel grid x float32 -> float64), and values are cast
// to float32 exactly where the reference casts: the sampling coordinates, the reprojected depth and
// pixel, the relative depth difference and the depth sum. No fmaf: numpy's element-wise ops do not
// contract, and the build passes -ffp-contract=off.
//
// One thread per pixel, 256-thread blocks of 64 x 4 pixels as fusibile_kernel: a wave covers 64
// consecutive pixels of one row, so its own loads and stores are coalesced rows and the projected
// gathers of neighbouring lanes land on neighbouring source texels. The S <= 10 sources are walked
// in-register in order; the per-pair matrices are indexed by the (wave-uniform) loop counter.
#include "common.h"

namespace tmvs {

namespace df {
constexpr int PAIR = TMVS_DYNFUSE_PAIR_FLOATS;
constexpr int REF = TMVS_DYNFUSE_REF_FLOATS;
constexpr int LEVELS = 9;  // i = 2..10 (dynamic_fusion.py:134)
// offsets into a pair block (transmvsnet_amd.dynamic_fusion.pair_constants)
constexpr int KINV_REF = 0, T_RS = 9, K_SRC = 21, KINV_SRC = 30, T_SR = 39, K_REF = 51;
// offsets into the reference block
constexpr int R_KINV = 0, R_EINV = 9;
}  // namespace df

// y = M x, M 3x3 float32 row-major promoted to double (np.matmul(float32 [3,3], float64 [3,N]))
__device__ __forceinline__ void df_mul3(const float* __restrict__ m, double a, double b, double c, double* y) {
  y[0] = ((double)m[0] * a + (double)m[1] * b) + (double)m[2] * c;
  y[1] = ((double)m[3] * a + (double)m[4] * b) + (double)m[5] * c;
  y[2] = ((double)m[6] * a + (double)m[7] * b) + (double)m[8] * c;
}

// y = (T [x; 1])[:3], T = rows 0-2 of a 4x4 float32 row-major
__device__ __forceinline__ void df_mul34(const float* __restrict__ t, const double* x, double* y) {
  y[0] = (((double)t[0] * x[0] + (double)t[1] * x[1]) + (double)t[2] * x[2]) + (double)t[3];
  y[1] = (((double)t[4] * x[0] + (double)t[5] * x[1]) + (double)t[6] * x[2]) + (double)t[7];
  y[2] = (((double)t[8] * x[0] + (double)t[9] * x[1]) + (double)t[10] * x[2]) + (double)t[11];
}

__device__ __forceinline__ float df_tap(const float* __restrict__ img, int H, int W, int x, int y) {
  return ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) ? img[(size_t)y * W + x] : 0.f;
}

// cv2.remap(img, x, y, INTER_LINEAR), constant border 0 (dynamic_fusion.py:98). BITS = 5: OpenCV's
// fixed-point path, coordinates rounded (half to even) to 1/32 pixel; BITS = 0: exact fractions.
// Weights and the left-to-right tap sum in float32; taps outside the image contribute 0.
template <int BITS>
__device__ __forceinline__ float df_remap(const float* __restrict__ img, int H, int W, float x, float y) {
  int ix, iy;
  float fx, fy;
  if (BITS > 0) {
    const float one = (float)(1 << BITS), lim = 1073741824.f;
    const float xs = x * one, ys = y * one;
    if (!(xs > -lim && xs < lim && ys > -lim && ys < lim)) return 0.f;  // also non-finite
    const int sx = (int)rintf(xs), sy = (int)rintf(ys);
    ix = sx >> BITS;
    iy = sy >> BITS;
    fx = (float)(sx & ((1 << BITS) - 1)) * (1.f / one);
    fy = (float)(sy & ((1 << BITS) - 1)) * (1.f / one);
  } else {
    const float lim = 1073741824.f;
    if (!(x > -lim && x < lim && y > -lim && y < lim)) return 0.f;
    const float xf = floorf(x), yf = floorf(y);
    ix = (int)xf;
    iy = (int)yf;
    fx = x - xf;
    fy = y - yf;
  }
  if (ix < -1 || ix >= W || iy < -1 || iy >= H) return 0.f;  // all four taps outside
  const float t00 = df_tap(img, H, W, ix, iy), t10 = df_tap(img, H, W, ix + 1, iy);
  const float t01 = df_tap(img, H, W, ix, iy + 1), t11 = df_tap(img, H, W, ix + 1, iy + 1);
  const float w00 = (1.f - fx) * (1.f - fy), w10 = fx * (1.f - fy), w01 = (1.f - fx) * fy, w11 = fx * fy;
  return ((t00 * w00 + t10 * w10) + t01 * w01) + t11 * w11;
}

template <int BITS>
__global__ __launch_bounds__(256) void dynamic_fusion_kernel(
    const float* __restrict__ depths, int V, int H, int W, int ref, const int* __restrict__ src_views, int S,
    const float* __restrict__ pairs, const float* __restrict__ ref_cam, const float* __restrict__ confidence,
    float photo_threshold, int thres_view, unsigned char* __restrict__ geo_count, unsigned char* __restrict__ mask,
    float* __restrict__ depth_avg, float* __restrict__ xyz) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const size_t HW = (size_t)H * W, o = (size_t)y * W + x;
  const float d_ref = depths[(size_t)ref * HW + o];
  const double xd = (double)x, yd = (double)y;
  // (x, y, 1) * depth: int64 * float32 -> float64 (:86)
  const double p0 = xd * (double)d_ref, p1 = yd * (double)d_ref, p2 = (double)d_ref;

  int cnt[df::LEVELS];
#pragma unroll
  for (int l = 0; l < df::LEVELS; ++l) cnt[l] = 0;
  float sum = 0.f;  // Python's sum() starts from int 0: 0 + a == a
  for (int s = 0; s < S; ++s) {
    const int sv = src_views[s];
    if ((unsigned)sv >= (unsigned)V) continue;  // contract: in [0, V); never read outside depths
    const float* __restrict__ pc = pairs + (size_t)s * df::PAIR;
    const float* __restrict__ dsrc = depths + (size_t)sv * HW;
    double a[3], b[3], c[3];
    // step 1 (:85-92): reference pixel -> source pixel
    df_mul3(pc + df::KINV_REF, p0, p1, p2, a);
    df_mul34(pc + df::T_RS, a, b);
    df_mul3(pc + df::K_SRC, b[0], b[1], b[2], c);
    const double xs = c[0] / c[2], ys = c[1] / c[2];
    // step 2 (:96-113): sample the source depth at the float32 coordinates, project back with the float64 ones
    const float dsamp = df_remap<BITS>(dsrc, H, W, (float)xs, (float)ys);
    df_mul3(pc + df::KINV_SRC, xs * (double)dsamp, ys * (double)dsamp, (double)dsamp, a);
    df_mul34(pc + df::T_SR, a, b);
    df_mul3(pc + df::K_REF, b[0], b[1], b[2], c);
    const float d_rep = (float)b[2];
    const float x_rep = (float)(c[0] / c[2]), y_rep = (float)(c[1] / c[2]);
    // :128-132: dist float64 (float32 - int64), relative depth difference float32
    const double dx = (double)x_rep - xd, dy = (double)y_rep - yd;
    const double dist = sqrt(dx * dx + dy * dy);
    const float rel = fabsf(d_rep - d_ref) / d_ref;
#pragma unroll
    for (int l = 0; l < df::LEVELS; ++l) {
      const int i = l + 2;
      const double td = (double)i / 4.0;
      const float tr = (float)((double)i / 1300.0);
      if (dist < td && rel < tr) ++cnt[l];  // NaN / inf fail every level
    }
    const bool loosest = dist < 10.0 / 4.0 && rel < (float)(10.0 / 1300.0);
    sum = sum + (loosest ? d_rep : 0.f);  // depth_reprojected[~mask] = 0 (:138), summed in source order (:228)
  }
  sum = sum + d_ref;

  const int n10 = cnt[df::LEVELS - 1];
  bool geo = n10 >= thres_view;  // :222
#pragma unroll
  for (int l = 0; l < df::LEVELS; ++l)
    if (l + 2 <= S && cnt[l] >= l + 2) geo = true;  // :224-225, levels 2..S only
  const bool photo = confidence[o] > photo_threshold;  // :182
  const bool fin = photo && geo;
  const double davg = (double)sum / (double)(n10 + 1);  // float32 / int32 -> float64 (:228)

  geo_count[o] = (unsigned char)n10;
  mask[o] = (unsigned char)((photo ? 1 : 0) | (geo ? 2 : 0) | (fin ? 4 : 0));
  depth_avg[o] = (float)davg;
  float X0 = 0.f, X1 = 0.f, X2 = 0.f;
  if (fin) {  // :259-262
    double a[3], w[3];
    df_mul3(ref_cam + df::R_KINV, xd * davg, yd * davg, davg, a);
    df_mul34(ref_cam + df::R_EINV, a, w);
    X0 = (float)w[0];
    X1 = (float)w[1];
    X2 = (float)w[2];
  }
  xyz[3 * o + 0] = X0;
  xyz[3 * o + 1] = X1;
  xyz[3 * o + 2] = X2;
}

}  // namespace tmvs

using namespace tmvs;

extern "C" int tmvs_dynamic_fusion(const float* depths, int n_views, int height, int width, int ref_view,
                                   const int* src_views, int n_src, const float* pair_blocks, const float* ref_block,
                                   const float* confidence, float photo_threshold, int thres_view, int subpixel_bits,
                                   unsigned char* geo_count, unsigned char* mask, float* depth_avg, float* xyz,
                                   void* stream) {
  if (!depths || !src_views || !pair_blocks || !ref_block || !confidence || !geo_count || !mask || !depth_avg || !xyz)
    return TMVS_ERR_ARG;
  if (n_views <= 0 || height <= 0 || width <= 0 || ref_view < 0 || ref_view >= n_views) return TMVS_ERR_ARG;
  if (n_src < 1 || n_src > TMVS_DYNFUSE_MAX_SRC || thres_view < 1) return TMVS_ERR_ARG;
  if (subpixel_bits != 0 && subpixel_bits != 5) return TMVS_ERR_ARG;
  const dim3 grid((width + 63) / 64, (height + 3) / 4);
  if (subpixel_bits == 5)
    hipLaunchKernelGGL(dynamic_fusion_kernel<5>, grid, dim3(256), 0, (hipStream_t)stream, depths, n_views, height,
                       width, ref_view, src_views, n_src, pair_blocks, ref_block, confidence, photo_threshold,
                       thres_view, geo_count, mask, depth_avg, xyz);
  else
    hipLaunchKernelGGL(dynamic_fusion_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, depths, n_views, height,
                       width, ref_view, src_views, n_src, pair_blocks, ref_block, confidence, photo_threshold,
                       thres_view, geo_count, mask, depth_avg, xyz);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}
