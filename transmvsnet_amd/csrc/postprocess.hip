// The stage between the network and the fusion kernels, and the image resize in front of the network.
//
// tmvs_depth_postprocess: test.py:119-158 for one reference view (the two coarse confidence maps resized
// to the depth map's size, the confidence product, the 0.01 mask on the depth, utils.depth_normal's 8-bit
// depth, the clipped 8-bit colours) plus fusibile's decode of what test.py wrote (main.cpp:126-138), so
// the (B, G, R, depth) texel tmvs_fusibile reads is produced without the PNG in between.
//
// tmvs_resize_bilinear_u8 / _f32: general_eval.read_img (:99-103) + the cv2.resize of scale_mvs_input
// (:106-124) as transmvsnet_amd.data.resize_bilinear restates it + the HWC -> CHW transpose.
//
// Arithmetic follows the host functions' dtypes so the results are bitwise theirs: the lerps are float32
// a * (1 - t) + b * t, horizontal first, then vertical, uncontracted (-ffp-contract=off; no fmaf); float32
// divisions are IEEE (hipcc's default correctly rounded divide); the 1/255. products of fusibile's
// convertTo are float64 products rounded to float32 once.
//
// Both kernels are pure streams: one thread per pixel, 256-thread blocks of 64 x 4 pixels as
// dynamic_fusion_kernel, so a wave covers 64 consecutive pixels of one row: its dword loads and stores
// are 256-byte rows, the rgba store one dword and the rgbd store 16 bytes per lane (1 KiB per wave).
#include "common.h"

namespace tmvs {

namespace pp {

// the two-pass lerp of data.resize_bilinear on the four taps of one output pixel
__device__ __forceinline__ float lerp2(float a00, float a01, float a10, float a11, float tx, float ty) {
  const float top = a00 * (1.f - tx) + a01 * tx;
  const float bot = a10 * (1.f - tx) + a11 * tx;
  return top * (1.f - ty) + bot * ty;
}

// data.resize_axis for output index o at ratio n_in / n_out = 1/2 or 1/4: the source coordinate
// (o + 0.5) * ratio - 0.5 and its fraction are exact in float32 (o < 2^20); the fraction is 0 where the
// left tap is clamped at either border
__device__ __forceinline__ void axis(int o, float ratio, int n_in, int& i0, int& i1, float& t) {
  const float f = ((float)o + 0.5f) * ratio - 0.5f;
  const float fl = floorf(f);
  t = f - fl;
  int i = (int)fl;
  if (i < 0) t = 0.f;
  i = min(max(i, 0), n_in - 1);
  if (i >= n_in - 1) t = 0.f;
  i0 = i;
  i1 = min(i + 1, n_in - 1);
}

// cv2.resize(src [h][w], (W, H)) at output pixel (x, y), W / w = H / h = 1 / ratio
__device__ __forceinline__ float upsample(const float* __restrict__ src, int h, int w, float ratio, int x, int y) {
  int x0, x1, y0, y1;
  float tx, ty;
  axis(x, ratio, w, x0, x1, tx);
  axis(y, ratio, h, y0, y1, ty);
  const float* __restrict__ r0 = src + (size_t)y0 * w;
  const float* __restrict__ r1 = src + (size_t)y1 * w;
  return lerp2(r0[x0], r0[x1], r1[x0], r1[x1], tx, ty);
}

// uint8(trunc(clip(v * 255, 0, 255))) (test.py:153); NaN -> 0
__device__ __forceinline__ unsigned colour_u8(float v) {
  float s = v * 255.f;
  s = s < 0.f ? 0.f : (s > 255.f ? 255.f : s);
  return (unsigned)(int)s;
}

// Mat::convertTo(CV_32F, 1 / 255.) of an 8-bit value (main.cpp:131): a float64 product, one rounding
__device__ __forceinline__ float unit_from_u8(unsigned u) { return (float)((double)u * (1.0 / 255.0)); }

}  // namespace pp

__global__ __launch_bounds__(256) void depth_postprocess_kernel(
    const float* __restrict__ depth, const float* __restrict__ conf3, const float* __restrict__ conf2,
    const float* __restrict__ conf1, const float* __restrict__ image, int H, int W, float conf_threshold,
    float depth_min, float depth_max, float* __restrict__ conf_final, float* __restrict__ depth_masked,
    unsigned* __restrict__ rgba, float4* __restrict__ rgbd) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const size_t HW = (size_t)H * W, o = (size_t)y * W + x;
  const float up1 = pp::upsample(conf1, H / 4, W / 4, 0.25f, x, y);
  const float up2 = pp::upsample(conf2, H / 2, W / 2, 0.5f, x, y);
  const float cf = (conf3[o] * up1) * up2;                // test.py:132, left to right
  const float d = cf < conf_threshold ? 0.f : depth[o];  // test.py:144; a NaN confidence does not mask
  conf_final[o] = cf;
  depth_masked[o] = d;
  if (!image) return;
  // utils.depth_normal (utils.py:11-22)
  const float dc = d < depth_min ? depth_min : (d > depth_max ? depth_max : d);
  const unsigned alpha = (unsigned)(int)(((dc - depth_min) / (depth_max - depth_min)) * 255.f);
  const unsigned r = pp::colour_u8(image[o]), g = pp::colour_u8(image[HW + o]), b = pp::colour_u8(image[2 * HW + o]);
  if (rgba) rgba[o] = r | (g << 8) | (b << 16) | (alpha << 24);
  if (rgbd) {
    const float a = pp::unit_from_u8(alpha);
    rgbd[o] = make_float4(pp::unit_from_u8(b), pp::unit_from_u8(g), pp::unit_from_u8(r),
                          (float)(425.0 + 512.0 * (double)a));  // main.cpp:136
  }
}

// one tap of the source image as read_img returns it: uint8 HWC / 255.0, or a float32 CHW plane
__device__ __forceinline__ float resize_tap(const unsigned char* __restrict__ src, int h, int w, int c, int y, int x) {
  return (float)src[((size_t)y * w + x) * 3 + c] / 255.0f;
}
__device__ __forceinline__ float resize_tap(const float* __restrict__ src, int h, int w, int c, int y, int x) {
  return src[((size_t)c * h + y) * w + x];
}

template <typename T>
__global__ __launch_bounds__(256) void resize_bilinear_kernel(
    const T* __restrict__ src, int C, int h, int w, const int* __restrict__ x0t, const int* __restrict__ x1t,
    const float* __restrict__ txt, const int* __restrict__ y0t, const int* __restrict__ y1t,
    const float* __restrict__ tyt, int H, int W, float* __restrict__ dst) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  // the tables are the caller's: clamp so that no table can make a tap leave the source
  const int x0 = min(max(x0t[x], 0), w - 1), x1 = min(max(x1t[x], 0), w - 1);
  const int y0 = min(max(y0t[y], 0), h - 1), y1 = min(max(y1t[y], 0), h - 1);
  const float tx = txt[x], ty = tyt[y];
  const size_t HW = (size_t)H * W, o = (size_t)y * W + x;
  for (int c = 0; c < C; ++c)
    dst[c * HW + o] = pp::lerp2(resize_tap(src, h, w, c, y0, x0), resize_tap(src, h, w, c, y0, x1),
                                resize_tap(src, h, w, c, y1, x0), resize_tap(src, h, w, c, y1, x1), tx, ty);
}

}  // namespace tmvs

using namespace tmvs;

extern "C" int tmvs_depth_postprocess(const float* depth, const float* conf3, const float* conf2, const float* conf1,
                                      const float* image, int height, int width, float conf_threshold,
                                      float depth_min, float depth_max, float* conf_final, float* depth_masked,
                                      unsigned char* rgba_u8, float* rgbd, void* stream) {
  if (!depth || !conf3 || !conf2 || !conf1 || !conf_final || !depth_masked) return TMVS_ERR_ARG;
  if (!image && (rgba_u8 || rgbd)) return TMVS_ERR_ARG;
  if (height <= 0 || width <= 0 || !(depth_max > depth_min)) return TMVS_ERR_ARG;
  if (((uintptr_t)rgba_u8 & 3) || ((uintptr_t)rgbd & 15)) return TMVS_ERR_ARG;  // dword / 16-byte stores
  if (height % 4 || width % 4 || height > (1 << 20) || width > (1 << 20)) return TMVS_ERR_SHAPE;
  const dim3 grid((width + 63) / 64, (height + 3) / 4);
  hipLaunchKernelGGL(depth_postprocess_kernel, grid, dim3(256), 0, (hipStream_t)stream, depth, conf3, conf2, conf1,
                     image, height, width, conf_threshold, depth_min, depth_max, conf_final, depth_masked,
                     (unsigned*)rgba_u8, (float4*)rgbd);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

template <typename T>
static int resize_bilinear(const T* src, int channels, int src_h, int src_w, const int* x0, const int* x1,
                           const float* tx, const int* y0, const int* y1, const float* ty, int dst_h, int dst_w,
                           float* dst, void* stream) {
  if (!src || !x0 || !x1 || !tx || !y0 || !y1 || !ty || !dst) return TMVS_ERR_ARG;
  if (channels <= 0 || src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0) return TMVS_ERR_ARG;
  const dim3 grid((dst_w + 63) / 64, (dst_h + 3) / 4);
  hipLaunchKernelGGL(resize_bilinear_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, src, channels, src_h, src_w,
                     x0, x1, tx, y0, y1, ty, dst_h, dst_w, dst);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_resize_bilinear_u8(const unsigned char* src_u8, int src_h, int src_w, const int* x0, const int* x1,
                                       const float* tx, const int* y0, const int* y1, const float* ty, int dst_h,
                                       int dst_w, float* dst, void* stream) {
  return resize_bilinear(src_u8, 3, src_h, src_w, x0, x1, tx, y0, y1, ty, dst_h, dst_w, dst, stream);
}

extern "C" int tmvs_resize_bilinear_f32(const float* src, int channels, int src_h, int src_w, const int* x0,
                                        const int* x1, const float* tx, const int* y0, const int* y1, const float* ty,
                                        int dst_h, int dst_w, float* dst, void* stream) {
  return resize_bilinear(src, channels, src_h, src_w, x0, x1, tx, y0, y1, ty, dst_h, dst_w, dst, stream);
}
