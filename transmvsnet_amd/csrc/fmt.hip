// Feature Matching Transformer (models/FMT.py) linear attention on MI355X.
//
// d_model = 32, 8 heads x 4 dims, tokens [nv][L][32] (channels-last stage-1 map). One
// EncoderLayer (FMT.py:96-111) is two launches plus a tiny combine:
//   fmt_kv_partial  : per source token K = elu(Wk x + bk) + 1, V = Wv x + bv, accumulate
//                     KV[h][m][d] = Σ_s K[h,d] V[h,m] and Ksum[h][d] = Σ_s K[h,d]  (FMT.py:23-32)
//                     per workgroup -> partial slab [nv][nblk][160]
//   fmt_kv_combine  : sums the slabs in a fixed order (bitwise reproducible; no atomics)
// (dense 32x32 linears of the FFN use W2 transposed, TMVS_ENC_W2T)
//   fmt_apply       : per query token: Q = elu(Wq x + bq) + 1, Z = 1/(Q·Ksum + 1e-6),
//                     msg = (Q·KV) Z, x = LN1(x + Wo msg + bo), x = LN2(x + W2 relu(W1 x + b1) + b2)
// Cross layers read the reference view's (KV, Ksum) for every source view (kv stride 0):
// the reference recomputes the identical values per view (FMT.py:170-176).
//   fmt_pair        : on the source views, self layer 2j and cross layer 2j+1 in one launch
//                     (fmt_apply_pair, for pipeline.hip). Both are per-token maps, and the cross layer's
//                     K/V comes from the reference view, so nothing is reduced over the source tokens
//                     between them: the tile stays in registers from one layer to the next (one token
//                     load and one store per pair) and the tokens are bitwise those of two fmt_apply
//                     launches -- the per-layer tile body apply_layer is the one copy both kernels run.
//                     Two layers' fragments and vectors are 52.7 KB of LDS. 4-wave blocks would fit 3
//                     times per CU, 3 waves/SIMD, and the one-round tiling of the C2 launch (15,552
//                     tiles) would quantise to 6 tiles per wave; 8-wave blocks fit twice (4 waves/SIMD,
//                     as the one-layer apply: 120 VGPRs) and stage the weights once per 8 waves.
//
// The token-wise linears are dense 32x32 / 32x64 / 64x32 GEMMs over tiles of 16 tokens on the
// exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32: D = A.B + C as an fp32 FMA chain, the VALU
// fp32 rate):
//   D[o][t] = sum_k W[o][k] X[t][k]   A = W (16 outputs x 4 k),  B = X^T (4 k x 16 tokens)
// The weights are staged once per workgroup into LDS as A fragments in read order (stage_afrag)
// and read back inside the tile loop, one ds_read_b128 per 4 k-steps; the tokens and every
// intermediate stay in registers.
// Lane l holds D[o = 16mb + 4(l>>4) + r][t = l&15]: a token's 32 features live in lanes
// t, t+16, t+32, t+48 (8 each), and head h = 4mb + (l>>4) is lane-local (4 consecutive features).
// K-step s of a linear takes, in lane group g = l>>4, input feature kfeat(s, g) = 16(s>>2) + 4g + (s&3):
// exactly the register (mb = s>>2, r = s&3) that lane already holds from the previous linear's
// accumulator -- so the linears chain with no data movement. Within a chain the input features
// are summed in that permuted order (an exact fp32 FMA chain; the reference's BLAS order is
// unknown anyway). History: the VALU version was bound by weight delivery (PMC); with
// the A fragments resident in VGPRs (96 of them) the apply was capped at 2 waves/SIMD.
#include "fmt_common.h"

namespace tmvs {

// tokens[v][p][c] = feat[v][c][p] + pe[c][y][x]: a block transposes 64 pixels x 32 channels through
// LDS for every view (coalesced 256-B channel rows in, 8 KB of contiguous token rows out), reading
// its positional-encoding tile once for all views.
__global__ __launch_bounds__(256) void fmt_embed_kernel(const float* __restrict__ feat, long view_stride,
                                                        const float* __restrict__ pe, int pe_h, int pe_w, int H, int W,
                                                        int nv, float* __restrict__ tokens) {
  __shared__ float tile[64][kD + 1];
  const int HW = H * W;
  const int p0 = blockIdx.x * 64;
  const int px = threadIdx.x & 63, c0 = threadIdx.x >> 6;  // loads: pixel px, channels c0 + 4k
  const int p = p0 + px;
  const bool in = p < HW;
  const int y = in ? p / W : 0, x = in ? p - y * W : 0;
  float pv[kD / 4];
#pragma unroll
  for (int k = 0; k < kD / 4; ++k) pv[k] = in ? pe[((size_t)(c0 + 4 * k) * pe_h + y) * pe_w + x] : 0.f;
  const int tp = threadIdx.x >> 3, q = threadIdx.x & 7;  // stores: token tp (and tp + 32), channel quad q
  float t[kD / 4];
  auto load = [&](int v) {
    const float* f = feat + (size_t)v * view_stride;
#pragma unroll
    for (int k = 0; k < kD / 4; ++k) t[k] = in ? f[(size_t)(c0 + 4 * k) * HW + p] : 0.f;
  };
  load(0);
#pragma unroll 1
  for (int v = 0; v < nv; ++v) {
    __syncthreads();  // the previous view's tile has been stored
#pragma unroll
    for (int k = 0; k < kD / 4; ++k) tile[px][c0 + 4 * k] = t[k] + pv[k];
    __syncthreads();
    if (v + 1 < nv) load(v + 1);  // in flight during this view's stores
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = tp + 32 * h;
      if (p0 + r < HW)
        *reinterpret_cast<float4*>(tokens + ((size_t)v * HW + p0 + r) * kD + 4 * q) =
            make_float4(tile[r][4 * q], tile[r][4 * q + 1], tile[r][4 * q + 2], tile[r][4 * q + 3]);
    }
  }
}

// A fragments of a [OUT][IN] linear (TRANS: the packed matrix is stored [IN][OUT]), staged in LDS in
// read order [mb][s/4][lane][4] with element (mb, s, l) = W[16mb + (l&15)][kfeat(s, l>>4)]: one
// ds_read_b128 per lane serves 4 consecutive k-steps of an MFMA chain, and the 64 lanes read 1 KiB
// contiguous (conflict-free).
// The copy walks the packed matrix in memory order, four consecutive floats per thread (coalesced; one
// 16-byte load where W is 16-byte aligned, as every TMVS_ENC_* offset of an aligned block is), and scatters
// into the fragment: feature i sits at (s4, g, j) = (i >> 4, (i >> 2) & 3, i & 3), the inverse of kfeat
// (the header comment's k-step order).
// Four consecutive inputs of one output are one 16-byte fragment entry; with TRANS the four are consecutive
// outputs, the same j of four neighbouring lanes.
template <int OUT, int IN, bool TRANS>
__device__ __forceinline__ void stage_afrag(const float* __restrict__ W, float* __restrict__ lds) {
  constexpr int N = OUT * IN;  // = (OUT/16) * (IN/16) * 64 lanes * 4
  const bool aligned = (reinterpret_cast<size_t>(W) & 15) == 0;  // block-uniform
  for (int e = 4 * threadIdx.x; e < N; e += 4 * blockDim.x) {
    const float4 t = aligned ? ld4(W + e) : make_float4(W[e], W[e + 1], W[e + 2], W[e + 3]);
    const int o = TRANS ? e % OUT : e / IN, i = TRANS ? e / OUT : e % IN;  // of t.x
    const int at = (((o >> 4) * (IN / 16) + (i >> 4)) * 64 + 16 * ((i >> 2) & 3) + (o & 15)) * 4 + (i & 3);
    if (TRANS) {
      lds[at] = t.x, lds[at + 4] = t.y, lds[at + 8] = t.z, lds[at + 12] = t.w;
    } else {
      *reinterpret_cast<float4*>(lds + at) = t;
    }
  }
}

// acc[mb] = sum_s A[mb][s] * in[s>>2][s&3] for one tile (in: the B operand registers, the D layout of
// the input), A from the LDS fragments fl
template <int OUT, int IN>
__device__ __forceinline__ void mfma_linear_lds(const float* __restrict__ fl, const floatx4_t (&in)[IN / 16],
                                                floatx4_t (&acc)[OUT / 16], int lane) {
#pragma unroll
  for (int mb = 0; mb < OUT / 16; ++mb) acc[mb] = floatx4_t{0.f, 0.f, 0.f, 0.f};
  // per s4: every output block's fragment first, then the MFMAs block-interleaved (each accumulator's
  // own order unchanged), so consecutive MFMAs feed different accumulators
#pragma unroll
  for (int s4 = 0; s4 < IN / 16; ++s4) {
    float4 a4[OUT / 16];
#pragma unroll
    for (int mb = 0; mb < OUT / 16; ++mb) a4[mb] = ld4(fl + ((mb * (IN / 16) + s4) * 64 + lane) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int mb = 0; mb < OUT / 16; ++mb)
        acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(j == 0 ? a4[mb].x : j == 1 ? a4[mb].y : j == 2 ? a4[mb].z : a4[mb].w,
                                                       in[s4][j], acc[mb], 0, 0, 0);
  }
}

// What the tile-walking kernels (fmt_kv_partial_kernel, fmt_apply_kernel, fmt_pair_kernel) share: WPB
// waves per block (4; the pair kernel 8), wave wv of block b walks tpw tiles of 16 tokens from tile
// (WPB b + wv) tpw.
//
// the wave index, wave-uniform (readfirstlane): the tile loop is then scalar control flow, not a divergent
// loop whose per-lane exits make the compiler wait vmcnt(0) (stores included) at its head
__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
template <int WPB = 4>
__device__ __forceinline__ int first_tile(int wv, int tpw) { return (blockIdx.x * WPB + wv) * tpw; }
// an opaque 0 to offset LDS pointers by: the fragment reads stay in the loop (not hoisted back into VGPRs).
// An SGPR: a VGPR here could alias a pending load (vmcnt wait)
__device__ __forceinline__ int opaque_zero() {
  int salt = 0;
  asm volatile("" : "+s"(salt));
  return salt;
}
// token t's row of an [n][32] view, clamped to the last one: the next tile is prefetched unconditionally
// (past the wave's range the value is never used) -- a branch there made the compiler wait vmcnt(0) for
// the prefetch before the tile's first MFMA
template <typename T>
__device__ __forceinline__ T* row(T* base, int t, int n) { return base + (size_t)(t < n ? t : n - 1) * kD; }
// one 16-byte (LDS) read as four scalars
__device__ __forceinline__ void ld4(const float* p, float (&a)[4]) {
  const float4 t = ld4(p);
  a[0] = t.x, a[1] = t.y, a[2] = t.z, a[3] = t.w;
}

// a token's 32 features are spread over lanes t, t+16, t+32, t+48 (8 per lane)
__device__ __forceinline__ float token_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

__device__ __forceinline__ void layer_norm_frag(floatx4_t (&x)[2], const float* __restrict__ g,
                                                const float* __restrict__ b, int lane) {
  float s = 0.f;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) s += x[mb][r];
  const float mean = token_sum(s) / (float)kD;
  float v = 0.f;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float d = x[mb][r] - mean;
      v = fmaf(d, d, v);
    }
  const float rstd = 1.f / sqrtf(token_sum(v) / (float)kD + kLnEps);
  const float bias = -rstd * mean;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    // features 16 mb + 4 (lane >> 4) + r, r < 4: one 16-byte read each of gamma and beta (aligned)
    float gg[4], bb[4];
    ld4(g + 16 * mb + 4 * (lane >> 4), gg);
    ld4(b + 16 * mb + 4 * (lane >> 4), bb);
#pragma unroll
    for (int r = 0; r < 4; ++r) x[mb][r] = fmaf(fmaf(x[mb][r], rstd, bias), gg[r], bb[r]);
  }
}

__device__ __forceinline__ void load_token_frag(const float* __restrict__ row, floatx4_t (&x)[2], int lane) {
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    const float4 t = ld4(row + 16 * mb + 4 * (lane >> 4));
    x[mb] = floatx4_t{t.x, t.y, t.z, t.w};
  }
}

constexpr int kKvTilesPerWave = 8;     // kv: at most this many tiles per wave (see kv_tiles_per_wave)

// x + x[lane ^ 1], then ^2, ^4, ^8: the butterfly sum over a 16-lane row. The partner values move by
// DPP (xor_lane_dpp, common.h), not by ds_bpermute through the LDS unit: the same values in the same
// additions, so the sums are bitwise those of __shfl_xor.
template <int OFF>
__device__ __forceinline__ float xor_add(float x) {
  return x + __int_as_float(xor_lane_dpp<OFF>(__float_as_int(x)));
}
__device__ __forceinline__ float xor_sum16(float x) { return xor_add<8>(xor_add<4>(xor_add<2>(xor_add<1>(x)))); }

// (KV, Ksum) partial sums: per wave, tiles of 16 source tokens; K, V by MFMA; per lane the
// two heads it owns are accumulated over its tokens, then summed over the 16 token lanes.
__global__ __launch_bounds__(256) void fmt_kv_partial_kernel(const float* __restrict__ src, int S,
                                                              const float* __restrict__ w,
                                                              float* __restrict__ partial, int tpw) {
  __shared__ float red[4][kKV];
  __shared__ __attribute__((aligned(16))) float frag[2 * 32 * 32];  // Wk, Wv fragments (see stage_afrag)
  const int v = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = wave_index();
  const int g = lane >> 4;
  stage_afrag<32, 32, true>(w + TMVS_ENC_WK, frag);
  stage_afrag<32, 32, true>(w + TMVS_ENC_WV, frag + 1024);
  float bk[2][4], bv[2][4];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bk[mb][r] = w[TMVS_ENC_BK + 16 * mb + 4 * g + r];
      bv[mb][r] = w[TMVS_ENC_BV + 16 * mb + 4 * g + r];
    }
  float kv[2][16], ks[2][4];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
    for (int i = 0; i < 16; ++i) kv[mb][i] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) ks[mb][i] = 0.f;
  }
  __syncthreads();
  const float* sv = src + (size_t)v * S * kD;
  const int tile0 = first_tile(wv, tpw);
  floatx4_t xa[2], xb[2];  // this tile's tokens, the next tile's (loaded while this one computes)
  if (tile0 * 16 < S) load_token_frag(row(sv, tile0 * 16 + (lane & 15), S), xa, lane);
  auto tile = [&](int it, floatx4_t (&cur)[2], floatx4_t (&nxt)[2]) {
    const float* fr = frag + opaque_zero();
    const int t = (tile0 + it) * 16 + (lane & 15);
    const bool ok = t < S;
    const floatx4_t xin[2] = {cur[0], cur[1]};
    floatx4_t kk[2], vv[2];
    load_token_frag(row(sv, t + 16, S), nxt, lane);
    mfma_linear_lds<32, 32>(fr, xin, kk, lane);
    mfma_linear_lds<32, 32>(fr + 1024, xin, vv, lane);
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      float kh[4], vh[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        kh[r] = ok ? elu1(kk[mb][r] + bk[mb][r]) : 0.f;
        vh[r] = ok ? vv[mb][r] + bv[mb][r] : 0.f;
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int d = 0; d < 4; ++d) kv[mb][m * 4 + d] = fmaf(kh[d], vh[m], kv[mb][m * 4 + d]);
#pragma unroll
      for (int d = 0; d < 4; ++d) ks[mb][d] += kh[d];
    }
  };
  // (unrolled by two like the apply it needed 144 VGPRs, 3 waves/SIMD: one buffer, copied per tile)
#pragma unroll 1
  for (int it = 0; it < tpw; ++it) {
    if ((tile0 + it) * 16 >= S) break;  // wave-uniform
    tile(it, xa, xb);
    xa[0] = xb[0];
    xa[1] = xb[1];
  }
  // sum over the 16 token lanes of each lane group (fixed butterfly)
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
    for (int i = 0; i < 16; ++i) kv[mb][i] = xor_sum16(kv[mb][i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) ks[mb][i] = xor_sum16(ks[mb][i]);
  }
  if ((lane & 15) == 0) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int h = 4 * mb + g;
#pragma unroll
      for (int i = 0; i < 16; ++i) red[wv][kv_at(h, i >> 2, i & 3)] = kv[mb][i];
#pragma unroll
      for (int i = 0; i < 4; ++i) red[wv][ksum_at(h, i)] = ks[mb][i];
    }
  }
  __syncthreads();
  if (threadIdx.x < kKV) {
    const int i = threadIdx.x;
    partial[((size_t)v * gridDim.x + blockIdx.x) * kKV + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
  }
}

// grid (nv, 5): 32 groups x 32 entries; group g sums partial blocks g, g+32, ... with all
// loads independent, then the 32 group sums are added in a fixed order (bitwise reproducible).
__global__ __launch_bounds__(1024) void fmt_kv_combine_kernel(const float* __restrict__ partial, int nblk,
                                                              float* __restrict__ kv) {
  __shared__ float red[32][32];
  const int v = blockIdx.x;
  const int e = blockIdx.y * 32 + (threadIdx.x & 31);
  const int g = threadIdx.x >> 5;
  float s = 0.f;
#pragma unroll 4
  for (int b = g; b < nblk; b += 32) s += partial[((size_t)v * nblk + b) * kKV + e];
  red[g][threadIdx.x & 31] = s;
  __syncthreads();
  if (g == 0) {
    float t = red[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < 32; ++k) t += red[k][threadIdx.x];
    kv[(size_t)v * kKV + e] = t;
  }
}

// One encoder layer's share of LDS in the applies: the view's K/V summary, the per-feature vectors (read
// from LDS in the tile loop: a global load there is a full memory latency, and its vmcnt(0) wait also
// drains the next tile's token prefetch) and the Wq, Wo, W1, W2 fragments.
// vec: [0, 32) BQ  [32, 64) BO  [64, 128) B1  [128, 160) B2  [160, 288) LN1G LN1B LN2G LN2B
constexpr int kVB2 = 128, kVLN = 160, kVec = 288;
constexpr int kApplyFrag = 32 * 32 * 2 + 64 * 32 * 2;
__device__ __forceinline__ void stage_layer(const float* __restrict__ w, const float* __restrict__ kv,
                                            float* __restrict__ kvs, float* __restrict__ vec,
                                            float* __restrict__ frag) {
  if (threadIdx.x < kKV) kvs[threadIdx.x] = kv[threadIdx.x];
  for (int i = threadIdx.x; i < kVec; i += blockDim.x)
    vec[i] = i < 32 ? w[TMVS_ENC_BQ + i] : i < 64 ? w[TMVS_ENC_BO + i - 32] : i < 128 ? w[TMVS_ENC_B1 + i - 64]
                                                                                      : w[TMVS_ENC_B2 + i - kVB2];
  stage_afrag<32, 32, false>(w + TMVS_ENC_WQ, frag);
  stage_afrag<32, 32, false>(w + TMVS_ENC_WO, frag + 1024);
  stage_afrag<64, 32, false>(w + TMVS_ENC_W1, frag + 2048);
  stage_afrag<32, 64, true>(w + TMVS_ENC_W2T, frag + 4096);
}

// The rest of EncoderLayer.forward for one tile of 16 query tokens xs, entirely in registers: the one
// copy of the per-token arithmetic, shared by fmt_apply_kernel and fmt_pair_kernel (fr, vb, kvs: the
// layer's LDS as staged by stage_layer).
__device__ __forceinline__ void apply_layer(floatx4_t (&xs)[2], const float* fr, const float* vb, const float* kvs,
                                            int lane) {
  const int g = lane >> 4;
  floatx4_t q[2], msg[2];
  mfma_linear_lds<32, 32>(fr, xs, q, lane);
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    const int h = 4 * mb + g;
    // head h's K/V summary, bias and Ksum as 16-byte LDS reads issued together
    float bq[4], ksum[4], kvm[4][4];
    ld4(vb + 4 * h, bq);
    ld4(kvs + ksum_at(h, 0), ksum);
#pragma unroll
    for (int m = 0; m < 4; ++m) ld4(kvs + kv_at(h, m, 0), kvm[m]);
    float qe[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) qe[d] = elu1(q[mb][d] + bq[d]);
    float den = 0.f;
#pragma unroll
    for (int d = 0; d < 4; ++d) den = fmaf(qe[d], ksum[d], den);
    const float z = 1.f / (den + kAttnEps);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      float num = 0.f;
#pragma unroll
      for (int d = 0; d < 4; ++d) num = fmaf(qe[d], kvm[m][d], num);
      msg[mb][m] = num * z;
    }
  }
  floatx4_t a[2];
  mfma_linear_lds<32, 32>(fr + 1024, msg, a, lane);
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    float bo[4];
    ld4(vb + 32 + 16 * mb + 4 * g, bo);
#pragma unroll
    for (int r = 0; r < 4; ++r) xs[mb][r] = xs[mb][r] + (a[mb][r] + bo[r]);
  }
  layer_norm_frag(xs, vb + kVLN, vb + kVLN + kD, lane);
  floatx4_t hdn[4], ff[2];
  mfma_linear_lds<64, 32>(fr + 2048, xs, hdn, lane);
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    float b1[4];
    ld4(vb + 64 + 16 * mb + 4 * g, b1);
#pragma unroll
    for (int r = 0; r < 4; ++r) hdn[mb][r] = relu(hdn[mb][r] + b1[r]);
  }
  mfma_linear_lds<32, 64>(fr + 4096, hdn, ff, lane);
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    float b2[4];
    ld4(vb + kVB2 + 16 * mb + 4 * g, b2);
#pragma unroll
    for (int r = 0; r < 4; ++r) xs[mb][r] = xs[mb][r] + (ff[mb][r] + b2[r]);
  }
  layer_norm_frag(xs, vb + kVLN + 2 * kD, vb + kVLN + 3 * kD, lane);
}

// NL encoder layers in a row on each 16-token tile of view blockIdx.y, WPB waves per block: the tile is
// loaded once, stays in registers between the layers and is stored once. Layer i has weights w[i] and
// reads view v's K/V summary at kv[i] + v kv_stride[i] (stride 0: one summary for every view).
struct LayerArgs {
  const float* w;
  const float* kv;
  long kv_stride;
};
template <int NL, int WPB>
__device__ __forceinline__ void apply_tiles(float* __restrict__ x, int L, const LayerArgs (&layer)[NL], int tpw) {
  __shared__ __attribute__((aligned(16))) float kvs[NL][kKV];
  __shared__ __attribute__((aligned(16))) float vec[NL][kVec];
  __shared__ __attribute__((aligned(16))) float frag[NL][kApplyFrag];
  const int v = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = wave_index();
  const int g = lane >> 4;
#pragma unroll
  for (int i = 0; i < NL; ++i)
    stage_layer(layer[i].w, layer[i].kv + (size_t)v * layer[i].kv_stride, kvs[i], vec[i], frag[i]);
  __syncthreads();
  float* xv = x + (size_t)v * L * kD;
  const int tile0 = first_tile<WPB>(wv, tpw);
  // two token buffers used alternately (the loop unrolled by two, so they swap by name: a
  // loop-carried copy made the compiler wait vmcnt(0) -- this tile's stores included -- at the latch)
  floatx4_t xa[2], xb[2];
  load_token_frag(row(xv, tile0 * 16 + (lane & 15), L), xa, lane);
  auto tile = [&](int it, floatx4_t (&cur)[2], floatx4_t (&nxt)[2]) {
    const int salt = opaque_zero();
    const int t = (tile0 + it) * 16 + (lane & 15);
    const bool ok = t < L;
    float* out = row(xv, t, L);
    floatx4_t xs[2] = {cur[0], cur[1]};
    load_token_frag(row(xv, t + 16, L), nxt, lane);
    // (written out, not a loop over NL: as an unrolled loop of one trip the one-layer kernel came out at 240
    // VGPRs, 2 waves/SIMD, instead of 101 + 24 AGPRs)
    static_assert(NL == 1 || NL == 2, "layers per launch");
    apply_layer(xs, frag[0] + salt, vec[0] + salt, kvs[0], lane);
    if constexpr (NL == 2) apply_layer(xs, frag[1] + salt, vec[1] + salt, kvs[1], lane);
    if (ok) {
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
        *reinterpret_cast<float4*>(out + 16 * mb + 4 * g) = make_float4(xs[mb][0], xs[mb][1], xs[mb][2], xs[mb][3]);
    }
  };
#pragma unroll 1
  for (int it = 0; it < tpw; it += 2) {
    if ((tile0 + it) * 16 >= L) break;  // wave-uniform
    tile(it, xa, xb);
    if (it + 1 >= tpw || (tile0 + it + 1) * 16 >= L) break;
    tile(it + 1, xb, xa);
  }
}

// One encoder layer on every view of the launch.
// (amdgpu_waves_per_eu(5) fits it in 94 VGPRs without AGPRs, 5 waves/SIMD instead of 4: the 8 applies
// measured 456.6 vs 448.1 us per step, 6 waves (80 VGPRs + scratch) 472.0 -- profiles/r11n: not kept.
// Two tiles per call of the tile lambda, their MFMA chains interleaved, was an option nobody selected.)
__global__ __launch_bounds__(256) void fmt_apply_kernel(float* __restrict__ x, int L, const float* __restrict__ kvg,
                                                        long kv_stride, const float* __restrict__ w, int tpw) {
  const LayerArgs layer[1] = {{w, kvg, kv_stride}};
  apply_tiles<1, 4>(x, L, layer, tpw);
}

// Self layer 2j with each source view's own K/V (w0, kv0), then cross layer 2j+1 with the reference
// view's (w1, kv1, stride 0), on the source views: both are per-token maps and no reduction over the source
// tokens sits between them, so the tokens are bitwise those of two fmt_apply_kernel launches without the
// round trip through memory in between. Blocks of 8 waves: two layers' fragments are 52 KB, which 4-wave
// blocks would fit 3 times per CU (3 waves/SIMD); two 8-wave blocks keep the apply's 4 waves/SIMD and
// stage the weights half as often.
constexpr int kPairWaves = 8;
__global__ __launch_bounds__(64 * kPairWaves) __attribute__((amdgpu_waves_per_eu(4))) void fmt_pair_kernel(float* __restrict__ x, int L,
                                                                   const float* __restrict__ kv0, long kv0_stride,
                                                                   const float* __restrict__ w0,
                                                                   const float* __restrict__ kv1, long kv1_stride,
                                                                   const float* __restrict__ w1, int tpw) {
  const LayerArgs layer[2] = {{w0, kv0, kv0_stride}, {w1, kv1, kv1_stride}};
  apply_tiles<2, kPairWaves>(x, L, layer, tpw);
}

// Resident blocks of `kernel` on the whole GPU (its occupancy at `threads` per block: VGPRs, LDS)
template <typename K>
static long block_slots(K kernel, int threads = 256) {
  int dev = 0, cus = 0, per = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, threads, 0) != hipSuccess || per <= 0)
    per = 1024 / threads;
  return (long)(cus > 0 ? cus : 256) * per;
}
static int wave_slots_apply() {
  static long slots = 0;
  if (!slots) slots = 4 * block_slots(fmt_apply_kernel);
  return (int)slots;
}
static int wave_slots_pair() {
  static long slots = 0;
  if (!slots) slots = kPairWaves * block_slots(fmt_pair_kernel, 64 * kPairWaves);
  return (int)slots;
}

// Tiles per wave: as many as possible (small partial slabs, short combine) while the launch still
// has >= 2048 waves (2 per SIMD); the one-view cross-attention K/V otherwise runs at 0.1 waves/SIMD.
// (Sizing it from the occupancy like the apply measured 28.6 -> 26.4 us for the 5-view launch, but it
// changes the partial sums' grouping -- the K/V bits -- and with them a C2 near-tie at stage 2 whose
// flip then moves stage 3's hypotheses (tests/test_gpu_fullsize.py, r11g): kept as before.)
static int kv_tiles_per_wave(int nv, int S) {
  const int tiles = (S + 15) / 16;
  int tpw = kKvTilesPerWave;
  while (tpw > 2 && (long)nv * ((tiles + tpw - 1) / tpw) < 2048) tpw >>= 1;
  return tpw;
}
static int kv_nblk(int nv, int S) {
  const int per = 16 * 4 * kv_tiles_per_wave(nv, S);
  return (S + per - 1) / per;
}
// Tiles per wave for the apply: the whole launch in ONE round of resident waves (5 per SIMD at its
// 92 VGPRs since the bias vectors moved to LDS): with a fixed 4 tiles per wave the C2 grid (5 x 3888
// tiles = 4.75 waves per SIMD at 4/SIMD) ran as a full round plus a 3/4-empty second one (2.4
// waves/SIMD on average, r05f).
static int apply_tiles_per_wave(int nv, int L, int wave_slots) {
  const long tiles = (long)nv * ((L + 15) / 16);
  return (int)std::max<long>(1, (tiles + wave_slots - 1) / wave_slots);
}
static int apply_nblk(int L, int tpw, int wpb) { return (L + 16 * wpb * tpw - 1) / (16 * wpb * tpw); }

}  // namespace tmvs

using namespace tmvs;

extern "C" int tmvs_fmt_embed(const float* feat, long feat_view_stride, const float* pe, int pe_h, int pe_w, int nv,
                              int channels, int height, int width, float* tokens, void* stream) {
  if (!feat || !pe || !tokens || nv <= 0 || height <= 0 || width <= 0) return TMVS_ERR_ARG;
  if (channels != kD || height > pe_h || width > pe_w) return TMVS_ERR_SHAPE;
  const int HW = height * width;
  hipLaunchKernelGGL(fmt_embed_kernel, dim3((HW + 63) / 64), dim3(256), 0, (hipStream_t)stream, feat,
                     feat_view_stride, pe, pe_h, pe_w, height, width, nv, tokens);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" size_t tmvs_fmt_kv_grouped_workspace(int nv, int group_nv, int s_tokens) {
  if (nv <= 0 || group_nv <= 0 || s_tokens <= 0) return 0;
  return (size_t)nv * kv_nblk(group_nv, s_tokens) * kKV * sizeof(float);
}

extern "C" size_t tmvs_fmt_kv_workspace(int nv, int s_tokens) { return tmvs_fmt_kv_grouped_workspace(nv, nv, s_tokens); }

// The tiling (tiles per wave, hence each view's partial-sum grouping) is the one a launch over group_nv
// views uses, so a view's K/V is bitwise the same whichever subset of views a launch carries.
extern "C" int tmvs_fmt_kv_grouped(const float* source, int nv, int group_nv, int s_tokens, const float* enc_w,
                                   void* workspace, size_t workspace_bytes, float* kv, void* stream) {
  if (!source || !enc_w || !workspace || !kv || nv <= 0 || group_nv <= 0 || s_tokens <= 0) return TMVS_ERR_ARG;
  if (workspace_bytes < tmvs_fmt_kv_grouped_workspace(nv, group_nv, s_tokens)) return TMVS_ERR_ARG;
  const int nblk = kv_nblk(group_nv, s_tokens);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fmt_kv_partial_kernel, dim3(nblk, nv), dim3(256), 0, st, source, s_tokens, enc_w,
                     (float*)workspace, kv_tiles_per_wave(group_nv, s_tokens));
  TMVS_CHECK_LAUNCH();
  hipLaunchKernelGGL(fmt_kv_combine_kernel, dim3(nv, kKV / 32), dim3(1024), 0, st, (const float*)workspace, nblk, kv);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_fmt_kv(const float* source, int nv, int s_tokens, const float* enc_w, void* workspace,
                           size_t workspace_bytes, float* kv, void* stream) {
  return tmvs_fmt_kv_grouped(source, nv, nv, s_tokens, enc_w, workspace, workspace_bytes, kv, stream);
}

// tiles_per_wave > 0 overrides the occupancy-sized tiling (the per-token arithmetic, hence the output, is the same)
extern "C" int tmvs_fmt_apply_tiled(float* x, int nv, int l_tokens, const float* kv, long kv_view_stride,
                                    const float* enc_w, int tiles_per_wave, void* stream) {
  if (!x || !kv || !enc_w || nv <= 0 || l_tokens <= 0 || kv_view_stride < 0) return TMVS_ERR_ARG;
  const int tpw = tiles_per_wave > 0 ? tiles_per_wave : apply_tiles_per_wave(nv, l_tokens, wave_slots_apply());
  hipLaunchKernelGGL(fmt_apply_kernel, dim3(apply_nblk(l_tokens, tpw, 4), nv), dim3(256), 0, (hipStream_t)stream, x,
                     l_tokens, kv, kv_view_stride, enc_w, tpw);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

extern "C" int tmvs_fmt_apply(float* x, int nv, int l_tokens, const float* kv, long kv_view_stride,
                              const float* enc_w, void* stream) {
  return tmvs_fmt_apply_tiled(x, nv, l_tokens, kv, kv_view_stride, enc_w, 0, stream);
}

// Layers (w0, kv0: per view) then (w1, kv1: one summary for every view) on each token of x [nv][L][32] in one
// launch (fmt_pair_kernel): bitwise tmvs_fmt_apply with kv0, then tmvs_fmt_apply with kv1 and stride 0.
// Library-internal (common.h): reached through tmvs_fmt_forward and tmvs_fmt_forward_split.
int tmvs::fmt_apply_pair(float* x, int nv, int l_tokens, const float* kv0, const float* enc_w0, const float* kv1,
                         const float* enc_w1, void* stream) {
  if (!x || !kv0 || !enc_w0 || !kv1 || !enc_w1 || nv <= 0 || l_tokens <= 0) return TMVS_ERR_ARG;
  const int tpw = apply_tiles_per_wave(nv, l_tokens, wave_slots_pair());
  hipLaunchKernelGGL(fmt_pair_kernel, dim3(apply_nblk(l_tokens, tpw, kPairWaves), nv), dim3(64 * kPairWaves), 0,
                     (hipStream_t)stream, x, l_tokens, kv0, (long)kKV, enc_w0, kv1, 0L, enc_w1, tpw);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}
