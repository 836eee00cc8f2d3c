// CostRegNet (models/module.py:425-456) on MI355X.
//
// Layout: NDHWC fp32 activations. Eval-mode BN is an (alpha, shift) epilogue,
// y = relu(fmaf(acc, alpha, shift)) (tmvs_bn_fold; the reference CPU kernel's exact form). The MFMA
// layers' epilogue is act(v, lo) = v > lo ? v : lo: lo = 0 is that ReLU; lo = -inf with alpha = 1,
// shift = 0 and no skip gives the raw convolution the training path runs them for
// (tmvs_conv3d_mfma: train-mode forward before BatchNorm, and the data gradients).
//
// Mid layers (conv1..conv6, deconv conv7/9/11) are LDS-staged implicit GEMMs on the exact-fp32 matrix
// cores, v_mfma_f32_16x16x4_f32 (64 FLOP/clk/SIMD, the fp32 peak; no xf32 on gfx950):
//   A (16 x 4) = weights   [cout][k]   lane l: cout = l&15, k = l>>4
//   B (4 x 16) = input     [k][voxel]  lane l: k = l>>4,   voxel = l&15
//   D (16 x16)                          lane l: cout = 4*(l>>4)+r, voxel = l&15  -> one float4
//                                       store of 4 consecutive channels (NDHWC) per lane.
// K runs over (tap, channel): per tap and 16-channel chunk a lane loads 4 consecutive
// channels of one voxel (one float4) and issues 4 MFMAs, MFMA j taking channel
// chunk + (l>>4)*4 + j in both operands (conv1's 8 input channels: tap pairs, see its kernel).
// A "task" (one wave) is NBW rows of 16 output
// voxels x MBW blocks of 16 output channels; the 4 waves of a workgroup share the rows and
// split the output channels, so their input taps hit in L1.
// The transposed convs (ConvTranspose3d k3 s2 p1 op1) use the sub-pixel decomposition: a
// wave's 16 outputs share one parity per dimension, hence one tap set of 1, 2, 4 or 8 taps.
// conv0 (Cin 1) and prob (Cout 1) are direct VALU convolutions.
#include "common.h"

#include <utility>

namespace tmvs {

typedef float floatx4 __attribute__((ext_vector_type(4)));

// 4 consecutive channels of one voxel (B) or weight row (A): the operands of 4 MFMAs
struct Vec4 {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x;
    v[1] = t.y;
    v[2] = t.z;
    v[3] = t.w;
  }
  __device__ __forceinline__ void zero() { v[0] = v[1] = v[2] = v[3] = 0.f; }
};

// Range-checked raw buffer over one tensor: a lane whose 32-bit byte offset is out of range reads
// zeros (the buffer unit's bound check), so padding taps need no exec-mask branch and no 64-bit
// address per load; the wave-uniform part of an offset goes in the scalar offset. Branch-free load
// streams keep the compiler's vmcnt waits exact (a branch per load made it wait vmcnt(0)).
struct Buf {
  __amdgpu_buffer_rsrc_t r;
  __device__ __forceinline__ Buf(const float* base, uint32_t nbytes)
      : r(__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), (short)0, (int)nbytes, 0x00020000)) {}
  static constexpr int kOOB = (int)0x80000000u;  // any offset >= the range reads zeros
  __device__ __forceinline__ float4 ld4(int voff, int soff = 0) const {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
  }
  __device__ __forceinline__ void st4(float4 v, int voff) const {  // an out-of-range lane stores nothing
    typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
    const uintx4 u{__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(u, r, voff, 0, 0);
  }
};
__device__ __forceinline__ void buf_load(Vec4& d, const Buf& b, int voff, int soff = 0) {
  const float4 t = b.ld4(voff, soff);
  d.v[0] = t.x, d.v[1] = t.y, d.v[2] = t.z, d.v[3] = t.w;
}

struct Geo {
  int Di, Hi, Wi;  // input dims
  int Do, Ho, Wo;  // output dims
  float lo;        // epilogue floor: 0 = ReLU, -inf = none
  static Geo conv(int d, int h, int w, int stride, float lo) {  // k3 p1
    return stride == 1 ? Geo{d, h, w, d, h, w, lo} : Geo{d, h, w, (d - 1) / 2 + 1, (h - 1) / 2 + 1, (w - 1) / 2 + 1, lo};
  }
  static Geo deconv(int d, int h, int w, float lo) { return Geo{d, h, w, 2 * d, 2 * h, 2 * w, lo}; }  // k3 s2 p1 op1
};

__device__ __forceinline__ float act(float v, float lo) { return v > lo ? v : lo; }

// ---------------------------------------------------------------- shared by the MFMA kernels
// the epilogue of one D fragment: eval-mode BN and the activation floor on a lane's 4 channels
__device__ __forceinline__ float4 bn_act4(floatx4 acc, float4 alpha, float4 shift, float lo) {
  return make_float4(act(fmaf(acc[0], alpha.x, shift.x), lo), act(fmaf(acc[1], alpha.y, shift.y), lo),
                     act(fmaf(acc[2], alpha.z, shift.z), lo), act(fmaf(acc[3], alpha.w, shift.w), lo));
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// The LDS format of every 16-channel tile and weight block: float offset of channel quad q (4 floats,
// one ds_read_b128) of voxel / weight row `vox`. Voxel stride 16 floats and the quad swizzle are chosen
// so the 4 lane groups of every ds_read_b128 are bank-conflict free (exhaustive search over the gfx950
// b128 lane grouping); stride-2 reads included (conv3's instance). Two places spell the same
// layout out, for the reason given there: conv3d_lds_kernel and conv11's 8-row weight staging.
__device__ __forceinline__ int swz16(int vox, int q) { return vox * 16 + 4 * (q ^ ((vox >> 1) & 3)); }
template <typename T>  // the quad's address in the tile / weight block at `base`
__device__ __forceinline__ T* swz16(T* base, int vox, int q) {
  return base + vox * 16 + 4 * (q ^ ((vox >> 1) & 3));
}

// Weights [27 taps][COUT][CIN] -> LDS [27][16][16] for output rows row0 .. row0 + 15 and input channels
// ch0 .. ch0 + 15, the rows quad-swizzled like the tile's voxels so the A-fragment ds_read_b128 is
// bank-conflict free. 256 threads.
template <int COUT, int CIN>
__device__ __forceinline__ void stage_weights16(float* wts, const float* __restrict__ wpk, int row0, int ch0) {
  for (int idx = threadIdx.x; idx < 27 * 16 * 4; idx += 256) {
    const int q = idx & 3, row = (idx >> 2) & 15, tap = idx >> 6;
    const float4 v = *reinterpret_cast<const float4*>(wpk + ((size_t)tap * COUT + row0 + row) * CIN + ch0 + 4 * q);
    *reinterpret_cast<float4*>(swz16(wts + tap * 256, row, q)) = v;
  }
}

// Tile t of a volume cut into nds x nhs x nws tiles of TD x TH x 16 voxels per sample, w fastest
struct TileCoord {
  int n, d0, h0, w0;
};
__device__ __forceinline__ TileCoord tile_coord(int t, int nws, int nhs, int nds, int TH, int TD) {
  TileCoord c;
  c.w0 = (t % nws) * 16;
  t /= nws;
  c.h0 = (t % nhs) * TH;
  t /= nhs;
  c.d0 = (t % nds) * TD;
  c.n = t / nds;
  return c;
}

// A persistent workgroup's share of the ntiles tiles: first(), first() + step, ... below end.
// XCD-contiguous ranges (an XCD's workgroups share one L2: neighbouring tiles share their halo voxels):
// workgroup b runs on XCD b % 8 (round-robin dispatch), so XCD x's workgroups deal out tiles
// [ntiles x / 8, ntiles (x + 1) / 8) among themselves.
struct TileRange {
  int lo, k, end, step;  // the XCD's first tile, the workgroup's place among the XCD's, the XCD's end, its workgroups
  __device__ __forceinline__ explicit TileRange(int ntiles) {
    const int nxcd = gridDim.x >= 8 ? 8 : 1, per_xcd = gridDim.x / nxcd;
    const int xcd = blockIdx.x % nxcd, kx = blockIdx.x / nxcd;
    const int t_lo = (int)((long)ntiles * xcd / nxcd), t_hi = (int)((long)ntiles * (xcd + 1) / nxcd);
    lo = t_lo, k = kx, end = t_hi, step = per_xcd;
  }
  __device__ __forceinline__ bool idle() const { return k >= step; }  // grid not a multiple of 8: the remainder idles
  __device__ __forceinline__ int first() const { return lo + k; }
};

// ConvTranspose3d k3 s2 p1 op1, one dimension: output o = 2i - 1 + k, so an even output (parity 0) has the
// one tap (k = 1, i = o/2) and an odd one (parity 1) two: t = 0 -> (k = 0, i = o/2 + 1), t = 1 -> (k = 2, i = o/2).
struct ParityTap {
  int k, off;  // kernel index, input offset from o/2
};
constexpr ParityTap parity_tap(int p, int t) { return ParityTap{p ? (t ? 2 : 0) : 1, (p && !t) ? 1 : 0}; }
// A parity class cls = 4 pd + 2 ph + pw (16 outputs with one parity per dimension) has (1 + pd)(1 + ph)(1 + pw) taps
struct DeconvTap {
  int cls, tap, off;  // parity class, weight tap, input voxel offset (bit 2: depth, 1: row, 0: column)
};
constexpr int deconv_class_taps(int cls) { return (1 + (cls >> 2)) * (1 + ((cls >> 1) & 1)) * (1 + (cls & 1)); }
// tap i of class cls, in (td, th, tw) order: the K order of every transposed kernel
constexpr DeconvTap deconv_class_tap(int cls, int i) {
  const int pd = cls >> 2, ph = (cls >> 1) & 1, pw = cls & 1;
  const ParityTap d = parity_tap(pd, i / ((1 + ph) * (1 + pw))), h = parity_tap(ph, i / (1 + pw) % (1 + ph)),
                  w = parity_tap(pw, i % (1 + pw));
  return DeconvTap{cls, d.k * 9 + h.k * 3 + w.k, d.off * 4 + h.off * 2 + w.off};
}
constexpr bool deconv_taps_cover() {  // 27 distinct taps over the 8 classes, 1, 2, 2, 4, 2, 4, 4, 8 per class
  constexpr int want[8] = {1, 2, 2, 4, 2, 4, 4, 8};
  bool seen[27] = {};
  int n = 0;
  for (int cls = 0; cls < 8; ++cls) {
    if (deconv_class_taps(cls) != want[cls]) return false;
    for (int i = 0; i < deconv_class_taps(cls); ++i, ++n) {
      const int tap = deconv_class_tap(cls, i).tap;
      if (tap < 0 || tap >= 27 || seen[tap]) return false;
      seen[tap] = true;
    }
  }
  return n == 27;
}
static_assert(deconv_taps_cover(), "the parity rule enumerates the 27 taps once");

// ---------------------------------------------------------------- conv3d k3 p1, stride S
// Workgroup tile: 16 output voxels along w x TH rows x TD depth slices, MBB blocks of 16
// output channels. Per 16-channel chunk the input tile (+halo) is staged once into LDS
// (swz16's layout: the 16 lanes of a row hit distinct banks), then each wave runs
// its NBW = TD*TH/4 rows through the 27 taps: A (weights) from global/L2, requested two taps
// ahead, B from LDS. The next chunk's tile is fetched into registers during the current
// chunk's MFMAs.
// TAPOUT: every channel chunk's tile is staged at once and the K walk runs taps outer, channel chunks
// inner -- K order (tap, chunk, lane channel), the order the oracle-parity tests pin; the default walks
// chunks outer (one chunk's tile in LDS at a time), which re-associates the K sum when CIN > 16.
// TAPOUT needs TD = 1 (the kd slices in the depth padding are skipped per workgroup, exact zeros).
constexpr int kLdsWavesPerEu = 3;
template <int CIN, int COUT, int S, int TD, int TH, int MBB, int WS = 1, bool KDSKIP = false, bool TAPOUT = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kLdsWavesPerEu, kLdsWavesPerEu))) void conv3d_lds_kernel(const float* __restrict__ x, const float* __restrict__ wpk,
                                                         const float* __restrict__ alpha,
                                                         const float* __restrict__ shift, float* __restrict__ y,
                                                         Geo g) {
  constexpr int CK = 16, PL = 4;  // channels per chunk, per lane (one float4, 4 MFMAs)
  constexpr int MB = COUT / 16;
  constexpr int MG = MB / MBB;
  static_assert(CIN % 16 == 0 && COUT % 16 == 0, "16-channel input chunks, 16-channel output blocks");
  // WS: the 4 waves are WS block groups x 4/WS row groups; a wave runs NBW rows x MBW blocks (WS = 1:
  // every wave all MBB blocks of TD*TH/4 rows -- the 4 waves then request identical weight fragments)
  static_assert(WS == 1 || WS == 2 || WS == 4, "WS");
  static_assert(MBB % WS == 0 && (TD * TH * WS) % 4 == 0, "wave split");
  constexpr int NBW = TD * TH * WS / 4, MBW = MBB / WS;
  constexpr int LW = 15 * S + 3, LH = (TH - 1) * S + 3, LD = (TD - 1) * S + 3;
  // This kernel spells out swz16's layout (commit_from, bload_at), its tile decode and the weight loads' dead
  // `co < COUT` select as before: through the helpers, or without the select, every instance compiled to
  // another instruction stream, and conv4's measured 0.3 us slower (profiles/costreg_scaffold_resources.md).
  constexpr int VST = 16;  // (stride 2 included: conv3's instance)
  constexpr int NVOX = LD * LH * LW;
  static_assert(MB % MBB == 0, "tile");
  static_assert(!TAPOUT || (TD == 1 && !KDSKIP), "TAPOUT: one output slice per workgroup, its own kd skip");
  __shared__ __attribute__((aligned(16))) float tile[(TAPOUT ? CIN / CK : 1) * NVOX * VST];

  const int nws = (g.Wo + 15) / 16, nhs = (g.Ho + TH - 1) / TH, nds = (g.Do + TD - 1) / TD;
  int t = xcd_remap(blockIdx.x, gridDim.x);  // contiguous tiles per XCD: halos share an L2
  const int mg = t % MG;
  t /= MG;
  const int ws = t % nws;
  t /= nws;
  const int hs = t % nhs;
  t /= nhs;
  const int ds = t % nds;
  const int n = t / nds;
  const int ow0 = ws * 16, oh0 = hs * TH, od0 = ds * TD;
  const int iw0 = ow0 * S - 1, ih0 = oh0 * S - 1, id0 = od0 * S - 1;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int col = lane & 15, kgrp = lane >> 4;
  const int rg = __builtin_amdgcn_readfirstlane(wv / WS), bg = __builtin_amdgcn_readfirstlane(wv % WS);
  const int mb0 = mg * MBB + bg * MBW;  // the wave's first 16-channel output block
  const size_t in_n = (size_t)n * g.Di * g.Hi * g.Wi;

  floatx4 acc[NBW][MBW];
#pragma unroll
  for (int r = 0; r < NBW; ++r)
#pragma unroll
    for (int m = 0; m < MBW; ++m) acc[r][m] = floatx4{0.f, 0.f, 0.f, 0.f};

  // channel chunk ch's tile: global -> registers (issued one chunk ahead) -> LDS
  constexpr int NCH = CIN / CK, NLD = (NVOX * PL + 255) / 256;
  const Buf xb(x + in_n * CIN, (uint32_t)g.Di * g.Hi * g.Wi * CIN * 4);  // this sample (host: < 2 GB)
  const Buf wb(wpk, 27u * COUT * CIN * 4);
  float4 pf[NLD];
  auto fetch_to = [&](int ch, float4(&dst)[NLD]) {
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int idx = threadIdx.x + 256 * k;
      const int vox = idx / PL, q = idx - vox * PL;
      const int lw = vox % LW, rest = vox / LW, lh = rest % LH, ld = rest / LH;
      const int iw = iw0 + lw, ih = ih0 + lh, id = id0 + ld;
      // branch-free: padding lanes load x[0..3] and select zero, so the loads stay in one basic
      // block and the compiler's vmcnt waits count them exactly (a branch per load made it wait
      // vmcnt(0) every third tap, exposing the L2 latency of the two-tap-ahead weight loads)
      const bool ok = idx < NVOX * PL && iw >= 0 && iw < g.Wi && ih >= 0 && ih < g.Hi && id >= 0 && id < g.Di;
      dst[k] = xb.ld4(ok ? (((id * g.Hi + ih) * g.Wi + iw) * CIN + 4 * q) * 4 : Buf::kOOB, ch * CK * 4);
    }
  };
  auto fetch = [&](int ch) { fetch_to(ch, pf); };
  auto commit_from = [&](const float4(&src)[NLD], float* base) {
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int idx = threadIdx.x + 256 * k;
      const int vox = idx / PL, q = idx - vox * PL;
      const int qs = q ^ ((vox >> 1) & 3);
      if (idx < NVOX * PL) *reinterpret_cast<float4*>(base + vox * VST + 4 * qs) = src[k];
    }
  };
  auto commit = [&]() { commit_from(pf, tile); };
  // KDSKIP (launched only for output depth <= 2, where every wave has one): the kd slices whose
  // input plane lies wholly in the depth padding of the wave's output slice are not run (their
  // products are exact zeros). The taps then run as a loop over the kept slices (9 unrolled taps
  // each); the full-depth instance keeps the straight 27-tap schedule.
  static_assert(!KDSKIP || TH % NBW == 0, "KDSKIP needs one output slice per wave");
  int kd_lo = 0, kd_hi = 2;
  if constexpr (KDSKIP) {
    const int od = od0 + (rg * NBW) / TH;
    const int id_base = od * S - 1;  // input slice of kd = 0
    kd_lo = id_base < 0 ? -id_base : 0;
    kd_hi = g.Di - 1 - id_base < 2 ? g.Di - 1 - id_base : 2;
    if (od >= g.Do) kd_hi = -1;  // rows past the volume: nothing to compute
  }
  // A fragments (chunk ch, tap) from global/L2, requested two taps ahead of their MFMAs; the
  // chunk's last two taps request the next chunk's first two
  auto wload = [&](int ch, int tap, Vec4(&a)[MBW]) {
#pragma unroll
    for (int m = 0; m < MBW; ++m) {
      const int co = (mb0 + m) * 16 + col;  // channels >= COUT read zeros
      buf_load(a[m], wb, (co < COUT ? co * CIN + kgrp * PL : Buf::kOOB / 4) * 4, (tap * COUT * CIN + ch * CK) * 4);
    }
  };
  Vec4 aw[3][MBW];
  // B fragments of one tap from the LDS tile
  auto bload_at = [&](const float* base, int kd, int kh, int kw, Vec4(&b)[NBW]) {
#pragma unroll
    for (int r = 0; r < NBW; ++r) {
      const int rr = rg * NBW + r;
      const int odl = rr / TH, ohl = rr - odl * TH;
      const int lvox = ((odl * S + kd) * LH + ohl * S + kh) * LW + col * S + kw;
      const int qs = kgrp ^ ((lvox >> 1) & 3);
      b[r].load(base + lvox * VST + qs * PL);
    }
  };
  auto bload = [&](int kd, int kh, int kw, Vec4(&b)[NBW]) { bload_at(tile, kd, kh, kw, b); };
  // one tap: NBW x MBB x PL MFMAs on fragments already in registers
  auto tap_mfma = [&](const Vec4* a, const Vec4* b) {
#pragma unroll
    for (int j = 0; j < PL; ++j)
#pragma unroll
      for (int r = 0; r < NBW; ++r)
#pragma unroll
        for (int m = 0; m < MBW; ++m)
          acc[r][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m].v[j], b[r].v[j], acc[r][m], 0, 0, 0);
    // one-MFMA schedule groups keep the accumulators' chains interleaved as written (the scheduler
    // otherwise issued each accumulator's PL dependent MFMAs back to back: 40-cycle dependent issue
    // against 32 for an independent one)
#pragma unroll
    for (int i = 0; i < PL * NBW * MBW; ++i) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_barrier(0);  // keep the lookahead schedule (and the VGPR budget)
  };
  // B of tap t + 1 is read from LDS before tap t's MFMAs (read right before its own MFMAs its
  // latency sat between every tap's MFMA groups)
  Vec4 bw[2][NBW];
  if constexpr (TAPOUT) {
    // all chunks staged (every chunk's loads in flight before the first commit), then per kept kd slice
    // 9 taps x NCH chunks as one step sequence with the same two-step weight / one-step B lookahead
    float4 pfc[NCH][NLD];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) fetch_to(ch, pfc[ch]);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) commit_from(pfc[ch], tile + ch * NVOX * VST);
    __syncthreads();
    const int id_base = od0 * S - 1;  // input slice of kd = 0 (workgroup-uniform: TD = 1)
    const int klo = id_base < 0 ? -id_base : 0;
    const int khi = od0 >= g.Do ? -1 : (g.Di - 1 - id_base < 2 ? g.Di - 1 - id_base : 2);
    constexpr int NS = 9 * NCH;  // steps per slice; a multiple of 3, so the weight ring lines up across slices
    auto wstep = [&](int kd, int s, Vec4(&a)[MBW]) { wload(s % NCH, kd * 9 + s / NCH, a); };
    auto bstep = [&](int kd, int s, Vec4(&b)[NBW]) {
      const int t9 = s / NCH;
      bload_at(tile + (s % NCH) * NVOX * VST, kd, t9 / 3, t9 % 3, b);
    };
    if (klo <= khi) {
      wstep(klo, 0, aw[0]);
      wstep(klo, 1, aw[1]);
    }
#pragma unroll 1
    for (int kd = klo; kd <= khi; ++kd) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (s + 2 < NS)
          wstep(kd, s + 2, aw[(s + 2) % 3]);
        else if (kd < khi)  // uniform: the next slice's first two steps
          wstep(kd + 1, s + 2 - NS, aw[(s + 2) % 3]);
        if (s == 0) bstep(kd, 0, bw[0]);
        if (s + 1 < NS) bstep(kd, s + 1, bw[(s + 1) & 1]);
        tap_mfma(aw[s % 3], bw[s & 1]);
      }
    }
  } else {
  // The next chunk's tile is requested right after the chunk's last weight load (3 taps before
  // its end), not ahead of the chunk's first: vmcnt retires loads in issue order, so any weight
  // load issued behind the tile loads waits for them (fetching at the chunk's start measured the
  // same, r17a).
  fetch(0);
  commit();
  __syncthreads();
  if constexpr (KDSKIP) {
    if (kd_lo <= kd_hi) {
      wload(0, kd_lo * 9, aw[0]);
      wload(0, kd_lo * 9 + 1, aw[1]);
    }
  } else {
    wload(0, 0, aw[0]);
    wload(0, 1, aw[1]);
  }
  // one channel chunk; MORE (compile time, so no branch splits the load stream and the vmcnt
  // waits stay exact): the next chunk's first weights and tile are requested at its end
  auto chunk = [&](int ch, auto more_c) {
    constexpr bool MORE = decltype(more_c)::value;
    if (MORE && KDSKIP && kd_lo > kd_hi) fetch(ch + 1);  // a wave with no slices still stages its share
    if constexpr (KDSKIP) {
#pragma unroll 1
      for (int kd = kd_lo; kd <= kd_hi; ++kd)
#pragma unroll
        for (int k9 = 0; k9 < 9; ++k9) {
          if (k9 + 2 < 9) {
            wload(ch, kd * 9 + k9 + 2, aw[(k9 + 2) % 3]);
          } else {  // uniform branch: the next slice's first taps, or the next chunk's
            if (kd < kd_hi)
              wload(ch, kd * 9 + k9 + 2, aw[(k9 + 2) % 3]);
            else if (MORE)
              wload(ch + 1, kd_lo * 9 + k9 - 7, aw[(k9 + 2) % 3]);
          }
          if (MORE && k9 == 6 && kd == kd_hi) fetch(ch + 1);
          // B prefetch within the slice (9 taps: the parity would flip across the rolled kd loop)
          if (k9 == 0) bload(kd, k9 / 3, k9 % 3, bw[k9 & 1]);
          if (k9 + 1 < 9) bload(kd, (k9 + 1) / 3, (k9 + 1) % 3, bw[(k9 + 1) & 1]);
          tap_mfma(aw[k9 % 3], bw[k9 & 1]);
        }
    } else {
#pragma unroll
      for (int tap = 0; tap < 27; ++tap) {
        if (tap + 2 < 27)
          wload(ch, tap + 2, aw[(tap + 2) % 3]);
        else if (MORE)
          wload(ch + 1, tap - 25, aw[(tap + 2) % 3]);
        if (MORE && tap == 24) fetch(ch + 1);
        if (tap == 0) bload(tap / 9, (tap / 3) % 3, tap % 3, bw[tap & 1]);
        if (tap + 1 < 27) bload((tap + 1) / 9, ((tap + 1) / 3) % 3, (tap + 1) % 3, bw[(tap + 1) & 1]);
        tap_mfma(aw[tap % 3], bw[tap & 1]);
      }
    }
    if (MORE) {
      __syncthreads();
      commit();
      __syncthreads();
    }
  };
#pragma unroll 1
  for (int ch = 0; ch + 1 < NCH; ++ch) chunk(ch, std::true_type{});
  chunk(NCH - 1, std::false_type{});
  }
  const int ow = ow0 + col;
  if (ow >= g.Wo) return;
  const size_t out_n = (size_t)n * g.Do * g.Ho * g.Wo;
#pragma unroll
  for (int m = 0; m < MBW; ++m) {
    const int co = (mb0 + m) * 16 + kgrp * 4;
    const float4 al = *reinterpret_cast<const float4*>(alpha + co);
    const float4 sh = *reinterpret_cast<const float4*>(shift + co);
#pragma unroll
    for (int r = 0; r < NBW; ++r) {
      const int rr = rg * NBW + r;
      const int od = od0 + rr / TH, oh = oh0 + rr % TH;
      if (od >= g.Do || oh >= g.Ho) continue;
      *reinterpret_cast<float4*>(y + (out_n + ((size_t)od * g.Ho + oh) * g.Wo + ow) * COUT + co) =
          bn_act4(acc[r][m], al, sh, g.lo);
    }
  }
}

// ---------------------------------------------------------------- ConvTranspose3d k3 s2 p1 op1
// Workgroup tile in input-grid coordinates: 16 columns x THI rows x TDI slices (outputs
// 32 x 2THI x 2TDI), one block of 16 output channels. Each wave owns TDI*THI/4 input-grid rows and
// all 8 output parity classes of them (a class = one tap set of 1, 2, 4 or 8 taps, deconv_class_tap),
// so the waves carry equal work. Input tile (+1 halo) staged in LDS.
template <int CIN, int COUT, int TDI, int THI>
__global__ __launch_bounds__(256) void deconv3d_lds_kernel(const float* __restrict__ x,
                                                           const float* __restrict__ wpk,
                                                           const float* __restrict__ alpha,
                                                           const float* __restrict__ shift,
                                                           const float* __restrict__ skip, float* __restrict__ y,
                                                           Geo g) {
  constexpr int CK = 16, PL = 4;  // channels per chunk, per lane (one float4, 4 MFMAs)
  constexpr int MG = COUT / 16;
  constexpr int NBW = TDI * THI / 4;
  constexpr int LW = 17, LH = THI + 1, LD = TDI + 1;
  constexpr int NVOX = LD * LH * LW;
  static_assert((TDI * THI) % 4 == 0, "tile");
  static_assert(CIN % 16 == 0 && COUT % 16 == 0, "16-channel input chunks, 16-channel output blocks");
  // weights of the current channel chunk in LDS (stage_weights16; a per-tap global load right
  // before its MFMAs exposed a full memory latency per tap: MFMA busy 35 %)
  __shared__ __attribute__((aligned(16))) float tile[NVOX * 16];
  __shared__ __attribute__((aligned(16))) float wts[27 * 16 * 16];

  const int nws = (g.Wi + 15) / 16, nhs = (g.Hi + THI - 1) / THI, nds = (g.Di + TDI - 1) / TDI;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);  // contiguous tiles per XCD: halos share an L2
  const int mg = wg % MG;
  const TileCoord c = tile_coord(wg / MG, nws, nhs, nds, THI, TDI);
  const int n = c.n, mw0 = c.w0, mh0 = c.h0, md0 = c.d0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int col = lane & 15, kgrp = lane >> 4;
  const size_t in_n = (size_t)n * g.Di * g.Hi * g.Wi;

  floatx4 acc[NBW][8];
#pragma unroll
  for (int r = 0; r < NBW; ++r)
#pragma unroll
    for (int cls = 0; cls < 8; ++cls) acc[r][cls] = floatx4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int ch = 0; ch < CIN / CK; ++ch) {
    if (ch) __syncthreads();
    for (int idx = threadIdx.x; idx < NVOX * PL; idx += 256) {
      const int vox = idx / PL, q = idx - vox * PL;
      const int lw = vox % LW, rest = vox / LW, lh = rest % LH, ld = rest / LH;
      const int iw = mw0 + lw, ih = mh0 + lh, id = md0 + ld;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (iw < g.Wi && ih < g.Hi && id < g.Di)
        v = *reinterpret_cast<const float4*>(x + (in_n + ((size_t)id * g.Hi + ih) * g.Wi + iw) * CIN + ch * CK + 4 * q);
      *reinterpret_cast<float4*>(swz16(tile, vox, q)) = v;
    }
    stage_weights16<COUT, CIN>(wts, wpk, mg * 16, ch * CK);
    __syncthreads();
#pragma unroll
    for (int cls = 0; cls < 8; ++cls) {
#pragma unroll
      for (int i = 0; i < deconv_class_taps(cls); ++i) {
        const DeconvTap t = deconv_class_tap(cls, i);
        Vec4 a;
        a.load(swz16(wts + t.tap * 256, col, kgrp));
#pragma unroll
        for (int r = 0; r < NBW; ++r) {
          const int rr = wv * NBW + r;
          const int mdl = rr / THI, mhl = rr - mdl * THI;
          Vec4 b;
          const int lvox = ((mdl + (t.off >> 2)) * LH + mhl + ((t.off >> 1) & 1)) * LW + col + (t.off & 1);
          b.load(swz16(tile, lvox, kgrp));
#pragma unroll
          for (int j = 0; j < PL; ++j)
            acc[r][cls] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], acc[r][cls], 0, 0, 0);
        }
      }
    }
  }
  const size_t out_n = (size_t)n * g.Do * g.Ho * g.Wo;
  const int mw = mw0 + col;
  if (mw >= g.Wi) return;
  const int co = mg * 16 + kgrp * 4;
  const float4 al = *reinterpret_cast<const float4*>(alpha + co);
  const float4 sh = *reinterpret_cast<const float4*>(shift + co);
#pragma unroll
  for (int r = 0; r < NBW; ++r) {
    const int rr = wv * NBW + r;
    const int md = md0 + rr / THI, mh = mh0 + rr % THI;
    if (md >= g.Di || mh >= g.Hi) continue;
#pragma unroll
    for (int cls = 0; cls < 8; ++cls) {
      const int od = 2 * md + (cls >> 2), oh = 2 * mh + ((cls >> 1) & 1), ow = 2 * mw + (cls & 1);
      const size_t o = (out_n + ((size_t)od * g.Ho + oh) * g.Wo + ow) * COUT + co;
      const float4 s = skip ? *reinterpret_cast<const float4*>(skip + o) : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(y + o) = add4(s, bn_act4(acc[r][cls], al, sh, g.lo));
    }
  }
}

constexpr int kDChunk = 8;  // depth planes per thread in the full-resolution VALU convs

// ---------------------------------------------------------------- conv0: Cin=1 -> 8, VALU
// Same row-segment layout as prob_kernel below: a wave owns 62 output columns of one row, lane l
// column w0 + l - 1 (lanes 0 / 63 are the kw halo). Each input row is one coalesced dword per
// lane; kw neighbours come by DPP. The thread walks D with a 3-plane ring of its 3x3 windows;
// the next plane's raw rows are in flight while an output plane is computed.
// The 8 output channels are 4 packed pairs: one v_pk_fma per (tap, pair) with the weight pair
// {W[t][2cp], W[t][2cp+1]} (packing [27][Co]) and the tap value broadcast, the 4 chains
// interleaved (a dependent v_pk_fma issued back to back stalls a cycle). Every output still
// sees its taps in (kd, kh, kw) order. A lane stores its voxel's 8 channels (32 bytes): staging
// them through LDS for lane-contiguous stores measured slower here.
constexpr int kProbCols = 62;
typedef float float2_v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float lane_from_left(float v) {  // lane l <- lane l-1 (wave_shr:1)
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xF, 0xF, false));
}
__device__ __forceinline__ float lane_from_right(float v) {  // lane l <- lane l+1 (wave_shl:1)
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xF, 0xF, false));
}

__global__ __launch_bounds__(256) void conv0_kernel(const float* __restrict__ x, float* __restrict__ y, int D, int H,
                                                    int W, const float* __restrict__ wt,
                                                    const float* __restrict__ alpha,
                                                    const float* __restrict__ shift, float lo) {
  const int HW = H * W;
  const int nseg = (W + kProbCols - 1) / kProbCols, nrow = (H + 3) / 4, ndc = (D + kDChunk - 1) / kDChunk;
  int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int seg = lb % nseg;
  lb /= nseg;
  const int rowb = lb % nrow;
  lb /= nrow;
  const int dc = lb % ndc;
  const int n = lb / ndc;
  const int lane = threadIdx.x & 63;
  const int h = rowb * 4 + (threadIdx.x >> 6);
  if (h >= H) return;  // whole wave
  const int w = seg * kProbCols + lane - 1;
  const bool writes = lane >= 1 && lane <= kProbCols && w < W;
  const int d0 = dc * kDChunk, d1 = min(D, d0 + kDChunk);
  const __amdgpu_buffer_rsrc_t rx = raw_rsrc(x + (size_t)n * D * HW, (unsigned)(D * HW * 4));
  float* yp = y + ((size_t)n * D * HW + (size_t)h * W + w) * 8;
  const unsigned offw = (unsigned)w < (unsigned)W ? (unsigned)w * 4u : kOffOut;
  unsigned offh[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) offh[k] = (unsigned)(h - 1 + k) < (unsigned)H ? (unsigned)((h - 1 + k) * W) * 4u : kOffOut;
  auto load_raw = [&](int d, float (&o)[3]) {
    const unsigned offd = (unsigned)d < (unsigned)D ? (unsigned)d * (unsigned)HW * 4u : kOffOut;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const unsigned off = offd | offh[kh] | offw;  // any out-of-range term keeps the top bit
      o[kh] = buf_load_f32(rx, (offd + offh[kh] + offw) | (off & kOffOut));
    }
  };
  auto expand = [&](const float (&r)[3], float (&o)[3][3]) {
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      o[kh][0] = lane_from_left(r[kh]);
      o[kh][1] = r[kh];
      o[kh][2] = lane_from_right(r[kh]);
    }
  };
  float al[8], sh[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    al[c] = alpha[c];
    sh[c] = shift[c];
  }
  float win[3][3][3];
  // one output plane; `raw` holds plane d+1's rows and is refilled with plane d+2's
  auto step = [&](int d, float (&raw)[3]) {
    expand(raw, win[2]);
    load_raw(d + 2, raw);
    const float* wk = wt;
    float2_v a[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int t = 0; t < 27; ++t) {
      const float xv = win[t / 9][(t / 3) % 3][t % 3];
#pragma unroll
      for (int cp = 0; cp < 4; ++cp)
        a[cp] = __builtin_elementwise_fma(*reinterpret_cast<const float2_v*>(wk + t * 8 + 2 * cp), float2_v{xv, xv},
                                          a[cp]);
    }
    float o[8];
#pragma unroll
    for (int cp = 0; cp < 4; ++cp) {
      o[2 * cp] = act(fmaf(a[cp].x, al[2 * cp], sh[2 * cp]), lo);
      o[2 * cp + 1] = act(fmaf(a[cp].y, al[2 * cp + 1], sh[2 * cp + 1]), lo);
    }
    if (writes) {
      float4* q = reinterpret_cast<float4*>(yp + (size_t)d * HW * 8);
      q[0] = make_float4(o[0], o[1], o[2], o[3]);
      q[1] = make_float4(o[4], o[5], o[6], o[7]);
    }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        win[0][kh][k] = win[1][kh][k];
        win[1][kh][k] = win[2][kh][k];
      }
  };
  float ra[3];
  load_raw(d0 - 1, ra);
  expand(ra, win[0]);
  load_raw(d0, ra);
  expand(ra, win[1]);
  load_raw(d0 + 1, ra);
  for (int d = d0; d < d1; ++d) step(d, ra);
}

// ---------------------------------------------------------------- prob: 8 -> 1, VALU
// A wave owns NR consecutive rows of one segment of 62 output columns; lane l holds column
// w0 + l - 1 (lanes 0 and 63 are the kw halo and write nothing). Every input row is one coalesced
// 32-byte load per lane (the segment's 64 pixels are 2 KB contiguous); the kw = 0 / 2 neighbours come
// from lanes l -+ 1 by wave-wide DPP shifts instead of re-gathering them (the 3x re-read of the
// 1-pixel-per-thread form made this kernel address-unit bound). The thread walks kDChunk output
// planes (prob_walk_rows).

// The D walk both prob kernels run, for the NR output rows h .. h+NR-1 of a wave: input plane i
// (NR+2 rows x 3 taps x 8 channels) feeds outputs i+1 (kd=0), i (kd=1) and i-1 (kd=2), each output's
// FMA chain in (kd, kh, kw, c) order:
// c12 = {output i (kd=0 done, adds kd=1), output i-1 (kd=0,1 done, adds kd=2)}, one packed FMA per
// (tap, channel) with the weight pair {W[kd=1], W[kd=2]} (an aligned SGPR pair, see the host
// packing in include/transmvs.h) and x broadcast; acc_next (output i+1, kd=0) is scalar.
// Plane i's rows h-1 .. h+NR are loaded once (NR+2 row loads per plane instead of 3 NR: the row
// re-reads had the kernels address-unit bound) and each row feeds the outputs it borders, so the
// logits do not depend on NR.
// Planes d0-1 .. d0+8 (kDChunk + 2), double-buffered: plane i+1's rows are in flight while plane i
// is consumed (with one row of lookahead a wave had a single load outstanding and the kernels ran at
// 2.3-2.5 TB/s). emit(r, d, logit) for d = d0 .. d0+7 (the caller bounds d by D).
template <int NR, typename Emit>
__device__ __forceinline__ void prob_walk_rows(__amdgpu_buffer_rsrc_t rx, int w, int h, int D, int H, int W, int d0,
                                               const float* __restrict__ wt, Emit emit) {
  constexpr int NL = NR + 2;
  // d0 is the wave's depth chunk: wave-uniform, but derived from threadIdx.x, so without this the plane
  // loop is a divergent (exec-mask) loop whose latch waits vmcnt(0) for the prefetched plane
  d0 = __builtin_amdgcn_readfirstlane(d0);
  const unsigned offw = (unsigned)w < (unsigned)W ? (unsigned)w * 32u : kOffOut;
  auto load_plane = [&](int i, float4 (&o)[NL][2]) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int ih = h - 1 + j;
      const unsigned offr = ((unsigned)i < (unsigned)D && (unsigned)ih < (unsigned)H)
                                ? ((unsigned)i * (unsigned)H + (unsigned)ih) * (unsigned)W * 32u
                                : kOffOut;
      const unsigned off = (offr + offw) | ((offr | offw) & kOffOut);
      const floatx4 u = buf_load_f32x4(rx, off);
      const floatx4 v = buf_load_f32x4(rx, off + 16u);
      o[j][0] = make_float4(u[0], u[1], u[2], u[3]);
      o[j][1] = make_float4(v[0], v[1], v[2], v[3]);
    }
  };
  float2_v c12[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) c12[r] = float2_v{0.f, 0.f};
  auto plane = [&](int i, const float4 (&p)[NL][2]) {
    float acc_next[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc_next[r] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      // the row's 72 weights through an opaque (uniform) offset: loaded where the row is consumed
      // instead of all 216 hoisted out of the plane loop into SGPRs (spills)
      int wo = kh * 72;
      asm volatile("" : "+s"(wo));
      const float* wk = wt + __builtin_amdgcn_readfirstlane(wo);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int j = r + kh;  // input row h-1+j feeds output row h+r through weight row kh
        const float xc[8] = {p[j][0].x, p[j][0].y, p[j][0].z, p[j][0].w, p[j][1].x, p[j][1].y, p[j][1].z, p[j][1].w};
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const float xv = kw == 0 ? lane_from_left(xc[c]) : kw == 1 ? xc[c] : lane_from_right(xc[c]);
            const float2_v wp = *reinterpret_cast<const float2_v*>(wk + 2 * (kw * 8 + c));
            acc_next[r] = fmaf(wk[48 + kw * 8 + c], xv, acc_next[r]);
            c12[r] = __builtin_elementwise_fma(wp, float2_v{xv, xv}, c12[r]);
          }
        }
        // both chains complete per row (no FMA sunk past the row: its shifted taps die here)
        asm volatile("" : "+v"(acc_next[r]), "+v"(c12[r]));
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (i - 1 >= d0) emit(r, i - 1, c12[r].y);  // output i-1 complete
      c12[r] = float2_v{acc_next[r], c12[r].x};
    }
  };
  float4 pa[NL][2], pb[NL][2];
  load_plane(d0 - 1, pa);
  // unrolled: no loop-carried plane buffers, whose register copies at the latch waited vmcnt(0)
#pragma unroll
  for (int j = 0; j < kDChunk + 2; j += 2) {
    const int i = d0 - 1 + j;  // planes i (in pa) and i + 1 (in pb)
    load_plane(i + 1, pb);
    plane(i, pa);
    load_plane(i + 2, pa);  // (past the last plane: rows the next chunk reads anyway)
    plane(i + 1, pb);
  }
}

// raw logits, NR output rows per wave (4 waves: 4 NR rows per workgroup), one depth chunk per workgroup
template <int NR>
__global__ __launch_bounds__(256) void prob_kernel(const float* __restrict__ x, float* __restrict__ y, int D, int H,
                                                   int W, const float* __restrict__ wt) {
  const int HW = H * W;
  const int nseg = (W + kProbCols - 1) / kProbCols, nrow = (H + 4 * NR - 1) / (4 * NR), ndc = (D + kDChunk - 1) / kDChunk;
  int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int seg = lb % nseg;
  lb /= nseg;
  const int rowb = lb % nrow;
  lb /= nrow;
  const int dc = lb % ndc;
  const int n = lb / ndc;
  const int lane = threadIdx.x & 63;
  const int h = (rowb * 4 + (threadIdx.x >> 6)) * NR;
  if (h >= H) return;  // whole wave
  const int w = seg * kProbCols + lane - 1;
  const bool writes = lane >= 1 && lane <= kProbCols && w < W;
  const int d0 = dc * kDChunk, d1 = min(D, d0 + kDChunk);
  const __amdgpu_buffer_rsrc_t rx = raw_rsrc(x + (size_t)n * D * HW * 8, (unsigned)(D * HW * 32));
  float* yn = y + (size_t)n * D * HW + (size_t)h * W + w;
  prob_walk_rows<NR>(rx, w, h, D, H, W, d0, wt, [&](int r, int d, float v) {
    if (d < d1 && writes && h + r < H) yn[(size_t)d * HW + (size_t)r * W] = v;
  });
}

// ---------------------------------------------------------------- prob + softmax / WTA, fused
// prob_kernel's row-segment D walk with the D / 8 depth chunks of NR rows of one segment as the waves
// of one workgroup (wave k walks planes 8k-1 .. 8k+8 of all NR rows, exactly prob_kernel's chunk k);
// each wave parks its 8 logits per column in LDS ([NR][D][64]) instead of HBM, and after one barrier
// the first waves run softmax_first_max (common.h, the code softmax_wta_kernel runs) per column of one
// row each (wave 0 of all rows when D = 8) and gather the winning hypothesis
// (models/TransMVSNet.py:97-103,217-221). Same FMA chains as prob_kernel, so prob / depth / conf equal
// prob_kernel + softmax_wta_kernel bit for bit, without the logits' 8·D bytes per pixel of HBM traffic
// and one launch.
template <int D, int NR>
__global__ __launch_bounds__(64 * (D / kDChunk)) void prob_wta_rows_kernel(
    const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ hyp, int H, int W, float lo,
    float hi, float* __restrict__ prob, float* __restrict__ depth, float* __restrict__ depth_raw,
    float* __restrict__ conf) {
  constexpr int NW = D / kDChunk;
  __shared__ float lg[NR][D * 64];
  const int HW = H * W;
  const int nseg = (W + kProbCols - 1) / kProbCols, nrow = (H + NR - 1) / NR;
  int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int seg = lb % nseg;
  lb /= nseg;
  const int h0 = (lb % nrow) * NR;
  const int n = lb / nrow;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int d0 = wv * kDChunk;
  const int w = seg * kProbCols + lane - 1;
  const bool writes = lane >= 1 && lane <= kProbCols && w < W;
  const __amdgpu_buffer_rsrc_t rx = raw_rsrc(x + (size_t)n * D * HW * 8, (unsigned)(D * HW * 32));
  prob_walk_rows<NR>(rx, w, h0, D, H, W, d0, wt, [&](int r, int d, float v) { lg[r][d * 64 + lane] = v; });
  __syncthreads();
  if (!writes) return;
  for (int r = wv; r < NR; r += NW) {
    const int h = h0 + r;
    if (h >= H) break;
    float xl[D];
#pragma unroll
    for (int d = 0; d < D; ++d) xl[d] = lg[r][d * 64 + lane];
    const size_t base = (size_t)n * D * HW + (size_t)h * W + w;
    float best;
    const int bi = softmax_first_max<D>(xl, [&](int d, float pr) { prob[base + (size_t)d * HW] = pr; }, best);
    const size_t o = (size_t)n * HW + (size_t)h * W + w;
    const float dr = hyp[base + (size_t)bi * HW];
    depth_raw[o] = dr;
    depth[o] = fminf(fmaxf(dr, lo), hi);
    conf[o] = best;
  }
}

// ---------------------------------------------------------------- conv 16 -> 16, stride 1 (conv2)
// Persistent form of conv3d_lds_kernel for the one stride-1 layer whose weights fit in LDS next
// to a tile (27 x 16 x 16 fp32 = 27 KB): a workgroup stages them once, then walks its share of
// 2x4x16-voxel output tiles; the next tile's input is fetched into registers while the
// current tile's 27 taps run on the MFMAs, and committed to LDS between two barriers.
// Same fragment layouts, tap order and epilogue as conv3d_lds_kernel.
template <int TD, int TH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void conv3d_c16_kernel(const float* __restrict__ x, const float* __restrict__ wpk,
                                                         const float* __restrict__ alpha,
                                                         const float* __restrict__ shift, float* __restrict__ y, Geo g,
                                                         int ntiles) {
  constexpr int C = 16, PL = 4, NWV = 4, NBW = TD * TH / NWV, NTH = NWV * 64;  // 4 waves per workgroup
  static_assert(TD * TH % NWV == 0, "rows split evenly over the waves");
  constexpr int LW = 18, LH = TH + 2, LD = TD + 2;
  constexpr int NVOX = LD * LH * LW;
  constexpr int NLD = (NVOX * 4 + NTH - 1) / NTH;
  __shared__ __attribute__((aligned(16))) float tile[NVOX * 16];
  __shared__ __attribute__((aligned(16))) float wts[27 * 16 * 16];
  const int nws = (g.Wo + 15) / 16, nhs = (g.Ho + TH - 1) / TH, nds = (g.Do + TD - 1) / TD;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int col = lane & 15, kgrp = lane >> 4;
  const TileRange tr(ntiles);
  if (tr.idle()) return;
  auto coord = [&](int t) { return tile_coord(t, nws, nhs, nds, TH, TD); };
  float4 pf[NLD];
  auto fetch = [&](int t) {
    const TileCoord c = coord(t);
    const size_t in_n = (size_t)c.n * g.Di * g.Hi * g.Wi;
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int idx = threadIdx.x + NTH * k;
      const int vox = idx >> 2, q = idx & 3;
      const int lw = vox % LW, rest = vox / LW, lh = rest % LH, ld = rest / LH;
      const int iw = c.w0 - 1 + lw, ih = c.h0 - 1 + lh, id = c.d0 - 1 + ld;
      pf[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (vox < NVOX && (unsigned)iw < (unsigned)g.Wi && (unsigned)ih < (unsigned)g.Hi && (unsigned)id < (unsigned)g.Di)
        pf[k] = *reinterpret_cast<const float4*>(x + (in_n + ((size_t)id * g.Hi + ih) * g.Wi + iw) * C + 4 * q);
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int idx = threadIdx.x + NTH * k;
      const int vox = idx >> 2, q = idx & 3;
      if (vox < NVOX) *reinterpret_cast<float4*>(swz16(tile, vox, q)) = pf[k];
    }
  };
  stage_weights16<C, C>(wts, wpk, 0, 0);
  const float4 al = *reinterpret_cast<const float4*>(alpha + kgrp * 4);
  const float4 sh = *reinterpret_cast<const float4*>(shift + kgrp * 4);
  int t = tr.first();
  if (t < tr.end) {
    fetch(t);
    commit();
  }
  __syncthreads();
  for (; t < tr.end; t += tr.step) {
    const TileCoord c = coord(t);
    const int tn = t + tr.step;
    if (tn < tr.end) fetch(tn);
    floatx4 acc[NBW];
#pragma unroll
    for (int r = 0; r < NBW; ++r) acc[r] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) {
      const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
      Vec4 a;
      a.load(swz16(wts + tap * 256, col, kgrp));
      Vec4 b[NBW];
#pragma unroll
      for (int r = 0; r < NBW; ++r) {
        const int rr = wv * NBW + r;
        const int odl = rr / TH, ohl = rr - odl * TH;
        const int lvox = ((odl + kd) * LH + ohl + kh) * LW + col + kw;
        b[r].load(swz16(tile, lvox, kgrp));
      }
#pragma unroll
      for (int j = 0; j < PL; ++j)
#pragma unroll
        for (int r = 0; r < NBW; ++r)
          acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b[r].v[j], acc[r], 0, 0, 0);
      if (tap % (NBW > 2 ? 3 : 9) == (NBW > 2 ? 2 : 8)) __builtin_amdgcn_sched_barrier(0);  // bound the fragments in flight
    }
    const int ow = c.w0 + col;
    const size_t out_n = (size_t)c.n * g.Do * g.Ho * g.Wo;
#pragma unroll
    for (int r = 0; r < NBW; ++r) {
      const int rr = wv * NBW + r;
      const int od = c.d0 + rr / TH, oh = c.h0 + rr % TH;
      if (ow >= g.Wo || od >= g.Do || oh >= g.Ho) continue;
      *reinterpret_cast<float4*>(y + (out_n + ((size_t)od * g.Ho + oh) * g.Wo + ow) * C + kgrp * 4) =
          bn_act4(acc[r], al, sh, g.lo);
    }
    __syncthreads();  // every wave is done with the tile
    if (tn < tr.end) commit();
    __syncthreads();
  }
}

// residency of a persistent kernel (256 threads): resident workgroups per CU x CUs (queried once per kernel)
template <typename K>
static int persistent_grid(K kernel, long ntiles) {
  struct Entry {
    const void* fn;
    int dev, cap;
  };
  static Entry cache[16];
  static int used = 0;
  int dev = 0;
  hipGetDevice(&dev);
  for (int i = 0; i < used; ++i)
    if (cache[i].fn == (const void*)kernel && cache[i].dev == dev) return (int)std::min<long>(ntiles, cache[i].cap);
  int cus = 0, per = 0;
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, 256, 0);
  const int cap = std::max(8, cus * std::max(per, 1));
  if (used < 16) cache[used++] = Entry{(const void*)kernel, dev, cap};
  return (int)std::min<long>(ntiles, cap);
}

// tiles of TD x TH x 16 voxels over B volumes of d x h x w (the output grid of a conv, the input grid of a deconv)
static long tile_count(int B, int d, int h, int w, int TD, int TH) {
  return (long)B * ((d + TD - 1) / TD) * ((h + TH - 1) / TH) * ((w + 15) / 16);
}

// a persistent kernel (..., int ntiles) on min(ntiles, its residency) workgroups; max_wgs > 0 bounds the grid further
template <typename K, typename... Args>
static int launch_persistent(K kernel, long ntiles, int max_wgs, hipStream_t st, Args... args) {
  long grid = persistent_grid(kernel, ntiles);
  if (max_wgs > 0) grid = std::min<long>(grid, max_wgs);
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, st, args..., (int)ntiles);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

template <int TD, int TH>
static int launch_conv_c16(const float* x, const float* w, const float* al, const float* sh, float* y, int B,
                           const Geo& g, hipStream_t st) {
  return launch_persistent(conv3d_c16_kernel<TD, TH>, tile_count(B, g.Do, g.Ho, g.Wo, TD, TH), 0, st, x, w, al, sh, y, g);
}

// ---------------------------------------------------------------- conv1: 8 -> 16, stride 2, persistent
// A persistent workgroup keeps the 13.8 KB of
// weights in LDS and walks 2x4x16-output tiles; a tile's 5x9x33-voxel input footprint (8
// channels, 32 B per voxel) is staged with W split by parity -- [d][h][w&1][w>>1][8] -- so the
// stride-2 taps of 16 consecutive outputs read 16 consecutive voxels (kw 0/1/2 -> parity
// 0/1/0, index col + kw/2): conflict-free ds_read_b128 with no address-unit waste. The next
// tile is fetched into registers during the current tile's MFMAs.
// Tap pairs: with 8 input channels a per-tap B fragment would be 2 channels per lane. The 27
// taps are taken in pairs (a, b): lanes kgrp 0/1 read channel quads 0/1 of tap a, lanes 2/3
// of tap b, one 16-byte read each; MFMA j contracts k = (tap, quad) over channel j of each
// quad, and the A fragments are laid out to match (the 14th pair is half empty).
template <int TD, int TH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1))) void conv3d_s2c8_tile_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ wpk,
                                                               const float* __restrict__ alpha,
                                                               const float* __restrict__ shift, float* __restrict__ y,
                                                               Geo g, int ntiles) {
  constexpr int CIN = 8, COUT = 16, NWV = 4, NBW = TD * TH / NWV, NTH = NWV * 64;  // 4 waves per workgroup
  static_assert(TD * TH % NWV == 0, "rows split evenly over the waves");
  // (SW = 20, which offsets the staging writes' odd-column voxels by 32 banks, measured the same: r16g)
  constexpr int LW = 33, LH = 2 * TH + 1, LD = 2 * TD + 1, SW = 17;
  constexpr int NROW = LD * LH, NQ = NROW * LW * 2;  // float4 quads per tile
  constexpr int NLD = (NQ + NTH - 1) / NTH;
  __shared__ __attribute__((aligned(16))) float tile[NROW * 2 * SW * 8];
  __shared__ __attribute__((aligned(16))) float wts[28 * 16 * 8];
  const int nws = (g.Wo + 15) / 16, nhs = (g.Ho + TH - 1) / TH, nds = (g.Do + TD - 1) / TD;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int col = lane & 15, kgrp = lane >> 4;
  const int half = kgrp & 1, side = kgrp >> 1;
  const TileRange tr(ntiles);
  if (tr.idle()) return;
  auto coord = [&](int t) { return tile_coord(t, nws, nhs, nds, TH, TD); };
  float4 pf[NLD];
  auto fetch = [&](int t) {
    const TileCoord c = coord(t);
    const size_t in_n = (size_t)c.n * g.Di * g.Hi * g.Wi;
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int idx = threadIdx.x + NTH * k;
      const int q = idx & 1, v = idx >> 1;
      const int lw = v % LW, row = v / LW, lh = row % LH, ld = row / LH;
      const int iw = 2 * c.w0 - 1 + lw, ih = 2 * c.h0 - 1 + lh, id = 2 * c.d0 - 1 + ld;
      pf[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < NQ && (unsigned)iw < (unsigned)g.Wi && (unsigned)ih < (unsigned)g.Hi && (unsigned)id < (unsigned)g.Di)
        pf[k] = *reinterpret_cast<const float4*>(x + (in_n + ((size_t)id * g.Hi + ih) * g.Wi + iw) * CIN + 4 * q);
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int idx = threadIdx.x + NTH * k;
      const int q = idx & 1, v = idx >> 1;
      const int lw = v % LW, row = v / LW;
      if (idx < NQ) *reinterpret_cast<float4*>(tile + ((row * 2 + (lw & 1)) * SW + (lw >> 1)) * 8 + 4 * q) = pf[k];
    }
  };
  for (int idx = threadIdx.x; idx < 28 * 16 * 2; idx += NTH) {  // tap 27: zero (the empty half of pair 13)
    const int q = idx & 1, row = (idx >> 1) & 15, tap = idx >> 5;
    const float4 v = tap < 27 ? *reinterpret_cast<const float4*>(wpk + ((size_t)tap * COUT + row) * CIN + 4 * q)
                              : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(wts + (tap * 16 + row) * 8 + 4 * q) = v;
  }
  const int co = kgrp * 4;
  const float4 al = *reinterpret_cast<const float4*>(alpha + co);
  const float4 sh = *reinterpret_cast<const float4*>(shift + co);
  int t = tr.first();
  if (t < tr.end) {
    fetch(t);
    commit();
  }
  __syncthreads();
  for (; t < tr.end; t += tr.step) {
    const TileCoord c = coord(t);
    const int tn = t + tr.step;
    if (tn < tr.end) fetch(tn);
    floatx4 acc[NBW];
#pragma unroll
    for (int r = 0; r < NBW; ++r) acc[r] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int pr = 0; pr < 14; ++pr) {
      const int tap = 2 * pr + side;
      const int tp = tap < 27 ? tap : 26;  // the empty tap reads a real voxel against zero weights
      const int kd = tp / 9, kh = (tp / 3) % 3, kw = tp % 3;
      const float4 a = *reinterpret_cast<const float4*>(wts + (tap * 16 + col) * 8 + 4 * half);
      float4 b[NBW];
#pragma unroll
      for (int r = 0; r < NBW; ++r) {
        const int rr = wv * NBW + r;
        const int odl = rr / TH, ohl = rr - odl * TH;
        const int row = (2 * odl + kd) * LH + 2 * ohl + kh;
        b[r] = *reinterpret_cast<const float4*>(tile + ((row * 2 + (kw & 1)) * SW + col + (kw >> 1)) * 8 + 4 * half);
      }
      // component-major: consecutive MFMAs alternate accumulators (no back-to-back dependence)
#pragma unroll
      for (int r = 0; r < NBW; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[r].x, acc[r], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < NBW; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[r].y, acc[r], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < NBW; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[r].z, acc[r], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < NBW; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[r].w, acc[r], 0, 0, 0);
    }
    const int ow = c.w0 + col;
    const size_t out_n = (size_t)c.n * g.Do * g.Ho * g.Wo;
#pragma unroll
    for (int r = 0; r < NBW; ++r) {
      const int rr = wv * NBW + r;
      const int od = c.d0 + rr / TH, oh = c.h0 + rr % TH;
      if (ow >= g.Wo || od >= g.Do || oh >= g.Ho) continue;
      *reinterpret_cast<float4*>(y + (out_n + ((size_t)od * g.Ho + oh) * g.Wo + ow) * COUT + co) =
          bn_act4(acc[r], al, sh, g.lo);
    }
    __syncthreads();
    if (tn < tr.end) commit();
    __syncthreads();
  }
}

template <int TD, int TH>
static int launch_conv_s2c8_tile(const float* x, const float* w, const float* al, const float* sh, float* y, int B,
                                 const Geo& g, hipStream_t st) {
  return launch_persistent(conv3d_s2c8_tile_kernel<TD, TH>, tile_count(B, g.Do, g.Ho, g.Wo, TD, TH), 0, st, x, w, al, sh, y,
                           g);
}

// ---------------------------------------------------------------- launchers
// workgroup tile of a conv3d_lds_kernel instance: (TD, TH, MBB, WS)
template <int TD_, int TH_, int MBB_, int WS_>
struct LdsTile {
  static constexpr int TD = TD_, TH = TH_, MBB = MBB_, WS = WS_;
};

// one conv3d_lds_kernel instance; the caller names the tap schedule (straight, KDSKIP or TAPOUT)
template <int CIN, int COUT, int S, typename T, bool KDSKIP = false, bool TAPOUT = false>
static int launch_conv(const float* x, const float* w, const float* al, const float* sh, float* y, int B,
                       const Geo& g, hipStream_t st) {
  const long nblk = tile_count(B, g.Do, g.Ho, g.Wo, T::TD, T::TH) * (COUT / 16 / T::MBB);
  hipLaunchKernelGGL((conv3d_lds_kernel<CIN, COUT, S, T::TD, T::TH, T::MBB, T::WS, KDSKIP, TAPOUT>),
                     dim3((unsigned)nblk), dim3(256), 0, st, x, w, al, sh, y, g);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

// ---------------------------------------------------------------- deconv 16 -> 8 (conv11)
// With 8 output channels a 16-row MFMA block would be half empty. Here rows 0-7 and 8-15 hold
// the two W-parity outputs 2m and 2m+1 of one input column m: for each (d, h) tap the first
// MFMA group applies kw=1 (rows 0-7) and kw=2 (rows 8-15) to input column m, the second
// applies kw=0 (rows 8-15 only) to column m+1 -- 8 instead of 12 MFMAs per (d, h) tap and all
// 64 lanes carry output.
// Persistent: a workgroup stages the 13.8 KB of weights in LDS once and then walks its share
// of the tiles (restaging them per 4-row tile moved as many bytes as the input itself). Input
// tiles are double-buffered in LDS -- the next tile's global loads are issued before the
// current tile's MFMAs and land in the other buffer after them -- and the skip (conv0) rows
// are requested before the MFMAs too, so neither latency sits between MFMA phases.
// Tiles are dealt out XCD-contiguously (an XCD's workgroups share one L2: neighbouring tiles
// share their halo voxels).
template <int TDI, int THI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void deconv3d_c8_kernel(const float* __restrict__ x, const float* __restrict__ wpk,
                                                          const float* __restrict__ alpha,
                                                          const float* __restrict__ shift,
                                                          const float* __restrict__ skip, float* __restrict__ y,
                                                          Geo g, int ntiles) {
  constexpr int CIN = 16, COUT = 8, PL = 4;
  constexpr int NBW = TDI * THI / 4;
  constexpr int LW = 17, LH = THI + 1, LD = TDI + 1, VST = 16;
  constexpr int NVOX = LD * LH * LW;
  constexpr int NLD = (NVOX * 4 + 255) / 256;  // float4 staging loads per thread and tile
  static_assert((TDI * THI) % 4 == 0, "tile");
  __shared__ __attribute__((aligned(16))) float tile[2][NVOX * VST];
  __shared__ __attribute__((aligned(16))) float wts[27 * 8 * 16];
  __shared__ __attribute__((aligned(16))) float ep[4][32 * 8];

  const int nws = (g.Wi + 15) / 16, nhs = (g.Hi + THI - 1) / THI, nds = (g.Di + TDI - 1) / TDI;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int col = lane & 15, kgrp = lane >> 4;
  const TileRange tr(ntiles);
  if (tr.idle()) return;

  auto coord = [&](int t) { return tile_coord(t, nws, nhs, nds, THI, TDI); };  // input-grid coordinates
  float4 pf[NLD];
  auto fetch = [&](int t) {  // global -> registers
    const TileCoord c = coord(t);
    const size_t in_n = (size_t)c.n * g.Di * g.Hi * g.Wi;
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int idx = threadIdx.x + 256 * k;
      const int vox = idx >> 2, q = idx & 3;
      const int lw = vox % LW, rest = vox / LW, lh = rest % LH, ld = rest / LH;
      const int iw = c.w0 + lw, ih = c.h0 + lh, id = c.d0 + ld;
      pf[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (vox < NVOX && iw < g.Wi && ih < g.Hi && id < g.Di)
        pf[k] = *reinterpret_cast<const float4*>(x + (in_n + ((size_t)id * g.Hi + ih) * g.Wi + iw) * CIN + 4 * q);
    }
  };
  auto commit = [&](float* buf) {  // registers -> LDS (quad-swizzled voxels)
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int idx = threadIdx.x + 256 * k;
      const int vox = idx >> 2, q = idx & 3;
      if (vox < NVOX) *reinterpret_cast<float4*>(swz16(buf, vox, q)) = pf[k];
    }
  };

  // stage_weights16 for 8 rows, spelled out: through a helper the kernel compiled to another instruction
  // stream and measured slower at stage 3 (profiles/costreg_scaffold_resources.md)
  for (int idx = threadIdx.x; idx < 27 * 8 * 4; idx += 256) {
    const int q = idx & 3, row = (idx >> 2) & 7, tap = idx >> 5;
    const float4 v = *reinterpret_cast<const float4*>(wpk + ((size_t)tap * COUT + row) * CIN + 4 * q);
    *reinterpret_cast<float4*>(wts + (tap * 8 + row) * 16 + 4 * (q ^ ((row >> 1) & 3))) = v;
  }
  const int co = col & 7;    // A row -> output channel
  const bool hi = col >= 8;  // rows 8-15: the odd-w output
  float* eb = ep[wv];
  const int cq = 4 * (kgrp & 1);
  const float4 al = *reinterpret_cast<const float4*>(alpha + cq);
  const float4 sh = *reinterpret_cast<const float4*>(shift + cq);
  auto wfrag = [&](int tap, Vec4& a) { a.load(swz16(wts + tap * 128, co, kgrp)); };

  int t = tr.first();
  if (t < tr.end) {
    fetch(t);
    commit(tile[0]);
  }
  __syncthreads();
  for (int it = 0; t < tr.end; t += tr.step, ++it) {
    const float* cur = tile[it & 1];
    const TileCoord c = coord(t);
    const int tn = t + tr.step;
    if (tn < tr.end) fetch(tn);
    // skip rows of this tile: lane (pair) j of a 1 KiB output row, as the epilogue stores it (storing each
    // lane's own MFMA outputs without the exchange measured 110.2 -> 112.6 us in the step, r16g)
    const size_t out_n = (size_t)c.n * g.Do * g.Ho * g.Wo;
    const int ow = 2 * c.w0 + (lane >> 1);
    const size_t plane = (size_t)g.Ho * g.Wo * 8, row = (size_t)g.Wo * 8;  // output strides (floats)
    float4 sk[NBW][4];
    size_t oo[NBW];
    bool ok[NBW];
#pragma unroll
    for (int r = 0; r < NBW; ++r) {
      const int rr = wv * NBW + r;
      const int md = c.d0 + rr / THI, mh = c.h0 + rr % THI;
      ok[r] = md < g.Di && mh < g.Hi && ow < 2 * g.Wi;
      oo[r] = (out_n + ((size_t)(2 * md) * g.Ho + 2 * mh) * g.Wo + ow) * 8 + (lane & 1) * 4;
#pragma unroll
      for (int pdh = 0; pdh < 4; ++pdh)
        sk[r][pdh] = (ok[r] && skip) ? *reinterpret_cast<const float4*>(skip + oo[r] + (pdh >> 1) * plane + (pdh & 1) * row)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    floatx4 acc[NBW][4];
#pragma unroll
    for (int r = 0; r < NBW; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[r][q] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int pdh = 0; pdh < 4; ++pdh) {
      const int pd = pdh >> 1, ph = pdh & 1;
#pragma unroll
      for (int td = 0; td < 1 + pd; ++td)
#pragma unroll
        for (int th = 0; th < 1 + ph; ++th) {
          const ParityTap d = parity_tap(pd, td), h = parity_tap(ph, th);
          const int tap_base = d.k * 9 + h.k * 3;
          Vec4 a1, a2;
          wfrag(tap_base + (hi ? 2 : 1), a1);  // rows 0-7: kw=1, rows 8-15: kw=2 (input column m)
          if (hi)
            wfrag(tap_base + 0, a2);           // rows 8-15: kw=0 (input column m+1)
          else
            a2.zero();
#pragma unroll
          for (int r = 0; r < NBW; ++r) {
            const int rr = wv * NBW + r;
            const int mdl = rr / THI, mhl = rr - mdl * THI;
            const int lv = ((mdl + d.off) * LH + mhl + h.off) * LW + col;
            Vec4 b1, b2;
            b1.load(swz16(cur, lv, kgrp));
            b2.load(swz16(cur, lv + 1, kgrp));
#pragma unroll
            for (int j = 0; j < PL; ++j)
              acc[r][pdh] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.v[j], b1.v[j], acc[r][pdh], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < PL; ++j)
              acc[r][pdh] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.v[j], b2.v[j], acc[r][pdh], 0, 0, 0);
          }
          __builtin_amdgcn_sched_barrier(0);  // one tap's fragments live at a time (VGPR budget)
        }
    }
    // epilogue: lane (col, kgrp) holds channels 4*(kgrp&1).. of output w 2*(mw0+col) + (kgrp>>1);
    // exchanged through LDS so the skip read and the store are contiguous 1 KiB rows
#pragma unroll
    for (int r = 0; r < NBW; ++r)
#pragma unroll
      for (int pdh = 0; pdh < 4; ++pdh) {
        *reinterpret_cast<float4*>(eb + (2 * col + (kgrp >> 1)) * 8 + cq) = bn_act4(acc[r][pdh], al, sh, g.lo);
        __builtin_amdgcn_wave_barrier();
        const float4 v = *reinterpret_cast<const float4*>(eb + lane * 4);
        __builtin_amdgcn_wave_barrier();
        if (ok[r]) *reinterpret_cast<float4*>(y + oo[r] + (pdh >> 1) * plane + (pdh & 1) * row) = add4(sk[r][pdh], v);
      }
    if (tn < tr.end) commit(tile[(it + 1) & 1]);
    __syncthreads();
  }
}

template <int TDI, int THI>
static int launch_deconv_c8(const float* x, const float* w, const float* al, const float* sh, const float* skip,
                            float* y, int B, const Geo& g, hipStream_t st) {
  return launch_persistent(deconv3d_c8_kernel<TDI, THI>, tile_count(B, g.Di, g.Hi, g.Wi, TDI, THI), 0, st, x, w, al, sh, skip,
                           y, g);
}

// ---------------------------------------------------------------- deconv 32 -> 16 (conv9), persistent
// deconv3d_lds_kernel<32, 16, ...> restages its 27.6 KB of weights per channel chunk and workgroup (107 MB
// of staging at stages 2 / 3 against 16 MB of input) and overlaps nothing with a workgroup's staging but
// the other resident workgroups. Here a workgroup stages both chunks' weights once (55.3 KB), then walks
// its XCD-contiguous share of the tiles as conv3d_c16_kernel does, with both 16-channel planes of a tile
// in LDS (74.9 KB in all: 2 workgroups per CU) and the next tile committed between two barriers.
// Every output keeps deconv3d_lds_kernel's K order (chunk, then its class's taps, then the 4 k-steps, one
// MFMA chain per class), so the results are bitwise the same; only the interleaving of the 8 independent
// chains differs: the 27 taps of a chunk run as two streams (classes 0, 3, 7 / classes 1, 2, 4, 5, 6)
// whose MFMAs alternate, so no MFMA waits on the one issued right before it. The 8 distinct B fragments
// of a chunk (input voxel offsets {0,1}^3) are read from LDS once instead of once per tap.
// The layer moves about as many bytes as HBM delivers in its MFMA time (143 MB; without the MFMAs the
// kernel runs 28 us, without the global traffic 34 us), so the memory instructions are spread over the
// tile's 28 MFMA steps instead of issued in bursts around them: one load per step in the first chunk (this
// tile's 8 skip voxels, then the next tile's staging loads) and each class's stores right behind its last
// MFMA in the second. Stage 2 / 3 per call: 53.6 / 52.0 us generic, 48 us for the plain persistent form,
// 38.5 / 37.7 us as scheduled here.
// tap i (0 .. 12 / 13) of one stream, in deconv3d_lds_kernel's (class, tap of the class) order
constexpr DeconvTap deconv_stream_tap(int stream, int i) {
  for (int cls = 0; cls < 8; ++cls) {
    if ((cls == 0 || cls == 3 || cls == 7) != (stream == 0)) continue;
    if (i < deconv_class_taps(cls)) return deconv_class_tap(cls, i);
    i -= deconv_class_taps(cls);
  }
  return DeconvTap{-1, 0, 0};
}
// the class whose last tap is pair i of its stream (at most one per pair), or -1
constexpr int deconv_class_done(int i) {
  for (int st = 0; st < 2; ++st) {
    const DeconvTap t = deconv_stream_tap(st, i);
    if (t.cls >= 0 && deconv_stream_tap(st, i + 1).cls != t.cls) return t.cls;
  }
  return -1;
}
static_assert(deconv_stream_tap(0, 12).cls == 7 && deconv_stream_tap(0, 13).cls < 0, "stream 0: 13 taps");
static_assert(deconv_stream_tap(1, 13).cls == 6 && deconv_stream_tap(1, 14).cls < 0, "stream 1: 14 taps");

template <typename F, int... I>
__device__ __forceinline__ void static_for(std::integer_sequence<int, I...>, F f) {
  (f(std::integral_constant<int, I>{}), ...);
}

template <int TDI, int THI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void deconv3d_c16p_kernel(
    const float* __restrict__ x, const float* __restrict__ wpk, const float* __restrict__ alpha,
    const float* __restrict__ shift, const float* __restrict__ skip, float* __restrict__ y, Geo g, int ntiles) {
  constexpr int CIN = 32, COUT = 16, PL = 4, NCH = 2;
  static_assert(TDI * THI == 4, "one input-grid row per wave");
  constexpr int LW = 17, LH = THI + 1, LD = TDI + 1;
  constexpr int NVOX = LD * LH * LW;
  constexpr int NQ = NVOX * 2 * PL;          // float4 quads per tile: a voxel's 32 channels are 8
  constexpr int NLD = (NQ + 255) / 256;      // staging loads per thread and tile
  __shared__ __attribute__((aligned(16))) float tile[NCH][NVOX * 16];
  __shared__ __attribute__((aligned(16))) float wts[NCH][27 * 16 * 16];

  const int nws = (g.Wi + 15) / 16, nhs = (g.Hi + THI - 1) / THI, nds = (g.Di + TDI - 1) / TDI;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15, kgrp = lane >> 4;
  const TileRange tr(ntiles);
  if (tr.idle()) return;
  auto coord = [&](int t) { return tile_coord(t, nws, nhs, nds, THI, TDI); };  // input-grid coordinates
  const uint32_t in_bytes = (uint32_t)g.Di * g.Hi * g.Wi * CIN * 4;     // one sample (host: < 2 GB)
  const uint32_t out_bytes = (uint32_t)g.Do * g.Ho * g.Wo * COUT * 4;   // (host: < 2 GB)
  float4 pf[NLD];
  // global -> registers, branch-free: lanes outside the volume (and every lane when there is no next
  // tile) read zeros through the buffer's range check, so the vmcnt waits stay exact
  struct Fetch {  // the wave-uniform part of a tile's staging loads
    Buf xb;
    TileCoord c;
    int soff;
    bool live;
  };
  auto fetch_of = [&](int t, bool live) {
    const TileCoord c = coord(live ? t : 0);
    return Fetch{Buf(x + (size_t)c.n * g.Di * g.Hi * g.Wi * CIN, in_bytes), c,
                 ((c.d0 * g.Hi + c.h0) * g.Wi + c.w0) * CIN * 4 /* the tile's first voxel */, live};
  };
  auto fetch1 = [&](const Fetch& f, int k) {
    const int idx = threadIdx.x + 256 * k;
    const int vox = idx >> 3, q8 = idx & 7;
    const int lw = vox % LW, rest = vox / LW, lh = rest % LH, ld = rest / LH;
    const bool ok = f.live && idx < NQ && f.c.w0 + lw < g.Wi && f.c.h0 + lh < g.Hi && f.c.d0 + ld < g.Di;
    pf[k] = f.xb.ld4(ok ? (((ld * g.Hi + lh) * g.Wi + lw) * CIN + 4 * q8) * 4 : Buf::kOOB, f.soff);
  };
  auto fetch = [&](int t, bool live) {
    const Fetch f = fetch_of(t, live);
#pragma unroll
    for (int k = 0; k < NLD; ++k) fetch1(f, k);
  };
  auto commit = [&]() {  // registers -> LDS: two 16-channel planes of quad-swizzled voxels
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int idx = threadIdx.x + 256 * k;
      const int vox = idx >> 3, q8 = idx & 7;
      const int ch = q8 >> 2, q = q8 & 3;
      if (idx < NQ) *reinterpret_cast<float4*>(swz16(tile[ch], vox, q)) = pf[k];
    }
  };

  // the weights: every load in flight at once, with the first tile's behind them (a load -> LDS write loop
  // paid one L2 round trip per 4 KB, 14 in a row, before the first MFMA)
  constexpr int NWQ = NCH * 27 * 16 * 4, NWL = (NWQ + 255) / 256;
  const Buf wb(wpk, 27u * COUT * CIN * 4);
  float4 wreg[NWL];
#pragma unroll
  for (int k = 0; k < NWL; ++k) {
    const int idx = threadIdx.x + 256 * k;  // quad idx of wpk: [tap][row][ch][q]
    wreg[k] = wb.ld4(idx < NWQ ? idx * 16 : Buf::kOOB);
  }
  int t = tr.first();
  fetch(t, t < tr.end);
#pragma unroll
  for (int k = 0; k < NWL; ++k) {
    const int idx = threadIdx.x + 256 * k;
    const int q = idx & 3, ch = (idx >> 2) & 1, row = (idx >> 3) & 15, tap = idx >> 7;
    if (idx < NWQ) *reinterpret_cast<float4*>(swz16(wts[ch] + tap * 256, row, q)) = wreg[k];
  }
  const int co = kgrp * 4;
  const float4 al = *reinterpret_cast<const float4*>(alpha + co);
  const float4 sh = *reinterpret_cast<const float4*>(shift + co);
  const int mdl = wv / THI, mhl = wv - mdl * THI;  // the wave's input-grid row of the tile
  const int woff = swz16(col, kgrp);  // the lane's A fragment within a tap

  commit();
  __syncthreads();
  for (; t < tr.end; t += tr.step) {
    const TileCoord c = coord(t);
    const int tn = t + tr.step;
    const bool more = tn < tr.end;
    const Fetch fn = fetch_of(tn, more);
    const int md = c.d0 + mdl, mh = c.h0 + mhl, mw = c.w0 + col;
    const bool ok = md < g.Di && mh < g.Hi && mw < g.Wi;
    const size_t out_n = (size_t)c.n * g.Do * g.Ho * g.Wo * COUT;
    const Buf sb(skip ? skip + out_n : nullptr, skip ? out_bytes : 0u), yb(y + out_n, out_bytes);
    const int o0 = (((2 * md) * g.Ho + 2 * mh) * g.Wo + 2 * mw) * COUT + co;  // class 0 (floats)
    int so[8];  // byte offset of the lane's 4 channels of each class's output voxel
    float4 sk[8];  // the skip voxels
#pragma unroll
    for (int cls = 0; cls < 8; ++cls) {
      const int rel = (((cls >> 2) * g.Ho + ((cls >> 1) & 1)) * g.Wo + (cls & 1)) * COUT;
      so[cls] = ok ? (o0 + rel) * 4 : Buf::kOOB;
    }
    floatx4 acc[8];
#pragma unroll
    for (int cls = 0; cls < 8; ++cls) acc[cls] = floatx4{0.f, 0.f, 0.f, 0.f};
    // deconv3d_lds_kernel's epilogue of one class (a lane outside the volume stores nothing)
    auto epilogue = [&](auto cc) {
      constexpr int cls = decltype(cc)::value;
      yb.st4(add4(sk[cls], bn_act4(acc[cls], al, sh, g.lo)), so[cls]);
    };
    // 28 steps (chunk, tap pair). The A fragments of step s + 1 are read from LDS before step s's MFMAs
    // (read right before their own MFMAs, every step opened with an exposed LDS round trip), and chunk 1's
    // B fragments one per step during chunk 0's first 8.
    Vec4 b[NCH][8], a[2][2];
    auto bload = [&](int ch, int off) {
      const int lvox = ((mdl + (off >> 2)) * LH + mhl + ((off >> 1) & 1)) * LW + col + (off & 1);
      b[ch][off].load(swz16(tile[ch], lvox, kgrp));
    };
#pragma unroll
    for (int off = 0; off < 8; ++off) bload(0, off);
    a[0][0].load(wts[0] + deconv_stream_tap(0, 0).tap * 256 + woff);
    a[0][1].load(wts[0] + deconv_stream_tap(1, 0).tap * 256 + woff);
    __builtin_amdgcn_sched_barrier(0);
    static_for(std::make_integer_sequence<int, 14 * NCH>{}, [&](auto sc) {
      constexpr int s = decltype(sc)::value, ch = s / 14, i = s % 14;
      constexpr DeconvTap t0 = deconv_stream_tap(0, i), t1 = deconv_stream_tap(1, i);
      constexpr int s1 = s + 1, ch1 = s1 / 14, i1 = s1 % 14;
      constexpr bool next = s1 < 14 * NCH, next0 = next && deconv_stream_tap(0, i1).cls >= 0;
      if constexpr (next0) a[s1 & 1][0].load(wts[ch1] + deconv_stream_tap(0, i1).tap * 256 + woff);
      if constexpr (next) a[s1 & 1][1].load(wts[ch1] + deconv_stream_tap(1, i1).tap * 256 + woff);
      if constexpr (s < 8) bload(1, s);
      // one global load per step of chunk 0: this tile's 8 skip voxels, then the next tile's staging loads
      // (all 13 ahead of the MFMAs measured 39.6 -> 37.7 us at stage 3)
      if constexpr (s < 8) sk[s] = sb.ld4(so[s]);
      if constexpr (s >= 8 && s < 8 + NLD) fetch1(fn, s - 8);
#pragma unroll
      for (int j = 0; j < PL; ++j) {
        if constexpr (t0.cls >= 0)
          acc[t0.cls] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s & 1][0].v[j], b[ch][t0.off].v[j], acc[t0.cls], 0, 0, 0);
        acc[t1.cls] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s & 1][1].v[j], b[ch][t1.off].v[j], acc[t1.cls], 0, 0, 0);
      }
      // the step's LDS reads first, then its MFMAs in the order written
      __builtin_amdgcn_sched_group_barrier(0x100, (next0 ? 1 : 0) + (next ? 1 : 0) + (s < 8 ? 1 : 0), 0);
      __builtin_amdgcn_sched_group_barrier(0x008, t0.cls >= 0 ? 2 * PL : PL, 0);
      // a class's epilogue one step behind its last MFMA: the stores leave spread over the second chunk's
      // MFMAs (all 8 behind the tile measured 42.7 -> 39.6 us at stage 3)
      if constexpr (ch == NCH - 1 && i >= 1 && deconv_class_done(i - 1) >= 0)
        epilogue(std::integral_constant<int, deconv_class_done(i - 1)>{});
      __builtin_amdgcn_sched_barrier(0);
    });
    epilogue(std::integral_constant<int, deconv_class_done(13)>{});
    __syncthreads();  // every wave is done with the tile
    commit();         // (zeros behind the last tile)
    __syncthreads();
  }
}

// resident workgroups of the device for one persistent kernel (persistent_grid's cap)
template <typename K>
static int persistent_cap(K kernel) {
  return persistent_grid(kernel, 1L << 40);
}

// deconv_dispatch takes this kernel from 1.5 tiles per resident workgroup on: measured faster than the
// one-tile-per-workgroup kernel at 1.6 (stage 1: 29.8 -> 24.6 us) and 3.8 (stages 2 / 3); not measured below
constexpr int kC16pMinTilesNum = 3, kC16pMinTilesDen = 2;

// max_wgs > 0 bounds the grid below the device's residency (tests: a multi-tile walk on a small volume)
template <int TDI, int THI>
static int launch_deconv_c16p(const float* x, const float* w, const float* al, const float* sh, const float* skip,
                              float* y, int B, const Geo& g, hipStream_t st, int max_wgs = 0) {
  return launch_persistent(deconv3d_c16p_kernel<TDI, THI>, tile_count(B, g.Di, g.Hi, g.Wi, TDI, THI), max_wgs, st, x, w, al,
                           sh, skip, y, g);
}

template <int CIN, int COUT, int TDI, int THI>
static int launch_deconv(const float* x, const float* w, const float* al, const float* sh, const float* skip,
                         float* y, int B, const Geo& g, hipStream_t st) {
  const long nblk = tile_count(B, g.Di, g.Hi, g.Wi, TDI, THI) * (COUT / 16);
  hipLaunchKernelGGL((deconv3d_lds_kernel<CIN, COUT, TDI, THI>), dim3((unsigned)nblk), dim3(256), 0, st, x, w,
                     al, sh, skip, y, g);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

static int conv_dispatch(const float* x, int B, int cin, int d, int h, int w, const float* wpk, const float* al,
                         const float* sh, int cout, int stride, float* y, hipStream_t st, float lo = 0.f) {
  const Geo g = Geo::conv(d, h, w, stride, lo);
  // the MFMA kernels address one sample's input through a buffer with 32-bit byte offsets
  if ((long long)d * h * w * cin * 4 >= (1LL << 31)) return TMVS_ERR_SHAPE;
  // output depth <= 2 (the coarse levels of a D = 8 stage): every wave has a kd slice that lies wholly in
  // the depth padding, which the KDSKIP instances do not run
  constexpr int kKdSkipMaxDo = 2;
  const bool kdskip = g.Do <= kKdSkipMaxDo;
  constexpr bool KD = true, TAPOUT = true;
  using Conv3Tile = LdsTile<2, 2, 2, 2>;    // 50.4 -> 46.0 us at stage 3 (r17n)
  using Conv4Tile = LdsTile<2, 2, 2, 2>;    // output depth > 2 (r17h)
  using Conv4TileKd = LdsTile<2, 4, 2, 1>;  // output depth <= 2
  using Conv5Tile = LdsTile<1, 2, 4, 4>;    // each wave one output block: 30.4 / 15.5 / 19.1 us at stages 2 / 1 / 3 (r17j)
  using Conv6Tile = LdsTile<1, 2, 4, 4>;    // each wave one output block (r17g)
  int (*launch)(const float*, const float*, const float*, const float*, float*, int, const Geo&, hipStream_t) = nullptr;
  if (stride == 1) {
    if (cin == 16 && cout == 16)  // conv2: persistent, weights in LDS, 2x4x16-voxel tiles
      launch = launch_conv_c16<2, 4>;
    else if (cin == 32 && cout == 32)  // conv4
      launch = kdskip ? launch_conv<32, 32, 1, Conv4TileKd, KD> : launch_conv<32, 32, 1, Conv4Tile>;
    else if (cin == 64 && cout == 64)  // conv6
      launch = kdskip ? launch_conv<64, 64, 1, Conv6Tile, KD> : launch_conv<64, 64, 1, Conv6Tile>;
  } else {
    // conv1's 2x2 tiles: 3 workgroups per CU (41.5 KB LDS); 2x4 measured 103 vs 97-98 us (r12e)
    if (cin == 8 && cout == 16)  // conv1: persistent, weights in LDS, tap pairs
      launch = launch_conv_s2c8_tile<2, 2>;
    else if (cin == 16 && cout == 32)  // conv3
      launch = kdskip ? launch_conv<16, 32, 2, Conv3Tile, KD> : launch_conv<16, 32, 2, Conv3Tile>;
    else if (cin == 32 && cout == 64)  // conv5: taps outer, the K order the oracle-parity tests pin
      launch = launch_conv<32, 64, 2, Conv5Tile, false, TAPOUT>;
  }
  return launch ? launch(x, wpk, al, sh, y, B, g, st) : TMVS_ERR_SHAPE;
}

// which kernel a layer that has a persistent form runs on: by its geometry (the product), or pinned
enum class Route { kAuto, kGeneric, kPersistent };

static int deconv_dispatch(const float* x, int B, int cin, int d, int h, int w, const float* wpk, const float* al,
                           const float* sh, int cout, const float* skip, float* y, hipStream_t st, float lo = 0.f,
                           Route route = Route::kAuto, int max_wgs = 0) {
  const Geo g = Geo::deconv(d, h, w, lo);
  // (TDI, THI) input tile: 2 x 2 for an even input depth, 1 x 4 for an odd one
  const bool even = g.Di % 2 == 0;
  int (*launch)(const float*, const float*, const float*, const float*, const float*, float*, int, const Geo&,
                hipStream_t) = nullptr;
  if (cin == 64 && cout == 32)
    launch = even ? launch_deconv<64, 32, 2, 2> : launch_deconv<64, 32, 1, 4>;
  else if (cin == 32 && cout == 16)
    launch = even ? launch_deconv<32, 16, 2, 2> : launch_deconv<32, 16, 1, 4>;
  else if (cin == 16 && cout == 8)  // W-parity outputs packed into the 16 MFMA rows
    launch = even ? launch_deconv_c8<2, 2> : launch_deconv_c8<1, 4>;
  if (cin == 32 && cout == 16 && route != Route::kGeneric) {
    // conv9, persistent: it addresses one sample's input and output through buffers with 32-bit byte
    // offsets, and is taken from kC16pMinTilesNum / kC16pMinTilesDen tiles per resident workgroup on
    const bool fits = (long long)g.Do * g.Ho * g.Wo * cout * 4 < (1LL << 31);  // (the input is a quarter of it)
    const int tdi = even ? 2 : 1, thi = even ? 2 : 4;
    const long ntiles = tile_count(B, d, h, w, tdi, thi);
    const int cap = even ? persistent_cap(deconv3d_c16p_kernel<2, 2>) : persistent_cap(deconv3d_c16p_kernel<1, 4>);
    if (route == Route::kPersistent && !fits) return TMVS_ERR_SHAPE;
    if (route == Route::kPersistent || (fits && ntiles * kC16pMinTilesDen >= (long)cap * kC16pMinTilesNum))
      return even ? launch_deconv_c16p<2, 2>(x, wpk, al, sh, skip, y, B, g, st, max_wgs)
                  : launch_deconv_c16p<1, 4>(x, wpk, al, sh, skip, y, B, g, st, max_wgs);
  } else if (route == Route::kPersistent) {
    return TMVS_ERR_SHAPE;  // no persistent form of this layer
  }
  return launch ? launch(x, wpk, al, sh, skip, y, B, g, st) : TMVS_ERR_SHAPE;
}


}  // namespace tmvs

using namespace tmvs;

extern "C" int tmvs_conv3d_bn_relu(const float* x, int batch, int cin, int d, int h, int w, const float* wpk,
                                   const float* alpha, const float* shift, int cout, int stride, float* y,
                                   void* stream) {
  if (!x || !wpk || !alpha || !shift || !y || batch <= 0 || d <= 0 || h <= 0 || w <= 0) return TMVS_ERR_ARG;
  if (stride != 1 && stride != 2) return TMVS_ERR_ARG;
  return conv_dispatch(x, batch, cin, d, h, w, wpk, alpha, shift, cout, stride, y, (hipStream_t)stream);
}

extern "C" int tmvs_deconv3d_bn_relu_add(const float* x, int batch, int cin, int d, int h, int w, const float* wpk,
                                         const float* alpha, const float* shift, int cout, const float* skip,
                                         float* y, void* stream) {
  if (!x || !wpk || !alpha || !shift || !skip || !y || batch <= 0 || d <= 0 || h <= 0 || w <= 0)
    return TMVS_ERR_ARG;
  return deconv_dispatch(x, batch, cin, d, h, w, wpk, alpha, shift, cout, skip, y, (hipStream_t)stream);
}

extern "C" int tmvs_deconv3d_bn_relu_add_generic(const float* x, int batch, int cin, int d, int h, int w,
                                                 const float* wpk, const float* alpha, const float* shift, int cout,
                                                 const float* skip, float* y, void* stream) {
  if (!x || !wpk || !alpha || !shift || !skip || !y || batch <= 0 || d <= 0 || h <= 0 || w <= 0)
    return TMVS_ERR_ARG;
  return deconv_dispatch(x, batch, cin, d, h, w, wpk, alpha, shift, cout, skip, y, (hipStream_t)stream, 0.f,
                         Route::kGeneric);
}

extern "C" int tmvs_deconv3d_bn_relu_add_persistent(const float* x, int batch, int cin, int d, int h, int w,
                                                    const float* wpk, const float* alpha, const float* shift,
                                                    int cout, const float* skip, float* y, int max_workgroups,
                                                    void* stream) {
  if (!x || !wpk || !alpha || !shift || !skip || !y || batch <= 0 || d <= 0 || h <= 0 || w <= 0 || max_workgroups < 0)
    return TMVS_ERR_ARG;
  return deconv_dispatch(x, batch, cin, d, h, w, wpk, alpha, shift, cout, skip, y, (hipStream_t)stream, 0.f,
                         Route::kPersistent, max_workgroups);
}

static int launch_conv0(const float* x, float* y, int batch, int D, int H, int W, const float* wt, const float* al,
                        const float* sh, float lo, hipStream_t st) {
  const dim3 grid((unsigned)(((W + kProbCols - 1) / kProbCols) * ((H + 3) / 4) * batch * ((D + kDChunk - 1) / kDChunk)));
  hipLaunchKernelGGL(conv0_kernel, grid, dim3(256), 0, st, x, y, D, H, W, wt, al, sh, lo);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

// prob (8 -> 1) raw logits: one row per wave (two measured 42.3 -> 44.9 us at stage 1's D = 48, r16c)
static int launch_prob(const float* x, float* y, int batch, int D, int H, int W, const float* wt, hipStream_t st) {
  constexpr int NR = 1;
  const dim3 grid((unsigned)(((W + kProbCols - 1) / kProbCols) * ((H + 4 * NR - 1) / (4 * NR)) * batch *
                             ((D + kDChunk - 1) / kDChunk)));
  hipLaunchKernelGGL(prob_kernel<NR>, grid, dim3(256), 0, st, x, y, D, H, W, wt);
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}

// alpha = 1, shift = 0 for the raw (training) form of the MFMA layers (64 = the widest layer)
__device__ float kUnitAlpha[64] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f,
                                   1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f,
                                   1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f,
                                   1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
__device__ float kZeroShift[64];

extern "C" int tmvs_conv3d_mfma(const float* x, int batch, int cin, int d, int h, int w, const float* wpk, int cout,
                                int stride, int transposed, const float* skip, float* y, void* stream) {
  if (!x || !wpk || !y || batch <= 0 || d <= 0 || h <= 0 || w <= 0) return TMVS_ERR_ARG;
  if (transposed ? stride != 2 : (stride != 1 && stride != 2)) return TMVS_ERR_ARG;
  if (skip && !transposed) return TMVS_ERR_ARG;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return TMVS_ERR_HIP;
  static const float* unit[64][2];  // per device: the symbols' addresses
  if (!unit[dev][0]) {
    void *a, *b;
    if (hipGetSymbolAddress(&a, HIP_SYMBOL(kUnitAlpha)) != hipSuccess ||
        hipGetSymbolAddress(&b, HIP_SYMBOL(kZeroShift)) != hipSuccess)
      return TMVS_ERR_HIP;
    unit[dev][1] = (const float*)b;
    unit[dev][0] = (const float*)a;
  }
  const float *al = unit[dev][0], *sh = unit[dev][1];
  const float lo = -__builtin_huge_valf();
  hipStream_t st = (hipStream_t)stream;
  if (!transposed && stride == 1 && cin == 1 && cout == 8) {  // conv0's VALU kernel, raw epilogue
    if ((long long)d * h * w * 32 >= (1LL << 31)) return TMVS_ERR_SHAPE;
    return launch_conv0(x, y, batch, d, h, w, wpk, al, sh, lo, st);
  }
  if (!transposed && stride == 1 && cin == 8 && cout == 1) {  // prob's VALU kernel (prob packing)
    if ((long long)d * h * w * 32 >= (1LL << 31)) return TMVS_ERR_SHAPE;
    return launch_prob(x, y, batch, d, h, w, wpk, st);
  }
  if (transposed) return deconv_dispatch(x, batch, cin, d, h, w, wpk, al, sh, cout, skip, y, st, lo);
  return conv_dispatch(x, batch, cin, d, h, w, wpk, al, sh, cout, stride, y, st, lo);
}

static size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" size_t tmvs_costregnet_workspace(int batch, int depth, int height, int width, int base_ch) {
  const size_t v0 = (size_t)batch * depth * height * width;
  const size_t v1 = v0 / 8, v2 = v0 / 64, v3 = v0 / 512;
  const size_t c = (size_t)base_ch;
  // conv0, conv1, conv2, conv3, conv4, conv5, conv6, x7, x9, x11
  size_t bytes = 0;
  bytes += align_up(v0 * c * 4);          // conv0
  bytes += align_up(v1 * 2 * c * 4) * 2;  // conv1, conv2
  bytes += align_up(v2 * 4 * c * 4) * 2;  // conv3, conv4
  bytes += align_up(v3 * 8 * c * 4) * 2;  // conv5, conv6
  bytes += align_up(v2 * 4 * c * 4);      // conv4 + conv7(x)
  bytes += align_up(v1 * 2 * c * 4);      // conv2 + conv9(x)
  bytes += align_up(v0 * c * 4);          // conv0 + conv11(x)
  return bytes;
}

// CostRegNet up to conv11 + skip (models/module.py:447-455); *x11_out = the 8-channel
// full-resolution NDHWC volume the prob conv reads, *c0_out = conv0's (dead once x11 exists).
static int costregnet_trunk(const float* x, int batch, int depth, int height, int width, const TmvsCostRegWeights* w,
                            void* workspace, size_t workspace_bytes, hipStream_t st, float** x11_out,
                            float** c0_out) {
  if (!x || !w || !workspace || batch <= 0) return TMVS_ERR_ARG;
  if (depth % 8 || height % 8 || width % 8) return TMVS_ERR_SHAPE;
  if (w->base_ch != 8) return TMVS_ERR_SHAPE;
  // conv0 / prob address one sample's 8-channel full-resolution volume with 32-bit offsets
  if ((long long)depth * height * width * 32 >= (1LL << 31)) return TMVS_ERR_SHAPE;
  for (int i = 0; i < 11; ++i)
    if (!w->w[i]) return TMVS_ERR_ARG;
  for (int i = 0; i < 10; ++i)
    if (!w->alpha[i] || !w->shift[i]) return TMVS_ERR_ARG;
  if (workspace_bytes < tmvs_costregnet_workspace(batch, depth, height, width, w->base_ch)) return TMVS_ERR_ARG;
  const int c = w->base_ch;
  const size_t v0 = (size_t)batch * depth * height * width;
  const size_t v1 = v0 / 8, v2 = v0 / 64, v3 = v0 / 512;
  char* ws = (char*)workspace;
  auto take = [&](size_t n) {
    float* p = (float*)ws;
    ws += align_up(n * 4);
    return p;
  };
  float* c0 = take(v0 * c);
  float* c1 = take(v1 * 2 * c);
  float* c2 = take(v1 * 2 * c);
  float* c3 = take(v2 * 4 * c);
  float* c4 = take(v2 * 4 * c);
  float* c5 = take(v3 * 8 * c);
  float* c6 = take(v3 * 8 * c);
  float* x7 = take(v2 * 4 * c);
  float* x9 = take(v1 * 2 * c);
  float* x11 = take(v0 * c);
  const int D0 = depth, H0 = height, W0 = width;
  const int D1 = D0 / 2, H1 = H0 / 2, W1 = W0 / 2;
  const int D2 = D1 / 2, H2 = H1 / 2, W2 = W1 / 2;
  const int D3 = D2 / 2, H3 = H2 / 2, W3 = W2 / 2;
  int rc;
  if ((rc = launch_conv0(x, c0, batch, D0, H0, W0, w->w[0], w->alpha[0], w->shift[0], 0.f, st))) return rc;
  if ((rc = conv_dispatch(c0, batch, c, D0, H0, W0, w->w[1], w->alpha[1], w->shift[1], 2 * c, 2, c1, st))) return rc;
  if ((rc = conv_dispatch(c1, batch, 2 * c, D1, H1, W1, w->w[2], w->alpha[2], w->shift[2], 2 * c, 1, c2, st)))
    return rc;
  if ((rc = conv_dispatch(c2, batch, 2 * c, D1, H1, W1, w->w[3], w->alpha[3], w->shift[3], 4 * c, 2, c3, st)))
    return rc;
  if ((rc = conv_dispatch(c3, batch, 4 * c, D2, H2, W2, w->w[4], w->alpha[4], w->shift[4], 4 * c, 1, c4, st)))
    return rc;
  if ((rc = conv_dispatch(c4, batch, 4 * c, D2, H2, W2, w->w[5], w->alpha[5], w->shift[5], 8 * c, 2, c5, st)))
    return rc;
  if ((rc = conv_dispatch(c5, batch, 8 * c, D3, H3, W3, w->w[6], w->alpha[6], w->shift[6], 8 * c, 1, c6, st)))
    return rc;
  if ((rc = deconv_dispatch(c6, batch, 8 * c, D3, H3, W3, w->w[7], w->alpha[7], w->shift[7], 4 * c, c4, x7, st)))
    return rc;
  if ((rc = deconv_dispatch(x7, batch, 4 * c, D2, H2, W2, w->w[8], w->alpha[8], w->shift[8], 2 * c, c2, x9, st)))
    return rc;
  if ((rc = deconv_dispatch(x9, batch, 2 * c, D1, H1, W1, w->w[9], w->alpha[9], w->shift[9], c, c0, x11, st)))
    return rc;
  *x11_out = x11;
  *c0_out = c0;
  return TMVS_OK;
}

extern "C" int tmvs_costregnet(const float* x, int batch, int depth, int height, int width,
                               const TmvsCostRegWeights* w, void* workspace, size_t workspace_bytes, float* logits,
                               void* stream) {
  if (!logits) return TMVS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  float *x11, *c0;
  int rc;
  if ((rc = costregnet_trunk(x, batch, depth, height, width, w, workspace, workspace_bytes, st, &x11, &c0))) return rc;
  return launch_prob(x11, logits, batch, depth, height, width, w->w[10], st);
}

extern "C" int tmvs_costregnet_wta(const float* x, const float* hyp, int batch, int depth, int height, int width,
                                   const TmvsCostRegWeights* w, void* workspace, size_t workspace_bytes,
                                   float clamp_lo, float clamp_hi, float* prob, float* depth_out, float* depth_raw,
                                   float* conf, void* stream) {
  if (!hyp || !prob || !depth_out || !depth_raw || !conf) return TMVS_ERR_ARG;
  switch (depth) {  // the D values tmvs_softmax_wta takes that CostRegNet's depth % 8 rule admits
    case 8: case 16: case 24: case 32: case 48: case 64: break;
    default: return TMVS_ERR_SHAPE;
  }
  hipStream_t st = (hipStream_t)stream;
  float *x11, *c0;
  int rc;
  if ((rc = costregnet_trunk(x, batch, depth, height, width, w, workspace, workspace_bytes, st, &x11, &c0))) return rc;
  if (depth > 32) {
    // D = 48 (stage 1) fused measured 53.8 us vs 40.1 + 10.3 us split (r07d vs r07b): few columns
    // and a 48-deep softmax tail behind the barrier. Split: the depth-chunked prob kernel, its
    // logits in conv0's buffer (dead once conv11 has consumed it as its skip), then the softmax kernel
    if ((rc = launch_prob(x11, c0, batch, depth, height, width, w->w[10], st))) return rc;
    return tmvs_softmax_wta(c0, hyp, batch, depth, height, width, clamp_lo, clamp_hi, prob, depth_out, depth_raw,
                            conf, stream);
  }
  // D <= 32: one workgroup per (sample, row pair, 62-column segment), its D/8 waves prob_kernel's depth
  // chunks. Measured (r07d vs r07b): D = 32 114.0 vs 108.4 + 15.7 us, D = 8 104.3 vs 90.9 + 18.6 us;
  // two rows per wave: the raw walk's two-row form measured 96.0 -> 92.1 / 90.9 -> 87.8 us at stages 2 / 3 (r16c)
  constexpr int kProbWtaRows = 2;
  const dim3 gf((unsigned)(((width + kProbCols - 1) / kProbCols) * ((height + kProbWtaRows - 1) / kProbWtaRows) * batch));
  const dim3 bf((unsigned)(64 * (depth / kDChunk)));
  auto fused = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, gf, bf, 0, st, x11, w->w[10], hyp, height, width, clamp_lo, clamp_hi, prob, depth_out,
                       depth_raw, conf);
  };
  switch (depth) {
    case 8: fused(prob_wta_rows_kernel<8, kProbWtaRows>); break;
    case 16: fused(prob_wta_rows_kernel<16, kProbWtaRows>); break;
    case 24: fused(prob_wta_rows_kernel<24, kProbWtaRows>); break;
    case 32: fused(prob_wta_rows_kernel<32, kProbWtaRows>); break;
  }
  TMVS_CHECK_LAUNCH();
  return TMVS_OK;
}
