"""The training convolution, weight-gradient and BatchNorm kernels, each called on its own through its
transmvsnet_amd.ops wrapper, at the tail shapes the whole-network tests never reach: odd extents under a
stride-2 gather, rows narrower than 4 voxels, depth and height of 1, batch boundaries inside a 64-row
chunk, the last chunk's tail, padding blocks of the 1-D weight-gradient grid, the sizes at which a
reduction's block doubles, the scalar and float4 BatchNorm paths.

  csrc/costreg_train.hip     conv3d_generic, conv3d_wgrad (matrix-core tile and taps kernels, csrc/reduce_mfma.h),
                             bn_stats, bn_relu_train, bn_relu_backward and their grouped forms
  csrc/featurenet_train.hip  conv2d_generic

Every reference is plain torch on the CPU, written out below (nothing from oracle/, train.py or
featurenet_train.py; the [taps][cout][cin] weight layout is spelled out here), and evaluated in fp32 and in
fp64. Error = max|got - ref64| / max|ref64|; the bar is err_gpu <= max(2 x err_fp32ref, 1e-5) where
err_fp32ref is the CPU fp32 reference's own error against fp64 on the same inputs (tests/_primitives.py,
shared with test_gpu_train_primitives.py). Outputs the caller supplies are contiguous slices of larger
buffers whose other rows hold a sentinel that must survive bit for bit; the reductions documented as
fixed-order are run twice and must repeat bit for bit.

BatchNorm's backward is discontinuous where the pre-activation relu() sees is 0, so the BN inputs are
conditioned on the CPU (_bn_condition) until every pre-activation, evaluated in fp64, is at least
tau = 4 * 8 * 2^-23 * (|z alpha| + |mean alpha| + |beta|) away from 0 -- 4 x the fp32 rounding bound of
fmaf(z, alpha, shift) with alpha and shift formed in fp32 -- and the test asserts that before it touches
the GPU. No element is excluded from any comparison.

Measured on an MI355X, worst (err_gpu, err_fp32ref) over all cases of an op: conv3d_wgrad (2.9e-7, 3.2e-5 --
the CPU's fp32 sum over 1,052,969 voxels drifts, the kernel's fp64 chunk sums do not), conv3d_generic
(5.6e-6, 5.6e-6), conv2d_generic (1.7e-6, 1.8e-6), bn_stats (4.7e-8, 5.1e-7), bn_relu_train (8.0e-7, 1.2e-6),
bn_relu_backward (3.8e-7, 1.3e-6), grouped: stats (5.2e-8, 1.4e-7), train (2.7e-6, 2.6e-6), backward
(2.1e-7, 1.3e-6): the 1e-5 floor is the bar nearly everywhere. 366 cases, about 11 s.
"""
import pytest
import torch
import torch.nn.functional as F

from tests._primitives import DEV, _assert_guard, _bits, _gen, _guarded, _judge
from transmvsnet_amd import ops

pytestmark = pytest.mark.gpu
DTS = (torch.float32, torch.float64)


# ------------------------------------------------------------------------------------------ conv3d_wgrad
WG_PAIRS = [(8, 1), (1, 8), (8, 8), (16, 8), (8, 16), (16, 16), (32, 16), (16, 32), (32, 32), (64, 32), (32, 64),
            (64, 64)]
WG_EDGE_PAIRS = [(8, 8), (64, 64), (8, 1), (1, 8)]


def _wg_geo(b, p, stride, g=None):
    """(B, P, G, stride); G defaults to P (stride 1) or 2P - 1 (stride 2: the k = 2 tap of the last voxel
    falls outside)"""
    if g is None:
        g = tuple(p) if stride == 1 else tuple(2 * e - 1 for e in p)
    return (b, tuple(p), tuple(g), stride)


def _conv_extent(g):
    return tuple((e - 1) // 2 + 1 for e in g)


WG_BASE = [
    _wg_geo(3, (2, 3, 5), 1),                        # 90 voxels: Pw = 5 wraps 12 times per chunk, batches end mid-chunk
    _wg_geo(3, (2, 3, 5), 2),                        # G = 2P - 1 in all three axes
    _wg_geo(2, (3, 7, 49), 2, (6, 14, 98)),          # 2058 voxels: ten rows past the first 2048-voxel block; G = 2P
]
WG_EDGE = [
    _wg_geo(1, (1, 1, 1), 1), _wg_geo(1, (1, 1, 1), 2),
    _wg_geo(1, (1, 1, 63), 1), _wg_geo(1, (1, 1, 65), 1), _wg_geo(1, (1, 1, 65), 2),
    _wg_geo(2, (1, 1, 2), 1), _wg_geo(2, (1, 1, 2), 2),
    _wg_geo(1, (5, 1, 3), 2, (9, 1, 1)),             # G taken independently of P: Gw = 1 under Pw = 3
    _wg_geo(1, _conv_extent((5, 1, 1)), 2, (5, 1, 1)),  # P from G as the conv does: (3, 1, 1), Gw = 1
    _wg_geo(1, _conv_extent((5, 1, 3)), 2, (5, 1, 3)),  # (3, 1, 2)
    _wg_geo(1, (4, 33, 140), 1),                     # 18480 voxels: 10 range blocks in a grid padded to 16; the
                                                     # combine runs one full round of its 8 chains plus a tail
]
WG_DOUBLING = _wg_geo(1, (17, 241, 257), 1)          # 1,052,969 voxels: the first doubling of wgrad_vpb (> 512 * 2048)


def _wg_id(geo):
    b, p, g, s = geo
    return f"B{b}-P{'x'.join(map(str, p))}-G{'x'.join(map(str, g))}-s{s}"


def _wgrad_ref(dt, direct, gath, stride):
    """dW[k][a][b] = sum_p direct[p][a] * gathered_zero_padded[p*s - 1 + k][b], k = kd*9 + kh*3 + kw, as 27
    shifted slices of the zero-padded `gathered`; G is whatever `gath` has, independent of P"""
    B, Pd, Ph, Pw, A = direct.shape
    _, Gd, Gh, Gw, BC = gath.shape
    ext = [max(G, (P - 1) * stride + 2) + 1 for G, P in ((Gd, Pd), (Gh, Ph), (Gw, Pw))]
    gp = torch.zeros(B, *ext, BC, dtype=dt)
    gp[:, 1:1 + Gd, 1:1 + Gh, 1:1 + Gw] = gath.to(dt)  # padded index = gathered index + 1
    d = direct.to(dt).reshape(-1, A)
    dw = torch.empty(27, A, BC, dtype=dt)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                sl = gp[:, kd:kd + (Pd - 1) * stride + 1:stride, kh:kh + (Ph - 1) * stride + 1:stride,
                        kw:kw + (Pw - 1) * stride + 1:stride]
                dw[kd * 9 + kh * 3 + kw] = torch.einsum("pa,pb->ab", d, sl.reshape(-1, BC))
    return dw


def _wgrad_case(a, bc, geo, twice=False):
    b, p, g, stride = geo
    gen = _gen(a, bc, b, *p, *g, stride)
    direct = torch.randn(b, *p, a, generator=gen)
    gath = torch.randn(b, *g, bc, generator=gen)
    dd, gd = direct.to(DEV), gath.to(DEV)
    dw = ops.conv3d_wgrad(dd, gd, stride)
    if twice:
        assert torch.equal(_bits(dw), _bits(ops.conv3d_wgrad(dd, gd, stride)))  # fixed-order reduction
    r32, r64 = (_wgrad_ref(dt, direct, gath, stride) for dt in DTS)
    tag = f"conv3d_wgrad ({a},{bc}) {_wg_id(geo)}"
    _judge(tag, dw, r32, r64)
    # the taps that read the far border on their own (the k = 2 planes), and the centre tap
    far = torch.tensor([k for k in range(27) if k // 9 == 2 or (k // 3) % 3 == 2 or k % 3 == 2])
    if float(r64[far].abs().max()) > 0:
        _judge(tag + " [far-border taps]", dw.cpu()[far], r32[far], r64[far])
    _judge(tag + " [centre tap]", dw[13], r32[13], r64[13])


@pytest.mark.parametrize("geo", WG_BASE, ids=_wg_id)
@pytest.mark.parametrize("a,bc", WG_PAIRS)
def test_conv3d_wgrad_pairs(a, bc, geo):
    """All 12 dispatched (direct, gathered) channel pairs at the three base geometries."""
    _wgrad_case(a, bc, geo)


@pytest.mark.parametrize("geo", WG_EDGE, ids=_wg_id)
@pytest.mark.parametrize("a,bc", WG_EDGE_PAIRS)
def test_conv3d_wgrad_edges(a, bc, geo):
    """One voxel; one row of 63 / 65 voxels (one short of and one past a 64-row chunk); two batches of two
    voxels; a gathered width of 1; 18480 voxels (10 range blocks, 6 padding blocks, the combine's tail) --
    for a tile pair with zero-padded operands (8, 8), the largest tile (64, 64) and both taps-kernel pairs."""
    _wgrad_case(a, bc, geo)


@pytest.mark.parametrize("a,bc", [(8, 8), (8, 1), (1, 8)])
def test_conv3d_wgrad_block_doubles(a, bc):
    """1,052,969 voxels: the first size past 512 x 2048 voxels, where wgrad_vpb doubles to 4096."""
    _wgrad_case(a, bc, WG_DOUBLING)


@pytest.mark.parametrize("a,bc", [(32, 16), (8, 1)])
def test_conv3d_wgrad_repeats_bitwise(a, bc):
    """The matrix-core tile and the taps kernel, twice on the same inputs: the same bits."""
    _wgrad_case(a, bc, WG_BASE[2], twice=True)


# ---------------------------------------------------------------------------------------- conv3d_generic
CH3 = [1, 8, 16, 32, 64]
# (name, transposed, stride, output_padding)
MODES3 = [("conv-s1", False, 1, 0), ("conv-s2", False, 2, 0), ("deconv-s1", True, 1, 0), ("deconv-s2-even", True, 2, 1),
          ("deconv-s2-odd", True, 2, 0)]
GEO3 = [(2, 3, 5, 7), (1, 1, 6, 37)]  # (B, D, H, W) of the input; the second has depth 1 and an odd W


def _out_extent(n, transposed, stride, op):
    return (n - 1) * stride + 1 + op if transposed else (n - 1) // stride + 1


def _conv3d_ref(dt, x, wpk, transposed, stride, op):
    """x NDHWC, wpk [27][cout][cin] with tap = kd*9 + kh*3 + kw.
    strided:    y[o] = sum_k W[k] x[o*s - 1 + k]       = conv3d with weight[co][ci][kd][kh][kw] = W[k][co][ci]
    transposed: y[o] = sum_k W[k] x[(o + 1 - k) / s]   = conv_transpose3d with weight[ci][co][kd][kh][kw] = W[k][co][ci]"""
    cout, cin = wpk.shape[1:]
    xn = x.to(dt).permute(0, 4, 1, 2, 3)
    w5 = wpk.to(dt).reshape(3, 3, 3, cout, cin)
    if transposed:
        y = F.conv_transpose3d(xn, w5.permute(4, 3, 0, 1, 2), stride=stride, padding=1, output_padding=op)
    else:
        y = F.conv3d(xn, w5.permute(3, 4, 0, 1, 2), stride=stride, padding=1)
    return y.permute(0, 2, 3, 4, 1).contiguous()


def _conv3d_case(cin, cout, mode, geo, accumulate=False):
    name, transposed, stride, op = mode
    b, d, h, w = geo
    gen = _gen(cin, cout, MODES3.index(mode) + 1, b, d, h, w)
    x = torch.randn(b, d, h, w, cin, generator=gen)
    wpk = torch.randn(27, cout, cin, generator=gen)
    out_dhw = tuple(_out_extent(n, transposed, stride, op) for n in (d, h, w))
    tag = f"conv3d_generic {cin}->{cout} {name} in {b}x{d}x{h}x{w}"
    if accumulate:
        pre = torch.randn(b, *out_dhw, cout, generator=gen) * 3
        buf, out = _guarded((b, *out_dhw, cout), 1, pre)
        got = ops.conv3d_generic(x.to(DEV), wpk.to(DEV), cout, out_dhw, stride, transposed=transposed, out=out)
        assert got.data_ptr() == out.data_ptr()
        _assert_guard(buf, 1, b, tag + " (out=)")
        r32, r64 = (pre.to(dt) + _conv3d_ref(dt, x, wpk, transposed, stride, op) for dt in DTS)
        tag += " accumulate"
    else:
        got = ops.conv3d_generic(x.to(DEV), wpk.to(DEV), cout, out_dhw, stride, transposed=transposed)
        r32, r64 = (_conv3d_ref(dt, x, wpk, transposed, stride, op) for dt in DTS)
    _judge(tag, got, r32, r64)
    _judge(tag + " [last column]", got[:, :, :, -1], r32[:, :, :, -1], r64[:, :, :, -1])
    _judge(tag + " [last voxel]", got[-1, -1, -1, -1], r32[-1, -1, -1, -1], r64[-1, -1, -1, -1])
    if not accumulate and got.numel() >= 64:
        assert bool((got < 0).any()), "raw convolution: no ReLU"


@pytest.mark.parametrize("mode", MODES3, ids=[m[0] for m in MODES3])
@pytest.mark.parametrize("cout", CH3)
@pytest.mark.parametrize("cin", CH3)
def test_conv3d_generic(cin, cout, mode):
    """All 25 channel pairs, strided (Conv3d k3 p1) and transposed (ConvTranspose3d k3 p1) with stride 1 and
    2, against F.conv3d / F.conv_transpose3d. Transposed stride 2 both as out = 2 in (output_padding 1) and
    as out = 2 in - 1 (output_padding 0: the data gradient of a stride-2 conv on odd extents); W = 7 and 37
    give the even / odd column permutation an even (14, 74) and an odd (13, 73) Wo."""
    for geo in GEO3:
        _conv3d_case(cin, cout, mode, geo)


@pytest.mark.parametrize("mode", MODES3, ids=[m[0] for m in MODES3])
@pytest.mark.parametrize("cin,cout", [(1, 1), (8, 8), (64, 16), (16, 1)])
def test_conv3d_generic_single_column(cin, cout, mode):
    """An input one voxel wide: Wo = 1 (2 under the even transposed form), one pair per COB family."""
    _conv3d_case(cin, cout, mode, (2, 2, 3, 1))


@pytest.mark.parametrize("mode", [MODES3[1], MODES3[2], MODES3[4]], ids=[MODES3[i][0] for i in (1, 2, 4)])
@pytest.mark.parametrize("cin,cout", [(8, 1), (64, 16), (16, 32)])
def test_conv3d_generic_accumulate(cin, cout, mode):
    """out=: the result is the buffer's former content plus the convolution, for one pair of each COB family
    (cout == 1, cin == 64, the rest); the rows around the output keep their sentinel."""
    _conv3d_case(cin, cout, mode, GEO3[0], accumulate=True)


# ---------------------------------------------------------------------------------------- conv2d_generic
C2_PAIRS = ([(ci, co) for ci in (3, 8, 16, 27, 32) for co in (8, 16, 32)] +
            [(ci, co) for ci in (8, 16, 32) for co in (9, 27)])  # COB = 8, then COB = 9
C2_KP = [(1, 0), (3, 1), (5, 2), (7, 3)]
MODES2 = [("conv-s1", False, 1, 0), ("conv-s2", False, 2, 0), ("deconv-s1", True, 1, 0), ("deconv-s2-odd", True, 2, 0),
          ("deconv-s2-even", True, 2, 1)]
GEO2 = [(2, 5, 7), (1, 9, 70)]  # (B, H, W) of the input


def _conv2d_ref(dt, x, wt, bias, k, stride, pad, transposed, op):
    """x NHWC, wt [k*k][cout][cin] with tap = kh*k + kw.
    strided:    y[o] = b + sum_t W[t] x[o*s - pad + t]     = conv2d with weight[co][ci][kh][kw] = W[t][co][ci]
    transposed: y[i] = b + sum_t W[t] x[(i + pad - t) / s] = conv_transpose2d with weight[ci][co][kh][kw] = W[t][co][ci]"""
    cout, cin = wt.shape[1:]
    xn = x.to(dt).permute(0, 3, 1, 2)
    w4 = wt.to(dt).reshape(k, k, cout, cin)
    bb = None if bias is None else bias.to(dt)
    if transposed:
        y = F.conv_transpose2d(xn, w4.permute(3, 2, 0, 1), bb, stride=stride, padding=pad, output_padding=op)
    else:
        y = F.conv2d(xn, w4.permute(2, 3, 0, 1), bb, stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).contiguous()


def _conv2d_case(cin, cout, mode, kp, geo, with_bias, accumulate=False):
    name, transposed, stride, op = mode
    k, pad = kp
    b, h, w = geo
    gen = _gen(cin, cout, MODES2.index(mode) + 1, k, b, h, w, int(with_bias))
    x = torch.randn(b, h, w, cin, generator=gen)
    wt = torch.randn(k * k, cout, cin, generator=gen)
    bias = torch.randn(cout, generator=gen) * 4 if with_bias else None
    if transposed:
        out_hw = tuple((n - 1) * stride - 2 * pad + k + op for n in (h, w))
    else:
        out_hw = tuple((n + 2 * pad - k) // stride + 1 for n in (h, w))
    tag = f"conv2d_generic {cin}->{cout} {name} k{k} {'bias' if with_bias else 'nobias'} in {b}x{h}x{w}"
    d = lambda t: None if t is None else t.to(DEV)
    if accumulate:
        pre = torch.randn(b, *out_hw, cout, generator=gen) * 3
        buf, out = _guarded((b, *out_hw, cout), 1, pre)
        got = ops.conv2d_generic(d(x), d(wt), cout, out_hw, k, stride, pad, bias=d(bias), transposed=transposed, out=out)
        assert got.data_ptr() == out.data_ptr()
        _assert_guard(buf, 1, b, tag + " (out=)")
        r32, r64 = (pre.to(dt) + _conv2d_ref(dt, x, wt, bias, k, stride, pad, transposed, op) for dt in DTS)
        tag += " accumulate"
    else:
        got = ops.conv2d_generic(d(x), d(wt), cout, out_hw, k, stride, pad, bias=d(bias), transposed=transposed)
        r32, r64 = (_conv2d_ref(dt, x, wt, bias, k, stride, pad, transposed, op) for dt in DTS)
    _judge(tag, got, r32, r64)
    _judge(tag + " [last column]", got[:, :, -1], r32[:, :, -1], r64[:, :, -1])
    _judge(tag + " [last channel]", got[..., -1], r32[..., -1], r64[..., -1])


@pytest.mark.parametrize("cin,cout", C2_PAIRS)
def test_conv2d_generic(cin, cout):
    """The case list's rule: every (cin, cout) of the two families (cin in {3, 8, 16, 27, 32} x cout in
    {8, 16, 32}: COB = 8; cin in {8, 16, 32} x cout in {9, 27}: COB = 9) runs every mode (strided and
    transposed, stride 1 and 2, the transposed stride-2 form with an odd and an even out_hw) with every
    (k, pad) of (1, 0), (3, 1), (5, 2), (7, 3) at both geometries; the bias alternates, on where
    mode + k index + geometry index is even, so every pair, mode and k sees it on and off. Against F.conv2d /
    F.conv_transpose2d."""
    for mi, mode in enumerate(MODES2):
        for ki, kp in enumerate(C2_KP):
            for gi, geo in enumerate(GEO2):
                _conv2d_case(cin, cout, mode, kp, geo, (mi + ki + gi) % 2 == 0)


@pytest.mark.parametrize("mode", [MODES2[1], MODES2[3], MODES2[4]], ids=[MODES2[i][0] for i in (1, 3, 4)])
@pytest.mark.parametrize("cin,cout", [(3, 8), (27, 16), (32, 27)])
def test_conv2d_generic_accumulate(cin, cout, mode):
    """out=: former content + bias + convolution into a slice of a sentinel-filled buffer."""
    _conv2d_case(cin, cout, mode, (3, 1), GEO2[0], True, accumulate=True)
    _conv2d_case(cin, cout, mode, (5, 2), GEO2[0], False, accumulate=True)


# --------------------------------------------------------------------------------------------- BatchNorm
EPS = 1e-5
# A channel without variance (a constant one; every channel when nvox = 1) has alpha = gamma / sqrt(eps) = 316 gamma
# and the exact pre-activation beta, which fmaf(z, alpha, shift) returns with one rounding error of up to half an
# ulp of z alpha -- in the kernel and in the fp32 reference alike, which of the two is larger being chance. Such
# channels therefore hold small values (3 / 256; a single voxel is scaled by 2^-7), so that this error,
# <= 2^-24 * 316 * 1.5 * |z| <= 1.6e-6 for |z| <= 2^-4, is below the 1e-5 floor (|beta| >= 0.3) on both sides.
CONST = 3.0 / 256
BN_C = [1, 2, 4, 8, 16, 32, 64, 256]


def _bn_nvox(C):
    """rs = 256 / C rows per step: the list walks the pair of 4-row groups and the scalar tail loop"""
    rs = 256 // C
    full = [1, rs - 1, 4 * rs - 1, 4 * rs, 4 * rs + 1, 8 * rs + 1, 12 * rs + 3, 1023, 1024, 1025, 2049 + rs]
    some = [1, 4 * rs + 1, 1025, 2049 + rs]
    return sorted({max(n, 1) for n in (full if C in (8, 64) else some)})


BN_CASES = [(C, n) for C in BN_C for n in _bn_nvox(C)]


def _bn_pre(z, gamma, beta):
    """fp64: the pre-activation y = z alpha + shift of the batch statistics, and tau (module docstring)"""
    z64, g64, b64 = z.double(), gamma.double(), beta.double()
    mean = z64.mean(0)
    var = ((z64 - mean) ** 2).mean(0)
    alpha = g64 / torch.sqrt(var + EPS)
    shift = b64 - mean * alpha
    y = z64 * alpha + shift
    tau = 4 * 8 * 2.0 ** -23 * ((z64 * alpha).abs() + (mean * alpha).abs() + b64.abs())
    return y, tau, alpha, shift


def _bn_condition(z, gamma, beta):
    """Move every z whose pre-activation is within tau of 0 to +-2 tau; the statistics move with it, so
    repeat (one pass is enough for every case of this file). Returns min |y| / tau of the final inputs."""
    for _ in range(4):
        y, tau, alpha, shift = _bn_pre(z, gamma, beta)
        bad = y.abs() < tau
        if not bool(bad.any()):
            break
        target = torch.where(y < 0, -2 * tau, 2 * tau)
        z[bad] = ((target - shift) / alpha)[bad].float()
    y, tau, _, _ = _bn_pre(z, gamma, beta)
    return float((y.abs() / tau).min())


def _bn_inputs(nvox, C, *seed, special=None, scale=1.0, offset=0.0):
    """z [nvox][C] with per-channel spreads in [0.5, 2) and offsets; gamma in +-[0.5, 1.5), |beta| in [0.3, 1.3)
    (a constant channel's pre-activation is beta); group `scale` / `offset` for the grouped forms. With C >= 4, channel 0 is constant (variance 0), channel 1
    has mean = 8 std and channel 2 a negative gamma; C < 4 puts `special` on the last channel."""
    g = _gen(nvox, C, *seed)
    std = torch.rand(C, generator=g) * 1.5 + 0.5
    mu = torch.randn(C, generator=g)
    z = (torch.randn(nvox, C, generator=g) * std + mu) * scale + offset
    gamma = torch.rand(C, generator=g) + 0.5
    beta = (torch.rand(C, generator=g) + 0.3) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    where = {"const": 0, "mean8": 1, "neg": 2} if C >= 4 else ({special: C - 1} if special else {})
    for kind, c in where.items():
        if kind == "const":
            z[:, c] = CONST * scale
        elif kind == "mean8":
            r = torch.randn(nvox, generator=g, dtype=torch.float64)
            if nvox > 1:  # exactly 8 sample deviations, whatever the sample
                r = (r - r.mean()) / r.var(unbiased=False).sqrt()
            z[:, c] = ((r + 8.0) * float(std[c]) * scale).float()
        else:
            gamma[c] = -gamma[c]
    if nvox == 1:
        z *= 2.0 ** -7
    dy = torch.randn(nvox, C, generator=g)
    skip = torch.randn(nvox, C, generator=g)
    ratio = _bn_condition(z, gamma, beta)
    assert ratio >= 1.0, ("a pre-activation within tau of 0", nvox, C, ratio)  # on the CPU, before any GPU call
    return z, dy, skip, gamma, beta, where


def _bn_ref(dt, z, dy, skip, gamma, beta):
    """From the definition -> mean, var (biased), y, y + skip, dz, dgamma, dbeta"""
    z, dy, skip, gamma, beta = (t.to(dt) for t in (z, dy, skip, gamma, beta))
    n = z.shape[0]
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + EPS)
    alpha = gamma * rstd
    pre = z * alpha + (beta - mean * alpha)
    y = torch.relu(pre)
    xhat = (z - mean) * rstd
    g = torch.where(pre > 0, dy, torch.zeros_like(dy))
    dbeta = g.sum(0)
    dgamma = (g * xhat).sum(0)
    dz = alpha / n * (n * g - dbeta - xhat * dgamma)
    return mean, var, y, skip + y, dz, dgamma, dbeta


def _judge_cols(tag, got, r32, r64, where, const_alone=True):
    """[nvox][C] results: all of it, then the special channels and the ordinary ones on their own (a constant
    channel's dz is 1 / sqrt(eps) times the others' and would set the scale for all of them)"""
    _judge(tag, got, r32, r64)
    if got.shape[0] > 3:
        _judge(tag + " [last 3 rows]", got[-3:], r32[-3:], r64[-3:])
    if not where:
        return
    rest = torch.tensor([c for c in range(got.shape[1]) if c not in where.values()])
    gc = got.cpu()
    for kind, c in where.items():
        if float(r64[:, c].abs().max()) > 0 and (const_alone or kind != "const"):
            _judge(f"{tag} [{kind} channel]", gc[:, c], r32[:, c], r64[:, c])
    if len(rest):
        _judge(tag + " [ordinary channels]", gc[:, rest], r32[:, rest], r64[:, rest])


def _bn_case(nvox, C, special=None):
    z, dy, skip, gamma, beta, where = _bn_inputs(nvox, C, 1, special=special)
    zd, dyd, sd, gd, bd = (t.to(DEV) for t in (z, dy, skip, gamma, beta))
    r32, r64 = (_bn_ref(dt, z, dy, skip, gamma, beta) for dt in DTS)
    tag = f"bn C={C} nvox={nvox}" + (f" {special}" if special else "")

    mean, var = ops.bn_stats(zd)
    mean2, var2 = ops.bn_stats(zd)
    assert torch.equal(_bits(mean), _bits(mean2)) and torch.equal(_bits(var), _bits(var2))  # fixed-order reduction
    _judge(tag + " mean", mean, r32[0], r64[0])
    # the variance is judged through rstd = 1 / sqrt(var + eps), the only form in which any kernel uses it (a
    # constant channel's variance is an exact 0 on both sides)
    rs = lambda v: 1.0 / torch.sqrt(v.double().cpu() + EPS)
    _judge(tag + " rstd(var)", rs(var), rs(r32[1]), rs(r64[1]))
    _judge(tag + " var", var, r32[1], r64[1])

    y = ops.bn_relu_train(zd, mean, var, gd, bd, EPS)
    _judge_cols(tag + " y", y, r32[2], r64[2], where, const_alone=False)  # (there y is beta or 0)
    assert torch.equal(y.cpu() == 0, r64[2] == 0)  # exactly the masked entries are zeros
    ys = ops.bn_relu_train(zd, mean, var, gd, bd, EPS, skip=sd)
    _judge_cols(tag + " y+skip", ys, r32[3], r64[3], where, const_alone=False)
    assert torch.equal(sd.cpu(), skip) and torch.equal(zd.cpu(), z)  # inputs are read, never written
    buf, out = _guarded((nvox, C), 2)
    got = ops.bn_relu_train(zd, mean, var, gd, bd, EPS, skip=sd, out=out)
    assert got.data_ptr() == out.data_ptr()
    _assert_guard(buf, 2, nvox, "bn_relu_train(out=)")
    assert torch.equal(_bits(out), _bits(ys))

    dz, dg, db = ops.bn_relu_backward(dyd, zd, mean, var, gd, bd, EPS)
    buf, dzo = _guarded((nvox, C), 2)
    dz2, dg2, db2 = ops.bn_relu_backward(dyd, zd, mean, var, gd, bd, EPS, dz=dzo)
    assert dz2.data_ptr() == dzo.data_ptr()
    _assert_guard(buf, 2, nvox, "bn_relu_backward(dz=)")
    assert torch.equal(_bits(dg), _bits(dg2)) and torch.equal(_bits(db), _bits(db2))  # fixed-order reduction
    assert torch.equal(_bits(dz), _bits(dzo))
    _judge_cols(tag + " dz", dz, r32[4], r64[4], where)
    _judge(tag + " dgamma", dg, r32[5], r64[5])
    _judge(tag + " dbeta", db, r32[6], r64[6])
    if where and C >= 4:  # a constant channel's dgamma is an exact 0; the others on their own
        rest = torch.tensor([c for c in range(C) if c != where["const"]])
        _judge(tag + " dgamma [non-constant channels]", dg.cpu()[rest], r32[5][rest], r64[5][rest])
    return z, dy, skip, gamma, beta


@pytest.mark.parametrize("C,nvox", BN_CASES)
def test_bn_stats_train_backward(C, nvox):
    """bn_stats, bn_relu_train (without skip, with skip, with out=) and bn_relu_backward (with and without dz=)
    against the definition. rs = 256 / C rows per step; nvox walks the hand-unrolled pair of 4-row groups and
    its scalar tail (rs - 1, 4 rs - 1, 4 rs, 4 rs + 1, 8 rs + 1, 12 rs + 3) and the 1024-row block (1023,
    1024, 1025, 2049 + rs). C = 1 and 2 take the scalar apply kernels, the rest the float4 ones. With
    C >= 4, channel 0 is constant (variance 0, beta != 0), channel 1 has mean = 8 std, channel 2 a negative gamma."""
    _bn_case(nvox, C)


@pytest.mark.parametrize("special", ["const", "mean8", "neg"])
@pytest.mark.parametrize("C", [1, 2])
def test_bn_special_channel_scalar_path(C, special):
    """The constant, mean = 8 std and negative-gamma channels on the scalar apply path."""
    _bn_case(4 * (256 // C) + 1, C, special=special)


@pytest.mark.parametrize("C", [1, 4])
def test_bn_block_doubles(C):
    """nvox = 4096 * 1024 + 1: the first size at which bn_vpb doubles to 2048 rows per block, on the scalar
    (C = 1, 17 MB) and the float4 (C = 4, 67 MB) apply path."""
    _bn_case(4096 * 1024 + 1, C)


def _offset_by_one_float(t):
    """the same values in a tensor that starts 4 bytes into a larger buffer: not 16-byte aligned"""
    buf = torch.empty(t.numel() + 8, device=DEV)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("C,nvox", [(4, 257), (8, 129), (8, 1025), (64, 17), (64, 2053), (256, 5), (256, 1025)])
def test_bn_float4_and_scalar_paths_agree_bitwise(C, nvox):
    """The same z, dy and skip once in 16-byte aligned tensors (the float4 apply kernels) and once in tensors
    that start 4 bytes into a larger buffer (the scalar ones): y, dz, mean, var, dgamma, dbeta agree bit for bit."""
    z, dy, skip, gamma, beta, _ = _bn_inputs(nvox, C, 2)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    res = []
    for place in (lambda t: t.to(DEV), _offset_by_one_float):
        zd, dyd, sd = place(z), place(dy), place(skip)
        assert (zd.data_ptr() % 16 == 0) == (len(res) == 0)
        mean, var = ops.bn_stats(zd)
        y = ops.bn_relu_train(zd, mean, var, gd, bd, EPS, skip=sd)
        out = place(torch.zeros(nvox, C))
        ops.bn_relu_train(zd, mean, var, gd, bd, EPS, out=out)
        dzo = place(torch.zeros(nvox, C))
        dz, dg, db = ops.bn_relu_backward(dyd, zd, mean, var, gd, bd, EPS, dz=dzo)
        res.append((mean, var, y, out, dz, dg, db))
    for name, a, b in zip(("mean", "var", "y + skip", "y (out=)", "dz", "dgamma", "dbeta"), *res):
        assert torch.equal(_bits(a), _bits(b)), name
    r32, r64 = (_bn_ref(dt, z, dy, skip, gamma, beta) for dt in DTS)
    _judge(f"bn unaligned C={C} nvox={nvox} y+skip", res[1][2], r32[3], r64[3])
    _judge(f"bn unaligned C={C} nvox={nvox} dz [ordinary channels]", res[1][4][:, 3:], r32[4][:, 3:], r64[4][:, 3:])


@pytest.mark.parametrize("nvox_kind", ["1", "4rs+1", "1025"])
@pytest.mark.parametrize("C", [8, 16, 32])
@pytest.mark.parametrize("G", [1, 2, 3, 5])
def test_bn_grouped(G, C, nvox_kind):
    """The grouped forms (independent statistics of G consecutive [nvox][C] slabs, one gamma / beta): each
    group against the definition, dgamma / dbeta added over the groups. The groups differ strongly (group g is
    scaled by 1 + g and shifted by 3 g), so another group's statistics are far off. G = 1 equals the ungrouped
    op bit for bit; every group's mean, var, y, dz equal, bit for bit, the ungrouped op on that slab alone."""
    nvox = {"1": 1, "4rs+1": 4 * (256 // C) + 1, "1025": 1025}[nvox_kind]
    gamma = beta = None
    zs, dys, refs = [], [], []
    for gi in range(G):
        z, dy, skip, ga, be, where = _bn_inputs(nvox, C, 3, gi, scale=1.0 + gi, offset=3.0 * gi)
        if gamma is None:
            gamma, beta = ga, be
        else:  # one gamma / beta for all groups: condition this group's z for them
            assert _bn_condition(z, gamma, beta) >= 1.0
        zs.append(z)
        dys.append(dy)
    for gi in range(G):
        refs.append([_bn_ref(dt, zs[gi], dys[gi], dys[gi], gamma, beta) for dt in DTS])
    zd, dyd = torch.stack(zs).to(DEV), torch.stack(dys).to(DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    mean, var = ops.bn_stats_grouped(zd)
    y = ops.bn_relu_train_grouped(zd, mean, var, gd, bd, EPS)
    dz, dg, db = ops.bn_relu_backward_grouped(dyd, zd, mean, var, gd, bd, EPS)
    assert mean.shape == (G, C) and var.shape == (G, C) and y.shape == zd.shape and dz.shape == zd.shape
    tag = f"bn grouped G={G} C={C} nvox={nvox}"
    for gi in range(G):
        (r32, r64), t = refs[gi], f"{tag} [group {gi}]"
        _judge(t + " mean", mean[gi], r32[0], r64[0])
        _judge(t + " var", var[gi], r32[1], r64[1])
        _judge_cols(t + " y", y[gi], r32[2], r64[2], where, const_alone=False)
        _judge_cols(t + " dz", dz[gi], r32[4], r64[4], where)
        # the ungrouped op on this slab alone: the same bits
        m1, v1 = ops.bn_stats(zd[gi])
        y1 = ops.bn_relu_train(zd[gi], m1, v1, gd, bd, EPS)
        dz1, dg1, db1 = ops.bn_relu_backward(dyd[gi], zd[gi], m1, v1, gd, bd, EPS)
        for name, a, b in (("mean", mean[gi], m1), ("var", var[gi], v1), ("y", y[gi], y1), ("dz", dz[gi], dz1)):
            assert torch.equal(_bits(a), _bits(b)), (t, name)
        if G == 1:
            assert torch.equal(_bits(dg), _bits(dg1)) and torch.equal(_bits(db), _bits(db1))
    for i, (name, got) in ((5, ("dgamma", dg)), (6, ("dbeta", db))):
        r32 = sum(refs[gi][0][i] for gi in range(G))
        r64 = sum(refs[gi][1][i] for gi in range(G))
        _judge(f"{tag} {name}", got, r32, r64)
        rest = torch.arange(1, C)  # without the constant channel
        _judge(f"{tag} {name} [non-constant channels]", got.cpu()[rest], r32[rest], r64[rest])
    dz2, dg2, db2 = ops.bn_relu_backward_grouped(dyd, zd, mean, var, gd, bd, EPS)
    assert torch.equal(_bits(dg), _bits(dg2)) and torch.equal(_bits(db), _bits(db2)) and torch.equal(_bits(dz), _bits(dz2))


# ----------------------------------------------------------------------------------- what the wrappers refuse
def test_wrappers_refuse_sizes_the_entry_points_would_misread():
    """The entry points take one batch size, one channel count and one element count for all their tensors; a
    tensor of another size would be read (or written) past its end, so the wrappers raise before any launch."""
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    with pytest.raises(ValueError, match="same batch"):
        ops.conv3d_wgrad(z(2, 2, 3, 5, 8), z(1, 2, 3, 5, 8), 1)
    with pytest.raises(ValueError, match="same batch"):
        ops.conv2d_wgrad(z(2, 3, 5, 8), z(1, 3, 5, 8), 3, 1, 1)
    with pytest.raises(ValueError, match="w_packed"):
        ops.conv3d_generic(z(1, 2, 3, 5, 8), z(27, 8, 8), 16, (2, 3, 5), 1)
    with pytest.raises(ValueError, match="out must"):
        ops.conv3d_generic(z(1, 2, 3, 5, 8), z(27, 8, 8), 8, (2, 3, 5), 1, out=z(1, 2, 3, 4, 8))
    with pytest.raises(ValueError, match="w_taps"):
        ops.conv2d_generic(z(1, 3, 5, 8), z(9, 8, 8), 16, (3, 5), 3, 1, 1)
    with pytest.raises(ValueError, match="w_taps"):
        ops.conv2d_generic(z(1, 3, 5, 8), z(9, 8, 8), 8, (3, 5), 5, 1, 2)
    with pytest.raises(ValueError, match="bias"):
        ops.conv2d_generic(z(1, 3, 5, 8), z(9, 16, 8), 16, (3, 5), 3, 1, 1, bias=z(8))
    with pytest.raises(ValueError, match="out must"):
        ops.conv2d_generic(z(1, 3, 5, 8), z(9, 8, 8), 8, (3, 5), 3, 1, 1, out=z(1, 3, 4, 8))
    v8, v4, x = z(8), z(4), z(5, 8)
    for bad in range(4):
        stats = [v8, v8, v8, v8]
        stats[bad] = v4
        with pytest.raises(ValueError, match="must hold 8 floats"):
            ops.bn_relu_train(x, *stats, EPS)
        with pytest.raises(ValueError, match="must hold 8 floats"):
            ops.bn_relu_backward(x, x, *stats, EPS)
    with pytest.raises(ValueError, match="skip must have z's size"):
        ops.bn_relu_train(x, v8, v8, v8, v8, EPS, skip=z(4, 8))
    with pytest.raises(ValueError, match="out must have z's size"):
        ops.bn_relu_train(x, v8, v8, v8, v8, EPS, out=z(4, 8))
    with pytest.raises(ValueError, match="dy must have z's size"):
        ops.bn_relu_backward(z(4, 8), x, v8, v8, v8, v8, EPS)
    with pytest.raises(ValueError, match="dz must have z's size"):
        ops.bn_relu_backward(x, x, v8, v8, v8, v8, EPS, dz=z(4, 8))
    xg = z(3, 5, 8)
    with pytest.raises(ValueError, match="mean must hold 24 floats"):
        ops.bn_relu_train_grouped(xg, v8, z(3, 8), v8, v8, EPS)
    with pytest.raises(ValueError, match="var must hold 24 floats"):
        ops.bn_relu_backward_grouped(xg, xg, z(3, 8), v8, v8, v8, EPS)
    with pytest.raises(ValueError, match="dy must have z's size"):
        ops.bn_relu_backward_grouped(z(2, 5, 8), xg, z(3, 8), z(3, 8), v8, v8, EPS)
