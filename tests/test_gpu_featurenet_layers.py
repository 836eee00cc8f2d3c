"""The FeatureNet inference kernels (csrc/featurenet.hip, csrc/conv2d.hip), entry by entry, at the unit tails,
sampling edges and walks that tests/test_gpu_featurenet.py and the whole-network tests never reach: images of
1 x 1 and of exactly one unit, one row or column more and less than a unit, widths and heights below the 5 x 5
kernel of the stride-2 layers, batches whose unit counts are 1, below 8 and no multiple of the 8 XCDs, every
epilogue (bias / BN with negative alphas / ReLU) and output layout, DCN samples on the last corner of the LDS
window and one past it, exactly on the image border, far past the offset clamp, under saturated masks, and the
steady-state walk of the persistent kernels (a workgroup computing on a unit that fetch() staged during the
walk, not before it).

  tmvs_deform_conv2d       dcn_window_kernel<CO, false>          unit 12 rows x 16 pixels, halo 3, persistent
  tmvs_dcn_fused           dcn_window_kernel<CO, true>
  tmvs_dcn_forward_train   dcn_window_kernel<CO, true> with offset_mask_out
  tmvs_conv3x3_nhwc(_acc)  conv3x3_window_kernel                 unit 8 x 16, halo 1, persistent
  tmvs_conv2d_bn_relu      conv2d_bn_relu_kernel, 7 instances    unit 8 x 16 output pixels, persistent
  tmvs_fpn_merge           fpn_merge_kernel<8 / 16>              4 lanes per pixel, 64 pixels per block

Every reference is plain torch on the CPU (F.conv2d; oracle.transmvs_ref.deform_conv2d, one sample at a time;
F.interpolate(nearest) + a 1 x 1 conv), evaluated in fp32 and in fp64 with every operand in that type. Error =
max|got - ref64| / max|ref64|; the bar is err_gpu <= max(2 x err_fp32ref, 1e-5) (tests/_primitives.py), on the
whole output and, for B > 1, on the last sample on its own scale. Outputs are contiguous slices of larger
buffers whose other rows hold a sentinel that must survive bit for bit (a pixel the kernel leaves unwritten
keeps the sentinel and fails the comparison); x, the given offset_mask, prev and lat are slices of buffers
whose other rows are NaN and whose bits must be unchanged after the launch. The guarded launches go through
ops._launch with the wrapper's own argument order; once per entry the public wrapper must return the same bits.

Measured on an MI355X, worst (err_gpu, err_fp32ref) over all cases of an entry: tmvs_deform_conv2d (1.6e-6,
1.3e-6), tmvs_conv2d_bn_relu (9.9e-7, 9.9e-7), tmvs_conv3x3_nhwc (7.7e-7, 3.3e-7), tmvs_conv3x3_nhwc_acc (5.5e-7,
3.0e-7), tmvs_fpn_merge (1.4e-7, 1.7e-7), offset_mask_out (7.1e-7, 2.9e-7); tmvs_dcn_fused and
tmvs_dcn_forward_train (2.0e-6, 1.6e-6) and (1.8e-6, 1.6e-6) up to 25 x 33, (3.1e-5, 3.1e-5) and (4.1e-5, 4.1e-5)
in the 100 x 920 walk. There the error is the fp32 sample position's own rounding, which the fp32 reference shares
(px = column + offset has an ulp of 6e-5 px near column 900; the unfused walk's dyadic offsets are exact: (4.8e-7,
3.2e-7)), so the bar is 2 x err_fp32ref in the eight comparisons of those two cases and the 1e-5 floor everywhere
else. No class needed a floor of its own: the saturated masks (+-30, -100 through __expf / __frcp_rn) came to
(4.7e-7, 2.5e-7). Before the unfused kernel kept a unit's offset / mask logits apart from the prefetched ones, the
tmvs_deform_conv2d walk failed with err_gpu = 0.71. 160 tests, about 8 s.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import transmvs_ref as oracle
from tests._primitives import DEV, _assert_guard, _bits, _gen, _guarded, _judge
from transmvsnet_amd import ops

pytestmark = pytest.mark.gpu
DTS = (torch.float32, torch.float64)
NAN = float("nan")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


class _Input:
    """the CPU tensor `t` on the device between one NaN row (one sample's size) on either side"""

    def __init__(self, t):
        self.cpu = t.contiguous()
        self.buf = torch.full((t.shape[0] + 2, *t.shape[1:]), NAN, device=DEV)
        self.view = self.buf[1:1 + t.shape[0]]
        self.view.copy_(self.cpu)
        assert self.view.is_contiguous()
        self.intact("before the launch")

    def intact(self, tag):
        assert torch.equal(_bits(self.view), _bits(self.cpu)), tag + ": an input was written"
        assert bool(torch.isnan(self.buf[0]).all()) and bool(torch.isnan(self.buf[-1]).all()), tag


def _out(shape, want=True, fill=None):
    """(buffer, view) of a sentinel-guarded output, or (None, None)"""
    return _guarded(tuple(shape), 1, fill) if want else (None, None)


def _bn(gen, cout):
    """alpha in [0.5, 1.5) with every fourth channel negated, shift = 0.5 randn"""
    alpha = torch.rand(cout, generator=gen) + 0.5
    alpha[1::4] = -alpha[1::4]
    return alpha, 0.5 * torch.randn(cout, generator=gen)


def _epilogue(y, bn, relu):
    """(result, pre-activation) of the NCHW `y` in its own dtype"""
    if bn is not None:
        y = y * bn[0].to(y.dtype).view(1, -1, 1, 1) + bn[1].to(y.dtype).view(1, -1, 1, 1)
    return (torch.relu(y) if relu else y), y


def _relu_cuts(pre, tag):
    """the ReLU clips a share of the outputs and lets a share through"""
    assert bool((pre < 0).any()) and bool((pre > 0).any()), tag


def _judge_all(tag, got, r32, r64):
    _judge(tag, got, r32, r64)
    if got.shape[0] > 1:  # the last sample on its own scale
        _judge(tag + " [last sample]", got[-1], r32[-1], r64[-1])


def _dev(t):
    return None if t is None else t.to(DEV)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ============================================================================ the DCN: references and launches
DEFORM, FUSED, TRAIN = "tmvs_deform_conv2d", "tmvs_dcn_fused", "tmvs_dcn_forward_train"
DCN_ENTRIES = (DEFORM, FUSED, TRAIN)
DCN_ROWS, DCN_HALO, TW = 12, 3, 16  # the DCN unit: 12 rows x 16 pixels, window margin 3


def _dcn_units(b, h, w):
    """the launcher's own formula (dcn_launch)"""
    return b * -(-h // DCN_ROWS) * -(-w // TW)


def _dcn_refs(x, weight, bias, om=None, wom=None, bom=None):
    """[(deform_conv2d + bias NCHW, offset_mask) in fp32, the same in fp64], one sample at a time (the oracle's
    column tensor is 288 x H W per sample); offset_mask is `om`, or conv_offset_mask(x) in the same dtype"""
    refs = []
    for dt in DTS:
        ys, oms = [], []
        for s in range(x.shape[0]):
            xs = x[s:s + 1].to(dt)
            o = om[s:s + 1].to(dt) if om is not None else F.conv2d(xs, wom.to(dt), bom.to(dt), padding=1)
            ys.append(oracle.deform_conv2d(xs, o[:, :18], weight.to(dt), bias.to(dt), 1, torch.sigmoid(o[:, 18:])))
            oms.append(o)
        refs.append((torch.cat(ys), torch.cat(oms)))
    return refs


class _Dcn:
    """the device side of one DCN case"""

    def __init__(self, entry, x, weight, bias, om=None, wom=None, bom=None):
        self.entry, self.cout = entry, weight.shape[0]
        self.b, _, self.h, self.w = x.shape
        self.x = _Input(_nhwc(x))
        self.wpk, self.bias = ops.deform_conv2d_pack(weight).to(DEV), bias.to(DEV)
        if entry == DEFORM:
            self.om = _Input(om)
        else:
            self.wom, self.bom = ops.deform_conv2d_pack(wom).to(DEV), bom.to(DEV)

    def launch(self, bn, relu, layout, tag):
        """one guarded direct launch -> (out NCHW, out NHWC, offset_mask_out), None where not asked for"""
        b, h, w, cout = self.b, self.h, self.w, self.cout
        obuf, out = _out((b, cout, h, w), layout in ("nchw", "both"))
        nbuf, onh = _out((b, h, w, cout), layout in ("nhwc", "both"))
        mbuf, omo = _out((b, 27, h, w), self.entry == TRAIN)
        alpha, shift = (_dev(bn[0]), _dev(bn[1])) if bn is not None else (None, None)
        if self.entry == DEFORM:
            ops._launch(DEFORM, self.x.view, self.om.view, self.wpk, self.bias, alpha, shift, int(relu), b, 32, cout,
                        h, w, out, onh)
        elif self.entry == FUSED:
            ops._launch(FUSED, self.x.view, self.wom, self.bom, self.wpk, self.bias, alpha, shift, int(relu), b, 32,
                        cout, h, w, out, onh)
        else:
            assert bn is None and not relu
            ops._launch(TRAIN, self.x.view, self.wom, self.bom, self.wpk, self.bias, b, 32, cout, h, w, out, onh, omo)
        for buf in (obuf, nbuf, mbuf):
            if buf is not None:
                _assert_guard(buf, 1, b, tag)
        self.x.intact(tag)
        if self.entry == DEFORM:
            self.om.intact(tag)
        return out, onh, omo

    def check(self, refs, bn, relu, layout, tag):
        (y32, om32), (y64, om64) = refs
        tag = f"{self.entry} cout {self.cout} B {self.b} {self.h}x{self.w} {tag} bn={int(bn is not None)} " \
              f"relu={int(relu)} {layout}"
        (r32, _), (r64, pre) = _epilogue(y32, bn, relu), _epilogue(y64, bn, relu)
        if relu:
            _relu_cuts(pre, tag)
        out, onh, omo = self.launch(bn, relu, layout, tag)
        if out is not None:
            _judge_all(tag + " -> nchw", out, r32, r64)
        if onh is not None:
            _judge_all(tag + " -> nhwc", onh, _nhwc(r32), _nhwc(r64))
        if omo is not None:
            _judge_all(tag + " -> offset_mask_out", omo, om32, om64)


def _dcn_variants(entry):
    """(bn, relu, layout): the unfused entry needs `out`; the training entry has no BN / ReLU"""
    if entry == TRAIN:
        return [(False, False, lay) for lay in ("nhwc", "both", "nchw")]
    layouts = ("nchw", "both") if entry == DEFORM else ("nchw", "nhwc", "both")
    return [(bn, relu, lay) for bn in (False, True) for relu in (False, True) for lay in layouts]


def _dcn_weight(gen, cout):
    return torch.randn(cout, 32, 3, 3, generator=gen) * 0.06, torch.randn(cout, generator=gen) * 0.1


# ----------------------------------------------------------------------------------------- 1. unit tails: the DCN
# (H, W): 1 x 1, exactly one unit, one row and column more (4 units, the second band and step 1 wide), one less,
# two units and one row / column (9 units), a single column (the min(r & 15, W - 1 - x0t) clamps)
DCN_HW = [(1, 1), (12, 16), (13, 17), (11, 15), (25, 33), (13, 1)]
DCN_B = (1, 2, 3)
_UNITS = sorted({_dcn_units(b, h, w) for b in DCN_B for h, w in DCN_HW})
# launched unit counts (= workgroups, all below the resident grid): 1, counts below 8, and counts that are no
# multiple of 8 (xcd_remap with nblk & 7 != 0, the b decode)
assert _UNITS == [1, 2, 3, 4, 6, 8, 9, 12, 18, 27], _UNITS


@pytest.mark.parametrize("hw", DCN_HW, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("cout", [8, 16, 32])
@pytest.mark.parametrize("entry", DCN_ENTRIES)
def test_dcn_unit_tails(entry, cout, hw):
    """The three DCN entries at cout 8 (one MFMA tile: the two-chain `alt` path), 16 and 32, B = 1, 2, 3, every
    epilogue and layout the entry takes: no BN / BN with every fourth alpha negative, ReLU on and off, NCHW only,
    NHWC only (out == NULL, fused and training entries) and both; the training entry's offset_mask_out against
    conv_offset_mask. Offsets of a few pixels (unfused: 2.5 randn with a patch of exact zeros; fused: a 0.05
    randn conv with 0.5 randn biases), so samples straddle the window and leave the image."""
    h, w = hw
    for b in DCN_B:
        gen = _gen(DCN_ENTRIES.index(entry), cout, h, w, b)
        x = torch.randn(b, 32, h, w, generator=gen)
        weight, bias = _dcn_weight(gen, cout)
        if entry == DEFORM:
            om = torch.randn(b, 27, h, w, generator=gen)
            om[:, :18] *= 2.5
            om[0, :18, :3, :3] = 0.0
            kw = dict(om=om)
        else:
            kw = dict(wom=torch.randn(27, 32, 3, 3, generator=gen) * 0.05, bom=torch.randn(27, generator=gen) * 0.5)
        refs = _dcn_refs(x, weight, bias, **kw)
        bn = _bn(gen, cout)
        case = _Dcn(entry, x, weight, bias, **kw)
        for use_bn, relu, layout in _dcn_variants(entry):
            case.check(refs, bn if use_bn else None, relu, layout, "tails")


# ------------------------------------------------------------------------------------- 2. the DCN's sampling edges
def _dcn_geometry(om, h, w):
    """Where the samples of an offset_mask tensor fall, in fp64, by the kernel's own rules: py, px [B, 9, H, W];
    inside (the image, torchvision's rule); ry, rx = the sample's upper left corner relative to its unit's
    window, in the window for 0 <= ry <= 16 and 0 <= rx <= 20 (both corners of the 18 x 22 window); fast
    [B, H, steps] = every sample of the wave (row, 16-pixel step) in the window or outside the image."""
    om = om.double()
    b = om.shape[0]
    k = torch.arange(9)
    rows, cols = torch.arange(h).view(1, 1, h, 1), torch.arange(w).view(1, 1, 1, w)
    py = rows + (k // 3).view(1, 9, 1, 1) - 1 + om[:, 0:18:2]
    px = cols + (k % 3).view(1, 9, 1, 1) - 1 + om[:, 1:18:2]
    inside = (py > -1) & (py < h) & (px > -1) & (px < w)
    ry = torch.floor(py) - (rows // DCN_ROWS * DCN_ROWS - DCN_HALO)
    rx = torch.floor(px) - (cols // TW * TW - DCN_HALO)
    rowin = (ry >= 0) & (ry <= DCN_ROWS + 2 * DCN_HALO - 2)
    colin = (rx >= 0) & (rx <= TW + 2 * DCN_HALO - 2)
    lane = ((rowin & colin) | ~inside).all(dim=1)
    steps = -(-w // TW)
    lane = F.pad(lane, (0, steps * TW - w), value=True)
    return dict(py=py, px=px, inside=inside, ry=ry, rx=rx, rowin=rowin, colin=colin,
                fast=lane.view(b, h, steps, TW).all(dim=-1))


def _eighths(gen, shape, most=7):
    """dyadic offsets k / 8, |k| <= most: fp32 and fp64 agree exactly on every position, floor and `inside`"""
    return torch.randint(-most, most + 1, shape, generator=gen).float() / 8


def _om_all_fast(gen, b, h, w):
    om = torch.randn(b, 27, h, w, generator=gen)
    om[:, :18] = _eighths(gen, (b, 18, h, w))
    g = _dcn_geometry(om, h, w)
    assert float(om[:, :18].abs().max()) < 1 and bool(g["fast"].all())
    return om


def _om_all_fallback(gen, b, h, w):
    """every wave has a sample inside the image whose corner is past its window: the pixel at the step's right
    edge looks 4 to 5 1/8 px right through the centre tap, the pixel at its left edge as far left through tap 3"""
    om = torch.randn(b, 27, h, w, generator=gen)
    om[:, :18] = _eighths(gen, (b, 18, h, w))
    far = torch.tensor([4.0, 4.5, 5.125])
    for sign, col0, tap in ((1.0, TW - 1, 4), (-1.0, TW, 3)):
        n = len(range(col0, w, TW))
        om[:, 2 * tap + 1, :, col0::TW] = sign * far[torch.randint(0, 3, (b, h, n), generator=gen)]
    g = _dcn_geometry(om, h, w)
    assert not bool(g["fast"].any())
    steps = -(-w // TW)
    mx = F.pad(om[:, :18].abs().amax(dim=1), (0, steps * TW - w)).view(b, h, steps, TW).amax(dim=-1)
    assert bool((mx >= 4).all())  # an offset of 4 px or more in every row of every 16-pixel step
    return om


BIG = torch.tensor([-4, -3, -2.5, -2, -1.5, -1, -0.5, 0, 0.5, 1, 1.5, 2, 2.5, 3, 4])


def _om_mixed(gen, b, h, w):
    """Eighths, 2 % of them replaced by a draw from BIG, and on the unit's edges the last in-window corner (even
    samples) and the first corner past it (odd samples) for every tap: the inwin bound depends on the wave, the
    tap and the column, so wave 0 (rows 12, 24, ..: dy = -(2 + ki), then 1/8 more), wave 11 (rows 11, 23, ..:
    dy = 3 7/8 - ki, then 4 - ki), pixel 0 of a step (columns 16, 32, ..) and pixel 15 (columns 15, 31, ..)."""
    assert b >= 2
    om = torch.randn(b, 27, h, w, generator=gen)
    off = _eighths(gen, (b, 18, h, w))
    pick = torch.rand(b, 18, h, w, generator=gen) < 0.02
    off = torch.where(pick, BIG[torch.randint(0, len(BIG), (b, 18, h, w), generator=gen)], off)
    for s in range(b):
        past = s % 2
        for k in range(9):
            ki, kj = divmod(k, 3)
            off[s, 2 * k, DCN_ROWS::DCN_ROWS, :] = -(2 + ki) - 0.125 * past
            off[s, 2 * k, DCN_ROWS - 1::DCN_ROWS, :] = (4 - ki) if past else (3.875 - ki)
            off[s, 2 * k + 1, :, TW::TW] = -(2 + kj) - 0.125 * past
            off[s, 2 * k + 1, :, TW - 1::TW] = (4 - kj) if past else (3.875 - kj)
    om[:, :18] = off
    g = _dcn_geometry(om, h, w)
    top, bot, left, right = (slice(DCN_ROWS, None, DCN_ROWS), slice(DCN_ROWS - 1, None, DCN_ROWS),
                             slice(TW, None, TW), slice(TW - 1, None, TW))
    for s in range(b):
        past = s % 2
        assert bool((g["ry"][s, :, top] == (-1 if past else 0)).all())
        assert bool((g["ry"][s, :, bot] == (17 if past else 16)).all())
        assert bool((g["rx"][s, :, :, left] == (-1 if past else 0)).all())
        assert bool((g["rx"][s, :, :, right] == (21 if past else 20)).all())
        for where in ((slice(None), top), (slice(None), bot), (slice(None), slice(None), left),
                      (slice(None), slice(None), right)):
            assert bool(g["inside"][s][where].any())  # a real share of them is inside the image
    assert bool(g["fast"].any()) and not bool(g["fast"].all())
    return om


def _om_image_edges(gen, b, h, w):
    """sample 0: zero offsets on the border rows and columns, so taps sit exactly on -1 (excluded), H - 1 and
    W - 1 (included, fraction 0) and H and W (excluded); sample 1: an eighth either side of each"""
    assert b >= 2
    om = torch.randn(b, 27, h, w, generator=gen)
    off = _eighths(gen, (b, 18, h, w))
    e = 0.125
    for edge in (0, -1):
        off[0, 0::2, edge, :] = 0.0
        off[0, 1::2, :, edge] = 0.0
        off[1, 0::2, edge, 0::2], off[1, 0::2, edge, 1::2] = e, -e
        off[1, 1::2, 0::2, edge], off[1, 1::2, 1::2, edge] = -e, e
    om[:, :18] = off
    g = _dcn_geometry(om, h, w)
    for p, n in ((g["py"], h), (g["px"], w)):
        for at in (-1.0, -1 + e, -1 - e, n - 1.0, n - e, n - 1 - e, float(n), n + e):
            assert bool((p == at).any()), at
    return om


def _om_far(gen, b, h, w):
    """a tenth of the offsets at +-40000 and +-1e9, past the 32766 clamp and the (int) conversion: their samples
    are outside the image and contribute zero"""
    om = torch.randn(b, 27, h, w, generator=gen)
    off = _eighths(gen, (b, 18, h, w))
    far = torch.tensor([40000.0, -40000.0, 1e9, -1e9])
    pick = torch.rand(b, 18, h, w, generator=gen) < 0.1
    off = torch.where(pick, far[torch.randint(0, 4, (b, 18, h, w), generator=gen)], off)
    om[:, :18] = off
    g = _dcn_geometry(om, h, w)
    hit = (off[:, 0::2].abs() > 1e4) | (off[:, 1::2].abs() > 1e4)
    assert bool(hit.any()) and not bool((hit & g["inside"]).any()) and bool(g["inside"].any())
    for v in far:
        assert bool((off == v).any())
    return om


def _om_saturated(gen, b, h, w):
    """mask logits of +-30 and -100 (the sigmoid saturates: 1 - 1e-13, 1e-13, 0) among randn ones; offsets to
    +-2.5 px"""
    om = torch.randn(b, 27, h, w, generator=gen)
    om[:, :18] = _eighths(gen, (b, 18, h, w), most=20)
    sat = torch.tensor([30.0, -30.0, -100.0])
    which = torch.randint(0, 4, (b, 9, h, w), generator=gen)
    om[:, 18:] = torch.where(which < 3, sat[which.clamp(max=2)], om[:, 18:])
    for v in sat:
        assert bool((om[:, 18:] == v).any())
    return om


EDGE_CLASSES = {"all-fast": _om_all_fast, "all-fallback": _om_all_fallback, "mixed": _om_mixed,
                "image-edges": _om_image_edges, "far-offsets": _om_far, "saturated-masks": _om_saturated}
EDGE_HW = (25, 33)


@pytest.mark.parametrize("cout", [8, 32])
@pytest.mark.parametrize("cls", list(EDGE_CLASSES))
def test_deform_conv2d_sampling_edges(cls, cout):
    """tmvs_deform_conv2d, 25 x 33, B = 2, with chosen dyadic offsets: every wave on the branch-free tap loop;
    every wave on the global fallback; samples on the last in-window corner and one past it; samples exactly on
    the image border; offsets past the clamp; saturated masks. Each generator asserts from the fp64 positions
    that its class is what its name says."""
    b, (h, w) = 2, EDGE_HW
    gen = _gen(list(EDGE_CLASSES).index(cls), cout, 2)
    om = EDGE_CLASSES[cls](gen, b, h, w)
    x = torch.randn(b, 32, h, w, generator=gen)
    weight, bias = _dcn_weight(gen, cout)
    refs = _dcn_refs(x, weight, bias, om=om)
    case = _Dcn(DEFORM, x, weight, bias, om=om)
    case.check(refs, None, False, "both", cls)
    case.check(refs, _bn(gen, cout), True, "nchw", cls)


def _fused_offset_conv(gen, cls):
    """conv_offset_mask weights that reach a class through the kernel's own offset conv: near-zero weights and
    |bias| < 0.7 (all-fast); the same with dx biases of +4.5 on the centre tap and -4.5 on tap 3 (fallback in
    every wave, as _om_all_fallback; 4.5, not 4, so that the conv's part leaves every |offset| >= 4); a 0.05
    randn conv with unit randn biases (mixed)"""
    if cls == "mixed":
        return torch.randn(27, 32, 3, 3, generator=gen) * 0.05, torch.randn(27, generator=gen)
    wom = torch.randn(27, 32, 3, 3, generator=gen) * 0.002
    bom = (torch.rand(27, generator=gen) * 2 - 1) * 0.7
    if cls == "all-fallback":
        bom[2 * 4 + 1], bom[2 * 3 + 1] = 4.5, -4.5
    return wom, bom


@pytest.mark.parametrize("cls,cout", [("all-fast", 8), ("all-fast", 32), ("all-fallback", 16), ("all-fallback", 32),
                                      ("mixed", 8), ("mixed", 16)])
def test_dcn_fused_sampling_classes(cls, cout):
    """tmvs_dcn_fused and tmvs_dcn_forward_train, 25 x 33, B = 2, reaching the fast / fallback / mixed split
    through conv_offset_mask; the class is asserted from the fp64 offsets."""
    b, (h, w) = 2, EDGE_HW
    gen = _gen(["all-fast", "all-fallback", "mixed"].index(cls), cout, 3)
    wom, bom = _fused_offset_conv(gen, cls)
    x = torch.randn(b, 32, h, w, generator=gen)
    weight, bias = _dcn_weight(gen, cout)
    refs = _dcn_refs(x, weight, bias, wom=wom, bom=bom)
    om64 = refs[1][1]
    g = _dcn_geometry(om64, h, w)
    if cls == "all-fast":
        assert float(om64[:, :18].abs().max()) < 1 and bool(g["fast"].all())
    elif cls == "all-fallback":
        assert not bool(g["fast"].any())
        mx = F.pad(om64[:, :18].abs().amax(dim=1), (0, -w % TW)).view(b, h, -1, TW).amax(dim=-1)
        assert bool((mx >= 4).all())
    else:
        assert bool(g["fast"].any()) and not bool(g["fast"].all())
    fused = _Dcn(FUSED, x, weight, bias, wom=wom, bom=bom)
    fused.check(refs, None, False, "both", cls)
    fused.check(refs, _bn(gen, cout), True, "nhwc", cls)
    _Dcn(TRAIN, x, weight, bias, wom=wom, bom=bom).check(refs, None, False, "both", cls)


# ============================================================================= conv2d, conv3x3, fpn_merge: cases
CONV2D = [(3, 8, 3, 1), (8, 8, 3, 1), (8, 16, 5, 2), (16, 16, 3, 1), (16, 32, 5, 2), (32, 32, 3, 1), (32, 32, 1, 1)]
# input (H, W). Stride 1: the output extents 1 x 1, one unit, one row and column more. k5 s2 (Ho = (H - 1) // 2 + 1):
# the same extents from both parities of H and W (the last window row / column inside the image, then outside),
# then H or W of 1 .. 4, below the kernel size
S1_HW = [(1, 1), (8, 16), (9, 17)]
S2_HW = [(1, 1), (2, 2), (15, 31), (16, 32), (17, 33), (18, 34),
         (3, 3), (4, 4), (1, 4), (4, 1), (2, 3), (3, 2), (3, 36), (35, 4)]
CONV2D_CASES = [(inst, hw) for inst in CONV2D for hw in (S2_HW if inst[3] == 2 else S1_HW)]


def _conv_out(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


def _conv2d_units(b, h, w, k, s):
    """the launcher's own formula (conv2d_launch)"""
    return b * -(-_conv_out(h, k, s) // 8) * -(-_conv_out(w, k, s) // 16)


def _conv2d_case(inst, b, h, w):
    """tmvs_conv2d_bn_relu with bn=None, relu=False (the training path's use) and with BN + ReLU"""
    cin, cout, k, s = inst
    gen = _gen(cin, cout, k, s, b, h, w)
    x = torch.randn(b, cin, h, w, generator=gen)
    weight = torch.randn(cout, cin, k, k, generator=gen) / math.sqrt(cin * k * k)
    bn = _bn(gen, cout)
    y32, y64 = (F.conv2d(x.to(dt), weight.to(dt), stride=s, padding=k // 2) for dt in DTS)
    ho, wo = _conv_out(h, k, s), _conv_out(w, k, s)
    assert tuple(y64.shape) == (b, cout, ho, wo)
    xin = _Input(x if cin == 3 else _nhwc(x))  # the first layer reads the NCHW image
    wpk = ops.conv2d_pack(weight).to(DEV)
    for use_bn, relu in ((False, False), (True, True)):
        tag = f"tmvs_conv2d_bn_relu {cin}->{cout} k{k} s{s} B {b} {h}x{w} bn={int(use_bn)} relu={int(relu)}"
        (r32, _), (r64, pre) = (_epilogue(y, bn if use_bn else None, relu) for y in (y32, y64))
        if relu:
            _relu_cuts(pre, tag)
        obuf, out = _out((b, ho, wo, cout))
        ops._launch("tmvs_conv2d_bn_relu", xin.view, b, cin, h, w, wpk, cout, k, s, _dev(bn[0]) if use_bn else None,
                    _dev(bn[1]) if use_bn else None, int(relu), out)
        _assert_guard(obuf, 1, b, tag)
        xin.intact(tag)
        _judge_all(tag, out, _nhwc(r32), _nhwc(r64))


@pytest.mark.parametrize("inst,hw", CONV2D_CASES,
                         ids=[f"{i[0]}-{i[1]}-k{i[2]}s{i[3]}-{hw[0]}x{hw[1]}" for i, hw in CONV2D_CASES])
def test_conv2d_unit_tails(inst, hw):
    """All seven tmvs_conv2d_bn_relu instances, B = 3 (1, 3 and 12 units), at the smallest extents that reach
    the unit's edges, and the two 5 x 5 stride-2 instances on images narrower or lower than their kernel."""
    _conv2d_case(inst, 3, *hw)


C3_HW = [(1, 1), (8, 16), (9, 17), (17, 33)]


def _conv3_inputs(b, h, w, seed):
    gen = _gen(3, 3, b, h, w, seed)
    x = torch.randn(b, 32, h, w, generator=gen)
    weight = torch.randn(32, 32, 3, 3, generator=gen) / math.sqrt(288)
    return gen, x, weight


def _conv3_case(b, h, w, use_bias, use_bn, layouts=("nchw", "nhwc", "both")):
    gen, x, weight = _conv3_inputs(b, h, w, 2 * use_bias + use_bn)
    bias = 0.3 * torch.randn(32, generator=gen) if use_bias else None
    bn = _bn(gen, 32) if use_bn else None
    relu = use_bn
    refs = []
    for dt in DTS:
        refs.append(_epilogue(F.conv2d(x.to(dt), weight.to(dt), None if bias is None else bias.to(dt), padding=1), bn,
                              relu))
    (r32, _), (r64, pre) = refs
    xin = _Input(_nhwc(x))
    wpk = ops.deform_conv2d_pack(weight).to(DEV)
    for layout in layouts:
        tag = f"tmvs_conv3x3_nhwc B {b} {h}x{w} bias={int(use_bias)} bn={int(use_bn)} relu={int(relu)} {layout}"
        if relu:
            _relu_cuts(pre, tag)
        obuf, out = _out((b, 32, h, w), layout in ("nchw", "both"))
        nbuf, onh = _out((b, h, w, 32), layout in ("nhwc", "both"))
        ops._launch("tmvs_conv3x3_nhwc", xin.view, wpk, _dev(bias), _dev(bn[0]) if bn else None,
                    _dev(bn[1]) if bn else None, int(relu), b, 32, 32, h, w, out, onh)
        xin.intact(tag)
        if out is not None:
            _assert_guard(obuf, 1, b, tag)
            _judge_all(tag + " -> nchw", out, r32, r64)
        if onh is not None:
            _assert_guard(nbuf, 1, b, tag)
            _judge_all(tag + " -> nhwc", onh, _nhwc(r32), _nhwc(r64))


@pytest.mark.parametrize("use_bias,use_bn", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "bias", "bn", "bias-bn"])
@pytest.mark.parametrize("hw", C3_HW, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_conv3x3_unit_tails(hw, use_bias, use_bn):
    """tmvs_conv3x3_nhwc, B = 3, with bias, with BN (+ ReLU), with both, with neither; NCHW only, NHWC only and
    both."""
    _conv3_case(3, *hw, use_bias, use_bn)


def _conv3_acc_case(b, h, w):
    """tmvs_conv3x3_nhwc_acc into a pre-filled out_nhwc = o: bit-identical to o + y, y the same launch's
    non-accumulating NHWC output (the operand order the kernel documents), and o + conv under the bar"""
    gen, x, weight = _conv3_inputs(b, h, w, 9)
    o = torch.randn(b, h, w, 32, generator=gen)
    r32, r64 = (o.to(dt) + _nhwc(F.conv2d(x.to(dt), weight.to(dt), padding=1)) for dt in DTS)
    xin = _Input(_nhwc(x))
    wpk = ops.deform_conv2d_pack(weight).to(DEV)
    tag = f"tmvs_conv3x3_nhwc_acc B {b} {h}x{w}"
    ybuf, y = _out((b, h, w, 32))
    ops._launch("tmvs_conv3x3_nhwc", xin.view, wpk, None, None, None, 0, b, 32, 32, h, w, None, y)
    abuf, acc = _out((b, h, w, 32), fill=o)
    ops._launch("tmvs_conv3x3_nhwc_acc", xin.view, wpk, b, 32, 32, h, w, acc)
    for buf in (ybuf, abuf):
        _assert_guard(buf, 1, b, tag)
    xin.intact(tag)
    assert torch.equal(_bits(acc), _bits(o.to(DEV) + y)), tag + ": not out + conv, bit for bit"
    _judge_all(tag, acc, r32, r64)


@pytest.mark.parametrize("hw", C3_HW, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_conv3x3_acc_unit_tails(hw):
    """tmvs_conv3x3_nhwc_acc, B = 3: out + conv bit for bit, and under the bar."""
    _conv3_acc_case(3, *hw)


def _fpn_launch(prev, lat, cl, wi, bi, b, h, w):
    obuf, out = _out((b, 2 * h, 2 * w, 32))
    ops._launch("tmvs_fpn_merge", prev, lat, cl, wi, bi, b, h, w, out)
    return obuf, out


@pytest.mark.parametrize("b", [3, 1])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (4, 8)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("cl", [8, 16])
def test_fpn_merge_block_tails(cl, hw, b):
    """tmvs_fpn_merge = interpolate(prev, 2, nearest) + Conv2d(cl, 32, 1, bias): 4, 12, 60, 128, 180 and 384
    output pixels, either side of the 64 pixels of a block and multiples of it."""
    h, w = hw
    gen = _gen(cl, h, w, b)
    prev = torch.randn(b, 32, h, w, generator=gen)
    lat = torch.randn(b, cl, 2 * h, 2 * w, generator=gen)
    wi = torch.randn(32, cl, generator=gen) / math.sqrt(cl)
    bi = 0.3 * torch.randn(32, generator=gen)
    r32, r64 = (_nhwc(F.interpolate(prev.to(dt), scale_factor=2.0, mode="nearest")
                      + F.conv2d(lat.to(dt), wi.to(dt).view(32, cl, 1, 1), bi.to(dt))) for dt in DTS)
    pin, lin = _Input(_nhwc(prev)), _Input(_nhwc(lat))
    tag = f"tmvs_fpn_merge cl {cl} B {b} {h}x{w}"
    obuf, out = _fpn_launch(pin.view, lin.view, cl, wi.to(DEV), bi.to(DEV), b, h, w)
    _assert_guard(obuf, 1, b, tag)
    pin.intact(tag)
    lin.intact(tag)
    _judge_all(tag, out, r32, r64)


# ========================================================================= 3. the walk past the resident grid
# The launchers cap the grid at CUs x resident workgroups per CU and each workgroup walks [u_begin, u_end),
# prefetching unit u + 1 into registers while it works on unit u. No occupancy is assumed: a CU holds 32 waves,
# so at most 2 of the 12-wave DCN workgroups and 4 of the 8-wave conv ones; each case has more than
# 2 x CUs x that bound in units (asserted, from the launcher's formula and the device's CU count), so every
# workgroup walks at least two units whatever the real occupancy, with a ragged last band and a ragged last step.
# Launched grids on an MI355X (256 CUs), from a kernel trace of these tests: dcn_window_kernel<32, false>,
# <16, true> and <8, true> 256 workgroups each (one per CU: 4 or 5 units per workgroup); conv3x3_window_kernel 512
# (4 or 5 units each); conv2d_bn_relu_kernel<3, 8, 3, 1> and <32, 32, 1, 1> 1024 (2 or 3 units each), <8, 16, 5, 2>
# 768 (2 or 3), <16, 32, 5, 2> 256 (8 or 9).
DCN_WALK = (2, 100, 920)     # 2 x 9 bands x 58 steps = 1044 units
CONV_WALK_OUT = (100, 1254)  # 2 x 13 bands x 79 steps = 2054 units


def _assert_dcn_walk(b, h, w):
    units = _dcn_units(b, h, w)
    assert units > 2 * _cus() * 2, (units, _cus())
    assert h % DCN_ROWS != 0 and w % TW != 0


@pytest.mark.parametrize("entry,cout", [(DEFORM, 32), (FUSED, 16), (TRAIN, 8)], ids=["deform-32", "fused-16", "train-8"])
def test_dcn_walk_past_resident_grid(entry, cout):
    """Every workgroup of dcn_window_kernel computes at least two units: the unfused entry with the mixed offsets
    of section 2 (the unit being sampled must use its own offset / mask logits, not those the prefetch of the
    next unit loads), the fused entry, and the training entry with its offset_mask_out."""
    b, h, w = DCN_WALK
    _assert_dcn_walk(b, h, w)
    gen = _gen(DCN_ENTRIES.index(entry), cout, 4)
    x = torch.randn(b, 32, h, w, generator=gen)
    weight, bias = _dcn_weight(gen, cout)
    if entry == DEFORM:
        kw = dict(om=_om_mixed(gen, b, h, w))
    else:
        kw = dict(wom=torch.randn(27, 32, 3, 3, generator=gen) * 0.05, bom=torch.randn(27, generator=gen))
    refs = _dcn_refs(x, weight, bias, **kw)
    case = _Dcn(entry, x, weight, bias, **kw)
    if entry == TRAIN:
        case.check(refs, None, False, "both", "walk")
    else:
        case.check(refs, _bn(gen, cout), True, "both", "walk")


def _assert_conv_walk(units, ho, wo):
    assert units > 2 * _cus() * 4, (units, _cus())
    assert ho % 8 != 0 and wo % 16 != 0


@pytest.mark.parametrize("acc", [False, True], ids=["conv3x3", "conv3x3-acc"])
def test_conv3x3_walk_past_resident_grid(acc):
    """conv3x3_window_kernel, plain (bias, BN, ReLU, both layouts) and accumulating, at least two units per
    workgroup."""
    b, (h, w) = 2, CONV_WALK_OUT
    _assert_conv_walk(b * -(-h // 8) * -(-w // 16), h, w)
    if acc:
        _conv3_acc_case(b, h, w)
    else:
        _conv3_case(b, h, w, True, True, layouts=("both",))


@pytest.mark.parametrize("inst", [(3, 8, 3, 1), (8, 16, 5, 2), (16, 32, 5, 2), (32, 32, 1, 1)],
                         ids=lambda i: f"{i[0]}-{i[1]}-k{i[2]}s{i[3]}")
def test_conv2d_walk_past_resident_grid(inst):
    """conv2d_bn_relu_kernel, the NCHW first layer, both stride-2 layers and the 1 x 1, at least two units per
    workgroup."""
    _, _, k, s = inst
    ho, wo = CONV_WALK_OUT
    h, w = (2 * ho - 1, 2 * wo) if s == 2 else (ho, wo)  # stride 2: an odd height and an even width
    assert (_conv_out(h, k, s), _conv_out(w, k, s)) == (ho, wo)
    _assert_conv_walk(_conv2d_units(2, h, w, k, s), ho, wo)
    _conv2d_case(inst, 2, h, w)


# ================================================================= 4. the public wrappers return the same bits
def _same(a, b, tag):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), tag + ": the wrapper and the direct launch differ"


@pytest.mark.parametrize("entry", DCN_ENTRIES)
def test_dcn_wrapper_matches_direct_launch(entry):
    b, h, w, cout = 2, 13, 17, 16
    gen = _gen(DCN_ENTRIES.index(entry), 5)
    x = torch.randn(b, 32, h, w, generator=gen)
    weight, bias = _dcn_weight(gen, cout)
    om = torch.randn(b, 27, h, w, generator=gen) * 1.5
    wom, bom = torch.randn(27, 32, 3, 3, generator=gen) * 0.05, torch.randn(27, generator=gen) * 0.5
    bn = _bn(gen, cout)
    fold = (bn[0].to(DEV), bn[1].to(DEV))
    case = _Dcn(entry, x, weight, bias, **(dict(om=om) if entry == DEFORM else dict(wom=wom, bom=bom)))
    if entry == DEFORM:
        out, onh, _ = case.launch(bn, True, "both", entry)
        wout, wonh = ops.deform_conv2d(case.x.view, case.om.view, case.wpk, case.bias, cout, bn=fold, relu=True,
                                       want_nhwc=True)
    elif entry == FUSED:
        out, onh, _ = case.launch(bn, True, "both", entry)
        wout, wonh = ops.dcn_fused(case.x.view, case.wom, case.bom, case.wpk, case.bias, cout, bn=fold, relu=True,
                                   want_nchw=True, want_nhwc=True)
    else:
        out, onh, omo = case.launch(None, False, "both", entry)
        wonh, wom_out, wout = ops.dcn_forward_train(case.x.view, case.wom, case.bom, case.wpk, case.bias, cout,
                                                    want_nchw=True)
        _same(wom_out, omo, entry + " offset_mask_out")
    _same(wout, out, entry + " nchw")
    _same(wonh, onh, entry + " nhwc")


def test_conv_and_fpn_wrappers_match_direct_launch():
    b, h, w = 2, 9, 17
    gen = _gen(6, 6)
    x = torch.randn(b, h, w, 32, generator=gen).to(DEV)
    bn = _bn(gen, 32)
    fold = (bn[0].to(DEV), bn[1].to(DEV))
    # conv2d
    w5 = ops.conv2d_pack(torch.randn(32, 16, 5, 5, generator=gen) / 20).to(DEV)
    x16 = torch.randn(b, h, w, 16, generator=gen).to(DEV)
    ho, wo = _conv_out(h, 5, 2), _conv_out(w, 5, 2)
    _, out = _out((b, ho, wo, 32))
    ops._launch("tmvs_conv2d_bn_relu", x16, b, 16, h, w, w5, 32, 5, 2, fold[0], fold[1], 1, out)
    _same(ops.conv2d_bn_relu(x16, w5, 32, 5, 2, bn=fold, relu=True), out, "tmvs_conv2d_bn_relu")
    # conv3x3 and its accumulate form
    w3 = ops.deform_conv2d_pack(torch.randn(32, 32, 3, 3, generator=gen) / 17).to(DEV)
    bias = torch.randn(32, generator=gen).to(DEV)
    _, out = _out((b, 32, h, w))
    _, onh = _out((b, h, w, 32))
    ops._launch("tmvs_conv3x3_nhwc", x, w3, bias, fold[0], fold[1], 1, b, 32, 32, h, w, out, onh)
    wout, wonh = ops.conv3x3_nhwc(x, w3, bn=fold, relu=True, bias=bias, want_nchw=True, want_nhwc=True)
    _same(wout, out, "tmvs_conv3x3_nhwc nchw")
    _same(wonh, onh, "tmvs_conv3x3_nhwc nhwc")
    o = torch.randn(b, h, w, 32, generator=gen)
    _, acc = _out((b, h, w, 32), fill=o)
    ops._launch("tmvs_conv3x3_nhwc_acc", x, w3, b, 32, 32, h, w, acc)
    _same(ops.conv3x3_nhwc_acc(x, w3, o.to(DEV)), acc, "tmvs_conv3x3_nhwc_acc")
    # fpn_merge
    lat = torch.randn(b, 2 * h, 2 * w, 8, generator=gen).to(DEV)
    wi, bi = torch.randn(32, 8, generator=gen).to(DEV), torch.randn(32, generator=gen).to(DEV)
    _, out = _fpn_launch(x, lat, 8, wi, bi, b, h, w)
    _same(ops.fpn_merge(x, lat, wi, bi), out, "tmvs_fpn_merge")
