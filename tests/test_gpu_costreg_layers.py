"""The inference CostRegNet kernels (csrc/costreg.hip) and softmax / WTA (csrc/glue.hip), layer by layer, at
the tile tails and batch sizes the whole-network tests never reach: odd extents under the stride-2 gather,
widths that are no multiple of the 16-voxel tile, depth, height and width of 1, batch 2 (the `n` decode of a
tile, the per-sample buffer range, grids that are no multiple of the 8 XCDs), the KDSKIP / TAPOUT instances
either side of their output-depth threshold, both input-depth parities of the transposed layers, the
steady-state walk of the three persistent kernels past their resident cap, the 62-column segment edges of
the VALU kernels, and the 256-thread block edge of softmax / WTA.

  conv1  8 -> 16 s2   conv3d_s2c8_tile_kernel<2, 2>   persistent
  conv2  16 -> 16 s1  conv3d_c16_kernel<2, 4>         persistent
  conv3 .. conv6      conv3d_lds_kernel, straight / KDSKIP (output depth <= 2) / TAPOUT (conv5)
  conv7 64 -> 32      deconv3d_lds_kernel, 2 x 2 input tiles (even input depth) / 1 x 4 (odd)
  conv9 32 -> 16      deconv3d_lds_kernel at these shapes (below 1.5 tiles per resident workgroup); from there on
                      deconv3d_c16p_kernel, persistent (tests/test_gpu_costreg_persistent.py)
  conv11 16 -> 8      deconv3d_c8_kernel, 2 x 2 / 1 x 4, persistent
  conv0 1 -> 8, prob 8 -> 1   conv0_kernel / prob_kernel (VALU), prob_wta_rows_kernel through costregnet_wta

Every reference is plain torch on the CPU (F.conv3d / F.conv_transpose3d k3 p1, op1; softmax), evaluated in
fp32 and in fp64; the trunk's is oracle.transmvs_ref.cost_reg_net on the golden state dict. Error =
max|got - ref64| / max|ref64|; the bar is err_gpu <= max(2 x err_fp32ref, 1e-5) (tests/_primitives.py; the
trunk's floor is the 2e-5 of max|logit| test_costregnet_matches_golden holds). Outputs are contiguous slices
of larger buffers whose other rows hold a sentinel that must survive bit for bit (a voxel the kernel leaves
unwritten keeps the sentinel and fails the comparison); inputs are slices of buffers whose other rows are NaN,
so a read outside the samples poisons the output.

Measured on an MI355X, worst (err_gpu, err_fp32ref) over all cases of a layer: conv1 (5.8e-7, 6.6e-7), conv2
(8.0e-7, 6.5e-7), conv3 (6.3e-7, 5.8e-7), conv4 (7.9e-7, 4.9e-7), conv5 (7.7e-7, 4.9e-7), conv6 (1.1e-6, 3.9e-7),
conv7 (3.5e-7, 2.0e-7), conv9 (2.1e-7, 1.5e-7), conv11 (2.9e-7, 1.3e-7), conv0 raw (2.2e-7, 2.2e-7), prob raw
(5.1e-7, 5.1e-7), the trunk (8.1e-7, 6.1e-7), softmax prob and conf (2.4e-7, 2.4e-7): the floor is the bar
everywhere. 73 tests, about 4 s.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import transmvs_ref as oracle
from tests._primitives import DEV, _assert_guard, _bits, _gen, _guarded, _judge
from tests._util import golden_state_dict
from transmvsnet_amd import TransMVSNet, ops
from transmvsnet_amd.train import _pack_fwd

pytestmark = pytest.mark.gpu
DTS = (torch.float32, torch.float64)
NAN = float("nan")


def _ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _nan_guarded(t):
    """(buffer, view): `view` holds the CPU tensor `t` between one NaN row (one sample's size) on either side"""
    buf = torch.full((t.shape[0] + 2, *t.shape[1:]), NAN, device=DEV)
    view = buf[1:1 + t.shape[0]]
    view.copy_(t)
    assert view.is_contiguous() and bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())
    return buf, view


def _geo_id(geo):
    return "x".join(map(str, geo))


# --------------------------------------------------------------------- 1. layers through the BN / ReLU epilogue
# name -> (cin, cout, stride, transposed)
LAYERS = {"conv1": (8, 16, 2, False), "conv2": (16, 16, 1, False), "conv3": (16, 32, 2, False),
          "conv4": (32, 32, 1, False), "conv5": (32, 64, 2, False), "conv6": (64, 64, 1, False),
          "conv7": (64, 32, 2, True), "conv9": (32, 16, 2, True), "conv11": (16, 8, 2, True),
          "conv0": (1, 8, 1, False), "prob": (8, 1, 1, False)}
# input (B, D, H, W)
LAYER_CASES = [
    ("conv1", (2, 5, 7, 37)),   # 16 tiles, dealt over 8 XCDs
    ("conv1", (1, 3, 5, 9)),    # 2 tiles: the nxcd = 1 path
    ("conv1", (2, 1, 1, 1)),
    ("conv2", (2, 3, 5, 19)), ("conv2", (1, 1, 3, 17)), ("conv2", (2, 4, 9, 33)),
    ("conv3", (2, 9, 7, 35)),   # Do = 5: straight
    ("conv3", (2, 3, 5, 21)),   # Do = 2: KDSKIP
    ("conv4", (2, 3, 5, 19)),   # straight
    ("conv4", (2, 2, 5, 19)), ("conv4", (1, 1, 3, 17)),  # KDSKIP, the 2 x 4 tile
    ("conv5", (2, 5, 7, 35)), ("conv5", (1, 1, 2, 3)),   # TAPOUT
    ("conv6", (2, 3, 3, 19)),   # straight
    ("conv6", (2, 2, 5, 17)), ("conv6", (1, 1, 1, 1)),   # KDSKIP
    ("conv7", (2, 2, 3, 19)), ("conv7", (2, 3, 5, 19)), ("conv7", (1, 1, 1, 1)),  # even Di, odd Di
    ("conv9", (2, 2, 3, 19)), ("conv9", (2, 3, 5, 19)), ("conv9", (1, 1, 1, 1)),
    ("conv11", (2, 2, 3, 19)), ("conv11", (2, 3, 5, 21)), ("conv11", (1, 1, 1, 1)),
]


def _out_dhw(dhw, stride, transposed):
    return tuple(2 * n if transposed else (n - 1) // stride + 1 for n in dhw)


def _layer_inputs(layer, geo, epilogue):
    """CPU inputs of one case: x and skip NCDHW, the torch weight (randn / sqrt(27 cin)), alpha in [0.5, 1.5)
    with every fourth channel negated, shift = 0.5 randn"""
    cin, cout, stride, transposed = LAYERS[layer]
    b = geo[0]
    gen = _gen(cin, cout, stride, int(transposed), *geo, int(epilogue))
    x = torch.randn(b, cin, *geo[1:], generator=gen)
    wt = torch.randn(*((cin, cout) if transposed else (cout, cin)), 3, 3, 3, generator=gen) / math.sqrt(27 * cin)
    alpha = shift = None
    if epilogue:
        alpha = torch.rand(cout, generator=gen) + 0.5
        alpha[1::4] = -alpha[1::4]
        shift = 0.5 * torch.randn(cout, generator=gen)
    skip = torch.randn(b, cout, *_out_dhw(geo[1:], stride, transposed), generator=gen) if transposed else None
    return x, wt, alpha, shift, skip


def _layer_ref(dt, layer, x, wt, alpha, shift, skip):
    """(reference NDHWC, its part before the skip add): relu(conv(x) alpha + shift) (+ skip), or the raw
    convolution (+ skip) without alpha"""
    _, cout, stride, transposed = LAYERS[layer]
    if transposed:
        y = F.conv_transpose3d(x.to(dt), wt.to(dt), stride=2, padding=1, output_padding=1)
    else:
        y = F.conv3d(x.to(dt), wt.to(dt), stride=stride, padding=1)
    if alpha is not None:
        y = torch.relu(y * alpha.to(dt).view(1, cout, 1, 1, 1) + shift.to(dt).view(1, cout, 1, 1, 1))
    pre = y
    if skip is not None:
        y = y + skip.to(dt)
    return _ndhwc(y), pre


def _layer_case(layer, geo, epilogue=True):
    cin, cout, stride, transposed = LAYERS[layer]
    b = geo[0]
    x, wt, alpha, shift, skip = _layer_inputs(layer, geo, epilogue)
    (r32, _), (r64, pre) = (_layer_ref(dt, layer, x, wt, alpha, shift, skip) for dt in DTS)
    tag = f"{layer} {cin}->{cout} {'epilogue' if epilogue else 'raw'} in {_geo_id(geo)}"
    if epilogue:  # the ReLU clips a real share of the outputs, and lets a real share through
        assert bool((pre == 0).any()) and bool((pre > 0).any()), tag
    else:
        assert bool((pre < 0).any()), tag
    pk = _pack_fwd(wt, transposed)
    if layer == "prob":
        pk = ops.prob_pack(pk)
    xbuf, xd = _nan_guarded(_ndhwc(x))
    sbuf, sd = _nan_guarded(_ndhwc(skip)) if transposed else (None, None)
    obuf, out = _guarded(tuple(r64.shape), 1)
    if not epilogue:
        got = ops.conv3d_mfma(xd, pk.to(DEV), cout, stride, transposed, skip=sd, out=out)
    elif transposed:
        got = ops.deconv3d_bn_relu_add(xd, pk.to(DEV), alpha.to(DEV), shift.to(DEV), cout, sd, out=out)
    else:
        got = ops.conv3d_bn_relu(xd, pk.to(DEV), alpha.to(DEV), shift.to(DEV), cout, stride, out=out)
    assert got.data_ptr() == out.data_ptr()
    _assert_guard(obuf, 1, b, tag)
    assert torch.equal(_bits(xd), _bits(_ndhwc(x))), tag + ": the input was written"
    assert bool(torch.isnan(xbuf[0]).all()) and bool(torch.isnan(xbuf[-1]).all()), tag
    _judge(tag, got, r32, r64)
    if b > 1:  # the last sample on its own scale
        _judge(tag + " [last sample]", got[-1], r32[-1], r64[-1])


@pytest.mark.parametrize("layer,geo", LAYER_CASES, ids=[f"{l}-{_geo_id(g)}" for l, g in LAYER_CASES])
def test_layer_bn_relu(layer, geo):
    """tmvs_conv3d_bn_relu / tmvs_deconv3d_bn_relu_add against relu(conv(x) alpha + shift) (+ skip): per
    channel alpha (a quarter negative) and shift on ragged tiles, at the smallest shapes that reach each
    dispatch branch."""
    _layer_case(layer, geo)


# --------------------------------------------------------------- 2. the persistent kernels past their resident cap
# persistent_grid caps the grid at CUs x resident workgroups per CU; 256 CUs and, from the kernels' LDS and
# waves_per_eu: conv1 3 per CU (41.5 KB of LDS), conv2 2 per CU (waves_per_eu(2), 55 KB), conv11 at most 4
# (waves_per_eu(4, 4)). Each case has a little over twice its cap in tiles, so every workgroup walks two or
# three tiles through fetch(next) during the MFMAs and commit() behind the barrier.
# (layer, input (B, D, H, W), (TD, TH) of the tile in the grid the launcher tiles, assumed cap, tiles); conv11's
# odd input depth takes the kernel's 1 x 4 instance, whose walk is a double buffer of its own
CAP_CASES = [("conv1", (2, 17, 83, 271), (2, 2), 768, 1890),
             ("conv2", (2, 9, 42, 170), (2, 4), 512, 1210),
             ("conv11", (2, 10, 44, 150), (2, 2), 1024, 2200),
             ("conv11", (2, 11, 43, 150), (1, 4), 1024, 2420)]


@pytest.mark.parametrize("layer,geo,tile,cap,want_tiles", CAP_CASES, ids=[f"{c[0]}-{_geo_id(c[1])}" for c in CAP_CASES])
def test_persistent_walk_past_resident_cap(layer, geo, tile, cap, want_tiles):
    """conv3d_s2c8_tile_kernel, conv3d_c16_kernel and both deconv3d_c8_kernel instances with a little over
    twice as many tiles as workgroups: the only cases in which a workgroup computes on a tile that fetch() /
    commit() staged during the walk, not before it. Launched grids on an MI355X, from a kernel trace of this
    test: 768, 512, 1024 and 1024 workgroups, the caps assumed below."""
    _, _, stride, transposed = LAYERS[layer]
    # the launcher's own formula; the transposed layer tiles its input grid, the others their output grid
    ed, eh, ew = geo[1:] if transposed else _out_dhw(geo[1:], stride, False)
    tiles = geo[0] * -(-ed // tile[0]) * -(-eh // tile[1]) * -(-ew // 16)
    assert tiles == want_tiles and tiles > 2 * cap, (layer, tiles, cap)
    assert ew % 16 != 0  # a ragged last tile along W in every row of tiles
    _layer_case(layer, geo)


# ------------------------------------------------------------------ 3. conv0 and prob (the VALU kernels), raw
# 62-column segments (lanes 0 and 63 are the halo), 4-row blocks, 8-plane depth chunks; grids that are no
# multiple of 8
VALU_GEOS = [(2, 9, 5, 63), (2, 17, 6, 125), (1, 8, 4, 62), (2, 3, 1, 1), (1, 1, 7, 61)]


@pytest.mark.parametrize("geo", VALU_GEOS, ids=_geo_id)
@pytest.mark.parametrize("layer", ["conv0", "prob"])
def test_valu_conv_segment_tails(layer, geo):
    """tmvs_conv3d_mfma 1 -> 8 (conv0_kernel) and 8 -> 1 (prob_kernel, ops.prob_pack) against F.conv3d:
    widths of 61, 62, 63 and 125 (the segment's last lane, its first halo lane, a second segment one and
    63 columns wide), heights of 1, 4, 5, 6, 7, depths of 1, 3, 8, 9, 17."""
    _layer_case(layer, geo, epilogue=False)


@pytest.mark.parametrize("layer,geo", [("conv1", (2, 5, 7, 37)), ("conv2", (2, 3, 5, 19)), ("conv11", (2, 3, 5, 21))],
                         ids=["conv1", "conv2", "conv11"])
def test_raw_epilogue_into_out(layer, geo):
    """ops.conv3d_mfma(out=) on the three persistent kernels: the raw convolution (+ skip) lands in the
    caller's buffer."""
    _layer_case(layer, geo, epilogue=False)


# ------------------------------------------------------------------------------ 4. the trunk against the oracle
TRUNK_FLOOR = 2e-5  # of max |logit|: the bound test_costregnet_matches_golden holds
TRUNK_GEOS = [(2, 8, 24, 40),    # level 3 is 1 x 3 x 5: odd at every level below the first
              (1, 16, 40, 72),   # level 3 is 2 x 5 x 9
              (1, 32, 8, 8),
              (1, 24, 16, 64)]   # the second 62-column segment is 2 columns wide


@pytest.fixture(scope="module")
def sd():
    return golden_state_dict()


@pytest.fixture(scope="module")
def model(sd):
    m = TransMVSNet(ndepths=[8, 8, 8]).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def sd64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@pytest.mark.parametrize("geo", TRUNK_GEOS, ids=_geo_id)
@pytest.mark.parametrize("stage", [0, 1, 2])
def test_trunk_vs_oracle(sd, sd64, model, stage, geo):
    """ops.costregnet against oracle.cost_reg_net in fp64 and fp32, all three cost_regularization weight sets."""
    x = torch.randn(*geo, generator=_gen(stage, *geo))
    p = f"cost_regularization.{stage}."
    with torch.no_grad():
        r32 = oracle.cost_reg_net(sd, p, x[:, None])[:, 0]
        r64 = oracle.cost_reg_net(sd64, p, x.double()[:, None])[:, 0]
    st, _keep = model.cost_regularization[stage].packed(DEV)
    xbuf, xd = _nan_guarded(x)
    got = ops.costregnet(xd, st)
    _judge(f"costregnet set {stage} in {_geo_id(geo)}", got, r32, r64, floor=TRUNK_FLOOR)


# --------------------------------------------------------------------------- 5. softmax / WTA against a reference
SM_HW = [(1, 1), (3, 85), (1, 257), (7, 37)]  # 1, 255, 257 and 259 pixels: either side of the 256-thread block
SM_CLAMP = (500.0, 900.0)


def _softmax_inputs(d, h, w, scale):
    """fp32 logits [2, d, h, w] = scale * randn with an exact tie of the maximum planted at two or three
    planes in about 10 % of the pixels; sorted hypotheses in [425, 935) that the clamp cuts at both ends"""
    gen = _gen(d, h, w, int(scale))
    x = torch.randn(2, d, h, w, generator=gen) * scale
    tie = torch.rand(2, h, w, generator=gen) < (1.0 if h * w == 1 else 0.1)
    order = torch.rand(2, d, h, w, generator=gen).argsort(dim=1)  # a random permutation of the planes per pixel
    ntie = torch.randint(2, 4, (2, h, w), generator=gen)
    top = x.max(dim=1).values + scale  # one fp32 value per pixel, above every logit of the pixel
    rank = order.argsort(dim=1)  # plane -> its position in the permutation
    planted = tie[:, None] & (rank < ntie[:, None])
    x = torch.where(planted, top[:, None].expand_as(x), x).contiguous()
    hyp = (425.0 + 510.0 * torch.rand(2, d, h, w, generator=gen)).sort(dim=1).values.contiguous()
    return x, hyp, planted


@pytest.mark.parametrize("scale", [1.0, 50.0])
@pytest.mark.parametrize("d", [4, 8, 16, 24, 32, 48, 64])
def test_softmax_wta_vs_reference(d, scale):
    """tmvs_softmax_wta against the fp64 softmax of the same fp32 logits: prob and conf under the bar; the
    winner is the first maximum of the logits, exactly (depth_raw = hyp there, depth its clamp, conf = prob
    there, all bit for bit)."""
    for h, w in SM_HW:
        x, hyp, planted = _softmax_inputs(d, h, w, scale)
        m = x.max(dim=1, keepdim=True).values
        planes = torch.arange(d).view(1, d, 1, 1).expand_as(x)
        first = torch.where(x == m, planes, torch.full_like(planes, d)).min(dim=1, keepdim=True).values
        ntied = (x == m).sum(dim=1)
        assert bool((ntied >= 2).any()) and (h * w == 1 or bool((ntied == 1).any()))
        p64 = torch.softmax(x.double(), dim=1)
        p32 = torch.exp(F.log_softmax(x, dim=1))
        tag = f"softmax_wta D={d} {h}x{w} scale={scale:g}"
        xbuf, xd = _nan_guarded(x)
        hbuf, hd = _nan_guarded(hyp)
        prob, depth, raw, conf = ops.softmax_wta(xd, hd, SM_CLAMP)
        _judge(tag + " prob", prob, p32, p64)
        _judge(tag + " conf", conf, p32.max(dim=1).values, p64.max(dim=1).values)
        want_raw = hyp.gather(1, first)[:, 0]
        assert torch.equal(_bits(raw), _bits(want_raw)), tag + ": depth_raw is not hyp at the first maximum"
        assert torch.equal(_bits(depth), _bits(want_raw.clamp(*SM_CLAMP))), tag + ": depth is not the clamp of depth_raw"
        assert torch.equal(_bits(conf), _bits(prob.cpu().gather(1, first)[:, 0])), tag + ": conf is not prob at the winner"
        if h * w > 1:  # the clamp cuts both ends
            assert bool((want_raw < SM_CLAMP[0]).any()) and bool((want_raw > SM_CLAMP[1]).any()), tag


@pytest.mark.parametrize("geo", [(2, 8, 8, 64), (2, 16, 8, 128), (1, 32, 16, 192), (2, 24, 8, 56)], ids=_geo_id)
def test_costregnet_wta_bitwise_at_segment_widths(model, geo):
    """tmvs_costregnet_wta == tmvs_costregnet -> tmvs_softmax_wta, bit for bit, at widths of one segment plus
    2 columns, two plus 4, three plus 6, and less than one."""
    g = _gen(*geo)
    x = torch.randn(*geo, generator=g).to(DEV)
    hyp = (425.0 + torch.rand(*geo, generator=g).mul(510.0)).sort(dim=1).values.contiguous().to(DEV)
    st, _keep = model.cost_regularization[1].packed(DEV)
    ref = ops.softmax_wta(ops.costregnet(x, st), hyp, SM_CLAMP)
    got = ops.costregnet_wta(x, st, hyp, SM_CLAMP)
    for name, a, r in zip(("prob", "depth", "depth_raw", "conf"), got, ref):
        assert torch.equal(_bits(a), _bits(r)), name


# ----------------------------------------------------------------------------------- 6. what the wrappers refuse
def test_layer_wrappers_refuse_what_the_entry_points_would_misread():
    """The entry points take pointers and one (cin, cout) for all of them: a short weight, alpha or shift
    tensor, a skip or out of another shape, a strided view or a host tensor would be read (or written) past
    its end, so the wrappers raise before the call."""
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    x, w, a = z(1, 2, 3, 5, 16), z(27, 16, 16), z(16)
    xt, wt_, a8, sk = z(1, 2, 3, 5, 16), z(27, 8, 16), z(8), z(1, 4, 6, 10, 8)
    conv = lambda **k: ops.conv3d_bn_relu(k.get("x", x), k.get("w", w), k.get("alpha", a), k.get("shift", a), 16, 1,
                                          out=k.get("out"))
    deconv = lambda **k: ops.deconv3d_bn_relu_add(k.get("x", xt), k.get("w", wt_), k.get("alpha", a8),
                                                  k.get("shift", a8), 8, k.get("skip", sk), out=k.get("out"))
    raw = lambda **k: ops.conv3d_mfma(k.get("x", x), k.get("w", w), 16, 1, out=k.get("out"))
    rawt = lambda **k: ops.conv3d_mfma(k.get("x", xt), k.get("w", wt_), 8, 2, transposed=True, skip=k.get("skip"),
                                       out=k.get("out"))
    for call, good_w in ((conv, w), (deconv, wt_), (raw, w), (rawt, wt_)):
        with pytest.raises(ValueError, match="27 \\* cout \\* cin"):
            call(w=z(27, 8, 8))
        with pytest.raises(ValueError, match="contiguous"):
            call(w=z(*good_w.shape, 2)[..., 0])
        with pytest.raises(ValueError, match="GPU tensor"):
            call(w=good_w.cpu())
        with pytest.raises(ValueError, match="GPU tensor"):
            call(x=torch.zeros(1, 2, 3, 5, 16))
        with pytest.raises(ValueError, match="contiguous"):
            call(x=z(1, 2, 3, 5, 32)[..., ::2])
        with pytest.raises(ValueError, match="out must"):
            call(out=z(1, 2, 3, 4, 16))
        with pytest.raises(ValueError, match="contiguous"):
            call(out=z(1, 4, 6, 10, 32)[..., ::2])
    for call, n in ((conv, 16), (deconv, 8)):
        for name in ("alpha", "shift"):
            with pytest.raises(ValueError, match=f"{name} must hold cout"):
                call(**{name: z(n - 4)})
            with pytest.raises(ValueError, match="GPU tensor"):
                call(**{name: torch.zeros(n)})
            with pytest.raises(ValueError, match="contiguous"):
                call(**{name: z(2 * n)[::2]})
    for call in (deconv, rawt):
        with pytest.raises(ValueError, match="skip must"):
            call(skip=z(1, 4, 6, 9, 8))
        with pytest.raises(ValueError, match="contiguous"):
            call(skip=z(1, 4, 6, 10, 16)[..., ::2])
        with pytest.raises(ValueError, match="GPU tensor"):
            call(skip=torch.zeros(1, 4, 6, 10, 8))
        with pytest.raises(ValueError, match="alias"):
            call(skip=sk, out=sk)
    # the well-formed calls go through
    assert conv().shape == (1, 2, 3, 5, 16) and deconv().shape == (1, 4, 6, 10, 8)
    assert raw().shape == (1, 2, 3, 5, 16) and rawt().shape == (1, 4, 6, 10, 8)
