"""conv9 (ConvTranspose3d 32 -> 16 + BN + ReLU + skip) on its persistent kernel, deconv3d_c16p_kernel, against
the one-tile-per-workgroup deconv3d_lds_kernel<32, 16, ...> it replaces at the large stage shapes: bit for bit.

Both kernels give every output the same K order (channel chunk, then the taps of its parity class, then the 4
k-steps, one MFMA chain per class), so the assertion is torch.equal on the bits, not a tolerance. Each case
runs the layer three ways: tmvs_deconv3d_bn_relu_add (the product's dispatch, which takes the persistent
kernel only from 1.5 tiles per resident workgroup on), tmvs_deconv3d_bn_relu_add_generic and
tmvs_deconv3d_bn_relu_add_persistent, the last with the device's residency as its grid and with bounded grids
that make a workgroup walk several tiles at these small shapes (fewer than 8 workgroups: one tile range; 13:
no multiple of the 8 XCDs, the remainder idles; 56: 7 per XCD over uneven XCD ranges).

Inputs are seeded random fp32 (x and skip of both signs, alpha in [0.5, 1.5) with every fourth channel negative,
shift = 0.5 randn, so the ReLU clips a share of the outputs). x and skip are slices of buffers whose other rows
are NaN and the outputs are slices of sentinel-filled buffers, so a read or a write outside the samples shows.
"""
import math

import pytest
import torch

from tests._primitives import DEV, _assert_guard, _bits, _gen, _guarded
from transmvsnet_amd import ops

pytestmark = pytest.mark.gpu
CIN, COUT = 32, 16
NAN = float("nan")

# input (B, D, H, W) -> bounded grids of the persistent route (0 = the device's residency)
DECONV9_CASES = [
    ((1, 2, 2, 16), (0,)),            # one tile
    ((1, 2, 3, 17), (0, 1, 3)),       # ragged H and W tails; 4 tiles on 1 and on 3 workgroups
    ((1, 3, 4, 33), (0, 2, 13)),      # odd depth: the 1 x 4 tile, a W tail; 9 tiles
    ((2, 4, 5, 40), (0, 3, 13)),      # batch 2: 36 tiles
    ((1, 4, 36, 72), (0, 56)),        # 180 tiles: 56 workgroups walk 3 or 4 each over XCD ranges of 22 / 23
]


def _nan_guarded(t):
    buf = torch.full((t.shape[0] + 2, *t.shape[1:]), NAN, device=DEV)
    view = buf[1:1 + t.shape[0]]
    view.copy_(t)
    assert view.is_contiguous()
    return buf, view


def _inputs(geo):
    b, d, h, w = geo
    gen = _gen(CIN, COUT, *geo)
    x = torch.randn(b, d, h, w, CIN, generator=gen)
    wpk = torch.randn(27, COUT, CIN, generator=gen) / math.sqrt(27 * CIN)
    alpha = torch.rand(COUT, generator=gen) + 0.5
    alpha[1::4] = -alpha[1::4]
    shift = 0.5 * torch.randn(COUT, generator=gen)
    skip = torch.randn(b, 2 * d, 2 * h, 2 * w, COUT, generator=gen)
    return x, wpk, alpha, shift, skip


@pytest.mark.parametrize("geo,grids", DECONV9_CASES, ids=["x".join(map(str, c[0])) for c in DECONV9_CASES])
def test_deconv9_persistent_equals_generic(geo, grids):
    b, d, h, w = geo
    x, wpk, alpha, shift, skip = _inputs(geo)
    xbuf, xd = _nan_guarded(x)
    sbuf, sd = _nan_guarded(skip)
    wd, ad, hd = wpk.to(DEV), alpha.to(DEV), shift.to(DEV)
    shape = (b, 2 * d, 2 * h, 2 * w, COUT)

    def run(tag, **route):
        obuf, out = _guarded(shape, 1)
        got = ops.deconv3d_bn_relu_add(xd, wd, ad, hd, COUT, sd, out=out, **route)
        assert got.data_ptr() == out.data_ptr()
        _assert_guard(obuf, 1, b, tag)
        return _bits(got)

    want = run("generic", route="generic")
    relu = _bits(skip) == want  # outputs the ReLU clipped to skip + 0
    assert bool(relu.any()) and not bool(relu.all())
    assert torch.equal(run("product"), want), f"product entry point != generic at {geo}"
    for mw in grids:
        got = run(f"persistent[{mw}]", route="persistent", max_workgroups=mw)
        diff = int((got != want).sum())
        assert diff == 0, f"persistent (max_workgroups {mw}) != generic at {geo}: {diff} of {want.numel()} words differ"
    assert torch.equal(_bits(xd), _bits(x)) and torch.equal(_bits(sd), _bits(skip)), "an input was written"
    for buf in (xbuf, sbuf):
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())


def test_deconv9_dispatch_takes_persistent_at_stage_shape():
    """The bench's stage-2 conv9 input (8 x 108 x 144: 1,944 tiles, from which the dispatch takes the persistent
    kernel on a device with up to 1,296 resident workgroups of it): the product entry point equals the generic
    kernel bit for bit, and so does the raw form (tmvs_conv3d_mfma: alpha 1, shift 0, no ReLU) with and without
    a skip, whose results differ by exactly the one fp32 add of the skip."""
    geo = (1, 8, 108, 144)
    gen = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(*geo, CIN, generator=gen, device=DEV)
    wpk = torch.randn(27, COUT, CIN, generator=gen, device=DEV) / math.sqrt(27 * CIN)
    alpha = torch.rand(COUT, generator=gen, device=DEV) + 0.5
    shift = 0.5 * torch.randn(COUT, generator=gen, device=DEV)
    skip = torch.randn(1, 16, 216, 288, COUT, generator=gen, device=DEV)
    want = ops.deconv3d_bn_relu_add(x, wpk, alpha, shift, COUT, skip, route="generic")
    got = ops.deconv3d_bn_relu_add(x, wpk, alpha, shift, COUT, skip)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    forced = ops.deconv3d_bn_relu_add(x, wpk, alpha, shift, COUT, skip, route="persistent")
    assert torch.equal(forced.view(torch.int32), want.view(torch.int32))
    raw = ops.conv3d_mfma(x, wpk, COUT, 2, transposed=True, skip=None)
    raw_skip = ops.conv3d_mfma(x, wpk, COUT, 2, transposed=True, skip=skip)
    assert bool((raw < 0).any())
    assert torch.equal((skip + raw).view(torch.int32), raw_skip.view(torch.int32))
    one, zero = torch.ones(COUT, device=DEV), torch.zeros(COUT, device=DEV)
    relu = ops.deconv3d_bn_relu_add(x, wpk, one, zero, COUT, skip, route="generic")
    assert torch.equal((skip + torch.relu(raw)).view(torch.int32), relu.view(torch.int32))


def test_persistent_route_rejects_other_layers():
    """Only the 32 -> 16 layer has a persistent kernel: the pinned entry point refuses conv7's and conv11's shapes."""
    for cin, cout in ((64, 32), (16, 8)):
        x = torch.zeros(1, 2, 2, 16, cin, device=DEV)
        wpk = torch.zeros(27, cout, cin, device=DEV)
        v = torch.zeros(cout, device=DEV)
        skip = torch.zeros(1, 4, 4, 32, cout, device=DEV)
        with pytest.raises(RuntimeError):
            ops.deconv3d_bn_relu_add(x, wpk, v, v, cout, skip, route="persistent")
