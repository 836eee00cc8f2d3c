"""The fused cost volume (csrc/warp_corr.hip: tmvs_warp_corr, tmvs_warp_corr_backward) and the hypothesis glue
next to it (tmvs_stage_hypotheses), entry point by entry point, at the tile tails, image borders and dispatch
cases the whole-network tests never reach.

Shapes (H, W): (5, 5), (3, 43), (17, 15), (9, 29), i.e. 25, 129, 255 and 261 pixels: less than one wave;
one more than a block of 32, 64 or 128 pixels; one less than every forward block and than the backward's 256;
256 + 5. Every height and width is odd. The given-weights case at vw_shift = 1 needs even sizes: (10, 26).

Hypotheses ("the mix"): per pixel sorted random planes over [425, 935), with a patch of decreasing planes, a
patch (holding the last pixel) with one plane behind the camera, a patch whose planes span the whole range and
a patch on the left border whose planes alternate between 430 and 930 mm (the tap changes on every plane).
Each test asserts from the oracle's own warp_grid that at least half of all samples have their 4 taps inside
the image and at least 5 % have a tap outside.

Border rig: reference E = K = I, source K = I and E = I + translation (sx d0, sy d0, 0), planes at d0 = 512
(lower half of D) and 1024 (upper half), so a sample lands at the pixel plus the shift (512) or half of it
(1024): exactly on integers for most pixels and within an ulp of one for the rest; shifts (0, 0), (-0.5, 0),
(1, 1), (0.25, -0.75), (W, 0), (-1, 0). The (W, 0) view is outside the image on every 512 plane.

Every output is a slice of a larger buffer whose other rows hold a sentinel that must survive bit for bit
(rows of a shared view-weight map that belong to another call's views included); every input sits between
NaN pads, so a read outside it poisons the result.

Group, bar, where the bar comes from, largest value measured on an MI355X (133 tests, about 4 s):
  forward vs oracle.build_cost_volume (the fp32 oracle, pinned to the reference's goldens; the kernel
    reproduces its coordinate rounding): 5e-7 abs on similarity and view weights, the bar of
    tests/test_gpu_parity.py. Dispatch matrix (all 36 instantiations): sim 2.4e-7, view weights 6.0e-8. Tap
    cache (C = 32, given weights): 1.1e-7; the oracle itself is 3.9e-7 from an fp64 evaluation of the same
    fp32 samples, so max(5e-7, 2 x that) would be 7.8e-7, but no case exceeded 5e-7 and the bar stays there.
    Border rig: 8.9e-8, the outside view exactly 0. Batch 2: 1.2e-7. The golden per-view similarity under the
    fixtures' rotation order: 1.8e-7 (the other order moves the similarity by up to 7.0e-7).
  tap cache vs no cache (the stage-1 kernel with a PixelwiseNet that gives every view the same weight):
    1e-6 = twice the 5e-7 each holds against the oracle; measured 4.5e-8.
  view-sharded vs unsharded: view weights bitwise; aggregate_finalize of the partial sums 2e-6 abs
    (tests/test_gpu_parity.py); measured 6.0e-8. Batch 2: each sample bitwise its own batch-1 call.
  backward vs torch autograd through oracle.homo_warping + mean (CPU fp32), the bars of
    test_warp_corr_views_forward_backward: sim 2e-5 abs, dref and dsrc 1e-5 of the gradient's max.
    Scatter: dref 1.5e-7, dsrc 4.3e-7 (two calls bitwise equal, flag word 0); border rig 1.7e-7, 2.9e-7, the
    outside view's dsrc exactly 0; planes 4.2e-7, 5.9e-7, with dref bitwise the scatter call's and dsrc 3.6e-7
    from it (bar 1e-5); warp_corr_views sims 1.2e-7, dref 1.8e-7, dsrc 3.4e-7.
  tmvs_stage_hypotheses vs oracle.stage_hypotheses: bit-exact, either side of the output size (H + W = 128) at
    which torch's CPU up-sampling changes its fp32 op order: see test_stage_hypotheses_ragged, which found the
    kernel following one order only.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import transmvs_ref as oracle
from tests._primitives import DEV, SENTINEL, _assert_guard, _bits, _gen, _guarded, _rel
from tests._util import GOLDEN_ROT_ORDER, golden, golden_state_dict
from transmvsnet_amd import TransMVSNet, _lib, ops, synthetic

pytestmark = pytest.mark.gpu
SHAPES = ((5, 5), (3, 43), (17, 15), (9, 29))
SIM_BAR = 5e-7      # similarity and view weights against the fp32 oracle (tests/test_gpu_parity.py)
SHARD_BAR = 2e-6    # sharded + finalize against unsharded (tests/test_gpu_parity.py)
NAN = float("nan")
NAN_PAD = 64        # floats: keeps the 16-byte alignment of the float4 loads


# ------------------------------------------------------------------------------------------------- inputs
def _cams(n_views, h, w, seed, batch=1):
    """the synthetic DTU rig at the feature resolution h x w"""
    return synthetic.synthetic_cameras(n_views, 4 * h, 4 * w, batch=batch, seed=seed)["stage1"]


def _hyp_mix(d, h, w, g):
    hyp = torch.sort(torch.rand(d, h, w, generator=g) * 510.0 + 425.0, dim=0).values
    hyp[:, 0:2, 1:4] = hyp[:, 0:2, 1:4].flip(0)                                     # decreasing
    hyp[d // 2, h - 2:h, w - 3:w] = -30.0                                           # behind the camera
    hyp[:, h // 2, w // 2:w // 2 + 3] = torch.linspace(425.0, 930.0, d).view(d, 1)  # the whole range
    zig = torch.where(torch.arange(d) % 2 == 0, 430.0, 930.0)
    hyp[:, h // 2, 0:2] = zig.view(d, 1)                                            # alternating near / far
    return hyp.contiguous()


def _border_proj(w):
    shifts = ((0.0, 0.0), (-0.5, 0.0), (1.0, 1.0), (0.25, -0.75), (float(w), 0.0), (-1.0, 0.0))
    proj = torch.zeros(1, 1 + len(shifts), 2, 4, 4)
    proj[:, :, 0] = torch.eye(4)
    proj[:, :, 1] = torch.eye(4)
    for v, (sx, sy) in enumerate(shifts):
        proj[0, 1 + v, 0, 0, 3] = sx * 512.0
        proj[0, 1 + v, 0, 1, 3] = sy * 512.0
    return proj


BORDER_OUTSIDE = 4  # index of the (W, 0) source view


def _border_hyp(d, h, w):
    plane = torch.where(torch.arange(d) < d // 2, 512.0, 1024.0)
    return plane.view(1, d, 1, 1).expand(1, d, h, w).contiguous()


def _sample_xy(proj, hyp):
    """per source view the oracle's own sample coordinates (ix, iy), fp32, each [B, D, h, w]"""
    b, d, h, w = hyp.shape
    projs = torch.unbind(proj, 1)
    out = []
    for sp in projs[1:]:
        grid = oracle.warp_grid(oracle.compose_proj(sp), oracle.compose_proj(projs[0]), hyp, h, w).view(b, d, h, w, 2)
        out.append(((grid[..., 0] + 1) * ((w - 1) / 2), (grid[..., 1] + 1) * ((h - 1) / 2)))
    return out


def _tap_share(proj, hyp):
    """(share of samples with all 4 taps inside the image, share with all 4 outside)"""
    h, w = hyp.shape[2:]
    full, none, total = 0, 0, 0
    for ix, iy in _sample_xy(proj, hyp):
        x0, y0 = torch.floor(ix), torch.floor(iy)
        full += int(((x0 >= 0) & (x0 + 1 <= w - 1) & (y0 >= 0) & (y0 + 1 <= h - 1)).sum())
        none += int(((x0 + 1 < 0) | (x0 > w - 1) | (y0 + 1 < 0) | (y0 > h - 1)).sum())
        total += ix.numel()
    return full / total, none / total


def _assert_mix(proj, hyp, what):
    full, none = _tap_share(proj, hyp)
    print(f"{what}: {100 * full:.0f} % of the samples have 4 taps inside, {100 * (1 - full):.0f} % a tap outside "
          f"({100 * none:.0f} % all 4)")
    assert full >= 0.5 and 1.0 - full >= 0.05, (what, full)


@functools.lru_cache(maxsize=None)
def _case(c, d, h, w, nsrc, seed, batch=1, hyps="mix"):
    """(feats: nsrc + 1 tensors [B, c, h, w], proj [B, nsrc + 1, 2, 4, 4], hyp [B, d, h, w]); shared, never modified"""
    g = _gen(c, d, h, w, nsrc, seed)
    feats = tuple(torch.randn(batch, c, h, w, generator=g) for _ in range(nsrc + 1))
    if hyps == "border":
        return feats, _border_proj(w), _border_hyp(d, h, w)
    proj = _cams(nsrc + 1, h, w, seed=seed, batch=batch)
    if hyps == "planes":
        hyp = torch.linspace(425.0, 935.0, d).view(1, d, 1, 1).expand(batch, d, h, w).contiguous()
    else:
        hyp = torch.stack([_hyp_mix(d, h, w, g) for _ in range(batch)])
    return feats, proj, hyp


def _weights(b, nsrc, h, w, *seed):
    return torch.rand(b, nsrc, h, w, generator=_gen(b, nsrc, h, w, *seed))


@pytest.fixture(scope="module")
def sd():
    return golden_state_dict()


@pytest.fixture(scope="module")
def pw(sd):
    m = TransMVSNet()
    m.load_state_dict(sd, strict=True)
    return m.DepthNet.pixel_wise_net.packed()


# ------------------------------------------------------------------------------------------------- device side
def _nan_in(t):
    """the CPU tensor `t` on the device between two pads of NaN"""
    n = t.numel()
    buf = torch.full((n + 2 * NAN_PAD,), NAN, device=DEV)
    view = buf[NAN_PAD:NAN_PAD + n].view(t.shape)
    view.copy_(t)
    return view


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _sentinel_rows(t):
    return torch.equal(_bits(t), _bits(torch.full(tuple(t.shape), SENTINEL)))


def _fwd(feats, proj, hyp, *, pw=None, vw=None, shift=0, offset=0, total=None, partial=False, rot_order="auto",
         vw_out=None):
    """ops.warp_corr on guarded buffers -> (sim [B,D,h,w] CPU, wsum [B,h,w] CPU or None, view weights of this call's
    views [B,nsrc,h,w] CPU or None). vw_out: a (buffer, view) pair from _guarded shared between calls."""
    b, d, h, w = hyp.shape
    nsrc = len(feats) - 1
    total = nsrc if total is None else total
    ref = _nan_in(_nhwc(feats[0]))
    src = _nan_in(torch.stack([_nhwc(f) for f in feats[1:]], 1))
    rows = ops.proj_rows(proj)
    sim_buf, sim = _guarded((b, d, h, w), 1)
    ws_buf, wsum = _guarded((b, h, w), 1) if partial else (None, None)
    kw = dict(vw_offset=offset, vw_total=total, partial=partial, sim_out=sim, wsum_out=wsum, rot_order=rot_order)
    if vw is None:
        vo_buf, vo = _guarded((b, total, h, w), 1) if vw_out is None else vw_out
        ops.warp_corr(ref, src, rows, _nan_in(hyp), pw_params=pw, view_w_out=vo, **kw)
    else:
        assert tuple(vw.shape) == (b, total, h >> shift, w >> shift)
        ops.warp_corr(ref, src, rows, _nan_in(hyp), view_w_in=_nan_in(vw), vw_shift=shift, **kw)
    torch.cuda.synchronize()
    _assert_guard(sim_buf, 1, b, "sim_out")
    if partial:
        _assert_guard(ws_buf, 1, b, "wsum_out")
    got_vw = None
    if vw is None:
        _assert_guard(vo_buf, 1, b, "view_w_out")
        if vw_out is None:
            assert _sentinel_rows(vo[:, :offset]) and _sentinel_rows(vo[:, offset + nsrc:]), \
                "view_w_out: rows of other calls' views were written"
        got_vw = vo[:, offset:offset + nsrc].cpu()
    return sim.cpu(), (wsum.cpu() if partial else None), got_vw


def _close(got, ref, atol, what):
    """assert max |got - ref| <= atol, printing the deviation and where it is"""
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    e = (got.double() - ref.double()).abs()
    err = float(e.max())
    at = tuple(int(i) for i in np.unravel_index(int(e.argmax()), tuple(e.shape)))
    print(f"{what}: max abs err {err:.2e} at {at} of {tuple(e.shape)} (bound {atol:.0e})")
    assert err <= atol, (what, err, at, atol)
    return err


def _oracle(sd, feats, proj, hyp, vw=None):
    with torch.no_grad():
        sim, vw_ref = oracle.build_cost_volume(sd, list(feats), proj, hyp, view_weights=vw)
    return sim[:, 0], vw_ref


def _oracle64(feats, proj, hyp, vw):
    """the similarity of the oracle's own fp32 samples evaluated in fp64 (features, interpolation, sums)"""
    b, d, h, w = hyp.shape
    projs = torch.unbind(proj, 1)
    ref = feats[0].double()
    num, den = 0.0, 1e-5
    for i, sp in enumerate(projs[1:]):
        grid = oracle.warp_grid(oracle.compose_proj(sp), oracle.compose_proj(projs[0]), hyp, h, w).double()
        warped = F.grid_sample(feats[1 + i].double(), grid, mode="bilinear", padding_mode="zeros",
                               align_corners=True).view(b, -1, d, h, w)
        wv = vw[:, i:i + 1].double()
        num = num + (warped * ref.unsqueeze(2)).mean(1) * wv
        den = den + wv
    return num / den


def _check_fwd(sd, pw, case, given, what, seed=0):
    """one unsharded call in either mode against the oracle"""
    feats, proj, hyp = case
    b, d, h, w = hyp.shape
    if given:
        vw = _weights(b, len(feats) - 1, h, w, seed)
        sim_ref, _ = _oracle({}, feats, proj, hyp, vw)
        sim, _, _ = _fwd(feats, proj, hyp, vw=vw)
        return _close(sim, sim_ref, SIM_BAR, f"{what} given sim")
    sim_ref, vw_ref = _oracle(sd, feats, proj, hyp)
    sim, _, vw_got = _fwd(feats, proj, hyp, pw=pw)
    _close(vw_got, vw_ref, SIM_BAR, f"{what} pw view weights")
    return _close(sim, sim_ref, SIM_BAR, f"{what} pw sim")


# ------------------------------------------------------------------------------------------------- forward
DEPTHS = (8, 16, 24, 32, 48, 64)
ROTATE = ((5, 5), (3, 43), (17, 15))


@pytest.mark.parametrize("given", [False, True], ids=["pw", "given"])
@pytest.mark.parametrize("c,d", [(c, d) for c in (8, 16, 32) for d in DEPTHS])
def test_dispatch_matrix(sd, pw, c, d, given):
    """Every (C, D, mode) instantiation of dispatch_depth on (9, 29) and on a second shape that rotates with D,
    so each of warp_corr_kernel<32>, <16>, <8> and warp_pair_kernel<16>, <8> meets all four shapes."""
    for h, w in ((9, 29), ROTATE[DEPTHS.index(d) % 3]):
        case = _case(c, d, h, w, 2, 1)
        _assert_mix(case[1], case[2], f"c{c} d{d} {h}x{w}")
        _check_fwd(sd, pw, case, given, f"dispatch c{c} d{d} {h}x{w}")


@pytest.mark.parametrize("h,w", SHAPES)
def test_tap_cache(h, w):
    """fetch_reuse (C = 32 with given weights) on the mix with 3 views and D = 32: against the oracle, and against
    fetch_full through the stage-1 kernel, whose PixelwiseNet here maps every similarity to the logit 0.3, so
    every view gets one weight; that weight map, fed back as given weights, makes the two calls differ in the
    order of the 4 taps only. Prints the oracle's own distance from fp64."""
    feats, proj, hyp = case = _case(32, 32, h, w, 3, 2)
    _assert_mix(proj, hyp, f"tap cache {h}x{w}")
    _check_fwd(None, None, case, True, f"tap cache {h}x{w}", seed=7)
    const = np.zeros(_lib.PW_NPARAMS, np.float32)
    const[200] = 0.3
    sim_full, _, vw_const = _fwd(feats, proj, hyp, pw=const)
    assert bool((vw_const == vw_const.flatten()[0]).all()) and 0.5 < float(vw_const.flatten()[0]) < 0.6
    sim_ref, _ = _oracle({}, feats, proj, hyp, vw_const)
    print(f"tap cache {h}x{w}: the fp32 oracle is {float((sim_ref.double() - _oracle64(feats, proj, hyp, vw_const)).abs().max()):.2e} from fp64")
    _close(sim_full, sim_ref, SIM_BAR, f"tap cache {h}x{w} fetch_full sim")
    sim_reuse, _, _ = _fwd(feats, proj, hyp, vw=vw_const)
    _close(sim_reuse, sim_ref, SIM_BAR, f"tap cache {h}x{w} fetch_reuse sim")
    _close(sim_reuse, sim_full, 2 * SIM_BAR, f"tap cache {h}x{w} fetch_reuse vs fetch_full")


@pytest.mark.parametrize("given", [False, True], ids=["pw", "given"])
@pytest.mark.parametrize("c", [8, 16, 32])
@pytest.mark.parametrize("h,w", [(9, 29), (17, 15)])
def test_border_rig(sd, pw, h, w, c, given):
    """Samples exactly on pixels, on the last row and column (x0 + 1 == W reads zero with weight zero), half a
    pixel outside either edge and a whole view outside: against the oracle, and the outside view alone
    (one view, PARTIAL: the similarity times its weight) exactly 0 on the 512 planes."""
    d = 8
    feats, proj, hyp = case = _case(c, d, h, w, 6, 3, hyps="border")
    xs = torch.stack([ix for ix, _ in _sample_xy(proj, hyp)])
    on_int = float((xs == torch.round(xs)).float().mean())
    near = float(((xs - torch.round(xs)).abs() <= 4e-6).float().mean())
    print(f"border {h}x{w}: {100 * on_int:.0f} % of the x coordinates are integers, {100 * near:.0f} % within 4e-6 of one")
    assert on_int >= 0.25 and float(xs.min()) < 0 and float(xs.max()) > w - 1 and bool((xs == w - 1).any())
    _check_fwd(sd, pw, case, given, f"border c{c} {h}x{w}")
    o = BORDER_OUTSIDE
    one = (feats[0], feats[1 + o])
    proj1 = proj[:, [0, 1 + o]]
    sim_ref, _ = _oracle({}, one, proj1, hyp, torch.ones(1, 1, h, w))   # weight 1, w_sum 1 + 1e-5
    assert bool((sim_ref[:, :d // 2] == 0).all()) and bool((sim_ref[:, d // 2:] != 0).any())
    if given:
        sim, wsum, _ = _fwd(one, proj1, hyp, vw=torch.ones(1, 1, h, w), partial=True)
    else:
        sim, wsum, vw1 = _fwd(one, proj1, hyp, pw=pw, partial=True)
        assert torch.equal(wsum, vw1[:, 0])
    assert bool((sim[:, :d // 2] == 0).all()), "the view outside the image contributes to the similarity"
    assert bool((sim[:, d // 2:] != 0).any())


@pytest.mark.parametrize("c,d", [(32, 48), (8, 8)])
@pytest.mark.parametrize("h,w", [(17, 15), (3, 43)])
def test_stage1_view_sharding(sd, pw, h, w, c, d):
    """PW && PARTIAL as distributed._hip_partial runs it: views 0-1 and 2-3 in two calls that share one
    view_w_out through vw_offset / vw_total."""
    feats, proj, hyp = _case(c, d, h, w, 4, 4)
    _assert_mix(proj, hyp, f"sharding c{c} {h}x{w}")
    sim, _, vw = _fwd(feats, proj, hyp, pw=pw)
    sim_ref, vw_ref = _oracle(sd, feats, proj, hyp)
    _close(vw, vw_ref, SIM_BAR, f"sharding c{c} {h}x{w} unsharded view weights")
    _close(sim, sim_ref, SIM_BAR, f"sharding c{c} {h}x{w} unsharded sim")
    shared = _guarded((1, 4, h, w), 1)
    fa, fb = (feats[0], *feats[1:3]), (feats[0], *feats[3:5])
    pa, pb = proj[:, [0, 1, 2]], proj[:, [0, 3, 4]]
    s_a, w_a, vw_a = _fwd(fa, pa, hyp, pw=pw, partial=True, offset=0, total=4, vw_out=shared)
    assert _sentinel_rows(shared[1][:, 2:]), "the first shard wrote the second shard's view weights"
    s_b, w_b, vw_b = _fwd(fb, pb, hyp, pw=pw, partial=True, offset=2, total=4, vw_out=shared)
    assert torch.equal(_bits(shared[1][:, :2]), _bits(vw_a)), "the second shard wrote the first shard's view weights"
    assert torch.equal(_bits(shared[1][0]), _bits(vw[0])), "sharded view weights differ from the unsharded call's"
    _fwd(fb, pb, hyp, pw=pw, partial=True, offset=2, total=4)  # own buffer: rows 0-1 must keep the sentinel
    fin = ops.aggregate_finalize((s_a + s_b).to(DEV), (w_a + w_b).to(DEV)).cpu()
    _close(fin, sim, SHARD_BAR, f"sharding c{c} {h}x{w} finalize vs unsharded")


@pytest.mark.parametrize("mode", ["pw", "pw_partial", "given_shift1", "given_shift1_partial"])
@pytest.mark.parametrize("c,d", [(32, 48), (16, 32), (8, 8)])
def test_batch_of_two(sd, pw, c, d, mode):
    """batch = 2 passed to tmvs_warp_corr directly (per-sample strides of view_w_in, view_w_out, wsum_out) with
    different cameras, features, hypotheses and weights per sample, the views at rows 1.. of a map one row
    larger (row 0: sentinel on output, NaN on input): each sample bitwise its own batch-1 call and within the
    bar of the oracle."""
    given, partial = mode.startswith("given"), mode.endswith("partial")
    h, w = (10, 26) if given else (9, 29)
    nsrc = 2
    feats, proj, hyp = _case(c, d, h, w, nsrc, 5, batch=2)
    _assert_mix(proj, hyp, f"batch2 c{c} {mode}")
    assert not torch.equal(proj[0], proj[1]) and not torch.equal(hyp[0], hyp[1])
    kw = dict(offset=1, total=nsrc + 1)
    if given:
        vw = torch.cat([torch.full((2, 1, h // 2, w // 2), NAN), _weights(2, nsrc, h // 2, w // 2, 9)], 1)
        up = F.interpolate(vw[:, 1:], scale_factor=2, mode="nearest")
        sim_ref, vw_ref = _oracle({}, feats, proj, hyp, up)
        run = lambda f, p, hy, s, part: _fwd(f, p, hy, vw=vw[s], shift=1, partial=part, **kw)
    else:
        sim_ref, vw_ref = _oracle(sd, feats, proj, hyp)
        run = lambda f, p, hy, s, part: _fwd(f, p, hy, pw=pw, partial=part, **kw)
    sim, wsum, vw_got = run(feats, proj, hyp, slice(0, 2), partial)
    for i in range(2):
        s = slice(i, i + 1)
        sim1, wsum1, vw1 = run(tuple(f[s] for f in feats), proj[s], hyp[s], s, partial)
        assert torch.equal(_bits(sim[s]), _bits(sim1)), f"sample {i}: sim differs from its batch-1 call"
        if partial:
            assert torch.equal(_bits(wsum[s]), _bits(wsum1)), f"sample {i}: wsum differs from its batch-1 call"
        if not given:
            assert torch.equal(_bits(vw_got[s]), _bits(vw1)), f"sample {i}: view weights differ from its batch-1 call"
    if not given:
        _close(vw_got, vw_ref, SIM_BAR, f"batch2 c{c} {mode} view weights")
    if partial:  # held to the unsharded batch-2 call, which is held to the oracle
        whole, _, _ = run(feats, proj, hyp, slice(0, 2), False)
        _close(whole, sim_ref, SIM_BAR, f"batch2 c{c} {mode} unsharded sim")
        fin = ops.aggregate_finalize(sim.to(DEV), wsum.to(DEV)).cpu()
        _close(fin, whole, SHARD_BAR, f"batch2 c{c} {mode} finalize(partial) vs unsharded")
    else:
        _close(sim, sim_ref, SIM_BAR, f"batch2 c{c} {mode} sim")


@pytest.mark.parametrize("c,d", [(32, 8), (16, 16), (8, 24)])
def test_rotation_order(sd, pw, c, d):
    """Both roundings of rot (x, y, 1). The oracle computes this host's only (ops.host_rot_order), so that order,
    passed by name, must give the bits of "auto" and hold the bar; the other order has no reference here and is
    held to itself: sharded view weights bitwise the unsharded ones, finalize within the sharding bar."""
    h, w = 9, 29
    feats, proj, hyp = _case(c, d, h, w, 2, 6)
    host = ops.host_rot_order(h * w)
    other = "plain" if host == "fma" else "fma"
    sim_ref, vw_ref = _oracle(sd, feats, proj, hyp)
    sim_auto, _, vw_auto = _fwd(feats, proj, hyp, pw=pw)
    sim_host, _, vw_host = _fwd(feats, proj, hyp, pw=pw, rot_order=host)
    assert torch.equal(_bits(sim_auto), _bits(sim_host)) and torch.equal(_bits(vw_auto), _bits(vw_host))
    _close(sim_host, sim_ref, SIM_BAR, f"rot_order {host} (host) c{c} sim")
    _close(vw_host, vw_ref, SIM_BAR, f"rot_order {host} (host) c{c} view weights")
    sim_o, _, vw_o = _fwd(feats, proj, hyp, pw=pw, rot_order=other)
    print(f"rot_order {other} c{c}: max |sim - host order's| {float((sim_o - sim_host).abs().max()):.2e}")
    s_a, w_a, vw_a = _fwd(feats[:2], proj[:, :2], hyp, pw=pw, partial=True, rot_order=other)
    s_b, w_b, vw_b = _fwd((feats[0], feats[2]), proj[:, [0, 2]], hyp, pw=pw, partial=True, rot_order=other)
    assert torch.equal(_bits(torch.cat([vw_a, vw_b], 1)), _bits(vw_o))
    fin = ops.aggregate_finalize((s_a + s_b).to(DEV), (w_a + w_b).to(DEV)).cpu()
    _close(fin, sim_o, SHARD_BAR, f"rot_order {other} c{c} finalize vs unsharded")


def test_rotation_order_golden():
    """The fixtures' rounding by name (tests/_util.GOLDEN_ROT_ORDER) against the golden per-view similarity:
    one view, weight 1, PARTIAL, so sim_out is that view's similarity."""
    g = {k: torch.from_numpy(v) for k, v in golden("ops.npz").items()}
    b, c, h, w = g["warp_src"].shape
    sim, wsum, _ = _fwd((g["warp_ref"], g["warp_src"]), g["warp_proj"], g["warp_hyp"], vw=torch.ones(b, 1, h, w),
                        partial=True, rot_order=GOLDEN_ROT_ORDER)
    assert bool((wsum == 1).all())
    _close(sim, g["warp_sim"][:, 0], SIM_BAR, f"golden warp_sim c{c} {h}x{w} ({GOLDEN_ROT_ORDER})")


# ------------------------------------------------------------------------------------------------- backward
def _dsim(nsrc, d, h, w, *seed):
    """d loss / d sim_v with exact zeros: a patch on every plane, another patch on every other plane (not the last
    pixel, which the lanes past the image are clamped to: its gradient stays non-zero on every plane)"""
    dsim = torch.randn(nsrc, d, h, w, generator=_gen(nsrc, d, h, w, *seed))
    dsim[:, :, 0:2, 0:3] = 0.0
    dsim[:, ::2, h - 2:h, w - 4:w - 1] = 0.0
    return dsim


@functools.lru_cache(maxsize=None)
def _autograd(c, d, h, w, nsrc, seed, hyps="mix"):
    """(per-view similarities [nsrc, d, h, w], dref [c, h, w], dsrc [nsrc, c, h, w]) by torch autograd through the
    oracle's homo_warping + mean, CPU fp32"""
    feats, proj, hyp = _case(c, d, h, w, nsrc, seed, hyps=hyps)
    dsim = _dsim_of(c, d, h, w, nsrc, seed, hyps)
    xs = [f.clone().requires_grad_() for f in feats]
    projs = torch.unbind(proj, 1)
    sims = []
    for i in range(nsrc):
        warped = oracle.homo_warping(xs[1 + i], oracle.compose_proj(projs[1 + i]), oracle.compose_proj(projs[0]), hyp)
        sims.append((warped * xs[0].unsqueeze(2)).mean(1))
    sims = torch.cat(sims, 0)
    sims.backward(dsim)
    return sims.detach(), xs[0].grad[0], torch.stack([x.grad[0] for x in xs[1:]])


def _dsim_of(c, d, h, w, nsrc, seed, hyps):
    dsim = _dsim(nsrc, d, h, w, c, seed)
    if hyps == "border":
        dsim[BORDER_OUTSIDE, d // 2:] = 0.0  # the (W, 0) view is inside the image on the 1024 planes
    return dsim


def _bwd(feats, proj, hyp, dsim, planes=False):
    """ops.warp_corr_backward on guarded buffers -> (dref [c,h,w], dsrc [nsrc,c,h,w], flag word), CPU"""
    _, c, h, w = feats[0].shape
    nsrc = len(feats) - 1
    ref = _nan_in(feats[0][0].permute(1, 2, 0).contiguous())
    src = _nan_in(torch.stack([f[0].permute(1, 2, 0) for f in feats[1:]]).contiguous())
    dr_buf, dref = _guarded((h, w, c), 2)
    ds_buf, dsrc = _guarded((nsrc, h, w, c), 1)
    _, _, flag = ops.warp_corr_backward(ref, src, ops.proj_rows(proj)[0], _nan_in(hyp[0]), _nan_in(dsim), planes=planes,
                                        dref_out=dref, dsrc_out=dsrc)
    torch.cuda.synchronize()
    _assert_guard(dr_buf, 2, h, "dref")
    _assert_guard(ds_buf, 1, nsrc, "dsrc")
    dref, dsrc = dref.cpu(), dsrc.cpu()
    assert bool(torch.isfinite(dref).all()) and bool(torch.isfinite(dsrc).all())
    return dref.permute(2, 0, 1), dsrc.permute(0, 3, 1, 2), int(flag.item())


def _hold_grads(what, dref, dsrc, dref_ref, dsrc_ref):
    e_ref = _rel(dref, dref_ref)
    e_src = max(_rel(dsrc[i], dsrc_ref[i]) for i in range(dsrc.shape[0]))
    print(f"{what}: dref {e_ref:.2e}, dsrc {e_src:.2e} of the gradient's max (bound 1e-05)")
    assert e_ref < 1e-5 and e_src < 1e-5, (what, e_ref, e_src)


def _reentries(proj, hyp):
    """pixel-views whose sample is inside the image, then has all 4 taps outside, then is inside again along D"""
    h, w = hyp.shape[2:]
    n = 0
    for ix, iy in _sample_xy(proj, hyp):
        x0, y0 = torch.floor(ix), torch.floor(iy)
        out = ((x0 + 1 < 0) | (x0 > w - 1) | (y0 + 1 < 0) | (y0 > h - 1))[0]
        seen_in = torch.cummax((~out).int(), 0).values.bool()
        later_in = torch.cummax((~out).int().flip(0), 0).values.bool().flip(0)
        n += int((out & seen_in & later_in).any(0).sum())
    return n


BWD_C, BWD_D = (8, 16, 32), (3, 4, 8, 12, 24)
# each C meets each D and each shape; the 5 last cases complete the 20 (D, shape) pairs
SCATTER = [(c, d, SHAPES[(i + ci) % 4]) for ci, c in enumerate(BWD_C) for i, d in enumerate(BWD_D)] + \
          [(BWD_C[i % 3], d, SHAPES[(i + 3) % 4]) for i, d in enumerate(BWD_D)]


@pytest.mark.parametrize("c,d,hw", SCATTER, ids=[f"c{c}-d{d}-{h}x{w}" for c, d, (h, w) in SCATTER])
def test_backward_scatter(c, d, hw):
    """tmvs_warp_corr_backward's fixed-point scatter with a partial last wave (`live`, pc = HW - 1, zero sref rows,
    the ballot), plane chunks that do not divide D (3, 4 < 8; 12 = 8 + 4), exact zeros in dsim and the mix, in
    which some pixel's taps leave the source image and come back along its planes (a slot flushed on a changed
    tap with an outside key in between)."""
    h, w = hw
    feats, proj, hyp = _case(c, d, h, w, 2, 7)
    _assert_mix(proj, hyp, f"scatter c{c} d{d} {h}x{w}")
    assert _reentries(proj, hyp) >= 1
    dsim = _dsim_of(c, d, h, w, 2, 7, "mix")
    _, dref_ref, dsrc_ref = _autograd(c, d, h, w, 2, 7)
    dref, dsrc, flag = _bwd(feats, proj, hyp, dsim)
    assert flag == 0, flag
    _hold_grads(f"scatter c{c} d{d} {h}x{w}", dref, dsrc, dref_ref, dsrc_ref)
    dref2, dsrc2, _ = _bwd(feats, proj, hyp, dsim)
    assert torch.equal(_bits(dref), _bits(dref2)) and torch.equal(_bits(dsrc), _bits(dsrc2)), "two calls differ"


@pytest.mark.parametrize("c", [8, 32])
@pytest.mark.parametrize("h,w", [(9, 29), (17, 15)])
def test_backward_border_rig(h, w, c):
    """the border rig through the scatter: integer coordinates (taps of weight exactly 0), samples on the last row
    and column, and a view outside the image wherever its dsim is not zero, whose dsrc must be exactly 0"""
    d = 8
    feats, proj, hyp = _case(c, d, h, w, 6, 3, hyps="border")
    dsim = _dsim_of(c, d, h, w, 6, 3, "border")
    _, dref_ref, dsrc_ref = _autograd(c, d, h, w, 6, 3, hyps="border")
    assert bool((dsrc_ref[BORDER_OUTSIDE] == 0).all()) and bool((dsrc_ref[BORDER_OUTSIDE - 1] != 0).any())
    dref, dsrc, flag = _bwd(feats, proj, hyp, dsim)
    assert flag == 0, flag
    _hold_grads(f"border backward c{c} {h}x{w}", dref, dsrc, dref_ref, dsrc_ref)
    assert bool((dsrc[BORDER_OUTSIDE] == 0).all()), "the view outside the image received a gradient"


PLANES_D = (3, 5, 8, 24, 64)
PLANES = [(BWD_C[(i + j) % 3], d, hw) for i, d in enumerate(PLANES_D) for j, hw in enumerate(SHAPES)]


@pytest.mark.parametrize("c,d,hw", PLANES, ids=[f"c{c}-d{d}-{h}x{w}" for c, d, (h, w) in PLANES])
def test_backward_planes(c, d, hw):
    """TMVS_WARP_BWD_PLANES (d src gathered per texel) with a ragged last block of 64 texels and plane quarters
    that leave waves without planes (D = 3, 5): against autograd and against the scatter of the same call."""
    h, w = hw
    feats, proj, hyp = _case(c, d, h, w, 2, 8, hyps="planes")
    dsim = _dsim_of(c, d, h, w, 2, 8, "planes")
    _, dref_ref, dsrc_ref = _autograd(c, d, h, w, 2, 8, hyps="planes")
    dref, dsrc, flag = _bwd(feats, proj, hyp, dsim, planes=True)
    assert flag == 0, flag
    _hold_grads(f"planes c{c} d{d} {h}x{w}", dref, dsrc, dref_ref, dsrc_ref)
    dref_s, dsrc_s, _ = _bwd(feats, proj, hyp, dsim)
    vs = max(_rel(dsrc[i], dsrc_s[i]) for i in range(2))
    print(f"planes c{c} d{d} {h}x{w}: dsrc vs scatter {vs:.2e} (bound 1e-05)")
    assert vs < 1e-5, vs
    assert torch.equal(_bits(dref), _bits(dref_s)), "dref differs from the scatter call's"


def test_backward_planes_depth_limit():
    """planes with D = 65 > 64 is TMVS_ERR_SHAPE and nothing is written"""
    h, w, c, d = 5, 5, 8, 65
    feats, proj, hyp = _case(c, d, h, w, 2, 8, hyps="planes")
    dr_buf, dref = _guarded((h, w, c), 2)
    ds_buf, dsrc = _guarded((2, h, w, c), 1)
    with pytest.raises(RuntimeError, match=r"unsupported shape \(-2\)"):
        ops.warp_corr_backward(_nan_in(feats[0][0].permute(1, 2, 0).contiguous()),
                               _nan_in(torch.stack([f[0].permute(1, 2, 0) for f in feats[1:]]).contiguous()),
                               ops.proj_rows(proj)[0], _nan_in(hyp[0]), _nan_in(_dsim(2, d, h, w, 1)), planes=True,
                               dref_out=dref, dsrc_out=dsrc)
    torch.cuda.synchronize()
    assert _sentinel_rows(dr_buf) and _sentinel_rows(ds_buf)


@pytest.mark.parametrize("c,d,hw,planes", [(32, 24, (9, 29), False), (16, 8, (17, 15), False), (8, 16, (3, 43), False),
                                           (32, 8, (5, 5), True)])
def test_warp_corr_views_ragged(c, d, hw, planes):
    """train.warp_corr_views (forward: one view per launch, weight 1, PARTIAL; backward: the entry point above)"""
    from transmvsnet_amd.train import warp_corr_views
    h, w = hw
    hyps = "planes" if planes else "mix"
    feats, proj, hyp = _case(c, d, h, w, 2, 9, hyps=hyps)
    dsim = _dsim_of(c, d, h, w, 2, 9, hyps)
    sims_ref, dref_ref, dsrc_ref = _autograd(c, d, h, w, 2, 9, hyps=hyps)
    ref_g = feats[0][0].permute(1, 2, 0).contiguous().to(DEV).requires_grad_()
    src_g = torch.stack([f[0].permute(1, 2, 0) for f in feats[1:]]).contiguous().to(DEV).requires_grad_()
    sims = warp_corr_views(ref_g, src_g, hyp[0].to(DEV), ops.proj_rows(proj)[0], planes=planes)
    sims.backward(dsim.to(DEV))
    torch.cuda.synchronize()
    _close(sims.detach().cpu(), sims_ref, 2e-5, f"warp_corr_views c{c} d{d} {h}x{w} sims")
    _hold_grads(f"warp_corr_views c{c} d{d} {h}x{w}", ref_g.grad.cpu().permute(2, 0, 1),
                src_g.grad.cpu().permute(0, 3, 1, 2), dref_ref, dsrc_ref)


# ------------------------------------------------------------------------------------------------- hypothesis glue
@pytest.mark.parametrize("stage", [1, 2, 3])
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("full", [(52, 76), (52, 84)], ids=["52x76", "52x84"])
def test_stage_hypotheses_ragged(full, batch, stage):
    """tmvs_stage_hypotheses at 52 x 76 (maps of 13 x 19, 26 x 38 and 52 x 76, previous depths of 13 x 19 and
    26 x 38) and at 52 x 84 (13 x 21, 26 x 42, 52 x 84) bit for bit against the oracle; batch 2 with different
    depth ranges, the interval of stages 2 and 3 taken from sample 0 as the reference does.

    The two sizes lie either side of a switch inside the reference: torch's CPU bilinear F.interpolate runs
    another kernel when the output's H + W <= 128 (52 + 76 is exactly 128), which sums the 4 taps times the
    products of the axis weights instead of interpolating along x, then y. This test caught the glue kernel
    using the separable order at every size: at 52 x 76, stages 2 and 3, 23-34 % of the hypotheses were up to
    2 ulp (1.22e-4 mm) from the oracle (7230 of 31616 and 10724 of 31616 values at batch 1). upsample_at now
    follows the reference's switch; sizes above it (64 x 80, the end-to-end sizes) keep their bits."""
    nd, ratios = (48, 32, 8), (4.0, 1.0, 0.5)
    (h, w), scale = full, (4, 2, 1)[stage - 1]
    hw = (h // scale, w // scale)
    prev_hw = None if stage == 1 else (h // (2 * scale), w // (2 * scale))
    dv = torch.cat([synthetic.synthetic_depth_values(1) + 2.0 * i for i in range(batch)], 0)
    prev = None if prev_hw is None else torch.rand(batch, *prev_hw, generator=_gen(batch, stage, w)) * 510.0 + 425.0
    ref = oracle.stage_hypotheses(prev, dv, stage - 1, full, nd, ratios)
    got = ops.stage_hypotheses(dv.to(DEV), None if prev is None else _nan_in(prev), nd[stage - 1], ratios[stage - 1], full,
                               scale).cpu()
    assert tuple(got.shape) == tuple(ref.shape) == (batch, nd[stage - 1], *hw)
    diff = int((_bits(got) != _bits(ref)).sum())
    print(f"stage_hypotheses {h}x{w} batch {batch} stage {stage} {hw}: {diff} of {ref.numel()} values differ, "
          f"max abs {float((got - ref).abs().max()):.2e}")
    assert diff == 0
