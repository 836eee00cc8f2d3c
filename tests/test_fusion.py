"""Depth-map fusion (gipuma/fusibile) and the output-side writers -- SURVEY.md 8f rank 4.

CPU tests: the host writers and camera decomposition against their reference formulas, the oracle
on a synthetic scene. GPU tests (-m gpu): tmvs_fusibile against the oracle (oracle/fusion_ref.py).
Parity unpinned by the reference (fusibile needs CUDA + OpenCV, absent; no fused clouds shipped).
Tolerances: float32 kernel vs float64 oracle. The kernel makes discrete decisions on rounded
values -- the 0.25 disparity threshold, floor() of the projected pixel (texel and 3D point), the
8-bit filter weights -- so a few pixels legitimately take the other branch: the fused mask may
differ on <= 0.2 % of pixels, and <= 2 % of the agreeing pixels may fall outside 1e-3 mm + 1e-5
rel (one view's neighbouring texel / pixel), all within 10 mm; colours likewise within 1e-5.

The lattice scene (tests/_fusion_lattice.py) has no such slack: every value the kernel forms on it is
a small dyadic, so float32 arithmetic is exact (asserted by test_lattice_exactness_preconditions) and
the kernel must equal the oracle on every pixel, bit for bit after the final float32 division.
"""
import ctypes
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import fusion_ref
from tests import _fusion_lattice as lat
from tests._fusion_scene import make_scene
from transmvsnet_amd import _lib, build, fusion


def test_depth_normal_and_decode():
    """utils.depth_normal (clamp to [425, 935], uint8 of (d - 425) / 510 * 255) and fusibile's
    425 + 512 * a / 255 decoding (main.cpp:136): the reference's 510-vs-512 scale mismatch is kept."""
    d = np.array([[100.0, 425.0, 600.0, 935.0, 2000.0]], np.float32)
    u = fusion.depth_normal(d)
    assert u.dtype == np.uint8
    np.testing.assert_array_equal(u, [[0, 0, 87, 255, 255]])
    dec = fusion.depth_decode(u)
    np.testing.assert_allclose(dec, [[425.0, 425.0, 425.0 + 512.0 * 87 / 255, 937.0, 937.0]], rtol=1e-6)


def test_write_read_cam_roundtrip():
    """test.write_cam writes P = K [R | t] (3 rows + blank line); fusibile reads 3 x 4 floats back."""
    _, _, _, ps = make_scene(v=2, h=16, w=24)
    with tempfile.TemporaryDirectory() as td:
        fn = os.path.join(td, "00000000.txt")
        k = np.zeros((4, 4), np.float32)
        k[:3, :3] = [[2080.0, 0, 576.0], [0, 2075.0, 432.0], [0, 0, 1]]
        e = np.eye(4, dtype=np.float32)
        e[:3, 3] = [-191.02, 3.28832, 22.5401]
        fusion.write_cam(fn, np.stack([e, k]))
        lines = open(fn).read().split("\n")
        assert len(lines) == 5 and lines[3] == "" and len(lines[0].split()) == 4
        np.testing.assert_allclose(fusion.read_cam(fn), (k @ e)[:3], rtol=1e-6)


def test_camera_params_recover_k_and_centre():
    """get_camera_parameters: fx from the RQ decomposition, C4 = the camera centre, RK_inv = inv(P33)."""
    rgbd, packs, dicts, ps = make_scene(v=3, h=16, w=24)
    for p, d, pk in zip(ps, dicts, packs):
        k, r = fusion._rq3(p[:, :3].astype(np.float64))
        np.testing.assert_allclose(k @ r, p[:, :3], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(r @ r.T, np.eye(3), atol=1e-9)
        assert abs(d["fx"] - 1.8 * 24) < 1e-3
        c_h = np.append(d["C4"], 1.0)
        np.testing.assert_allclose(p @ c_h, 0.0, atol=1e-2)  # P C = 0
        np.testing.assert_allclose(pk[:12], p.reshape(-1).astype(np.float32))
        np.testing.assert_allclose(d["RK_inv"] @ p[:, :3], np.eye(3), atol=1e-5)


def test_oracle_fuses_consistent_scene():
    """The restated fusibile on a scene whose views agree: most valid pixels fuse, the
    fused points lie on the plane n . X = 650, and the invalid-depth patch never fuses."""
    rgbd, packs, dicts, _ = make_scene()
    wr, cx, ct = fusion_ref.fusibile_ref(rgbd, dicts, 0)
    valid = rgbd[0, ..., 3] > fusion_ref.DEPTH_FLOOR
    assert wr[valid].mean() > 0.6 and not wr[~valid].any()  # image borders leave the other views
    n = np.array([0.05, -0.03, 1.0])
    np.testing.assert_allclose(cx[wr] @ n, 650.0, atol=5.0)  # 8-bit depth alpha: 2 mm steps
    assert np.all((ct[wr] >= 0) & (ct[wr] <= 1))


def test_save_point_cloud_format():
    """displayUtils.h save_point_cloud: binary little-endian PLY, 15 bytes per vertex, RGB from
    texture [2, 1, 0], non-finite coordinates written as 0."""
    x = np.array([[1.0, 2.0, 3.0], [np.inf, 1.0, 1.0]], np.float32)
    t = np.array([[0.1, 0.2, 0.3], [1.0, 0.0, 0.5]], np.float32)
    with tempfile.TemporaryDirectory() as td:
        fn = os.path.join(td, "3d_model.ply")
        fusion.save_point_cloud(fn, x, t)
        raw = open(fn, "rb").read()
    head, body = raw.split(b"end_header\n")
    assert b"element vertex 2" in head and len(body) == 2 * 15
    rec = np.frombuffer(body, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"),
                                     ("b", "u1")])
    assert tuple(rec[0])[:3] == (1.0, 2.0, 3.0) and tuple(rec[0])[3:] == (76, 51, 25)
    assert tuple(rec[1])[:3] == (0.0, 0.0, 0.0) and tuple(rec[1])[3:] == (127, 0, 255)


def _close_mostly(got, want, atol, worst, rtol=1e-5, frac=0.02):
    err = np.abs(got.astype(np.float64) - want).max(axis=-1)
    bad = err > atol + rtol * np.abs(want).max(axis=-1)
    assert bad.mean() <= frac, (bad.mean(), err.max())
    assert err.max() <= worst, err.max()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(6, 96, 128), (4, 61, 83), (9, 61, 83, 2)])
def test_fusibile_kernel_vs_oracle(shape):
    """tmvs_fusibile for every reference camera against the oracle (fresh buffers). The last case
    has consistent_threshold 2 with 8 source views, so the cap of 4 agreeing views binds."""
    from transmvsnet_amd import ops
    v, h, w = shape[:3]
    thr = shape[3] if len(shape) > 3 else 3
    rgbd, packs, dicts, _ = make_scene(v=v, h=h, w=w, seed=v + h)
    dev = "cuda"
    rg = torch.from_numpy(rgbd).to(dev)
    cams = torch.from_numpy(packs).to(dev)
    lib = _lib.load()
    for ref in range(v):
        coord = torch.zeros(h, w, 4, device=dev)
        tex = torch.zeros(h, w, 4, device=dev)
        _lib.check(lib.tmvs_fusibile(rg.data_ptr(), cams.data_ptr(), v, h, w, ref, thr, 0.25, coord.data_ptr(),
                                     tex.data_ptr(), ops._stream()), "tmvs_fusibile")
        coord, tex = coord.cpu().numpy(), tex.cpu().numpy()
        wr, cx, ct = fusion_ref.fusibile_ref(rgbd, dicts, ref, thr)
        got = coord[..., 2] != 0
        both = got & wr
        bad = np.abs(coord[both][:, :3] - cx[both]).max(-1) > 1e-3 + 1e-5 * np.abs(cx[both]).max(-1)
        print("V %d %dx%d thr %d ref %d: mask mismatch %.5f (budget 0.002), coord outside tolerance %.5f (budget "
              "0.02), worst %.3g (budget 10)" % (v, h, w, thr, ref, (got != wr).mean(), bad.mean(),
                                                 np.abs(coord[both][:, :3] - cx[both]).max()))
        assert (got != wr).mean() <= 2e-3, (ref, (got != wr).mean())
        assert both.sum() > 0.5 * wr.sum()
        _close_mostly(coord[both][:, :3], cx[both], 1e-3, 10.0)
        _close_mostly(tex[both][:, :3], ct[both], 1e-5, 0.5)
        assert np.all(coord[got][:, 3] == 0) and np.all(tex[got][:, 3] == 0)


@pytest.mark.gpu
def test_fuse_point_list_vs_oracle():
    """fusion.fuse (persistent buffer across cameras + pixel-order compaction, as the reference)
    against oracle.fuse_ref: same point count within 0.2 %, same point set where counts agree."""
    rgbd, packs, dicts, _ = make_scene(v=5, h=72, w=96, seed=3)
    xs, ts = fusion.fuse(torch.from_numpy(rgbd).cuda(), packs)
    rx, rt = fusion_ref.fuse_ref(rgbd, dicts)
    assert abs(len(xs) - len(rx)) <= 0.002 * len(rx) + 2
    if len(xs) == len(rx):
        _close_mostly(xs.cpu().numpy(), rx, 1e-3, 10.0)
        _close_mostly(ts.cpu().numpy(), rt, 1e-5, 0.5)


# ------------------------------------------------------------------ the lattice scene (exact)
LATTICE_CASES = [(9, 0), (9, 1), (9, 2), (9, 3), (11, 2)]  # (views, consistent_threshold)
THR_ABOVE = float(np.nextafter(np.float32(0.25), np.float32(1)))
SENTINEL = np.float32(-12345.678)
PAD = 4  # rows behind the image that no launch may touch


@functools.lru_cache(maxsize=None)
def _lattice(v, w=lat.W):
    return lat.make_lattice(lat.CENTRES[:v], w=w)


@functools.lru_cache(maxsize=None)
def _pair():
    """Two cameras one unit apart, depth 512 against depth 1024: every disparity difference is 0.25."""
    return lat.make_lattice(lat.PAIR, plane=[512.0, 1024.0], plant=False)


@functools.lru_cache(maxsize=None)
def _floor_pair():
    """Two cameras at one centre (every pixel projects onto itself, baseline 0, so every live pair
    agrees). At the principal point (32, 8) the back-projection is (cx, cy, d) for ANY depth d, so the
    float32 neighbours of the reference's double literal 425.001 stay exact there; FLOOR_DEAD sits
    at a column whose point is never formed."""
    rgbd, packs, dicts = lat.make_lattice([(1, 0.5)] * 2, plant=False)
    rgbd[:, 8, 32, 3] = lat.FLOOR_LIVE
    rgbd[:, 8, 30, 3] = lat.FLOOR_DEAD
    return rgbd, packs, dicts


@functools.lru_cache(maxsize=None)
def _single():
    """View 1 of the lattice scene on its own (it carries every kind of hole)."""
    rgbd, packs, dicts = _lattice(9)
    return rgbd[1:2], packs[1:2], dicts[1:2]


_SCENES = {"lattice9": (functools.partial(_lattice, 9), (1, 2, 3), (0.25,)),  # name: (scene, thresholds in use)
           "lattice11": (functools.partial(_lattice, 11), (2,), (0.25,)),
           "lattice9_w64": (functools.partial(_lattice, 9, 64), (3,), (0.25,)),
           "lattice9_w65": (functools.partial(_lattice, 9, 65), (3,), (0.25,)),
           "pair": (_pair, (1,), (0.25, THR_ABOVE)),
           "floor_pair": (_floor_pair, (1,), (0.25,)),
           "single": (_single, (1,), (0.25,))}


@functools.lru_cache(maxsize=None)
def _want(name, ref, thr, dthr=0.25):
    """(written, coord, tex, count) of the oracle with the float32 final division; shared, read-only."""
    rgbd, _, dicts = _SCENES[name][0]()
    out = lat.fusibile_f32(rgbd, dicts, ref, thr, dthr)
    for a in out:
        a.setflags(write=False)
    return out


def _f32_exact(a):
    a = np.asarray(a, np.float64)
    with np.errstate(all="ignore"):
        r = a.astype(np.float32).astype(np.float64)
    return (r == a) | (np.isnan(a) & np.isnan(r))


@pytest.mark.parametrize("name", sorted(_SCENES))
def test_lattice_exactness_preconditions(name):
    """What makes bit equality a fair demand, asserted for every ordered pair of views: the oracle's
    3-D points, projected coordinates, projected depths and sampled texels are float32 values; the
    sums accumulated in float32 in the kernel's order equal the oracle's float64 sums; and every
    |ddisp - tdisp| is 0, or >= 1e-3 from the threshold, or exactly the threshold with float32-exact
    operands (baseline, both disparities), where float32 forms the same difference."""
    scene, thrs, dthrs = _SCENES[name]
    rgbd, packs, dicts = scene()
    for d, pk in zip(dicts, packs):  # the oracle reads the float32 values the kernel reads
        np.testing.assert_array_equal(np.concatenate([d["P"].reshape(-1), d["RK_inv"].reshape(-1), d["C4"], [d["fx"]]]),
                                      pk[:25])
        assert all(a.dtype == np.float32 for a in (d["P"], d["RK_inv"], d["C4"], d["fx"]))
    np.testing.assert_array_equal(dicts[0]["RK_inv"], [[1 / 256, 0, -1 / 8], [0, 1 / 256, -1 / 32], [0, 0, 1]])
    assert dicts[0]["fx"] == 256
    planted = 0
    for thr in thrs:
        for dthr in dthrs:
            for ref in range(len(dicts)):
                t = lat.trace(rgbd, dicts, ref, thr, dthr)
                with np.errstate(all="ignore"):  # the planted NaN and inf depths
                    wr, _, _, count, sx, st = fusion_ref.fusibile_ref(rgbd, dicts, ref, thr, dthr, return_sums=True)
                al = t["alive"]
                np.testing.assert_array_equal(t["count"][al], count[al])  # the trace is the oracle's loop
                assert _f32_exact(t["values"]).all(), (name, ref)
                np.testing.assert_array_equal(t["sum32_x"][wr].astype(np.float64), sx[wr])
                np.testing.assert_array_equal(t["sum32_t"][wr].astype(np.float64), st[wr])
                diff = np.abs(t["dd"] - t["td"])
                exact = (diff == np.float32(0.25)) & _f32_exact(t["dd"]) & _f32_exact(t["td"]) & _f32_exact(t["base"])
                clear = (diff == 0) | (np.abs(diff - dthr) >= 1e-3)
                assert (clear | exact).all(), (name, ref, diff[~(clear | exact)][:5])
                planted += int(exact.sum())
    if name not in ("floor_pair", "single"):
        assert planted > 0  # the exactly-at-threshold case is there


def test_lattice_branch_census():
    """Every branch of the kernel is taken by some pixel of some reference view on the lattice scene,
    counted on the oracle's own loop, so a later edit of the scene cannot empty a case unnoticed."""
    total = {}
    for v, thr in LATTICE_CASES:
        if thr == 0:
            continue  # the view loop does not run
        rgbd, _, dicts = _lattice(v)
        cen = dict.fromkeys(("cap_binds", "count_eq_thr", "count_eq_thr_minus_1", "left", "right", "top", "bottom",
                             "hole", "mismatch", "clamp_x", "clamp_y", "nan_ref", "inf_ref", "nan_src", "at_threshold",
                             "weights_zero", "weights_half", "weights_quarter"), 0)
        for ref in range(v):
            t = lat.trace(rgbd, dicts, ref, thr)
            al = t["alive"]
            cen["cap_binds"] += int((al & (t["avail"] > 2 * thr)).sum())
            cen["count_eq_thr"] += int((al & (t["count"] == thr)).sum())
            cen["count_eq_thr_minus_1"] += int((al & (t["count"] == thr - 1)).sum())
            for k in ("left", "right", "top", "bottom", "hole", "mismatch", "clamp_x", "clamp_y", "nan_src"):
                cen[k] += int(t[k].sum())
            cen["nan_ref"] += int(np.isnan(rgbd[ref, ..., 3]).sum())
            cen["inf_ref"] += int(np.isinf(rgbd[ref, ..., 3]).sum())
            cen["at_threshold"] += int((np.abs(t["dd"] - t["td"]) == 0.25).sum())
            for i in range(v):  # disparity classes of the views that agreed somewhere
                if t["agree"][i].any():
                    dx = (np.subtract(lat.CENTRES[ref], lat.CENTRES[i]) / 2) % 1
                    cen["weights_zero"] += int((dx == 0).all())
                    cen["weights_half"] += int((dx == 0.5).any())
                    cen["weights_quarter"] += int(((dx == 0.25) | (dx == 0.75)).any())
        print("lattice census V=%d thr=%d: %s" % (v, thr, cen))
        assert all(n > 0 for n in cen.values()), (v, thr, cen)
        total[(v, thr)] = cen
    # a fused point with a coordinate exactly 0 (reference 0, row 8, where Y = 0): item 3 needs it
    wr, ex, _, _ = _want("lattice9", 0, 3)
    assert (wr[8] & (ex[8, :, 1] == 0)).sum() > 0


def test_lattice_strict_threshold_pair():
    """|f b / 512 - f b / 1024| = 0.25 exactly for cameras one unit apart: `<` fuses nothing at
    depth_threshold 0.25 and nearly everything one float32 step above it."""
    for ref in (0, 1):
        assert _want("pair", ref, 1, 0.25)[0].sum() == 0
        assert _want("pair", ref, 1, THR_ABOVE)[0].mean() > 0.95
    # the reference's double literal 425.001 lies between these two float32 depths
    wr, ex, _, count = _want("floor_pair", 0, 1)
    assert wr[8, 32] and count[8, 32] == 1 and not wr[8, 30]
    np.testing.assert_array_equal(ex[8, 32], [1.0, 0.5, lat.FLOOR_LIVE])


def test_fusibile_abi_validation_without_gpu():
    """tmvs_fusibile rejects bad arguments before any launch (the pointers are never read)."""
    build.build()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def call(v=3, h=8, w=8, ref_view=0, thr=3):
        return lib.tmvs_fusibile(p, p, v, h, w, ref_view, thr, 0.25, p, p, None)

    assert call(v=0) == -1 and call(v=-2) == -1
    assert call(h=0) == -1 and call(h=-1) == -1 and call(w=0) == -1 and call(w=-4) == -1
    assert call(ref_view=-1) == -1 and call(ref_view=3) == -1 and call(ref_view=4) == -1
    assert call(thr=-1) == -1
    for i in (0, 1, 8, 9):  # each pointer on its own
        args = [p, p, 3, 8, 8, 0, 3, 0.25, p, p, None]
        args[i] = None
        assert lib.tmvs_fusibile(*args) == -1, i


# ------------------------------------------------------------------ the lattice scene on the GPU
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _launch_padded(name, ref, thr, dthr=0.25):
    """One tmvs_fusibile launch into sentinel-filled (H + PAD) x W x 4 buffers; returns them as arrays."""
    from transmvsnet_amd import ops
    rgbd, packs, _ = _SCENES[name][0]()
    v, h, w, _ = rgbd.shape
    rg, cams = torch.from_numpy(rgbd).cuda(), torch.from_numpy(packs).cuda()
    coord = torch.full((h + PAD, w, 4), float(SENTINEL), device="cuda")
    tex = torch.full((h + PAD, w, 4), float(SENTINEL), device="cuda")
    ops._launch("tmvs_fusibile", rg, cams, v, h, w, ref, thr, dthr, coord, tex)
    return coord.cpu().numpy(), tex.cpu().numpy()


def _assert_exact(coord, tex, want, tag):
    """Buffers of _launch_padded against the oracle: the written mask on ALL pixels, the sentinel bit
    for bit everywhere else (padding rows included), .w = +0 and bitwise float32 quotients on the
    written pixels (NaN, which only an infinite reference depth produces, matches any NaN)."""
    wr, ex, et = want[:3]
    h = wr.shape[0]
    sent = _bits(SENTINEL)
    for name, buf, exp in (("coord", coord, ex), ("tex", tex, et)):
        b = _bits(buf)
        assert (b[h:] == sent).all(), (tag, name, "rows past H written")
        touched = (b[:h] != sent).any(-1)
        assert np.array_equal(touched, wr), (tag, name, "mask", np.argwhere(touched != wr)[:5])
        assert (b[:h][~wr] == sent).all(), (tag, name)
        got = buf[:h][wr]
        same = (_bits(got[:, :3]) == _bits(exp[wr])) | (np.isnan(got[:, :3]) & np.isnan(exp[wr]))
        assert same.all(), (tag, name, int((~same).sum()), np.argwhere(wr)[~same.all(-1)][:5], got[:, :3][~same][:5],
                            exp[wr][~same][:5])
        assert (_bits(got[:, 3]) == 0).all(), (tag, name, ".w")


@pytest.mark.gpu
@pytest.mark.parametrize("case", LATTICE_CASES)
def test_lattice_kernel_exact(case):
    """Every reference camera of the lattice scene: threshold 0 (every live pixel, n = 1), 1, 2 (the cap
    is 4 of 8 views), 3 (6 of 8), and 11 views at threshold 2. Mask, points and colours equal the oracle."""
    v, thr = case
    scene = "lattice%d" % v
    for ref in range(v):
        coord, tex = _launch_padded(scene, ref, thr)
        _assert_exact(coord, tex, _want(scene, ref, thr), (v, thr, ref))
    if thr == 0:
        wr, _, _, count = _want(scene, 1, 0)
        assert np.array_equal(wr, _lattice(v)[0][1, ..., 3].astype(np.float64) > fusion_ref.DEPTH_FLOOR)
        assert not count.any()


@pytest.mark.gpu
@pytest.mark.parametrize("w", [lat.W, 64, 65])
def test_lattice_untouched_memory(w):
    """Pixels that are not fused and the rows behind the image keep the buffer's contents bit for bit:
    W = 70 (6 live lanes in the tail block), 64 (no tail block) and 65 (one live lane)."""
    scene = "lattice9" if w == lat.W else "lattice9_w%d" % w
    unwritten = 0
    for ref in range(9):
        coord, tex = _launch_padded(scene, ref, 3)
        want = _want(scene, ref, 3)
        _assert_exact(coord, tex, want, (w, ref))
        unwritten += int((~want[0]).sum())
    assert unwritten > 0


@pytest.mark.gpu
def test_lattice_strict_threshold_kernel():
    """The disparity test is `<`: at exactly 0.25 nothing fuses; one float32 step above, the oracle's mask."""
    for ref in (0, 1):
        for dthr in (0.25, THR_ABOVE):
            coord, tex = _launch_padded("pair", ref, 1, dthr)
            _assert_exact(coord, tex, _want("pair", ref, 1, dthr), (ref, dthr))


@pytest.mark.gpu
def test_depth_floor_is_the_double_literal():
    """fusibile.cu:116 and :141 compare the float depth with the DOUBLE 425.001, so float32(425.001),
    which rounds up, is a live depth in the reference texel and in a sampled one, and its float32
    predecessor is not."""
    for ref in (0, 1):
        coord, tex = _launch_padded("floor_pair", ref, 1)
        _assert_exact(coord, tex, _want("floor_pair", ref, 1), ref)


@pytest.mark.gpu
def test_lattice_single_view():
    """V = 1: no view can agree, so threshold 1 writes nothing; threshold 0 writes every live pixel
    with its own back-projection and colour."""
    rgbd, _, dicts = _single()
    coord, tex = _launch_padded("single", 0, 1)
    assert not _want("single", 0, 1)[0].any()
    _assert_exact(coord, tex, _want("single", 0, 1), 1)
    coord, tex = _launch_padded("single", 0, 0)
    wr, ex, et, _ = _want("single", 0, 0)
    depth = rgbd[0, ..., 3]
    assert np.array_equal(wr, depth.astype(np.float64) > fusion_ref.DEPTH_FLOOR) and 0 < (~wr).sum() < 30
    fin = wr & np.isfinite(depth)
    ys, xs = np.nonzero(fin)
    np.testing.assert_array_equal(ex[fin], np.stack([2.0 * (xs - 32) + 2, 2.0 * (ys - 8), depth[fin]], -1))
    np.testing.assert_array_equal(et[fin], rgbd[0][fin][:, :3])
    _assert_exact(coord, tex, (wr, ex, et), 0)


@pytest.mark.gpu
def test_lattice_graph_capture():
    """One launch captured in a HIP graph (buffers allocated before the capture, a single stream)
    replays to the eager call's outputs: the entry point neither allocates nor synchronises."""
    from transmvsnet_amd import ops
    rgbd, packs, _ = _lattice(9)
    v, h, w, _ = rgbd.shape
    rg, cams = torch.from_numpy(rgbd).cuda(), torch.from_numpy(packs).cuda()
    eager = [torch.full((h, w, 4), float(SENTINEL), device="cuda") for _ in range(2)]
    ops._launch("tmvs_fusibile", rg, cams, v, h, w, 4, 3, 0.25, *eager)
    out = [torch.full((h, w, 4), float(SENTINEL), device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops._launch("tmvs_fusibile", rg, cams, v, h, w, 4, 3, 0.25, *out)
    for t in out:
        t.fill_(float(SENTINEL))
    g.replay()
    torch.cuda.synchronize()
    assert (eager[0][..., 3] == 0).any()
    for a, b in zip(out, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
def test_lattice_fuse_point_list_exact():
    """fusion.fuse on the lattice scene against the reference's host loop (one persistent zeroed buffer,
    all-nonzero compaction in pixel order after every camera) over the float32 quotients: same length,
    same order, same bits. Both quirks of that loop are exercised."""
    scene = "lattice9"
    rgbd, packs, _ = _lattice(9)
    v, h, w, _ = rgbd.shape
    buf_x, buf_t = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
    out_x, out_t, re_emitted, dropped = [], [], 0, 0
    for cam in range(v):
        wr, ex, et, _ = _want(scene, cam, 3)
        buf_x[wr], buf_t[wr] = ex[wr], et[wr]
        keep = (buf_x != 0).all(-1)
        out_x.append(buf_x[keep])
        out_t.append(buf_t[keep])
        re_emitted += int((keep & ~wr).sum())  # an earlier camera's point, emitted again
        dropped += int((wr & ~keep).sum())  # fused, but a coordinate is exactly 0
    assert re_emitted > 0 and dropped > 0
    xs, ts = fusion.fuse(torch.from_numpy(rgbd).cuda(), packs)
    want_x, want_t = np.concatenate(out_x), np.concatenate(out_t)
    assert tuple(xs.shape) == want_x.shape and tuple(ts.shape) == want_t.shape
    assert np.array_equal(_bits(xs.cpu().numpy()), _bits(want_x))
    assert np.array_equal(_bits(ts.cpu().numpy()), _bits(want_t))
