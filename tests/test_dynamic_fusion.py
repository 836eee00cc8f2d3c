"""Dynamic geometric-consistency fusion, the Tanks & Temples output path (dynamic_fusion.py).

CPU tests: the dtype-faithful restatement (tests/_dynfusion_ref.py) on the synthetic scene
(tests/_dynfusion_scene.py), the host readers / writers, and the C-ABI's argument validation.
GPU tests (-m gpu): tmvs_dynamic_fusion, filter_view, fuse_scene and fuse_scan against it.

Goldens from the reference itself are not possible: its module parses sys.argv and imports cv2 and
plyfile at import time, and both are absent. The oracle is therefore the restatement, whose
cv2.remap sampler (subpixel_bits=5) is itself unpinned against cv2.

Tolerances. The kernel follows the reference's dtypes (float32 matrices, float64 per-pixel
arithmetic, float32 casts at the same places), so away from thresholds the masks and counts are
EQUAL to the restatement. Pixels where some source's distance lies within 1e-6 of a level's i/4, or
its relative depth difference within 1e-7 of float32(i/1300), are "ambiguous" (a last-bit difference
of the float64 matrix products may flip them) and are not asserted on; the scene keeps them <= 0.5 %
(measured <= 0.23 %). Elsewhere depth_avg agrees to rtol 1e-6 (a float32 sum of <= 11 terms in the
same order) and the world point to rtol 1e-6 + 1e-4 (two float32 ulps at |X| ~ 700).
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import _dynfusion_ref as ref
from tests._dynfusion_scene import PLANE_D, PLANE_N, make_scene
from transmvsnet_amd import _lib, build, data
from transmvsnet_amd import dynamic_fusion as dynf

SHAPES = [(5, 48, 64, 3), (4, 61, 83, 3), (11, 40, 56, 5)]  # (V, H, W, thres_view)
PHOTO = 0.3


@functools.lru_cache(maxsize=None)
def _scene(v, h, w, noise=2e-3, patches=True):
    return make_scene(v, h, w, seed=v + h, noise=noise, patches=patches)


@functools.lru_cache(maxsize=None)
def _want(v, h, w, view, thres_view, bits):
    d, c, _, ks, es = _scene(v, h, w)
    return ref.filter_view_ref(d, c[view], ks, es, view, [i for i in range(v) if i != view], PHOTO, thres_view, bits)


# ------------------------------------------------------------------ CPU
def test_restatement_on_clean_scene():
    """Noise-free views of the plane agree: most pixels pass, the averaged depth is the input depth and
    the fused points lie on the plane."""
    d, c, _, ks, es = _scene(5, 48, 64, noise=0, patches=False)
    r = ref.filter_view_ref(d, c[0], ks, es, 0, [1, 2, 3, 4], -1.0, 3)
    assert r["photo"].all() and r["geo"].mean() > 0.6
    g = r["geo"]
    np.testing.assert_allclose(r["depth_avg"][g], d[0][g], rtol=1e-3)
    np.testing.assert_allclose(r["xyz"][r["final"]] @ PLANE_N, PLANE_D, atol=0.5)
    assert not r["xyz"][~r["final"]].any()


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_branches(shape):
    """With noise and patches: the depth-0 patch never passes, the dynamic OR term admits pixels that
    thres_view alone rejects, and the two sampler modes stay within the ambiguity budget."""
    v, h, w, tv = shape
    for bits in (0, 5):
        r = _want(v, h, w, 0, tv, bits)
        assert not r["geo"][h // 3:h // 3 + 6, w // 4:w // 4 + 9].any()
        assert (r["geo"] & ~r["geo_thres"]).mean() > 0.01
        assert 0.4 < r["geo"].mean() < 0.95
        assert r["ambiguous"].mean() <= 5e-3
        assert r["geo_count"].max() <= v - 1 and r["depth_avg"].dtype == np.float32


def test_restatement_remap_modes():
    """The sampler: integer coordinates return the texel in both modes, taps outside contribute 0,
    non-finite coordinates sample 0, and mode 5 rounds the coordinate to 1/32 pixel (half to even)."""
    img = np.arange(12, dtype=np.float32).reshape(3, 4) + 1
    xs, ys = np.meshgrid(np.arange(4, dtype=np.float32), np.arange(3, dtype=np.float32))
    for bits in (0, 5):
        np.testing.assert_array_equal(ref.remap_linear(img, xs, ys, bits), img)
        got = ref.remap_linear(img, np.float32([[-0.5, 3.5, np.nan, np.inf, -2.0]]), np.float32([[0, 0, 0, 1, 1]]), bits)
        np.testing.assert_array_equal(got, np.float32([[0.5, 2.0, 0, 0, 0]]))
    x = np.float32([[1.0 + 1.4 / 32, 1.0 + 1.5 / 32, 1.0 + 2.5 / 32]])  # -> 1/32, 2/32 (even), 2/32 (even)
    np.testing.assert_array_equal(ref.remap_linear(img, x, np.zeros_like(x), 5),
                                  np.float32([[2 + 1 / 32, 2 + 2 / 32, 2 + 2 / 32]]))
    np.testing.assert_allclose(ref.remap_linear(img, x, np.zeros_like(x), 0), x + 1, rtol=1e-6)


def test_pair_constants_bit_exact():
    _, _, _, ks, es = _scene(5, 48, 64)
    pk = dynf.pair_constants(ks[0], es[0], ks[3], es[3])
    assert pk.dtype == np.float32 and pk.shape == (_lib.DYNFUSE_PAIR_FLOATS,)
    want = [np.linalg.inv(ks[0]), np.matmul(es[3], np.linalg.inv(es[0]))[:3], ks[3], np.linalg.inv(ks[3]),
            np.matmul(es[0], np.linalg.inv(es[3]))[:3], ks[0]]
    assert all(a.dtype == np.float32 for a in want)
    flat = np.concatenate([a.reshape(-1) for a in want])
    assert flat.size == 60
    np.testing.assert_array_equal(pk[:60].view(np.uint32), flat.view(np.uint32))
    assert not pk[60:].any()
    rb = dynf.ref_constants(ks[0], es[0])
    np.testing.assert_array_equal(rb[:21], np.concatenate([np.linalg.inv(ks[0]).reshape(-1),
                                                           np.linalg.inv(es[0])[:3].reshape(-1)]))


def _write_cam(fn, k, e):
    with open(fn, "w") as f:
        f.write("extrinsic\n")
        for row in e:
            f.write(" ".join(repr(float(x)) for x in row) + "\n")
        f.write("\nintrinsic\n")
        for row in k:
            f.write(" ".join(repr(float(x)) for x in row) + "\n")
        f.write("\n425.0 2.5\n")


def test_read_camera_parameters(tmp_path):
    k = np.float32([[2892.33, 0, 823.205], [0, 2883.18, 619.07], [0, 0, 1]])
    e = np.float32([[0.97, 0.01, 0.24, -191.02], [-0.01, 0.99, 0.02, 3.29], [-0.24, -0.02, 0.97, 22.54], [0, 0, 0, 1]])
    fn = str(tmp_path / "00000000_cam.txt")
    _write_cam(fn, k, e)
    k0, e0 = dynf.read_camera_parameters(fn, 0.5, 3, 0)
    assert k0.dtype == np.float32 and e0.dtype == np.float32
    np.testing.assert_array_equal(e0, e)  # lines [1, 5)
    ks = k.copy()
    ks[:2] *= 0.5  # lines [7, 10), rows 0-1 scaled
    np.testing.assert_array_equal(k0[2], [0, 0, 1])
    np.testing.assert_array_equal(k0[:2, :2], ks[:2, :2])
    assert k0[0, 2] == ks[0, 2] - 3 and k0[1, 2] == ks[1, 2]
    k1, _ = dynf.read_camera_parameters(fn, 0.5, 3, 1)
    assert k1[0, 2] == ks[0, 2] and k1[1, 2] == ks[1, 2] - 3


def test_align_image_both_branches():
    rng = np.random.default_rng(0)
    img = rng.random((60, 100, 3)).astype(np.float32)
    out, scale, index, flag = dynf.align_image(img, (30, 48))  # scaled by height, width cropped
    assert (scale, index, flag) == (0.5, 1, 0) and out.shape == (30, 48, 3)
    np.testing.assert_array_equal(out, data.resize_bilinear(img, 50, 30)[:, 1:49])
    img = rng.random((100, 60, 3)).astype(np.float32)
    out, scale, index, flag = dynf.align_image(img, (48, 30))  # scaled by width, height cropped
    assert (scale, index, flag) == (0.5, 1, 1) and out.shape == (48, 30, 3)
    np.testing.assert_array_equal(out, data.resize_bilinear(img, 30, 50)[1:49])


def test_pair_reader_skips_empty_and_does_not_pad(tmp_path):
    fn = tmp_path / "pair.txt"
    fn.write_text("3\n0\n2 1 9.5 2 8.5\n1\n0\n2\n1 0 7.0\n")
    assert dynf.read_pair_file(str(fn)) == [(0, [1, 2]), (2, [0])]


def test_save_ply_roundtrip(tmp_path):
    pts = np.float32([[1.5, -2.25, 3.0], [1e-3, 700.125, -0.5], [0, 0, 0]])
    col = np.uint8([[1, 2, 3], [255, 0, 128], [9, 8, 7]])
    fn = str(tmp_path / "x.ply")
    dynf.save_ply(fn, pts, col)
    head, body = open(fn, "rb").read().split(b"end_header\n")
    assert head.decode() == ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\n"
                             "property float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
                             "property uchar blue\n")
    assert len(body) == 15 * 3
    rec = np.frombuffer(body, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    np.testing.assert_array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), pts)
    np.testing.assert_array_equal(np.stack([rec["r"], rec["g"], rec["b"]], 1), col)


def test_abi_validation_without_gpu():
    """tmvs_dynamic_fusion rejects bad arguments before any launch (the pointers are never read)."""
    build.build()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def call(v=3, h=8, w=8, ref_view=0, n_src=2, thres=3, bits=5, ptr=p):
        return lib.tmvs_dynamic_fusion(ptr, v, h, w, ref_view, ptr, n_src, ptr, ptr, ptr, 0.3, thres, bits,
                                       ptr, ptr, ptr, ptr, None)

    assert call(ptr=None) == -1
    assert call(n_src=0) == -1 and call(n_src=11) == -1
    assert call(bits=3) == -1
    assert call(thres=0) == -1
    assert call(ref_view=3) == -1 and call(ref_view=-1) == -1
    assert call(h=0) == -1 and call(w=-4) == -1 and call(v=0) == -1
    for i in (0, 5, 7, 8, 9, 13, 14, 15, 16):  # each pointer on its own
        args = [p, 3, 8, 8, 0, p, 2, p, p, p, 0.3, 3, 5, p, p, p, p, None]
        args[i] = None
        assert lib.tmvs_dynamic_fusion(*args) == -1, i


def test_filter_view_refuses_cpu_tensors_and_bad_views():
    d, c, _, ks, es = _scene(5, 48, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dynf.filter_view(torch.from_numpy(d), torch.from_numpy(c[0]), ks, es, 0, [1, 2])
    for srcs in ([], list(range(1, 5)) * 3, [0], [5], [-1]):
        with pytest.raises(ValueError):
            dynf.view_constants(ks, es, 0, srcs, "cpu")


# ------------------------------------------------------------------ GPU
def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _compare(got, want, tag):
    amb = want["ambiguous"]
    print(tag, "ambiguous %.5f" % amb.mean(), "geo %.3f" % want["geo"].mean(), "final %.3f" % want["final"].mean(),
          "count mismatches (incl. ambiguous) %d" % (got["geo_count"] != want["geo_count"]).sum())
    assert amb.mean() <= 5e-3, tag
    ok = ~amb
    for k in ("geo_count", "photo", "geo", "final"):
        bad = (got[k] != want[k]) & ok
        assert not bad.any(), (tag, k, int(bad.sum()), np.argwhere(bad)[:5])
    same = ok & (got["geo_count"] == want["geo_count"]) & (got["final"] == want["final"])
    with np.errstate(invalid="ignore"):
        np.testing.assert_allclose(got["depth_avg"][same], want["depth_avg"][same], rtol=1e-6, atol=0, err_msg=tag)
        np.testing.assert_allclose(got["xyz"][same], want["xyz"][same], rtol=1e-6, atol=1e-4, err_msg=tag)
    assert not got["xyz"][~got["final"]].any(), tag


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [0, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_vs_restatement(shape, bits):
    """filter_view against the restatement: reference view 0 and the last view, every other view a source
    (61 x 83: ragged blocks in both dimensions; V = 11: S = 10, all nine levels in the OR)."""
    v, h, w, tv = shape
    d, c, _, ks, es = _scene(v, h, w)
    dd, cd = torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()
    for view in (0, v - 1):
        srcs = [i for i in range(v) if i != view]
        got = _np(dynf.filter_view(dd, cd[view], ks, es, view, srcs, PHOTO, tv, bits))
        want = _want(v, h, w, view, tv, bits)
        assert got["geo_count"].dtype == np.uint8 and got["final"].dtype == np.bool_
        np.testing.assert_array_equal(got["final"], got["photo"] & got["geo"])
        _compare(got, want, (shape, bits, view))


@pytest.mark.gpu
def test_single_source():
    """S = 1: no level enters the OR, only the thres_view term (here 1) applies."""
    d, c, _, ks, es = _scene(2, 48, 64)
    dd, cd = torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()
    for bits in (0, 5):
        got = _np(dynf.filter_view(dd, cd[0], ks, es, 0, [1], PHOTO, 1, bits))
        want = _want(2, 48, 64, 0, 1, bits)
        np.testing.assert_array_equal(want["geo"], want["geo_thres"])
        assert 0.3 < want["geo"].mean() < 1.0
        _compare(got, want, ("S=1", bits))
        # thres_view = 2 can never be met by one source, and no level may rescue it
        got2 = _np(dynf.filter_view(dd, cd[0], ks, es, 0, [1], PHOTO, 2, bits))
        assert not got2["geo"].any() and not got2["xyz"].any()


@pytest.mark.gpu
def test_fuse_scene_vs_restatement():
    """All five views as references: the concatenated cloud, in pair and pixel order."""
    v, h, w = 5, 48, 64
    d, c, img, ks, es = _scene(v, h, w)
    pairs = [(r, [i for i in range(v) if i != r]) for r in range(v)]
    pts, cols = dynf.fuse_scene(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(img).cuda(),
                                ks, es, pairs, PHOTO, 3)
    assert pts.dtype == torch.float32 and cols.dtype == torch.uint8 and pts.shape[1] == 3 and cols.shape[1] == 3
    wp, wc, n_amb = ref.fuse_scene_ref(d, c, img, ks, es, pairs, PHOTO, 3)
    print("fuse_scene points", len(pts), "restatement", len(wp), "ambiguous pixels", n_amb)
    assert len(wp) > 0.3 * v * h * w
    assert abs(len(pts) - len(wp)) <= n_amb
    if len(pts) == len(wp):
        np.testing.assert_allclose(pts.cpu().numpy(), wp, rtol=1e-6, atol=1e-4)
        np.testing.assert_array_equal(cols.cpu().numpy(), wc)


def _write_scan(folder, d, c, img, ks, es, up=2):
    """The scan folder filter_depth reads; images (and the cam files' intrinsics) at `up` x the depth maps'
    resolution, so the alignment scales by 1 / up."""
    from PIL import Image
    for sub in ("depth_est", "confidence", "images", "cams"):
        os.makedirs(os.path.join(folder, sub))
    for i in range(len(d)):
        data.save_pfm(os.path.join(folder, "depth_est/{:0>8}.pfm".format(i)), d[i])
        data.save_pfm(os.path.join(folder, "confidence/{:0>8}.pfm".format(i)), c[i])
        big = np.repeat(np.repeat((img[i] * 255).astype(np.uint8), up, 0), up, 1)
        Image.fromarray(big).save(os.path.join(folder, "images/{:0>8}.jpg".format(i)), quality=95)
        k = ks[i].copy()
        k[:2] *= up
        _write_cam(os.path.join(folder, "cams/{:0>8}_cam.txt".format(i)), k, es[i])


@pytest.mark.gpu
def test_fuse_scan_from_files(tmp_path):
    """The CLI's worker on a scan folder: the PLY holds fuse_scene's cloud of the arrays it loaded, and the
    three mask images of every view are written with the masks' means."""
    import argparse

    from PIL import Image
    v, h, w = 4, 61, 83
    d, c, img, ks, es = _scene(v, h, w)
    root, scan = str(tmp_path / "in"), "Family"
    _write_scan(os.path.join(root, scan), d, c, img, ks, es)
    with open(os.path.join(root, scan, "pair.txt"), "w") as f:
        f.write("5\n0\n3 1 1.0 2 1.0 3 1.0\n1\n2 0 1.0 2 1.0\n2\n0\n3\n3 2 1.0 1 1.0 0 1.0\n4\n0\n")
    out = str(tmp_path / "out")
    args = argparse.Namespace(testpath=root, tntpath=root, outdir=out, photo_threshold=PHOTO, thres_view=2,
                              test_dataset="tnt")
    ply = dynf.worker(scan, args)
    assert ply == os.path.join(out, "Family.ply")
    head, body = open(ply, "rb").read().split(b"end_header\n")
    rec = np.frombuffer(body, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    assert ("element vertex %d\n" % len(rec)).encode() in head

    pairs = dynf.read_pair_file(os.path.join(root, scan, "pair.txt"))
    assert pairs == [(0, [1, 2, 3]), (1, [0, 2]), (3, [2, 1, 0])]
    ids, ld, lconf, limg, cams, slot_pairs = dynf.load_scan(os.path.join(root, scan), pairs)
    np.testing.assert_array_equal(ld, d[ids])
    lk, le = cams(0)
    np.testing.assert_allclose(lk, ks[ids], rtol=1e-6)  # scaled back by 1/2
    np.testing.assert_array_equal(le, es[ids])
    dd = torch.from_numpy(ld).cuda()
    cd = torch.zeros_like(dd)
    for s, a in lconf.items():
        cd[s] = torch.from_numpy(a).cuda()
    pts, cols = dynf.fuse_scene(dd, cd, limg, lk, le, slot_pairs, PHOTO, 2)
    assert len(rec) == len(pts) > 0.2 * 3 * h * w
    np.testing.assert_array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), pts.cpu().numpy())
    np.testing.assert_array_equal(np.stack([rec["r"], rec["g"], rec["b"]], 1), cols.cpu().numpy())
    # and the cloud is the restatement's on the loaded arrays
    wp, _, n_amb = ref.fuse_scene_ref(ld, {s: a for s, a in lconf.items()}, limg, lk, le, slot_pairs, PHOTO, 2)
    assert abs(len(wp) - len(pts)) <= n_amb
    for ref_slot, srcs in slot_pairs:
        r = dynf.filter_view(dd, cd[ref_slot], lk, le, ref_slot, srcs, PHOTO, 2)
        for kind in ("photo", "geo", "final"):
            png = np.array(Image.open(os.path.join(out, scan, "mask/{:0>8}_{}.png".format(ids[ref_slot], kind))))
            assert png.shape == (h, w) and set(np.unique(png)) <= {0, 255}
            np.testing.assert_array_equal(png > 0, r[kind].cpu().numpy())
            assert (png > 0).mean() == r[kind].cpu().numpy().mean()
    # dtu naming
    args.test_dataset, args.outdir = "dtu", str(tmp_path / "out_dtu")
    os.rename(os.path.join(root, scan), os.path.join(root, "scan9"))
    assert dynf.worker("scan9", args) == os.path.join(args.outdir, "mvsnet_009_l3.ply")
    assert open(os.path.join(args.outdir, "mvsnet_009_l3.ply"), "rb").read() == open(ply, "rb").read()


@pytest.mark.gpu
def test_graph_capture():
    """One filter_view launch captured in a HIP graph (constants uploaded and outputs allocated before
    the capture, a single stream) replays to the eager call's outputs: the entry point neither allocates
    nor synchronises."""
    v, h, w = 5, 48, 64
    d, c, _, ks, es = _scene(v, h, w)
    dd, cd = torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()[0].contiguous()
    srcs = [1, 2, 3, 4]
    consts = dynf.view_constants(ks, es, 0, srcs, dd.device)
    eager = {k: t.clone() for k, t in dynf.filter_view(dd, cd, ks, es, 0, srcs, PHOTO, 3, 5, consts=consts).items()}
    out = dynf.alloc_outputs(h, w, dd.device)
    for t in out.values():
        t.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = dynf.filter_view(dd, cd, ks, es, 0, srcs, PHOTO, 3, 5, consts=consts, out=out)
    for t in out.values():
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert eager["final"].any()
    for k in eager:
        assert torch.equal(res[k], eager[k]), k
