"""The scene reconstruction driver (transmvsnet_amd/reconstruct.py) without a GPU: the restatement
(tests/_postprocess_ref.py) against hand-computed values, ViewCache's size / intrinsics / depth-value
arithmetic against data.load_sample and load_sample_tnt, the writers' round trips, the command line's
arguments, and the two new C entry points' argument validation (they launch nothing on failure).
The GPU half is tests/test_gpu_reconstruct.py. Every comparison is exact: the code under test restates
float32 / float64 arithmetic numpy performs deterministically."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from tests import _postprocess_ref as ref
from tests.test_data_io import _write_scan
from transmvsnet_amd import _lib, build, data, fusion, reconstruct
from transmvsnet_amd import dynamic_fusion as dynf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement
def test_restatement_hand_computed_4x4():
    """conf1 is 1 x 1, so all its taps clamp; conf2's columns (0.25, 0.75) resize to (0.25, 0.375, 0.625,
    0.75): fractions 0 at both borders, 0.25 and 0.75 inside. conf3 = 1/16 everywhere, conf1 = 1/2:
    conf_final = (1/128, 3/256, 5/256, 3/128) per column, so column 0 alone is below 0.01."""
    conf3 = np.full((4, 4), 0.0625, np.float32)
    conf2 = np.float32([[0.25, 0.75], [0.25, 0.75]])
    conf1 = np.float32([[0.5]])
    depth = np.float32([[500.0, 425.0, 680.0, 935.0], [500.0, 400.0, 427.0, 1000.0],
                        [0.0, 933.0, 934.9, 425.5], [1.0, 426.0, 679.9, 600.0]])
    image = np.zeros((3, 4, 4), np.float32)
    image[0], image[1], image[2] = 0.5, 1.2, -0.1
    image[0, 0, 1], image[2, 0, 1] = 0.2, 1.0
    r = ref.postprocess_ref(depth, conf3, conf2, conf1, image)
    want_cf = np.tile(np.float32([1 / 128, 3 / 256, 5 / 256, 3 / 128]), (4, 1))
    np.testing.assert_array_equal(r["conf_final"], want_cf)
    want_d = depth.copy()
    want_d[:, 0] = 0
    np.testing.assert_array_equal(r["depth"], want_d)
    # alpha = uint8((clip(d) - 425) / 510 * 255): 680 -> 127.5 -> 127; 427 -> 2/510*255 = 1 (or just below)
    a = r["rgba_u8"][..., 3]
    np.testing.assert_array_equal(a[0], [0, 0, 127, 255])
    assert a[1, 1] == 0 and a[1, 3] == 255 and a[1, 2] in (0, 1) and a[3, 1] == 0 and a[2, 1] == 254
    assert a[1, 2] == np.uint8(np.float32(np.float32(2.0) / np.float32(510.0)) * np.float32(255))
    np.testing.assert_array_equal(r["rgba_u8"][1, 2, :3], [127, 255, 0])  # 0.5 -> 127.5 -> 127, clipped ends
    np.testing.assert_array_equal(r["rgba_u8"][0, 1, :3], [51, 255, 255])
    # rgbd = (B, G, R) * (1 / 255.) in float64 -> float32, depth = 425 + 512 * float32(alpha / 255.)
    np.testing.assert_array_equal(r["rgbd"][1, 2, :3], np.float32([0.0, 1.0, 127 * (1.0 / 255.0)]))
    assert r["rgbd"][0, 2, 3] == np.float32(425.0 + 512.0 * float(np.float32(127 * (1.0 / 255.0))))
    assert r["rgbd"][0, 3, 3] == np.float32(937.0) and r["rgbd"][0, 0, 3] == np.float32(425.0)
    assert set(ref.postprocess_ref(depth, conf3, conf2, conf1)) == {"conf_final", "depth"}


@pytest.mark.parametrize("shape", [(4, 4), (8, 12), (36, 52), (96, 128)])
def test_seeded_inputs_reach_every_branch(shape):
    h, w = shape
    depth, conf3, conf2, conf1, image = ref.seeded_inputs(h, w)
    r = ref.postprocess_ref(depth, conf3, conf2, conf1, image)
    cf = r["conf_final"]
    assert cf[0, 0] == np.float32(0.01) and cf[0, 1] < np.float32(0.01) < cf[1, 0] and np.isnan(cf[1, 1])
    assert r["depth"][0, 0] == depth[0, 0] and r["depth"][0, 1] == 0 and r["depth"][1, 1] == depth[1, 1]
    masked = cf < np.float32(0.01)
    assert masked.any() and (~masked).any()
    assert (depth < 425).any() and (depth > 935).any() and (depth == 425).any() and (depth == 935).any()
    assert r["rgba_u8"][..., 3].min() == 0 and r["rgba_u8"][..., 3].max() == 255


# ------------------------------------------------------------------ ViewCache's arithmetic
def _same_cameras(got, want):
    for k in ("stage1", "stage2", "stage3"):
        g, w = got["proj_matrix"][k], want["proj_matrix"][k]
        assert g.dtype == np.float32
        np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg=k)
    assert got["depth_values"].dtype == np.float32
    np.testing.assert_array_equal(got["depth_values"], want["depth_values"])
    assert got["hw"] == want["imgs"].shape[2:] and got["filename"] == want["filename"]


def _dtu_scan(td):
    """300 x 400 views; view 3's image is 200 x 400, so under a 216 x 288 cap it scales to 128 x 288 while
    the others scale to 192 x 288: the second resize."""
    from PIL import Image
    _write_scan(str(td), "scan1", 4, "cams", h=300, w=400, seed=6)
    rng = np.random.default_rng(9)
    Image.fromarray((rng.random((200, 400, 3)) * 255).astype(np.uint8)).save(
        os.path.join(str(td), "scan1", "images", "{:0>8}.jpg".format(3)))
    return data.read_pair_file(os.path.join(str(td), "scan1", "pair.txt"), nviews=4)


@pytest.mark.parametrize("cap", [(864, 1152), (216, 288)])
def test_view_cache_dtu_cameras_equal_load_sample(tmp_path, cap):
    metas = _dtu_scan(tmp_path)
    max_h, max_w = cap
    cache = reconstruct.ViewCache(str(tmp_path), "scan1", "dtu", nviews=4, max_h=max_h, max_w=max_w,
                                  interval_scale=1.06)
    for ref_view, srcs in metas:
        want = data.load_sample(str(tmp_path), "scan1", ref_view, srcs, nviews=4, interval_scale=1.06, max_h=max_h,
                                max_w=max_w)
        got = cache.sample(ref_view, srcs, images=False)
        assert "imgs" not in got
        _same_cameras(got, want)
    sizes = {v: cache.camera(v)["hw"] for v in range(4)}
    if cap == (216, 288):
        assert sizes == {0: (192, 288), 1: (192, 288), 2: (192, 288), 3: (128, 288)}
    else:
        assert sizes == {0: (288, 384), 1: (288, 384), 2: (288, 384), 3: (192, 384)}
    assert cache.decoded == 0  # cameras alone decode nothing


def test_view_cache_tnt_cameras_equal_load_sample_tnt(tmp_path):
    td = str(tmp_path)
    _write_scan(td, "Family", 4, "cams_1", tnt=True)
    metas = data.read_pair_file(os.path.join(td, "Family", "pair.txt"), pad=False)
    cache = reconstruct.ViewCache(td, "Family", "tnt")
    assert cache.nviews == 11 and cache.fixed_hw is None
    want = data.load_sample_tnt(td, "Family", metas[0][0], metas[0][1], nviews=11)
    got = cache.sample(metas[0][0], metas[0][1], images=False)
    _same_cameras(got, want)
    assert cache.fixed_hw == want["fixed_hw"] == (288, 384) and got["proj_matrix"]["stage1"].shape[0] == 4
    # a smaller cap with the run's resolution carried over: the second resize, intrinsics scaled twice
    cache2 = reconstruct.ViewCache(td, "Family", "tnt", image_size=(256, 192), fixed_hw=cache.fixed_hw)
    want2 = data.load_sample_tnt(td, "Family", 1, [0, 2], image_size=(256, 192), fixed_hw=want["fixed_hw"])
    got2 = cache2.sample(1, [0, 2], images=False)
    _same_cameras(got2, want2)
    assert cache2.camera(1)["hw"] == (192, 256) and got2["hw"] == (288, 384)
    # inverse-depth hypotheses
    cache3 = reconstruct.ViewCache(td, "Family", "tnt", inverse_depth=True)
    want3 = data.load_sample_tnt(td, "Family", 0, [1, 2, 3], inverse_depth=True)
    np.testing.assert_array_equal(cache3.sample(0, [1, 2, 3], images=False)["depth_values"], want3["depth_values"])


def test_resize_axis_is_resize_bilinear_s_axis():
    """The factored-out axis: the tables, and resize_bilinear composed from them by hand."""
    i0, i1, t = data.resize_axis(8, 2)
    np.testing.assert_array_equal(i0, [0, 0, 0, 0, 0, 0, 1, 1])
    np.testing.assert_array_equal(i1, [1, 1, 1, 1, 1, 1, 1, 1])  # weight 0 where the left tap is clamped
    np.testing.assert_array_equal(t, np.float32([0, 0, 0.125, 0.375, 0.625, 0.875, 0, 0]))
    assert t.dtype == np.float32
    img = np.random.default_rng(3).random((7, 9)).astype(np.float32)
    x0, x1, tx = data.resize_axis(5, 9)
    y0, y1, ty = data.resize_axis(11, 7)
    rows = img[:, x0] * (np.float32(1) - tx) + img[:, x1] * tx
    want = rows[y0] * (np.float32(1) - ty[:, None]) + rows[y1] * ty[:, None]
    np.testing.assert_array_equal(data.resize_bilinear(img, 5, 11), want)
    k = np.float32([[700.0, 0, 200.0], [0, 690.0, 150.0], [0, 0, 1]])
    nw, nh, k2 = data.scale_mvs_camera(300, 400, k, 288, 216)
    _, k3 = data.scale_mvs_input(np.zeros((300, 400, 3), np.float32), k, 288, 216)
    assert (nw, nh) == (288, 192) and isinstance(nw, int)
    np.testing.assert_array_equal(k2, k3)


# ------------------------------------------------------------------ writers
def test_cam_text_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    k = np.float32([[2892.33 / 3, 0, 823.205 / 7], [0, 2883.18 / 3, 619.07 / 7], [0, 0, 1]])
    e = np.eye(4, dtype=np.float32)
    e[:3] = rng.standard_normal((3, 4)).astype(np.float32) * np.float32(37.3)
    fn = str(tmp_path / "00000003_cam.txt")
    reconstruct.write_cam_tnt(fn, k, e, 425.0, 2.5)
    k0, e0 = dynf.read_camera_parameters(fn, 1.0, 0, 0)
    np.testing.assert_array_equal(k0.view(np.uint32), k.view(np.uint32))
    np.testing.assert_array_equal(e0.view(np.uint32), e.view(np.uint32))
    k1, e1, dmin, dint = data.read_cam_file(fn)  # the dataset readers' layout too
    np.testing.assert_array_equal(e1, e)
    assert (dmin, dint) == (425.0, 2.5) and k1[0, 0] == k[0, 0] / 4
    # the DTU projection matrix: write_cam's text read by fusibile's reader is the float32 of the float64 P
    cam = np.zeros((2, 4, 4), np.float32)
    cam[0], cam[1, :3, :3] = e, k
    fn2 = str(tmp_path / "00000003.txt")
    fusion.write_cam(fn2, cam)
    np.testing.assert_array_equal(fusion.read_cam(fn2), fusion.projection_matrix(cam).astype(np.float32))


def test_rgba_png_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    rgba = rng.integers(0, 256, (12, 20, 4), dtype=np.uint8)
    fn = str(tmp_path / "00000000.png")
    reconstruct.save_rgba_png(fn, rgba)
    from PIL import Image
    im = Image.open(fn)
    assert im.mode == "RGBA" and im.size == (20, 12)
    bgr, alpha = reconstruct.read_rgba_png(fn)
    np.testing.assert_array_equal(bgr, rgba[..., [2, 1, 0]])
    np.testing.assert_array_equal(alpha, rgba[..., 3])
    reconstruct.save_rgba_png(fn, torch.from_numpy(rgba))
    np.testing.assert_array_equal(reconstruct.read_rgba_png(fn)[1], rgba[..., 3])
    with pytest.raises(ValueError):
        reconstruct.save_rgba_png(fn, rgba[..., :3])


# ------------------------------------------------------------------ command line
def test_argument_parsing(tmp_path):
    p = reconstruct.make_parser()
    a = p.parse_args(["--loadckpt", "m.ckpt", "--testpath", str(tmp_path)])
    assert (a.dataset, a.testlist, a.outdir, a.max_h, a.max_w) == ("dtu", "all", "./outputs", 864, 1152)
    assert a.num_view is None and a.photo_threshold == 0.3 and a.thres_view == 3 and not a.save_outputs
    for s in ("scan9", "scan1"):
        os.makedirs(str(tmp_path / s))
    (tmp_path / "notes.txt").write_text("x")
    assert reconstruct.scan_list(a) == ["scan1", "scan9"]
    lst = tmp_path / "list.txt"
    lst.write_text("scan9\n\nscan4\n")
    a = p.parse_args(["--loadckpt", "m.ckpt", "--testpath", str(tmp_path), "--testlist", str(lst), "--dataset", "tnt",
                      "--num_view", "11", "--photo_threshold", "0.18", "--thres_view", "5", "--save_outputs",
                      "--max_h", "1080", "--max_w", "1920", "--outdir", "o"])
    assert reconstruct.scan_list(a) == ["scan9", "scan4"]
    assert (a.dataset, a.num_view, a.photo_threshold, a.thres_view, a.save_outputs) == ("tnt", 11, 0.18, 5, True)
    a = p.parse_args(["--loadckpt", "m.ckpt", "--testpath_single_scene", str(tmp_path / "scan9")])
    assert reconstruct.scan_list(a) == ["scan9"] and a.testpath == str(tmp_path)
    with pytest.raises(SystemExit):
        p.parse_args(["--testpath", "x"])  # --loadckpt is required
    with pytest.raises(SystemExit):
        reconstruct.scan_list(argparse.Namespace(testpath=None, testpath_single_scene=None, testlist="all"))


def test_driver_refuses_cpu_tensors_and_bad_arguments():
    z = lambda *s: torch.zeros(*s)
    outs = {"depth": z(1, 8, 8), "photo_confidence": z(1, 8, 8), "stage1": {"photo_confidence": z(1, 2, 2)},
            "stage2": {"photo_confidence": z(1, 4, 4)}}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reconstruct.postprocess_view(outs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reconstruct.resize_image(torch.zeros(4, 4, 3, dtype=torch.uint8), 2, 2)
    with pytest.raises(ValueError):
        reconstruct.ViewCache("x", "scan1", "eth3d")


# ------------------------------------------------------------------ C-ABI
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _aligned_ptr(buf, align=16):
    return (buf.ctypes.data + align - 1) & ~(align - 1)


def test_depth_postprocess_validation_without_gpu(lib):
    """Bad arguments are rejected with the documented status before any launch (the pointers, host memory
    here, are never read)."""
    buf = np.zeros(64, np.uint8)
    p = _aligned_ptr(buf)

    def call(h=8, w=8, image=p, rgba=p, rgbd=p, dmin=425.0, dmax=935.0, **ptrs):
        a = {k: ptrs.get(k, p) for k in ("depth", "conf3", "conf2", "conf1", "conf_final", "depth_masked")}
        return lib.tmvs_depth_postprocess(a["depth"], a["conf3"], a["conf2"], a["conf1"], image, h, w, 0.01, dmin,
                                          dmax, a["conf_final"], a["depth_masked"], rgba, rgbd, None)

    for k in ("depth", "conf3", "conf2", "conf1", "conf_final", "depth_masked"):
        assert call(**{k: None}) == -1, k
    assert call(image=None) == -1 and call(image=None, rgba=None) == -1 and call(image=None, rgbd=None) == -1
    assert call(h=0) == -1 and call(w=0) == -1 and call(h=-4) == -1 and call(w=-8) == -1
    assert call(dmin=935.0, dmax=425.0) == -1 and call(dmin=425.0, dmax=425.0) == -1
    assert call(rgbd=p + 4) == -1 and call(rgba=p + 2) == -1  # the 16-byte and dword stores' alignment
    for bad in (1, 2, 3, 6, 10, 13):
        assert call(h=bad) == -2 and call(w=bad) == -2, bad
    assert lib.tmvs_status_string(-2) and lib.tmvs_status_string(-1)


def test_resize_bilinear_validation_without_gpu(lib):
    buf = np.zeros(64, np.uint8)
    p = _aligned_ptr(buf)
    for i in (0, 3, 4, 5, 6, 7, 8, 11):  # each pointer on its own
        args = [p, 4, 4, p, p, p, p, p, p, 2, 2, p, None]
        args[i] = None
        assert lib.tmvs_resize_bilinear_u8(*args) == -1, i
    for i in (1, 2, 9, 10):  # each size, zero and negative
        for bad in (0, -3):
            args = [p, 4, 4, p, p, p, p, p, p, 2, 2, p, None]
            args[i] = bad
            assert lib.tmvs_resize_bilinear_u8(*args) == -1, (i, bad)
    for i in (0, 4, 9, 12):
        args = [p, 3, 4, 4, p, p, p, p, p, p, 2, 2, p, None]
        args[i] = None
        assert lib.tmvs_resize_bilinear_f32(*args) == -1, i
    for i in (1, 2, 3, 10, 11):
        args = [p, 3, 4, 4, p, p, p, p, p, p, 2, 2, p, None]
        args[i] = 0
        assert lib.tmvs_resize_bilinear_f32(*args) == -1, i


def test_header_binding_and_version_agree(lib):
    src = open(os.path.join(ROOT, "include", "transmvs.h")).read()
    assert int(re.search(r"#define\s+TMVS_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION == 11
    assert lib.tmvs_abi_version() == 11
    code = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    for name, nargs in (("tmvs_depth_postprocess", 15), ("tmvs_resize_bilinear_u8", 13),
                        ("tmvs_resize_bilinear_f32", 14)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m and m.group(1).count(",") + 1 == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    for cite in ("test.py:119-158", "utils.py:11-22", "main.cpp:126-138", "general_eval.py:106-124"):
        assert cite in src, cite


# ------------------------------------------------------------------ the planted scene leaves points
def test_planted_dtu_scene_fuses_on_the_cpu():
    """The scene of the GPU end-to-end test, through the restatement and the fusibile oracle: the cloud the
    driver has to reproduce is not empty."""
    from oracle import fusion_ref
    sc = ref.planted_scene()
    v = len(sc["depths"])
    rgbd, dicts = [], []
    for i in range(v):
        r = ref.postprocess_ref(sc["depths"][i], sc["conf3"][i], sc["conf2"][i], sc["conf1"][i],
                                np.ascontiguousarray(sc["images"][i].transpose(2, 0, 1)))
        rgbd.append(r["rgbd"])
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0], cam[1, :3, :3] = sc["Es"][i], sc["Ks"][i]
        dicts.append(fusion.camera_params(fusion.projection_matrix(cam).astype(np.float32))[1])
        assert 0.0 < (r["depth"] == 0).mean() < 0.2  # some pixels masked, most kept
    xs, _ = fusion_ref.fuse_ref(np.stack(rgbd), dicts)
    assert len(xs) > 0.2 * 64 * 96
