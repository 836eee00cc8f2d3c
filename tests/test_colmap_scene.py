"""COLMAP scene import without a GPU: the readers of both file formats (transmvsnet_amd.colmap), the numpy
restatement of view selection and depth ranges on scenes with closed-form answers (tests/_view_select_ref.py),
the scan folder colmap_scene.write_scan leaves against the dataset readers, and the command lines."""
import math
import os

import numpy as np
import pytest

from tests import _view_select_ref as ref
from transmvsnet_amd import colmap, colmap_scene, data, reconstruct, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the readers
def _quat(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([[math.cos(angle / 2)], math.sin(angle / 2) * axis])


def _handmade():
    """Image ids neither contiguous nor in file order, both pinhole models, an image without 2-D points, a view
    that sees point 11 twice, 2-D points without a 3-D point and one whose 3-D point the model lacks."""
    cameras = {5: ("SIMPLE_PINHOLE", 640, 480, np.array([500.25, 320.0, 240.5])),
               2: ("PINHOLE", 800, 600, np.array([700.125, 701.5, 400.0, 299.75]))}
    xy = lambda n: np.arange(2 * n, dtype=np.float64).reshape(n, 2) * 1.7 + 0.1  # noqa: E731
    images = {40: (_quat([0, 1, 0], 0.3), np.array([0.1, -0.2, 3.0]), 2, "b/forty.jpg", xy(4), np.array([11, -1, 11, 30])),
              2: (_quat([1, 2, 3], -0.7), np.array([1.5, 0.25, -0.125]), 5, "two.png", xy(0), np.zeros(0, np.int64)),
              7: (_quat([0, 0, 1], 1.1), np.array([-0.3, 0.0, 2.0]), 5, "seven.jpg", xy(3), np.array([30, 999, 4]))}
    points = {30: (np.array([0.1, 0.2, 5.0]), np.array([1, 2, 3], np.uint8), 0.5, np.array([[40, 3], [7, 0]], np.int32)),
              4: (np.array([-1.0, 0.5, 4.0]), np.array([255, 0, 9], np.uint8), 1.25, np.array([[7, 2]], np.int32)),
              11: (np.array([1 / 3, -2 / 3, 6.0]), np.array([7, 7, 7], np.uint8), 0.0, np.array([[40, 0], [40, 2]], np.int32))}
    return cameras, images, points, [40, 2, 7]


def _same_model(a, b):
    assert set(a) == set(b)
    for k in a:
        if k == "names":
            assert a[k] == b[k]
        else:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def test_text_and_binary_read_back_equal(tmp_path):
    cameras, images, points, order = _handmade()
    colmap.write_raw(str(tmp_path / "txt"), cameras, images, points, False, order)
    colmap.write_raw(str(tmp_path / "bin"), cameras, images, points, True, order)
    assert sorted(os.listdir(tmp_path / "txt")) == ["cameras.txt", "images.txt", "points3D.txt"]
    assert sorted(os.listdir(tmp_path / "bin")) == ["cameras.bin", "images.bin", "points3D.bin"]
    mt, mb = colmap.read_model(str(tmp_path / "txt")), colmap.read_model(str(tmp_path / "bin"))
    _same_model(mt, mb)
    for raw_t, raw_b in zip(colmap.read_raw(str(tmp_path / "txt")), colmap.read_raw(str(tmp_path / "bin"))):
        assert sorted(raw_t) == sorted(raw_b)
        for key in raw_t:
            for x, y in zip(raw_t[key], raw_b[key]):
                assert np.array_equal(np.asarray(x), np.asarray(y)), key
    m = mb
    assert m["image_ids"].tolist() == [2, 7, 40] and m["names"] == ["two.png", "seven.jpg", "b/forty.jpg"]
    assert m["point_ids"].tolist() == [4, 11, 30]
    # view 0 (id 2) sees nothing; view 1 (id 7) points 30 and 4 (999 is no point); view 2 (id 40) point 11 once and 30
    assert m["obs"].dtype == np.int32 and m["obs"].tolist() == [[1, 0], [1, 2], [2, 1], [2, 2]]
    np.testing.assert_array_equal(m["K"][0], [[500.25, 0, 320.0], [0, 500.25, 240.5], [0, 0, 1]])
    np.testing.assert_array_equal(m["K"][2], [[700.125, 0, 400.0], [0, 701.5, 299.75], [0, 0, 1]])
    assert m["sizes"].tolist() == [[640, 480], [640, 480], [800, 600]]
    for k in range(3):
        q, t = images[int(m["image_ids"][k])][:2]
        R = m["R"][k]
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-15)
        np.testing.assert_allclose(R @ m["centres"][k] + t, 0, atol=1e-15)
        assert np.array_equal(m["t"][k], t) and np.array_equal(m["q"][k], q)
    # R(q) is the Hamilton convention: a rotation by +1.1 about z turns x towards y
    np.testing.assert_allclose(m["R"][1] @ [1, 0, 0], [math.cos(1.1), math.sin(1.1), 0], atol=1e-15)
    np.testing.assert_array_equal(m["xyz"][1], [1 / 3, -2 / 3, 6.0])


def test_text_format_as_specified(tmp_path):
    """Files typed out by hand: comments, an empty second line, and a trailing image whose second line is missing."""
    (tmp_path / "cameras.txt").write_text("# Camera list\n1 SIMPLE_PINHOLE 100 80 90.5 50 40\n3 PINHOLE 100 80 90 91 50 40\n")
    (tmp_path / "images.txt").write_text(
        "# Image list with two lines of data per image:\n"
        "9 1 0 0 0 0 0 2 3 last.jpg\n"
        "10.5 20.25 6 30 40 -1 1 2 8\n"
        "4 0.5 0.5 0.5 0.5 1 2 3 1 my image.png\n"
        "\n"
        "6 1 0 0 0 0 0 0 1 end.jpg\n")
    (tmp_path / "points3D.txt").write_text("# points\n8 0 0 4 10 20 30 0.25 9 2\n6 1 1 4 1 2 3 0.5 9 0 4 1\n")
    m = colmap.read_model(str(tmp_path))
    assert m["image_ids"].tolist() == [4, 6, 9] and m["names"] == ["my image.png", "end.jpg", "last.jpg"]
    assert m["point_ids"].tolist() == [6, 8] and m["obs"].tolist() == [[2, 0], [2, 1]]
    np.testing.assert_array_equal(m["R"][2], np.eye(3))
    np.testing.assert_allclose(m["R"][0], [[0, 0, 1], [1, 0, 0], [0, 1, 0]], atol=1e-16)  # q = (1, 1, 1, 1) / 2
    np.testing.assert_array_equal(m["rgb"], [[1, 2, 3], [10, 20, 30]])
    np.testing.assert_array_equal(m["centres"][2], [0, 0, -2])


def test_binary_is_preferred(tmp_path):
    cameras, images, points, order = _handmade()
    colmap.write_raw(str(tmp_path), cameras, images, points, True, order)
    other = dict(points)
    other[5] = (np.zeros(3), np.zeros(3, np.uint8), 0.0, np.zeros((0, 2), np.int32))
    colmap.write_raw(str(tmp_path), cameras, images, other, False, order)
    assert colmap.read_model(str(tmp_path))["point_ids"].tolist() == [4, 11, 30]
    os.remove(tmp_path / "points3D.bin")
    assert colmap.read_model(str(tmp_path))["point_ids"].tolist() == [4, 5, 11, 30]


@pytest.mark.parametrize("binary", [True, False])
def test_bad_models_raise(tmp_path, binary):
    cameras, images, points, order = _handmade()
    ext = ".bin" if binary else ".txt"
    # a camera with distortion: names the image and the undistorter
    radial = dict(cameras)
    radial[5] = ("RADIAL", 640, 480, np.array([500.0, 320.0, 240.0, 0.01, 0.001]))
    colmap.write_raw(str(tmp_path / "radial"), radial, images, points, binary, order)
    with pytest.raises(ValueError, match=r"(?s)images" + ext + r".*'(two\.png|seven\.jpg)'.*RADIAL.*undistorter"):
        colmap.read_model(str(tmp_path / "radial"))
    # an image whose camera the cameras file lacks
    lacking = {2: cameras[2]}
    colmap.write_raw(str(tmp_path / "lacking"), lacking, images, points, binary, order)
    with pytest.raises(ValueError, match=r"images" + ext + r".*camera 5"):
        colmap.read_model(str(tmp_path / "lacking"))
    # every file cut short
    for stem in ("cameras", "images", "points3D"):
        d = tmp_path / ("cut_" + stem)
        colmap.write_raw(str(d), cameras, images, points, binary, order)
        blob = (d / (stem + ext)).read_bytes()
        (d / (stem + ext)).write_bytes(blob[:len(blob) - 5] if binary else blob[:blob.rstrip().rfind(b" ")])
        if binary or stem != "images":
            with pytest.raises(ValueError, match=stem + ext):
                colmap.read_model(str(d))
    if binary:
        d = tmp_path / "model_id"
        colmap.write_raw(str(d), cameras, images, points, True, order)
        blob = bytearray((d / "cameras.bin").read_bytes())
        blob[12:16] = (77).to_bytes(4, "little")  # the first camera's model id
        (d / "cameras.bin").write_bytes(bytes(blob))
        with pytest.raises(ValueError, match=r"cameras\.bin.*unknown model id 77"):
            colmap.read_model(str(d))
    else:
        d = tmp_path / "half_triple"
        colmap.write_raw(str(d), cameras, images, points, False, order)
        text = (d / "images.txt").read_text().replace(" 30\n", "\n", 1)  # a 2-D point that lost its POINT3D_ID
        (d / "images.txt").write_text(text)
        with pytest.raises(ValueError, match=r"images\.txt"):
            colmap.read_model(str(d))
    with pytest.raises(ValueError, match="neither"):
        colmap.read_model(str(tmp_path / "nothing_here"))


def test_synthetic_model_reads_back(tmp_path):
    for binary in (True, False):
        d = str(tmp_path / ("b" if binary else "t"))
        wrote = synthetic.write_colmap_model(d, n_views=4, n_points=60, seed=3, binary=binary)
        m = colmap.read_model(d)
        for k in ("image_ids", "K", "R", "t", "centres", "point_ids", "xyz", "obs"):
            assert np.array_equal(m[k], wrote[k]), k
        assert m["names"] == wrote["names"] and len(m["obs"]) > 40
        assert len(set(map(tuple, m["obs"].tolist()))) == len(m["obs"])


# ------------------------------------------------------------------ the restatement on analytic scenes
def _score_of(ci, cj, x):
    obs = np.array([[0, 0], [1, 0]], np.int32)
    s, c = ref.pair_scores(obs, 2, np.array([ci, cj], np.float64), np.array([x], np.float64))
    assert c.tolist() == [[0, 1], [1, 0]] and s[0, 0] == s[1, 1] == 0 and s[0, 1] == s[1, 0]
    return s[0, 1]


def test_restatement_score_closed_forms():
    """theta0 = 5, sigma1 = 1 at and below it, sigma2 = 10 above: exp(-(theta - 5)^2 / 2) or / 200."""
    x = [0.0, 0.0, 0.0]
    five = math.radians(5.0)
    assert abs(_score_of([3, 0, 0], [2 * math.cos(five), 2 * math.sin(five), 0], x) - 1.0) < 1e-12  # 5 degrees
    assert _score_of([1, 0, 0], [2, 0, 0], x) == pytest.approx(math.exp(-12.5), rel=1e-13)  # 0: exact coordinates
    assert _score_of([1, 0, 0], [1, 1, 0], x) == pytest.approx(math.exp(-8.0), rel=1e-12)  # 45
    assert _score_of([0, 0, 2], [0, 3, 0], x) == pytest.approx(math.exp(-36.125), rel=1e-12)  # 90
    assert _score_of([1, 0, 0], [-2, 0, 0], x) == pytest.approx(math.exp(-153.125), rel=1e-11)  # 180
    assert _score_of([1, 2, 3], [4, 4, 4], [1, 2, 3]) == pytest.approx(math.exp(-12.5), rel=1e-13)  # X = C_i: theta = 0
    # just below and above theta0 the two widths apply
    for deg, sigma in ((4.0, 1.0), (6.0, 10.0), (2.5, 1.0), (30.0, 10.0)):
        r = math.radians(deg)
        want = math.exp(-(deg - 5.0) ** 2 / (2 * sigma * sigma))
        assert _score_of([1, 0, 0], [math.cos(r), math.sin(r), 0], x) == pytest.approx(want, rel=1e-11), deg
    # other parameters, and two points adding up
    obs = np.array([[0, 0], [1, 0], [0, 1], [1, 1], [0, 2]], np.int32)
    s, c = ref.pair_scores(obs, 2, np.array([[1.0, 0, 0], [1, 1, 0]]), np.array([[0.0, 0, 0], [0, 0, 0], [9, 9, 9]]), 45.0, 2.0, 3.0)
    assert c[0, 1] == 2 and s[0, 1] == pytest.approx(2.0, rel=1e-12)


def test_restatement_depth_range_indices():
    rng = np.random.default_rng(0)
    want = {1: (1, 1), 99: (1, 99), 100: (2, 100), 101: (2, 100), 250: (3, 248)}
    for n, (lo, hi) in want.items():
        z = rng.permutation(np.concatenate([np.arange(1, n + 1, dtype=np.float64), [0.0, -3.0, -0.5]]))
        assert ref.depth_range(z) == (0.75 * lo, 1.25 * hi), n
    with pytest.raises(ValueError):
        ref.depth_range(np.array([0.0, -1.0]))
    # through obs_depth: a camera looking down +z from z = -2 sees (0, 0, 3) at depth 5
    R, t = np.eye(3)[None], np.array([[0.0, 0.0, 2.0]])
    assert ref.obs_depth(np.array([[0, 0]]), R, t, np.array([[0.3, -0.4, 3.0]])).tolist() == [5.0]


def test_restatement_ranking():
    s = np.array([[0, 3, 3, 1, 5.0], [3, 0, 2, 2, 2], [3, 2, 0, 0, 0], [1, 2, 0, 0, 9], [5, 2, 0, 9, 0]])
    assert ref.rank_sources(s, 3).tolist() == [[4, 1, 2], [0, 2, 3], [0, 1, 3], [4, 1, 0], [3, 0, 1]]
    assert ref.rank_sources(s, 10).shape == (5, 4)


# ------------------------------------------------------------------ the written folder
def test_written_folder_reads_back(tmp_path):
    from PIL import Image
    h, w, scan = 128, 160, "garden"
    model = synthetic.write_colmap_model(str(tmp_path / "sparse"), n_views=5, n_points=200, height=h, width=w, seed=2)
    sel = ref.select(model, n_src=3)
    out = str(tmp_path / "data" / scan)
    colmap_scene.write_scan(out, model["K"], model["R"], model["t"], sel["depth_min"], sel["depth_max"], sel["pairs"],
                            sel["scores"])
    os.makedirs(os.path.join(out, "images"))
    for i in range(5):
        Image.fromarray(np.full((h, w, 3), 40 * i, np.uint8)).save(os.path.join(out, "images", "{:0>8}.jpg".format(i)))
    pairs = data.read_pair_file(os.path.join(out, "pair.txt"), pad=False)
    assert pairs == [(i, sel["pairs"][i].tolist()) for i in range(5)]
    lines = open(os.path.join(out, "pair.txt")).read().split("\n")
    assert lines[0] == "5" and lines[1] == "0"
    first = lines[2].split()
    assert first[0] == "3" and [float(x) for x in first[2::2]] == [sel["scores"][0, j] for j in sel["pairs"][0]]
    cache = reconstruct.ViewCache(str(tmp_path / "data"), scan, "tnt", device="cpu", image_size=(w, h))
    for i in range(5):
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = model["R"][i], model["t"][i]
        K4 = model["K"][i].astype(np.float32)
        K4[:2] /= 4.0
        dmin, dmax = sel["depth_min"][i], sel["depth_max"][i]
        assert 0 < dmin < dmax
        k, e, lo, interval, hi = data.read_cam_file(os.path.join(out, "cams_1", "{:0>8}_cam.txt".format(i)), tnt=True)
        assert np.array_equal(k, K4) and np.array_equal(e, E.astype(np.float32))
        assert (lo, hi) == (dmin, dmax) and interval == (dmax - dmin) / 192
        k, e, lo, interval = data.read_cam_file(os.path.join(out, "cams", "{:0>8}_cam.txt".format(i)))
        assert np.array_equal(k, K4) and np.array_equal(e, E.astype(np.float32)) and lo == dmin
        fields = open(os.path.join(out, "cams", "{:0>8}_cam.txt".format(i))).read().split("\n")[11].split()
        assert [float(x) for x in fields] == [dmin, (dmax - dmin) / 191, 192.0, dmax] and fields[2] == "192"
        assert interval == (dmin + 192 * ((dmax - dmin) / 191) - dmin) / 192  # what the reader makes of that line
        s = cache.sample(i, sel["pairs"][i].tolist(), images=False)
        views = [i] + sel["pairs"][i].tolist()
        assert s["hw"] == (h, w) and s["proj_matrix"]["stage1"].shape == (4, 2, 4, 4)
        for slot, vid in enumerate(views):
            Ev = np.eye(4)
            Ev[:3, :3], Ev[:3, 3] = model["R"][vid], model["t"][vid]
            Kv = model["K"][vid].astype(np.float32)
            np.testing.assert_array_equal(s["proj_matrix"]["stage3"][slot, 0], Ev.astype(np.float32))
            np.testing.assert_array_equal(s["proj_matrix"]["stage3"][slot, 1, :3, :3], Kv)
        dv = s["depth_values"]
        assert dv[0] == np.float32(dmin) and len(dv) in (192, 193) and abs(dv[191] - (dmin + 191 * (dmax - dmin) / 192)) < 1e-3 * dmax


def test_image_copy(tmp_path):
    from PIL import Image
    rgb = np.random.default_rng(0).integers(0, 256, (24, 32, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "a.jpg", quality=80)
    Image.fromarray(rgb).save(tmp_path / "b.png")
    colmap_scene._copy_image(str(tmp_path / "a.jpg"), str(tmp_path / "a_out.jpg"))
    colmap_scene._copy_image(str(tmp_path / "b.png"), str(tmp_path / "b_out.jpg"))
    assert (tmp_path / "a_out.jpg").read_bytes() == (tmp_path / "a.jpg").read_bytes()
    with Image.open(tmp_path / "b_out.jpg") as im:
        assert im.format == "JPEG" and im.size == (32, 24) and im.mode == "RGB"
    Image.fromarray(rgb).save(tmp_path / "want.jpg", quality=95)
    assert (tmp_path / "b_out.jpg").read_bytes() == (tmp_path / "want.jpg").read_bytes()


# ------------------------------------------------------------------ command lines and the package's imports
def test_parsers():
    p = reconstruct.make_parser()
    a = p.parse_args(["--loadckpt", "m.ckpt", "--testpath", "x", "--dataset", "tnt", "--image_size", "256", "192"])
    assert a.image_size == [256, 192]
    assert p.parse_args(["--loadckpt", "m.ckpt", "--testpath", "x"]).image_size is None
    with pytest.raises(SystemExit):
        p.parse_args(["--loadckpt", "m.ckpt", "--testpath", "x", "--image_size", "256"])
    c = colmap_scene.make_parser().parse_args(["--model", "m", "--images", "i", "--out", "o"])
    assert (c.n_src, c.theta0, c.sigma1, c.sigma2) == (10, 5.0, 1.0, 10.0)


def test_main_passes_image_size(monkeypatch, tmp_path):
    seen = []
    monkeypatch.setattr(reconstruct, "load_model", lambda ckpt: "model")
    monkeypatch.setattr(reconstruct, "reconstruct_scan",
                        lambda *a, **k: seen.append(k.get("image_size")) or {"fixed_hw": (1, 1)})
    os.makedirs(tmp_path / "garden")
    reconstruct.main(["--loadckpt", "m", "--testpath", str(tmp_path), "--dataset", "tnt", "--image_size", "256", "192"])
    reconstruct.main(["--loadckpt", "m", "--testpath", str(tmp_path), "--dataset", "tnt"])
    assert seen == [(256, 192), None]


def test_package_does_not_import_the_restatement():
    for name in ("colmap_scene.py", "colmap.py", "view_select.py"):
        src = open(os.path.join(ROOT, "transmvsnet_amd", name)).read()
        assert "oracle" not in src and "_view_select_ref" not in src, name


def test_wrappers_refuse_cpu_tensors_and_bad_sizes():
    import torch

    from transmvsnet_amd import view_select
    i32 = lambda *a: torch.zeros(*a, dtype=torch.int32)  # noqa: E731
    f64 = lambda *a: torch.zeros(*a, dtype=torch.float64)  # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        view_select.set_bits(i32(4), i32(4), 2, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        view_select.obs_depth(i32(4), i32(4), f64(2, 3), f64(2), f64(10, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        view_select.pair_scores(torch.zeros(2, 1, dtype=torch.int64), 10, f64(2, 3), f64(10, 3))
    for v, p in ((1, 10), (0, 10), (2, 0), (2, 2 ** 31 - 64)):
        with pytest.raises(ValueError):
            view_select.check_sizes(v, p)
    view_select.check_sizes(2, 1)
    view_select.check_sizes(300, 10 ** 6)  # 37.5 MB
    assert 300 * view_select.words(10 ** 6) * 8 == 37_500_000
    with pytest.raises(ValueError, match="workspace cap"):
        view_select.check_sizes(9000, 10 ** 6)  # 1.125 GB


def test_entries_refuse_before_any_launch():
    """The C entries' own checks (the pointers are host memory that is never read)."""
    from transmvsnet_amd import _lib, build
    build.build()
    lib = _lib.load()
    ARG, SHAPE = -1, -2
    backing = np.zeros(64, np.float64)
    p = (backing.ctypes.data + 63) & ~63
    sb, od, ps = lib.tmvs_vs_set_bits, lib.tmvs_vs_obs_depth, lib.tmvs_vs_pair_scores
    for nul in range(4):
        a = [p] * 4
        a[nul] = None
        assert sb(a[0], a[1], 4, 2, 10, a[2], a[3], None) == ARG
    assert sb(p, p, 4, 2, 10, p + 4, p, None) == ARG  # bits not 8-byte aligned
    for nul in range(7):
        a = [p] * 7
        a[nul] = None
        assert od(a[0], a[1], 4, 2, 10, a[2], a[3], a[4], a[5], a[6], None) == ARG
    for nul in range(5):
        a = [p] * 5
        a[nul] = None
        assert ps(a[0], 2, 10, a[1], a[2], 5.0, 1.0, 10.0, a[3], a[4], None) == ARG
    for bad in ((float("nan"), 1.0, 10.0), (5.0, 0.0, 10.0), (5.0, 1.0, -1.0), (5.0, float("inf"), 10.0)):
        assert ps(p, 2, 10, p, p, *bad, p, p, None) == ARG
    for v, n in ((1, 10), (0, 10), (-3, 10), (2, 0), (2, -1), (2, 2 ** 31 - 64), (9000, 10 ** 6)):
        assert sb(p, p, 4, v, n, p, p, None) == SHAPE, (v, n)
        assert od(p, p, 4, v, n, p, p, p, p, p, None) == SHAPE, (v, n)
        assert ps(p, v, n, p, p, 5.0, 1.0, 10.0, p, p, None) == SHAPE, (v, n)
    for m in (0, -1, 2 ** 31 - 256):
        assert sb(p, p, m, 2, 10, p, p, None) == SHAPE and od(p, p, m, 2, 10, p, p, p, p, p, None) == SHAPE


def test_view_select_header_matches_binding():
    import re

    from transmvsnet_amd import _lib
    src = open(os.path.join(ROOT, "include", "transmvs_view_select.h")).read()
    consts = dict(re.findall(r"#define\s+(TMVS_\w+)\s+(-?\d+)", src))
    assert int(consts["TMVS_VS_MAX_BITS_BYTES"]) == _lib.VS_MAX_BITS_BYTES
    assert int(consts["TMVS_VS_MAX_BLOCKS"]) == _lib.VS_MAX_BLOCKS
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    decls = {m.group(1): m.group(2).count(",") + 1
             for m in re.finditer(r"\bint\s+(tmvs_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert set(decls) == set(_lib.VS_SIGNATURES) and len(decls) == 3
    for name, n in decls.items():
        assert len(_lib.VS_SIGNATURES[name][1]) == n, name
    assert not set(decls) & (set(_lib.SIGNATURES) | set(_lib.SYNC_SIGNATURES))
