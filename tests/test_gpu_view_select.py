"""View selection on the GPU (csrc/view_select.hip through transmvsnet_amd.view_select) against the numpy
restatement tests/_view_select_ref.py, colmap_scene.convert end to end in both file formats, and one run from a
COLMAP model through reconstruct_scan to a PLY.

Shapes are the smallest at which the kernels can go wrong. The score kernel's block is 256 threads, each owning
couples of 64-bit words, so W = ceil(P / 64) takes 1, 2 (one couple), 255, 256, 257 (odd rows take the 8-byte
loads, even rows the 16-byte ones; a last couple with one word) and 515 (a thread's second couple); the pair grid
is capped at 2048 blocks, which V = 70 (2415 pairs) exceeds.

The bar on the scores is relative 1e-10, from the definition: every term is positive, so nothing cancels; atan2
and exp are within a few ulp on both sides; the exponent moves by at most 5 per degree of theta; up to 1e5 terms
add n 2^-53. Together below 1e-11."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _view_select_ref as ref
from transmvsnet_amd import _lib, colmap, colmap_scene, reconstruct, synthetic, view_select

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-10


def _up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _packed(obs, v, p):
    """The bit matrix by numpy: [V, W] uint64, bit p % 64 of word p / 64."""
    w = view_select.words(p)
    vis = np.zeros((v, w * 64), bool)
    vis[obs[:, 0], obs[:, 1]] = True
    return np.packbits(vis, axis=1, bitorder="little").view("<u8").reshape(v, w)


def _as_u64(bits):
    return bits.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------ tmvs_vs_set_bits
@pytest.mark.parametrize("v", [2, 3])
@pytest.mark.parametrize("p", [1, 63, 64, 65, 130])
def test_set_bits_equals_packbits(v, p):
    rng = np.random.default_rng([v, p])
    m = max(3, (v * p) // 2)
    obs = np.stack([rng.integers(0, v, m), rng.integers(0, p, m)], 1).astype(np.int32)
    obs = np.concatenate([obs, obs[: m // 2 + 1], [[v - 1, p - 1], [0, 0], [v - 1, p - 1]]]).astype(np.int32)  # duplicates
    bits = view_select.set_bits(_up(obs[:, 0], np.int32), _up(obs[:, 1], np.int32), v, p)
    assert bits.shape == (v, view_select.words(p)) and bits.dtype == torch.int64
    got = _as_u64(bits)
    np.testing.assert_array_equal(got, _packed(obs, v, p))
    if p % 64:
        assert not (got[:, -1] >> np.uint64(p % 64)).any()  # the tail bits stay zero
    assert bool((got[v - 1, -1] >> np.uint64((p - 1) % 64)) & np.uint64(1))


@pytest.mark.parametrize("bad", [(3, 5), (-1, 5), (0, 130), (0, -1), (1, 191), (2 ** 31 - 1, 0), (0, 2 ** 31 - 1)])
def test_set_bits_out_of_range_raises_and_writes_nothing(bad):
    v, p = 3, 130
    w = view_select.words(p)
    good = np.array([[0, 0], [2, 129], [1, 64], [2, 63]], np.int32)
    obs = np.concatenate([good[:2], [bad], good[2:]]).astype(np.int32)
    guard = 0x5A5A5A5A5A5A5A5A
    slab = torch.full((v * w + 16,), guard, dtype=torch.int64, device=DEV)
    bits = slab[8:8 + v * w].view(v, w)
    bits.zero_()
    with pytest.raises(ValueError, match="1 observations"):
        view_select.set_bits(_up(obs[:, 0], np.int32), _up(obs[:, 1], np.int32), v, p, bits=bits)
    assert (slab[:8] == guard).all() and (slab[8 + v * w:] == guard).all()
    np.testing.assert_array_equal(_as_u64(bits), _packed(good, v, p))  # the good ones are set, the bad one nowhere


# ------------------------------------------------------------------ tmvs_vs_obs_depth
def test_obs_depth_equals_restatement():
    rng = np.random.default_rng(11)
    v, p, m = 5, 333, 1000
    R = np.stack([synthetic._rodrigues(rng.normal(size=3), rng.uniform(0, 3)) for _ in range(v)])
    t, xyz = rng.normal(size=(v, 3)) * 50, rng.normal(size=(p, 3)) * 300
    obs = np.stack([rng.integers(0, v, m), rng.integers(0, p, m)], 1).astype(np.int32)
    z = view_select.obs_depth(_up(obs[:, 0], np.int32), _up(obs[:, 1], np.int32), _up(R[:, 2, :], np.float64),
                              _up(t[:, 2], np.float64), _up(xyz, np.float64))
    assert z.dtype == torch.float64
    assert torch.equal(z.cpu(), torch.from_numpy(ref.obs_depth(obs, R, t, xyz)))
    bad = obs.copy()
    bad[7] = (v, 0)
    bad[8] = (0, p)
    with pytest.raises(ValueError, match="2 observations"):
        view_select.obs_depth(_up(bad[:, 0], np.int32), _up(bad[:, 1], np.int32), _up(R[:, 2, :], np.float64),
                              _up(t[:, 2], np.float64), _up(xyz, np.float64))


# ------------------------------------------------------------------ tmvs_vs_pair_scores
@functools.lru_cache(maxsize=None)
def _scene(v, p, density=0.3):
    """Cameras on a ring of radius ~10 round points in a ball of radius 3 (so the angles spread over 0..60
    degrees), random visibility; with V >= 3 view 1 sees nothing, with V >= 4 views 2 and 3 share no point.
    Returns (obs, centres, xyz, scores, counts) with the restatement's answers."""
    rng = np.random.default_rng([v, p, 9])
    ang = rng.uniform(0, 2 * np.pi, v)
    centres = np.stack([10 * np.cos(ang), 10 * np.sin(ang), rng.uniform(-2, 2, v)], 1) * rng.uniform(0.3, 1.2, (v, 1))
    xyz = rng.normal(size=(p, 3))
    xyz *= 3 * rng.uniform(0, 1, (p, 1)) ** (1 / 3) / np.linalg.norm(xyz, axis=1, keepdims=True)
    vis = rng.random((v, p)) < density
    vis[0, 0] = vis[v - 1, 0] = vis[0, p - 1] = vis[v - 1, p - 1] = True  # the first and the last point count
    if v >= 3:
        vis[1] = False
    if v >= 4:
        vis[2, 1::2] = False
        vis[3, 0::2] = False
    obs = np.argwhere(vis).astype(np.int32)
    obs = obs[rng.permutation(len(obs))]
    scores, counts = ref.pair_scores(obs, v, centres, xyz)
    return obs, centres, xyz, scores, counts


def _run(obs, v, p, centres, xyz, poison=True, **kw):
    bits = view_select.set_bits(_up(obs[:, 0], np.int32), _up(obs[:, 1], np.int32), v, p)
    if poison and p % 64:
        bits[:, -1] |= -(1 << (p % 64))  # ones in the unused tail bits of every row
    return view_select.pair_scores(bits, p, _up(centres, np.float64), _up(xyz, np.float64), **kw)


W_CASES = {1: 37, 2: 128, 255: 255 * 64 - 3, 256: 256 * 64, 257: 256 * 64 + 1, 515: 515 * 64 - 10}


@pytest.mark.parametrize("v", [2, 3, 7])
@pytest.mark.parametrize("w", sorted(W_CASES))
def test_pair_scores_equal_restatement(v, w):
    p = W_CASES[w]
    assert view_select.words(p) == w
    obs, centres, xyz, want_s, want_c = _scene(v, p)
    scores, counts = _run(obs, v, p, centres, xyz)
    assert scores.dtype == torch.float64 and counts.dtype == torch.int32 and scores.shape == counts.shape == (v, v)
    got_s, got_c = scores.cpu().numpy(), counts.cpu().numpy()
    np.testing.assert_array_equal(got_c, want_c)
    rel = np.abs(got_s - want_s).max() / want_s.max()
    print(f"V={v} W={w}: worst |difference| / largest score {rel:.3g}, largest count {want_c.max()}")
    np.testing.assert_allclose(got_s, want_s, rtol=RTOL, atol=0)
    assert want_c.max() > 0 and want_s.max() > 0
    assert torch.equal(scores, scores.T) and torch.equal(counts, counts.T)
    assert (torch.diagonal(scores) == 0).all() and (torch.diagonal(counts) == 0).all()
    if v >= 3:  # a view without an observation
        assert (got_s[1] == 0).all() and (got_c[1] == 0).all()
    if v >= 4:  # a pair without a common point: exactly nothing
        assert got_s[2, 3] == 0 and got_c[2, 3] == 0 and want_c[2, 4] > 0
    again, _ = _run(obs, v, p, centres, xyz)
    assert torch.equal(again, scores)  # bit for bit from run to run
    clean, _ = _run(obs, v, p, centres, xyz, poison=False)
    assert torch.equal(clean, scores)


def test_pair_scores_more_pairs_than_blocks():
    v, p = 70, 200
    assert v * (v - 1) // 2 == 2415 > _lib.VS_MAX_BLOCKS == 2048
    obs, centres, xyz, want_s, want_c = _scene(v, p)
    scores, counts = _run(obs, v, p, centres, xyz)
    np.testing.assert_array_equal(counts.cpu().numpy(), want_c)
    np.testing.assert_allclose(scores.cpu().numpy(), want_s, rtol=RTOL, atol=0)
    assert torch.equal(scores, scores.T) and torch.equal(_run(obs, v, p, centres, xyz)[0], scores)


def test_pair_scores_other_parameters_and_closed_form():
    obs = np.array([[0, 0], [1, 0], [0, 1], [1, 1], [0, 2]], np.int32)
    centres, xyz = np.array([[1.0, 0, 0], [1, 1, 0]]), np.array([[0.0, 0, 0], [0, 0, 0], [9, 9, 9]])
    s, c = _run(obs, 2, 3, centres, xyz, theta0=45.0, sigma1=2.0, sigma2=3.0)
    assert c.tolist() == [[0, 2], [2, 0]] and abs(s[0, 1].item() - 2.0) < 1e-12
    s, c = _run(obs, 2, 3, centres, xyz)  # 45 degrees against theta0 = 5, sigma2 = 10: exp(-8) twice
    np.testing.assert_allclose(s[0, 1].item(), 2 * np.exp(-8.0), rtol=RTOL)
    s, _ = _run(np.array([[0, 0], [1, 0]], np.int32), 2, 1, np.array([[1.0, 2, 3], [4, 4, 4]]), np.array([[1.0, 2, 3]]))
    np.testing.assert_allclose(s[0, 1].item(), np.exp(-12.5), rtol=RTOL)  # the point at a camera centre: theta = 0


# ------------------------------------------------------------------ colmap_scene.convert
SEED = 6  # chosen on the CPU: every adjacent gap among a view's ranked scores exceeds relative 1e-8 (asserted below)


def _write_images(image_dir, names, h, w):
    from PIL import Image
    os.makedirs(image_dir, exist_ok=True)
    for i, name in enumerate(names):
        y, x = np.mgrid[0:h, 0:w]
        rgb = np.stack([(x * 3 + i * 20) % 256, (y * 5) % 256, (x + y) % 256], -1).astype(np.uint8)
        Image.fromarray(rgb).save(os.path.join(image_dir, name))


@pytest.mark.parametrize("binary", [True, False])
def test_convert_equals_restatement(tmp_path, binary):
    h, w = 128, 160
    wrote = synthetic.write_colmap_model(str(tmp_path / "sparse"), n_views=6, n_points=300, height=h, width=w, seed=SEED,
                                         binary=binary)
    want = ref.select(wrote)
    for i in range(6):  # the comparison of the lists cannot hinge on a tie
        s = want["scores"][i, want["pairs"][i]]
        assert (s[:-1] - s[1:] > 1e-8 * s[:-1]).all(), (i, s)
    _write_images(str(tmp_path / "photos"), wrote["names"], h, w)
    out = str(tmp_path / "data" / "garden")
    res = colmap_scene.convert(str(tmp_path / "sparse"), str(tmp_path / "photos"), out)
    np.testing.assert_array_equal(res["depth_min"], want["depth_min"])
    np.testing.assert_array_equal(res["depth_max"], want["depth_max"])
    np.testing.assert_array_equal(res["counts"], want["counts"])
    np.testing.assert_allclose(res["scores"], want["scores"], rtol=RTOL, atol=0)
    assert res["pairs"].shape == (6, 5) and res["pairs"].tolist() == want["pairs"].tolist()
    from transmvsnet_amd import data
    assert data.read_pair_file(os.path.join(out, "pair.txt"), pad=False) == [(i, want["pairs"][i].tolist()) for i in range(6)]
    _, _, lo, _, hi = data.read_cam_file(os.path.join(out, "cams_1", "{:0>8}_cam.txt".format(3)), tnt=True)
    assert (lo, hi) == (want["depth_min"][3], want["depth_max"][3])
    assert sorted(os.listdir(os.path.join(out, "images"))) == ["{:0>8}.jpg".format(i) for i in range(6)]
    kept = colmap_scene.convert(str(tmp_path / "sparse"), None, str(tmp_path / "data" / "two"), n_src=2, copy_images=False)
    assert kept["pairs"].tolist() == want["pairs"][:, :2].tolist()


def test_convert_names_the_view_without_depths(tmp_path):
    wrote = synthetic.write_colmap_model(str(tmp_path / "a"), n_views=4, n_points=80, seed=SEED)
    images = dict(wrote["images"])
    q, t, cam, name, xy, ids = images[5]
    images[5] = (q, t, cam, name, xy, np.full_like(ids, -1))
    colmap.write_raw(str(tmp_path / "b"), wrote["cameras"], images, wrote["points3D"], True)
    with pytest.raises(ValueError, match="view_002.png"):
        colmap_scene.convert(str(tmp_path / "b"), None, str(tmp_path / "out"), copy_images=False)


# ------------------------------------------------------------------ COLMAP model -> scan folder -> point cloud
class _NearestStub:
    """tests/_postprocess_ref.StubModel for cameras that went through a quaternion and a text file: the reference
    view is the planted view whose extrinsics are nearest (they agree to float32 rounding)."""

    def __init__(self, scene):
        self.es = scene["Es"]
        self.t = {k: _up(scene[k], np.float32) for k in ("depths", "conf3", "conf2", "conf1")}
        self.calls = []

    def __call__(self, imgs, proj_matrix, depth_values):
        e = proj_matrix["stage3"][0, 0, 0].numpy()
        d = np.abs(self.es - e[None]).reshape(len(self.es), -1).max(1)
        i = int(np.argmin(d))
        assert d[i] < 1e-4, "reference view not recognised"
        self.calls.append(i)
        t = self.t
        return {"depth": t["depths"][i:i + 1], "photo_confidence": t["conf3"][i:i + 1],
                "stage1": {"photo_confidence": t["conf1"][i:i + 1]}, "stage2": {"photo_confidence": t["conf2"][i:i + 1]},
                "stage3": {"photo_confidence": t["conf3"][i:i + 1], "depth": t["depths"][i:i + 1]}}


def _planted_colmap(root, scene, step=6):
    """The planted scene as a COLMAP model: its cameras, and the depth maps' surface sampled every `step` pixels as
    the 3-D points, each seen by the views it projects into."""
    from PIL import Image
    v, h, w = scene["depths"].shape
    cameras, images, points, xyz = {}, {}, {}, []
    Ks, Es = scene["Ks"].astype(np.float64), scene["Es"].astype(np.float64)
    for i in range(v):
        ys, xs = np.mgrid[step // 2:h:step, step // 2:w:step]
        d = scene["depths"][i][ys, xs].astype(np.float64)
        rays = np.stack([(xs - Ks[i, 0, 2]) / Ks[i, 0, 0], (ys - Ks[i, 1, 2]) / Ks[i, 1, 1], np.ones_like(d)], -1)
        pc = (rays * d[..., None])[d > 0]
        xyz.append((pc - Es[i, :3, 3]) @ Es[i, :3, :3])  # R^T (X_cam - t)
    xyz = np.concatenate(xyz)
    tracks = [[] for _ in xyz]
    os.makedirs(os.path.join(root, "photos"))
    for i in range(v):
        pc = xyz @ Es[i, :3, :3].T + Es[i, :3, 3]
        uv = pc[:, :2] / pc[:, 2:3] * [Ks[i, 0, 0], Ks[i, 1, 1]] + [Ks[i, 0, 2], Ks[i, 1, 2]]
        seen = np.nonzero((pc[:, 2] > 0) & (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h))[0]
        for k, p in enumerate(seen):
            tracks[p].append((i + 1, k))
        cameras[i + 1] = ("PINHOLE", w, h, np.array([Ks[i, 0, 0], Ks[i, 1, 1], Ks[i, 0, 2], Ks[i, 1, 2]]))
        images[i + 1] = (synthetic._rot_to_quat(Es[i, :3, :3]), Es[i, :3, 3], i + 1, f"shot{i}.png", uv[seen], seen + 1)
        Image.fromarray((scene["images"][i] * 255).astype(np.uint8)).save(os.path.join(root, "photos", f"shot{i}.png"))
    for p in range(len(xyz)):
        points[p + 1] = (xyz[p], np.zeros(3, np.uint8), 0.0, np.array(tracks[p], np.int32).reshape(-1, 2))
    colmap.write_raw(os.path.join(root, "sparse"), cameras, images, points, True)


def test_colmap_model_to_point_cloud(tmp_path):
    from tests._postprocess_ref import planted_scene
    sc = planted_scene()
    v, (h, w) = len(sc["depths"]), sc["depths"].shape[1:]
    root = str(tmp_path)
    _planted_colmap(root, sc)
    conv = colmap_scene.convert(os.path.join(root, "sparse"), os.path.join(root, "photos"), os.path.join(root, "data", "yard"))
    assert conv["pairs"].shape == (v, v - 1) and (conv["counts"][~np.eye(v, dtype=bool)] > 0).all()
    plane = 650.0  # the planted surface lies about 650 in front of the cameras
    assert (conv["depth_min"] < plane).all() and (conv["depth_max"] > plane).all() and (conv["depth_min"] > 0.5 * plane).all()
    model = _NearestStub(sc)
    res = reconstruct.reconstruct_scan(model, os.path.join(root, "data"), "yard", dataset="tnt", outdir=os.path.join(root, "out"),
                                       image_size=(w, h))
    assert model.calls == list(range(v)) and res["fixed_hw"] == (h, w)
    print("colmap -> tnt: fused points", len(res["points"]), "of", v * h * w)
    assert len(res["points"]) > 0.1 * v * h * w
    head, body = open(res["ply"], "rb").read().split(b"end_header\n")
    assert res["ply"] == os.path.join(root, "out", "yard.ply")
    assert ("element vertex %d\n" % len(res["points"])).encode() in head and len(body) == 15 * len(res["points"])
