"""DTU evaluation on the GPU (-m gpu) against the numpy restatement tests/_dtu_eval_ref.py. Comparisons are
exact unless stated: the kernels and the restatement use the same fp64 arithmetic in the same order, so
no threshold case is ambiguous. All inputs are generated here."""
import functools

import numpy as np
import pytest
import torch

from tests import _dtu_eval_ref as ref
from transmvsnet_amd import dtu_eval

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _surface(n, seed, spacing=0.1, offset=300.0):
    """n points on a wavy patch, about `spacing` apart, coordinates round `offset` (float32 spacing 3e-5)."""
    g = np.random.default_rng(seed)
    side = max(np.sqrt(n) * spacing, spacing)
    xy = g.random((n, 2)) * side
    z = 0.5 * np.sin(xy[:, 0]) * np.cos(0.7 * xy[:, 1])
    return (np.concatenate([xy, z[:, None]], 1) + offset).astype(np.float32)


def _check_thin(xyz, radius, perm, candidates=None):
    want = ref.thin_points(xyz, radius, perm, candidates)
    keep, rounds = dtu_eval.thin_points(_gpu(xyz), radius, perm=torch.from_numpy(np.asarray(perm, np.int64)),
                                        return_rounds=True)
    got = keep.cpu().numpy()
    assert got.dtype == bool and got.shape == want.shape
    assert np.array_equal(got, want), (int(got.sum()), int(want.sum()), int((got != want).sum()))
    return want, rounds


# ----------------------------------------------------------------- thinning
@pytest.mark.parametrize("n", [1, 2, 63, 257, 6000])
def test_thin_points_equals_sequential_greedy(n):
    xyz = _surface(n, seed=n)
    want, rounds = _check_thin(xyz, 0.2, np.random.default_rng(100 + n).permutation(n))
    assert want.sum() >= 1 and rounds >= 1
    if n == 6000:
        assert want.sum() < n  # the patch is dense enough for the thinning to remove points


def test_thin_points_duplicates():
    xyz = np.repeat(_surface(257, seed=5), 4, axis=0)
    want, _ = _check_thin(xyz, 0.2, np.random.default_rng(6).permutation(len(xyz)))
    assert want.sum() <= 257


def test_thin_points_chain_needs_one_round_per_point():
    """300 points on a line 0.15 apart, visited in order: point k is decided only after point k - 1, so the
    rounds equal the chain's length; the loop must run them all and stop with the greedy answer."""
    n = 300
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 0] = np.float32(300.0) + np.float32(0.15) * np.arange(n, dtype=np.float32)
    xyz[:, 1:] = 300.0
    want, rounds = _check_thin(xyz, 0.2, np.arange(n))
    assert want.tolist() == [k % 2 == 0 for k in range(n)]
    assert n - 1 <= rounds <= n


def test_thin_points_radius_is_inclusive_across_cell_edges():
    """A lattice of spacing exactly 0.25 with radius 0.25: d2 == radius^2 exactly for the six axis
    neighbours, which straddle cell edges everywhere (the cell edge is just above the radius)."""
    i = np.arange(12)
    x, y, z = np.meshgrid(i, i[:9], i[:5], indexing="ij")
    xyz = (np.stack([x, y, z], -1).reshape(-1, 3) * 0.25 + 300.0).astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64), np.stack([x, y, z], -1).reshape(-1, 3) * 0.25 + 300.0)
    in_order, _ = _check_thin(xyz, 0.25, np.arange(len(xyz)))
    # in index order the survivors are the checkerboard: every axis neighbour is removed (inclusive)
    assert np.array_equal(in_order, ((x + y + z) % 2 == 0).ravel())
    _check_thin(xyz, 0.25, np.random.default_rng(3).permutation(len(xyz)))


def test_thin_points_one_overfull_cell():
    g = np.random.default_rng(8)
    v = g.standard_normal((2000, 3))
    xyz = (300.05 + 0.049 * v / np.linalg.norm(v, axis=1, keepdims=True) * g.random((2000, 1))).astype(np.float32)
    perm = g.permutation(2000)
    want, rounds = _check_thin(xyz, 0.2, perm)  # all within a ball of diameter < 0.1
    assert want.sum() == 1 and want[perm[0]] and rounds == 2


def test_thin_points_60000_against_kdtree_candidates():
    from scipy.spatial import cKDTree
    n = 60000
    xyz = _surface(n, seed=11)
    tree = cKDTree(xyz.astype(np.float64))
    want, rounds = _check_thin(xyz, 0.2, np.random.default_rng(12).permutation(n),
                               candidates=lambda i: tree.query_ball_point(xyz[i].astype(np.float64), 0.2 * 1.001))
    assert 0.05 * n < want.sum() < 0.5 * n and rounds < 64


def test_thin_points_seed_is_deterministic():
    xyz = _gpu(_surface(6000, seed=21))
    a, b = dtu_eval.thin_points(xyz, seed=7), dtu_eval.thin_points(xyz, seed=7)
    assert torch.equal(a, b)
    assert not torch.equal(a, dtu_eval.thin_points(xyz, seed=8))
    perm = torch.randperm(6000, generator=torch.Generator().manual_seed(7))
    assert np.array_equal(a.cpu().numpy(), ref.thin_points(xyz.cpu().numpy(), 0.2, perm.numpy()))
    with pytest.raises(ValueError, match="permutation"):
        dtu_eval.thin_points(xyz, perm=torch.zeros(6000, dtype=torch.int64))


# ----------------------------------------------------------------- nearest distance
BB = np.array([[280.0, 280.0, 280.0], [395.0, 340.0, 339.0]])  # blocks: x [280, 400), y [280, 400), z [280, 340)


def _check_nearest(q_from, q_to, max_dist=20.0, bb=BB, raw=None, **kw):
    q_from, q_to = np.asarray(q_from, np.float32).reshape(-1, 3), np.asarray(q_to, np.float32).reshape(-1, 3)
    raw = ref.min_d2(q_from, q_to) if raw is None else raw
    want2 = ref.nearest_d2(q_from, q_to, bb, max_dist, raw=raw)
    want = ref.nearest_distance(q_from, q_to, bb, max_dist, raw=raw)
    dist, d2 = dtu_eval.nearest_distance(_gpu(q_from), _gpu(q_to), bb, max_dist, 60.0, return_d2=True, **kw)
    assert dist.dtype == torch.float64 and d2.dtype == torch.float64
    dist, d2 = dist.cpu().numpy(), d2.cpu().numpy()
    bad = np.flatnonzero(d2 != want2)
    assert bad.size == 0, (bad[:5], d2[bad[:5]], want2[bad[:5]])
    assert np.all(np.abs(dist - want) <= 2 * np.spacing(want))  # the square root's rounding
    assert np.all(dist <= max_dist)
    return want


def _cloud(n, seed, lo=290.0, hi=330.0):
    """Half on a wavy surface, half anywhere in the box (those are mostly further than 5 from the surface)."""
    g = np.random.default_rng(seed)
    p = lo + g.random((n, 3)) * (hi - lo)
    k = n // 2
    p[:k, 2] = 310.0 + 2.0 * np.sin(0.3 * p[:k, 0]) * np.cos(0.2 * p[:k, 1])
    return p.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _brute_force_case(n_from, n_to):
    """(from, to, brute-force minimum d2), computed once for both max_dist."""
    g = np.random.default_rng(n_from)
    q_to = _cloud(n_to, seed=n_to)
    q_to[n_to // 2:, 2] = 310.0 + g.random(n_to - n_to // 2)  # to-points all near the surface: far from-points exist
    q_from = _cloud(n_from, seed=1000 + n_from, lo=285.0, hi=335.0)
    return q_from, q_to, ref.min_d2(q_from, q_to)


@pytest.mark.parametrize("max_dist", [5.0, 20.0])
@pytest.mark.parametrize("n_from,n_to", [(1, 1), (257, 63), (6000, 5000)])
def test_nearest_distance_equals_brute_force(n_from, n_to, max_dist):
    q_from, q_to, raw = _brute_force_case(n_from, n_to)
    want = _check_nearest(q_from, q_to, max_dist, raw=raw)
    if n_from == 6000:
        assert (want == max_dist).sum() > 100 and (want < 0.5).sum() > 100


def test_nearest_distance_edges_of_cells_blocks_and_range():
    g = np.random.default_rng(4)
    q_to = np.concatenate([_cloud(500, seed=9, lo=279.0, hi=300.0), [[277.0, 281.0, 281.0], [401.0, 399.0, 339.0]]])
    below = np.nextafter(np.float32(280.0), np.float32(0))
    edge = [[280, 280, 280], [281, 282, 283], [285, 290, 280], [340, 340, 300], [340, 300, 339.99],  # cell / block edges
            [below, 290, 290], [290, below, 290], [290, 290, below],  # just outside: max_dist
            [400, 290, 290], [290, 400, 290], [290, 290, 340],  # the range's open end
            [np.nextafter(np.float32(400), np.float32(0)), 399, np.nextafter(np.float32(340), np.float32(0))],
            [281, 281, 281]]  # its nearest to-point (277, 281, 281) lies outside BB, in the neighbouring block
    want = _check_nearest(np.float32(edge), q_to)
    assert np.all(want[5:11] == 20.0) and want[0] < 20.0
    assert want[11] < 3.0  # inside the range's last cell, next to the to-point beyond it
    lattice = 280.0 + g.integers(0, 40, (300, 3)).astype(np.float32)  # from-points on cell corners
    _check_nearest(lattice, q_to)
    _check_nearest(lattice, q_to, max_dist=5.0)


def test_nearest_distance_isolated_points_at_the_threshold():
    q_to = np.float32([[300, 300, 300]])  # n_to = 1
    q_from = np.float32([[300, 300, 319.9], [300, 300, 320.1], [300, 300, 320.0], [300, 300, 300], [311, 311, 311.5],
                         [300, 304.9, 300], [300, 305.1, 300]])
    want = _check_nearest(q_from, q_to)
    assert want[0] == np.float64(np.float32(319.9)) - 300 and want[0] < 20
    assert want[1] == 20 and want[2] == 20 and want[3] == 0 and 19 < want[4] < 20
    want = _check_nearest(q_from, q_to, max_dist=5.0)
    assert want[5] == 300 - np.float64(np.float32(295.1)) or want[5] < 5
    assert want[6] == 5 and want[0] == 5
    for cell in (0.5, 3.0):  # other grids, same answer
        _check_nearest(q_from, q_to, cell=cell)


def test_nearest_distance_empty_region_between_clusters():
    g = np.random.default_rng(13)
    a = (np.float32([300, 300, 300]) + g.random((400, 3)) * 2).astype(np.float32)
    b = (np.float32([330, 300, 300]) + g.random((400, 3)) * 2).astype(np.float32)
    between = np.stack([np.linspace(301, 331, 61), np.full(61, 301.0), np.full(61, 301.0)], 1).astype(np.float32)
    want = _check_nearest(np.concatenate([between, a[:50], b[:50]]), np.concatenate([a, b]))
    assert want[:61].max() > 13 and want[61:].max() == 0
    want = _check_nearest(between, np.concatenate([a, b]), max_dist=5.0)
    assert (want == 5).sum() > 20


# ----------------------------------------------------------------- mask and plane
def test_in_obs_mask_and_above_plane_equal_numpy():
    g = np.random.default_rng(17)
    mask = (g.random((7, 5, 3)) > 0.4).astype(np.uint8)
    mask[0, 0, 0] = mask[6, 4, 2] = 1
    bb = np.array([[300.0, 310.0, 320.0], [303.0, 312.0, 321.0]])
    res = 0.5
    idx = np.float32([-1, 0, 0.49, 0.5, 1, 1.5, 2.5, 6, 6.49, 6.5, 7, 7.5, 8])  # Qv before rounding, per axis
    grid = np.stack(np.meshgrid(idx, idx[:10], idx[:8], indexing="ij"), -1).reshape(-1, 3)
    pts = ((grid - 1) * res + bb[0]).astype(np.float32)  # exact: halves and quarters round 300
    pts = np.concatenate([pts, (bb[0] - 1 + g.random((2000, 3)) * 6).astype(np.float32)])
    want = ref.in_obs_mask(pts, mask, bb, res)
    got = dtu_eval.in_obs_mask(_gpu(pts), mask, bb, res).cpu().numpy()
    assert got.dtype == bool and np.array_equal(got, want) and 0 < want.sum() < len(want)
    full = np.ones((7, 5, 3), np.uint8)
    edge = ((np.float32([[0, 1, 1], [1, 1, 1], [7, 5, 3], [8, 5, 3], [7, 6, 3], [7, 5, 4], [0.5, 1, 1], [7.5, 5, 3],
                         [7.49, 5.49, 3.49]]) - 1) * res + bb[0]).astype(np.float32)
    assert dtu_eval.in_obs_mask(_gpu(edge), _gpu(full), bb, res).tolist() == [False, True, True, False, False, False,
                                                                              True, False, True]
    plane = np.array([0.25, -0.5, 1.0, -245.0])  # 0.25 x - 0.5 y + z = 245, exact for the points below
    on = np.float32([[300, 310, 325], [304, 312, 325], [300, 310, 325.25], [300, 310, 324.75]])
    assert dtu_eval.above_plane(_gpu(on), plane).tolist() == [False, False, True, False]
    want = ref.above_plane(pts, plane)
    assert np.array_equal(dtu_eval.above_plane(_gpu(pts), plane).cpu().numpy(), want) and 0 < want.sum() < len(want)


# ----------------------------------------------------------------- end to end
# the data lies 0.125 and 0.375 above a tilted lattice along its normal (481, 0, 904) / 4096 * 4, whose length
# is 0.25 + 1.2e-7 in coordinates that float32 holds exactly: the mean accuracy is 0.25 within 1e-6
SHIFT = np.array([481.0, 0.0, 904.0]) / 4096.0
STEP_U, STEP_V = np.array([904.0, 0.0, -481.0]) / 2048.0, np.array([0.0, 0.5, 0.0])


def _scan():
    g = np.random.default_rng(19)
    i, j = np.meshgrid(np.arange(40), np.arange(30), indexing="ij")
    i, j = i.ravel()[:, None], j.ravel()[:, None]
    stl = np.array([300.0, 300.0, 310.0]) + i * STEP_U + j * STEP_V
    below = np.array([300.0, 300.0, 290.0]) + (i * STEP_U + j * STEP_V)[::6]  # under the ground plane z = 295
    covered = (i.ravel() >= 5)  # a hole in the data: completeness distances vary there
    data = np.concatenate([stl[covered] + 0.5 * SHIFT, stl[covered] + 1.5 * SHIFT])
    data = np.repeat(data, 2, axis=0)  # duplicates for the thinning
    blob = np.array([300.0, 300.0, 310.0]) + 20 * STEP_U + 120 * SHIFT + g.integers(0, 64, (60, 3)) / 256.0  # 30 mm off
    data = np.concatenate([data, blob])[g.permutation(len(data) + 60)]
    for a in (stl, below, data):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    bb = np.array([[280.0, 280.0, 280.0], [330.0, 330.0, 339.0]])
    mask = np.zeros((51, 51, 60), np.uint8)
    mask[:30] = 1  # x < 309.5: the volume cut in half
    return (data.astype(np.float32), np.concatenate([stl, below]).astype(np.float32), mask, bb, 1.0,
            np.array([0.0, 0.0, 1.0, -295.0]))


def test_evaluate_cloud_end_to_end():
    data, stl, mask, bb, res, plane = _scan()
    perm = torch.randperm(len(data), generator=torch.Generator().manual_seed(5)).numpy()
    want = ref.evaluate_cloud(data, stl, mask, bb, res, plane, perm)
    got = dtu_eval.evaluate_cloud(_gpu(data), _gpu(stl), mask, bb, res, plane, seed=5)
    print({k: (got[k], want[k]) for k in want})
    assert set(got) == set(want)
    for k in ("n_input", "n_thinned", "n_data", "n_stl"):
        assert got[k] == want[k], k
    assert want["n_thinned"] < want["n_input"] // 2 + 60 and 0 < want["n_data"] < want["n_thinned"] - 60
    assert want["n_stl"] == 1200  # the points under the plane are left out
    for k in ("acc_median", "comp_median"):
        assert abs(got[k] - want[k]) <= 2 * np.spacing(want[k]), k
    for k in ("acc_mean", "comp_mean", "acc_var", "comp_var", "overall"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k  # fp64 sums in another order: n * 2^-53 << 1e-12
    assert abs(got["acc_mean"] - 0.25) <= 1e-6 and abs(got["acc_median"] - 0.25) <= 1e-6
    assert want["acc_var"] > 0.01 and want["comp_var"] > 0.01 and want["comp_mean"] > 0.125 + 1e-3


def test_driver_from_files_equals_evaluate_cloud(tmp_path):
    """python -m transmvsnet_amd.dtu_eval on files laid out as the reconstruct driver and the DTU data lay them
    out: the JSON holds evaluate_cloud's dict per scan and the means of the per-scan means."""
    import json
    import os

    from transmvsnet_amd import dynamic_fusion
    data, stl, mask, bb, res, plane = _scan()
    dtu = tmp_path / "dtu"
    os.makedirs(dtu / "Points" / "stl")
    os.makedirs(dtu / "ObsMask")
    for scan, sub in ((9, data), (118, data[::2])):
        os.makedirs(tmp_path / "out" / f"scan{scan}")
        dynamic_fusion.save_ply(str(tmp_path / "out" / f"scan{scan}" / "3d_model.ply"), sub, np.zeros_like(sub, np.uint8))
        dynamic_fusion.save_ply(str(dtu / "Points" / "stl" / f"stl{scan:03d}_total.ply"), stl, np.zeros_like(stl, np.uint8))
        np.savez(str(dtu / "ObsMask" / f"ObsMask{scan}_10.npz"), ObsMask=mask, BB=bb, Res=res)
        np.savez(str(dtu / "ObsMask" / f"Plane{scan}.npz"), P=plane.reshape(4, 1))
    out = tmp_path / "res" / "results.json"
    assert dtu_eval.main(["--plydir", str(tmp_path / "out"), "--datapath", str(dtu), "--scans", "9", "118", "--seed", "5",
                          "--device", DEV, "--out", str(out)]) == 0
    got = json.load(open(out))
    assert list(got["scans"]) == ["9", "118"]
    for scan, sub in (("9", data), ("118", data[::2])):
        assert got["scans"][scan] == dtu_eval.evaluate_cloud(_gpu(sub), _gpu(stl), mask, bb, res, plane, seed=5)
    means = [got["scans"][s]["acc_mean"] for s in ("9", "118")], [got["scans"][s]["comp_mean"] for s in ("9", "118")]
    assert got["summary"]["acc_mean"] == np.mean(means[0]) and got["summary"]["comp_mean"] == np.mean(means[1])
    assert got["summary"]["overall"] == (got["summary"]["acc_mean"] + got["summary"]["comp_mean"]) / 2
    assert got["summary"]["n_scans"] == 2
