"""DTU evaluation without a GPU: the numpy restatement (tests/_dtu_eval_ref.py) on analytic scenes and on
MATLAB's median / variance / rounding rules, the PLY and .mat / .npz readers, the C-ABI's argument
validation of every tmvs_dtu_* entry point, the refusal of CPU tensors, and the driver's arguments."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import _dtu_eval_ref as ref
from transmvsnet_amd import _lib, build, dtu_eval, dynamic_fusion, fusion, ops


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _lattice(nx, ny, step=0.5, origin=(10.0, 10.0, 10.0)):
    """A lattice in the plane z = origin z; step and origin are exact in float32."""
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    p = np.stack([x.ravel() * step, y.ravel() * step, np.zeros(x.size)], 1) + np.asarray(origin)
    return p.astype(np.float32)


def _scene(shift):
    stl = _lattice(12, 9)
    data = stl + np.float32([0, 0, shift])
    mask = np.ones((30, 30, 30), np.uint8)
    bb = np.array([[0.0, 0.0, 0.0], [29.0, 29.0, 29.0]])
    plane = np.array([0.0, 0.0, 1.0, -5.0])  # z > 5
    return data, stl, mask, bb, 1.0, plane


# ----------------------------------------------------------------- the restatement
def test_ref_coincident_lattices_give_zero():
    data, stl, mask, bb, res, plane = _scene(0.0)
    r = ref.evaluate_cloud(data, stl, mask, bb, res, plane, np.random.default_rng(0).permutation(len(data)))
    assert r["n_thinned"] == r["n_input"] == r["n_data"] == r["n_stl"] == len(stl)  # 0.5 apart: nothing thinned
    for k in ("acc_mean", "acc_median", "acc_var", "comp_mean", "comp_median", "comp_var", "overall"):
        assert r[k] == 0.0, k


def test_ref_shift_along_normal_is_the_distance():
    data, stl, mask, bb, res, plane = _scene(0.25)
    r = ref.evaluate_cloud(data, stl, mask, bb, res, plane, np.arange(len(data)))
    for k in ("acc_mean", "acc_median", "comp_mean", "comp_median", "overall"):
        assert r[k] == 0.25, k
    assert r["acc_var"] == 0.0 and r["comp_var"] == 0.0


def test_ref_thinning_is_greedy_and_inclusive():
    # a line at spacing 0.25 with radius 0.25 (d2 == r2 exactly): in index order every other point goes
    line = np.zeros((7, 3), np.float32)
    line[:, 0] = 300.0 + 0.25 * np.arange(7)
    assert ref.thin_points(line, 0.25, np.arange(7)).tolist() == [True, False, True, False, True, False, True]
    # the order matters: starting from the middle
    assert ref.thin_points(line, 0.25, [3, 0, 1, 2, 4, 5, 6]).tolist() == [True, False, False, True, False, True, False]
    # duplicates: one copy survives
    dup = np.repeat(line[:2] * np.float32([1, 0, 0]) * 4, 3, axis=0)
    assert ref.thin_points(dup, 0.2, np.arange(6)).sum() == 2


def test_ref_nearest_caps_and_block_range():
    bb = np.array([[0.0, 0.0, 0.0], [100.0, 50.0, 59.0]])
    lo, hi = ref.block_range(bb, 60.0)
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [120.0, 60.0, 60.0]
    to = np.float32([[10, 10, 10]])
    frm = np.float32([[10, 10, 29.9], [10, 10, 30.1], [119.5, 10, 10], [120.0, 10, 10], [-0.5, 10, 10], [0, 10, 10],
                      [10, 10, 10]])
    d = ref.nearest_distance(frm, to, bb)
    assert d[0] == np.sqrt(np.float64(np.float32(29.9) - np.float32(10)) ** 2) and d[0] < 20
    assert d[1] == 20 and d[2] == 20 and d[3] == 20 and d[4] == 20
    assert d[5] == 10 and d[6] == 0
    # a to-point outside BB, in the neighbouring block, is found
    assert ref.nearest_distance(np.float32([[1, 1, 1]]), np.float32([[-2, 1, 1]]), bb)[0] == 3


def test_matlab_median_and_variance_rules():
    assert ref.matlab_median([3.0, 1.0, 2.0]) == 2.0
    assert ref.matlab_median([4.0, 1.0, 2.0, 8.0]) == 3.0  # mean of the two middle values
    assert np.isnan(ref.matlab_median([]))
    m, med, var, n = ref.stats([1.0, 2.0, 3.0, 6.0])
    assert (m, med, n) == (3.0, 2.5, 4)
    assert var == pytest.approx(14.0 / 3.0, rel=1e-15)  # normalised by n - 1
    assert ref.stats([5.0]) == (5.0, 5.0, 0.0, 1)
    # the product's statistics follow the same rules (its GPU path is tested in test_gpu_dtu_eval.py)
    for v in ([3.0, 1.0, 2.0], [4.0, 1.0, 2.0, 8.0], [5.0], [0.0, 0.5]):
        got = dtu_eval._stats(torch.tensor(v, dtype=torch.float64))
        want = ref.stats(v)
        assert got[1] == want[1] and got[3] == want[3]
        assert got[0] == pytest.approx(want[0], rel=1e-15) and got[2] == pytest.approx(want[2], rel=1e-14)


def test_mask_index_rounds_half_away_from_zero():
    assert ref.matlab_round([0.5, 1.5, 2.5, -0.5, -1.5, 2.4999]).tolist() == [1, 2, 3, -1, -2, 2]
    mask = np.zeros((7, 5, 3), np.uint8)
    mask[1, 0, 0] = 1  # MATLAB ObsMask(2, 1, 1)
    bb = np.array([[0.0, 0.0, 0.0], [6.0, 4.0, 2.0]])
    # (x - 0) / 1 + 1 = 1.5 rounds to 2 (half to even would also give 2); 2.5 rounds to 3, not 2
    pts = np.float32([[0.5, 0, 0], [1.5, 0, 0], [0.49, 0, 0], [1.0, 0.5, 0], [1.0, 0, -0.5], [1.0, 0, -0.51]])
    assert ref.in_obs_mask(pts, mask, bb, 1.0).tolist() == [True, False, False, False, True, False]
    # axis order on a non-cubic mask, and the bounds 0, 1, size, size + 1
    full = np.ones((7, 5, 3), np.uint8)
    edge = np.float32([[-1, 0, 0], [0, 0, 0], [6, 4, 2], [7, 4, 2], [6, 5, 2], [6, 4, 3]])
    assert ref.in_obs_mask(edge, full, bb, 1.0).tolist() == [False, True, True, False, False, False]
    assert ref.above_plane(np.float32([[0, 0, 5], [0, 0, 5.5], [0, 0, 4]]), [0, 0, 1, -5]).tolist() == [False, True, False]


# ----------------------------------------------------------------- readers
def test_read_ply_project_writers(tmp_path):
    g = np.random.default_rng(1)
    xyz = (g.standard_normal((37, 3)) * 100).astype(np.float32)
    p1, p2 = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    fusion.save_point_cloud(p1, xyz, g.random((37, 3)).astype(np.float32))
    dynamic_fusion.save_ply(p2, xyz, g.integers(0, 255, (37, 3)).astype(np.uint8))
    for p in (p1, p2):
        got = dtu_eval.read_ply_xyz(p)
        assert got.dtype == np.float32 and np.array_equal(got, xyz)


def test_read_ply_ascii_and_double_with_faces(tmp_path):
    xyz = np.float32([[1.5, -2.25, 3.0], [0.1, 0.2, 0.3], [1e3, 2e3, -3e3]])
    a = tmp_path / "ascii.ply"
    a.write_text("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 3\nproperty float x\nproperty float y\n"
                 "property float z\nproperty uchar red\nelement face 1\nproperty list uchar int vertex_indices\n"
                 "end_header\n" + "".join(f"{float(x)!r} {float(y)!r} {float(z)!r} 7\n" for x, y, z in xyz) + "3 0 1 2\n")
    assert np.array_equal(dtu_eval.read_ply_xyz(str(a)), xyz)
    # the stl*_total.ply layout with doubles, an int property between the coordinates and a trailing face element
    rec = np.zeros(3, dtype=[("x", "<f8"), ("n", "<i4"), ("y", "<f8"), ("z", "<f8"), ("c", "u1")])
    rec["x"], rec["y"], rec["z"], rec["n"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], [5, 6, 7]
    b = tmp_path / "double.ply"
    with open(b, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty double x\nproperty int n\n"
                b"property double y\nproperty double z\nproperty uchar c\nelement face 1\n"
                b"property list uchar int vertex_indices\nend_header\n")
        f.write(rec.tobytes())
        f.write(bytes([3]) + np.int32([0, 1, 2]).tobytes())
    assert np.array_equal(dtu_eval.read_ply_xyz(str(b)), xyz)
    bad = tmp_path / "bad.ply"
    bad.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\n"
                    b"property float z\nend_header\n" + b"\0" * 20)
    with pytest.raises(ValueError, match="truncated"):
        dtu_eval.read_ply_xyz(str(bad))


def test_mat_and_npz_loaders(tmp_path):
    from scipy.io import savemat
    g = np.random.default_rng(2)
    mask = g.random((7, 5, 3)) > 0.5
    bb = np.array([[-1.5, 2.0, 3.0], [10.0, 20.0, 30.0]])
    plane = np.array([[0.1], [0.2], [0.9], [-3.0]])
    savemat(str(tmp_path / "ObsMask1_10.mat"), {"ObsMask": mask, "BB": bb, "Res": 0.8})
    savemat(str(tmp_path / "Plane1.mat"), {"P": plane})
    np.savez(str(tmp_path / "ObsMask1_10.npz"), ObsMask=mask, BB=bb, Res=0.8)
    np.savez(str(tmp_path / "Plane1.npz"), P=plane)
    for ext in (".mat", ".npz"):
        m, b, r = dtu_eval.load_obs_mask(str(tmp_path / ("ObsMask1_10" + ext)))
        assert m.dtype == np.uint8 and m.shape == (7, 5, 3) and m.flags["C_CONTIGUOUS"]  # [X, Y, Z] as MATLAB indexes
        assert np.array_equal(m != 0, mask) and np.array_equal(b, bb) and b.dtype == np.float64 and r == 0.8
        p = dtu_eval.load_plane(str(tmp_path / ("Plane1" + ext)))
        assert p.shape == (4,) and p.dtype == np.float64 and np.array_equal(p, plane.ravel())


# ----------------------------------------------------------------- the C-ABI without a GPU
def test_dtu_entry_points_validate_arguments(lib):
    """Bad arguments are rejected before any launch: the pointers are never read on the device."""
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data  # 16-byte aligned host memory, stands in for device pointers
    assert p % 16 == 0
    grid = np.array([0.0, 0.0, 0.0, 0.21])
    g = grid.ctypes.data
    bb = np.array([0.0, 0.0, 0.0, 100.0, 100.0, 100.0]).ctypes.data
    bad_grid = np.array([0.0, 0.0, 0.0, 0.0]).ctypes.data

    def each_bad(fn, good, bad):
        for i, values in bad.items():
            for v in values:
                args = list(good)
                args[i] = v
                assert fn(*args) == -1, (fn.__name__, i, v)

    each_bad(lib.tmvs_dtu_cell_keys, [p, 4, g, p, None], {0: [None], 1: [0, -2], 2: [None, bad_grid], 3: [None]})
    each_bad(lib.tmvs_dtu_gather_points, [p, p, p, 4, p, None], {0: [None], 1: [None], 3: [0, -1], 4: [None, p + 4]})
    assert lib.tmvs_dtu_grid_table_bytes(0) == 0 and lib.tmvs_dtu_grid_table_bytes(-5) == 0
    assert lib.tmvs_dtu_grid_table_bytes(3) >= 3 * 8 + 4 * 4
    need = lib.tmvs_dtu_grid_table_bytes(4)
    each_bad(lib.tmvs_dtu_grid_table, [p, p, 4, 4, p, need, None],
             {0: [None], 1: [None], 2: [0, -1], 3: [0, -1, 5], 4: [None], 5: [need - 1, 0]})  # 5: a short workspace
    each_bad(lib.tmvs_dtu_thin_round, [p, 4, p + 64, 4, g, 0.2, p + 128, p + 192, p + 256, None],
             {0: [None, p + 8], 1: [0, -1], 2: [None], 3: [0, 5], 4: [None, bad_grid], 5: [0.0, -1.0, 0.21, 0.3],
              6: [None], 7: [None, p + 128], 8: [None]})
    each_bad(lib.tmvs_dtu_nearest_pass, [p, 4, p, 4, p, 4, g, bb, 20.0, 60.0, 1, -1.0, p, None],
             {0: [None], 1: [0, -1], 2: [None], 3: [0, -1], 4: [None], 5: [0, 5], 6: [None, bad_grid], 7: [None],
              8: [0.0, -1.0, 60.5], 9: [0.0, 19.0], 10: [-1], 12: [None]})  # 8 / 9: max_dist > block
    each_bad(lib.tmvs_dtu_in_mask, [p, 4, p, 7, 5, 3, g, 1.0, p, None],
             {0: [None], 1: [0, -1], 2: [None], 3: [0], 4: [-1], 5: [0], 6: [None], 7: [0.0, -1.0], 8: [None]})
    each_bad(lib.tmvs_dtu_above_plane, [p, 4, g, p, None], {0: [None], 1: [0, -1], 2: [None], 3: [None]})
    # more points than an int32 position can index
    assert lib.tmvs_dtu_cell_keys(p, 2 ** 31, g, p, None) == -2


def test_dtu_refuses_cpu_tensors():
    xyz = torch.zeros(5, 3)
    mask, bb, plane = np.ones((2, 2, 2), np.uint8), np.array([[0.0] * 3, [1.0] * 3]), [0, 0, 1, 0]
    for call in (lambda: dtu_eval.thin_points(xyz), lambda: dtu_eval.nearest_distance(xyz, xyz, bb),
                 lambda: dtu_eval.in_obs_mask(xyz, mask, bb, 1.0), lambda: dtu_eval.above_plane(xyz, plane),
                 lambda: dtu_eval.evaluate_cloud(xyz, xyz, mask, bb, 1.0, plane),
                 lambda: ops.dtu_cell_keys(xyz, [0, 0, 0, 1]), lambda: ops.dtu_above_plane(xyz, plane),
                 lambda: ops.dtu_in_mask(xyz, torch.ones(2, 2, 2, dtype=torch.uint8), [0, 0, 0], 1.0),
                 lambda: ops.dtu_gather_points(xyz, torch.arange(5)),
                 lambda: ops.dtu_grid_table(torch.arange(5), torch.arange(5), 5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_product_path_does_not_import_the_oracle():
    src = open(dtu_eval.__file__).read()
    assert "oracle" not in src and "_dtu_eval_ref" not in src


# ----------------------------------------------------------------- the driver
def test_driver_arguments_and_patterns(tmp_path):
    a = dtu_eval.parse_args(["--plydir", "O", "--datapath", "D", "--out", "r.json"])
    assert a.scans == [1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118]
    assert len(a.scans) == 22 and a.pattern == "{scan}/3d_model.ply" and a.dst == 0.2 and a.max_dist == 20.0
    a = dtu_eval.parse_args(["--plydir", "O", "--datapath", "D", "--out", "r.json", "--scans", "9", "118", "--pattern",
                             "mvsnet{id:03d}_l3.ply", "--seed", "3"])
    assert a.scans == [9, 118] and a.seed == 3
    with pytest.raises(SystemExit):
        dtu_eval.parse_args(["--plydir", "O"])
    obs = tmp_path / "ObsMask"
    obs.mkdir()
    np.savez(str(obs / "ObsMask9_10.npz"), ObsMask=np.ones((2, 2, 2)), BB=np.zeros((2, 3)), Res=1.0)
    np.savez(str(obs / "Plane9.npz"), P=np.zeros(4))
    f = dtu_eval.scan_files("O", str(tmp_path), 9)
    assert f["ply"] == os.path.join("O", "scan9", "3d_model.ply")
    assert f["stl"] == os.path.join(str(tmp_path), "Points", "stl", "stl009_total.ply")
    assert f["mask"].endswith("ObsMask9_10.npz") and f["plane"].endswith("Plane9.npz")
    assert dtu_eval.scan_files("O", str(tmp_path), 9, a.pattern)["ply"] == os.path.join("O", "mvsnet009_l3.ply")
    with pytest.raises(FileNotFoundError):
        dtu_eval.scan_files("O", str(tmp_path), 10)
    s = dtu_eval.summarize([{"acc_mean": 0.3, "comp_mean": 0.5}, {"acc_mean": 0.5, "comp_mean": 0.1}])
    assert s["acc_mean"] == pytest.approx(0.4) and s["comp_mean"] == pytest.approx(0.3)
    assert s["overall"] == pytest.approx(0.35) and s["n_scans"] == 2
