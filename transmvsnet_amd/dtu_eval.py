"""DTU accuracy / completeness of fused point clouds on the GPU: what the reference's DTU-MATLAB
folder computes (BaseEvalMain_web.m, PointCompareMain.m, reducePts_haa.m, MaxDistCP.m,
ComputeStat_web.m), over the uniform-grid kernels of csrc/dtu_eval.hip.

    python -m transmvsnet_amd.dtu_eval --plydir OUT --datapath DTU --out results.json

For one scan: thin the fused cloud to one point per `dst` = 0.2 mm ball in a seeded random visiting
order, take the nearest distances cloud -> ground truth and ground truth -> cloud, keep the cloud points
inside the observability mask and the ground-truth points above the table plane, drop distances of
`max_dist` = 20 mm and more, and report mean / median / variance of what is left: accuracy and
completeness; overall is the mean of the two means. DESIGN.md "DTU evaluation" has the details, the
one deviation from MaxDistCP.m (distances of max_dist and more are reported as max_dist, which no
statistic sees) and the measured times. Everything runs on the GPU: there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from . import _lib, ops

# BaseEvalMain_web.m:22, ComputeStat_web.m:24
DTU_EVAL_SCANS = (1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118)
RECONSTRUCT_PATTERN = "{scan}/3d_model.ply"      # transmvsnet_amd.reconstruct
REFERENCE_PATTERN = "mvsnet{id:03d}_l3.ply"      # BaseEvalMain_web.m:32
THIN_CELL_FACTOR = 1.0001  # thinning cell edge / radius: strictly above 1, far above the index rounding

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


# ----------------------------------------------------------------- files
def read_ply_xyz(path):
    """The x, y, z of a PLY's vertex element as float32 [N, 3]: ASCII or binary little-endian, any mix
    of scalar vertex properties, elements after `vertex` ignored."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, n, props, in_vertex, seen_vertex = None, 0, [], False, False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: header has no end_header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                if tok[1] != "vertex" and not seen_vertex:
                    raise ValueError(f"{path}: element {tok[1]} before vertex is not supported")
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    seen_vertex, n = True, int(tok[2])
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list" or tok[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: vertex property type {tok[1]} is not supported")
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        names = [p[0] for p in props]
        if not seen_vertex or any(a not in names for a in "xyz"):
            raise ValueError(f"{path}: no vertex element with x, y, z")
        if fmt == "ascii":
            cols = [names.index(a) for a in "xyz"]
            rows = [f.readline().split() for _ in range(n)]
            if any(len(r) < len(names) for r in rows):
                raise ValueError(f"{path}: truncated vertex data")
            return np.array([[float(r[c]) for c in cols] for r in rows], np.float64).astype(np.float32).reshape(n, 3)
        if fmt != "binary_little_endian":
            raise ValueError(f"{path}: format {fmt} is not supported")
        dt = np.dtype([(name, "<" + t) for name, t in props])
        buf = f.read(n * dt.itemsize)
        if len(buf) != n * dt.itemsize:
            raise ValueError(f"{path}: truncated vertex data")
        rec = np.frombuffer(buf, dtype=dt, count=n)
        return np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float32).reshape(n, 3)


def _load_vars(path):
    if str(path).endswith(".npz"):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    from scipy.io import loadmat  # lazy: only .mat files need scipy
    return loadmat(path)


def load_obs_mask(path):
    """ObsMask%d_10.mat (or an .npz with the same keys) -> (mask uint8 [X, Y, Z], bb float64 [2, 3], res)."""
    v = _load_vars(path)
    mask = np.ascontiguousarray(np.asarray(v["ObsMask"]) != 0, dtype=np.uint8)
    if mask.ndim != 3:
        raise ValueError(f"{path}: ObsMask must be three-dimensional")
    bb = np.asarray(v["BB"], np.float64).reshape(2, 3)
    return mask, bb, float(np.asarray(v["Res"], np.float64).reshape(-1)[0])


def load_plane(path):
    """Plane%d.mat (or .npz) -> P float64 [4]."""
    return np.asarray(_load_vars(path)["P"], np.float64).reshape(4).copy()


# ----------------------------------------------------------------- grid index
def _gpu_xyz(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] == 0:
        raise ValueError(f"{name} must be [N, 3] with N >= 1")
    t = t.to(torch.float32).contiguous()
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} holds non-finite coordinates")
    return t


def _sorted_grid(xyz, grid, payload=None, table=True):
    """Sort xyz by cell key under grid: (float4 records in cell order, table, n_cells, sorting order)."""
    keys = ops.dtu_cell_keys(xyz, grid)
    keys, order = torch.sort(keys)
    pts = ops.dtu_gather_points(xyz, order, payload)
    if not table:
        return pts, None, 0, order
    head = torch.ones_like(keys)
    head[1:] = keys[1:] != keys[:-1]
    rank = torch.cumsum(head, 0)
    n_cells = int(rank[-1])
    return pts, ops.dtu_grid_table(keys, rank, n_cells), n_cells, order


# ----------------------------------------------------------------- the five steps
@torch.no_grad()
def thin_points(xyz, radius=0.2, perm=None, seed=0, return_rounds=False):
    """reducePts_haa.m: bool [N] keep mask (device) of the points that survive when the points are visited
    in the order `perm` (int64 [N], perm[k] = the point visited k-th; default torch.randperm under `seed`)
    and every visited point still kept removes all others within `radius` (inclusive)."""
    xyz = _gpu_xyz(xyz, "xyz")
    n = xyz.shape[0]
    if not radius > 0:
        raise ValueError("radius must be positive")
    if perm is None:
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))
    perm = torch.as_tensor(perm).to(device=xyz.device, dtype=torch.int64).reshape(-1)
    if perm.numel() != n or not torch.equal(torch.sort(perm)[0], torch.arange(n, device=xyz.device)):
        raise ValueError("perm must be a permutation of range(N)")
    rank = torch.empty(n, dtype=torch.int32, device=xyz.device)
    rank[perm] = torch.arange(n, dtype=torch.int32, device=xyz.device)
    grid = [*xyz.amin(0).double().tolist(), float(radius) * THIN_CELL_FACTOR]
    pts, table, n_cells, order = _sorted_grid(xyz, grid, rank)
    state = torch.full((n,), _lib.DTU_UNDECIDED, dtype=torch.uint8, device=xyz.device)
    nxt = torch.empty_like(state)
    count = torch.zeros(1, dtype=torch.int32, device=xyz.device)
    left, rounds = n, 0
    while left:
        count.zero_()
        ops.dtu_thin_round(pts, table, n_cells, grid, radius, state, nxt, count)
        state, nxt = nxt, state
        rounds += 1
        now = int(count)
        if now >= left:  # every round decides at least the undecided point of smallest rank
            raise RuntimeError(f"thin_points: round {rounds} decided nothing ({now} of {n} points undecided)")
        left = now
    keep = torch.zeros(n, dtype=torch.bool, device=xyz.device)
    keep[order] = state == _lib.DTU_KEPT
    return (keep, rounds) if return_rounds else keep


@torch.no_grad()
def nearest_distance(q_from, q_to, bb, max_dist=20.0, block=60.0, cell=1.0, coarse_cell=None, return_d2=False):
    """MaxDistCP.m with distances capped at max_dist <= block: float64 [N_from], for every from-point inside
    the block range of `bb` the exact distance to the nearest to-point where that is < max_dist, else
    max_dist; from-points outside the range get max_dist. `cell` / `coarse_cell` are the edges of the two
    search grids (performance only). return_d2 also returns the squared distances the kernel produced."""
    q_from, q_to = _gpu_xyz(q_from, "q_from"), _gpu_xyz(q_to, "q_to")
    if q_to.device != q_from.device:
        raise ValueError("q_from and q_to must be on the same device")
    bb = np.asarray(bb, np.float64).reshape(2, 3)
    max_dist, block, cell = float(max_dist), float(block), float(cell)
    if not 0 < max_dist <= block:
        raise ValueError("nearest_distance needs 0 < max_dist <= block")
    if coarse_cell is None:
        coarse_cell = max(max_dist / 4.0, 2.0 * cell)
    if not cell > 0 or not coarse_cell >= max_dist / 16.0:
        raise ValueError("nearest_distance needs cell > 0 and coarse_cell >= max_dist / 16")
    md2 = max_dist * max_dist
    d2 = torch.full((q_from.shape[0],), md2, dtype=torch.float64, device=q_from.device)
    fine = [*bb[0].tolist(), cell]
    src = _sorted_grid(q_from, fine, table=False)[0]
    # the fine grid's 3x3x3 cells settle every from-point whose nearest to-point is within one cell edge
    to4, table, n_cells, _ = _sorted_grid(q_to, fine)
    ops.dtu_nearest_pass(src, to4, table, n_cells, fine, bb, max_dist, block, 1, -1.0, d2)
    settled = (cell * (1.0 - 1e-5)) ** 2
    if settled < md2:  # the rest walk the coarse grid's rings out to max_dist
        coarse = [*bb[0].tolist(), float(coarse_cell)]
        to4, table, n_cells, _ = _sorted_grid(q_to, coarse)
        ops.dtu_nearest_pass(src, to4, table, n_cells, coarse, bb, max_dist, block,
                             int(math.ceil(max_dist / coarse_cell)) + 2, settled, d2)
    dist = torch.where(d2 < md2, torch.sqrt(d2), torch.full_like(d2, max_dist))
    return (dist, d2) if return_d2 else dist


@torch.no_grad()
def in_obs_mask(xyz, mask, bb, res):
    """PointCompareMain.m:37-45: bool [N], the point's voxel round((Q - BB1) / Res + 1) is inside ObsMask and set."""
    xyz = _gpu_xyz(xyz, "xyz")
    mask = torch.as_tensor(mask)
    mask = (mask != 0).to(device=xyz.device, dtype=torch.uint8).contiguous()
    return ops.dtu_in_mask(xyz, mask, np.asarray(bb, np.float64).reshape(2, 3)[0], res).bool()


@torch.no_grad()
def above_plane(xyz, plane):
    """PointCompareMain.m:57: bool [N], P' * [Q; 1] > 0."""
    return ops.dtu_above_plane(_gpu_xyz(xyz, "xyz"), plane).bool()


def _stats(d):
    """ComputeStat_web.m:44-54 on a float64 device vector: (mean, median, var, n) with MATLAB's rules --
    the median of an even count is the mean of the two middle values (a + (b - a) / 2, or (a + b) / 2 when
    the signs differ, as median.m forms it), var is unbiased and 0 for one value, all NaN for none."""
    n = d.numel()
    if n == 0:
        return float("nan"), float("nan"), float("nan"), 0
    s = torch.sort(d)[0]
    if n % 2:
        med = float(s[n // 2])
    else:
        a, b = float(s[n // 2 - 1]), float(s[n // 2])
        med = (a + b) / 2 if np.sign(a) != np.sign(b) or math.isinf(a) or math.isinf(b) else a + (b - a) / 2
    return float(d.mean()), med, (float(d.var(unbiased=True)) if n > 1 else 0.0), n


@torch.no_grad()
def evaluate_cloud(data_xyz, stl_xyz, mask, bb, res, plane, dst=0.2, max_dist=20.0, seed=0, timings=None):
    """PointCompareMain.m + ComputeStat_web.m for one scan; all inputs' point clouds on the GPU.
    `timings`, when a dict, receives the milliseconds of each step and the thinning's round count."""
    data_xyz, stl_xyz = _gpu_xyz(data_xyz, "data_xyz"), _gpu_xyz(stl_xyz, "stl_xyz")

    def timed(name, fn):
        if timings is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        timings[name + "_ms"] = e0.elapsed_time(e1)
        return r

    keep, rounds = timed("thin", lambda: thin_points(data_xyz, dst, seed=seed, return_rounds=True))
    thin = data_xyz[keep]
    d_data = timed("nearest_data_to_stl", lambda: nearest_distance(thin, stl_xyz, bb, max_dist, 60.0))
    d_stl = timed("nearest_stl_to_data", lambda: nearest_distance(stl_xyz, thin, bb, max_dist, 60.0))
    in_mask, above = timed("mask_plane", lambda: (in_obs_mask(thin, mask, bb, res), above_plane(stl_xyz, plane)))

    def stats():
        a, s = d_data[in_mask], d_stl[above]
        return _stats(a[a < max_dist]), _stats(s[s < max_dist])
    acc, comp = timed("stats", stats)
    if timings is not None:
        timings["thin_rounds"] = rounds
    return {"acc_mean": acc[0], "acc_median": acc[1], "acc_var": acc[2], "n_data": acc[3],
            "comp_mean": comp[0], "comp_median": comp[1], "comp_var": comp[2], "n_stl": comp[3],
            "overall": (acc[0] + comp[0]) / 2, "n_input": int(data_xyz.shape[0]), "n_thinned": int(thin.shape[0])}


# ----------------------------------------------------------------- scans and the command line
def _first_existing(*paths):
    for p in paths:
        if os.path.exists(p):
            return p
    raise FileNotFoundError(" / ".join(paths))


def scan_files(plydir, datapath, scan, pattern=RECONSTRUCT_PATTERN):
    """The four files of one scan (PointCompareMain.m:11,19,57; BaseEvalMain_web.m:32)."""
    obs = os.path.join(datapath, "ObsMask")
    return {"ply": os.path.join(plydir, pattern.format(scan=f"scan{scan}", id=scan)),
            "stl": os.path.join(datapath, "Points", "stl", f"stl{scan:03d}_total.ply"),
            "mask": _first_existing(os.path.join(obs, f"ObsMask{scan}_10.mat"), os.path.join(obs, f"ObsMask{scan}_10.npz")),
            "plane": _first_existing(os.path.join(obs, f"Plane{scan}.mat"), os.path.join(obs, f"Plane{scan}.npz"))}


def evaluate_scans(plydir, datapath, scans=DTU_EVAL_SCANS, pattern=RECONSTRUCT_PATTERN, dst=0.2, max_dist=20.0, seed=0,
                   device="cuda", log=None):
    """Every scan's evaluate_cloud and the summary ComputeStat_web.m prints: the means of the per-scan means."""
    per = {}
    for scan in scans:
        f = scan_files(plydir, datapath, scan, pattern)
        mask, bb, res = load_obs_mask(f["mask"])
        r = evaluate_cloud(torch.from_numpy(read_ply_xyz(f["ply"])).to(device),
                           torch.from_numpy(read_ply_xyz(f["stl"])).to(device), mask, bb, res, load_plane(f["plane"]),
                           dst, max_dist, seed)
        per[str(scan)] = r
        if log:
            log(f"scan{scan}: acc {r['acc_mean']:.4f} comp {r['comp_mean']:.4f} overall {r['overall']:.4f}")
    return {"scans": per, "summary": summarize(per.values())}


def summarize(results):
    results = list(results)
    acc = float(np.mean([r["acc_mean"] for r in results])) if results else float("nan")
    comp = float(np.mean([r["comp_mean"] for r in results])) if results else float("nan")
    return {"acc_mean": acc, "comp_mean": comp, "overall": (acc + comp) / 2, "n_scans": len(results)}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m transmvsnet_amd.dtu_eval", description=__doc__.split("\n\n")[0])
    ap.add_argument("--plydir", required=True, help="folder of the fused clouds")
    ap.add_argument("--datapath", required=True, help="DTU evaluation data: Points/stl and ObsMask")
    ap.add_argument("--scans", type=int, nargs="+", default=list(DTU_EVAL_SCANS))
    ap.add_argument("--pattern", default=RECONSTRUCT_PATTERN,
                    help=f"cloud file under --plydir; {{scan}} = scanN, {{id}} = N (e.g. {REFERENCE_PATTERN})")
    ap.add_argument("--dst", type=float, default=0.2)
    ap.add_argument("--max-dist", type=float, default=20.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", required=True, help="results JSON")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    res = evaluate_scans(a.plydir, a.datapath, a.scans, a.pattern, a.dst, a.max_dist, a.seed, a.device,
                         log=lambda m: print(m, flush=True))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    s = res["summary"]
    print(f"mean acc {s['acc_mean']:.4f} mean comp {s['comp_mean']:.4f} overall {s['overall']:.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
