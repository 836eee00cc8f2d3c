"""CPU restatement (numpy, float64) of the reference's DTU evaluation, DTU-MATLAB/: reducePts_haa.m
(thinning), MaxDistCP.m (nearest distances in 60 mm blocks), PointCompareMain.m (the observability mask
:37-45 and the ground plane :57) and ComputeStat_web.m (:38-54, the statistics), written from what those
files do.

Arithmetic: coordinates are float32 values promoted to float64; a squared distance is
dx = a.x - b.x, d2 = (dx*dx + dy*dy) + dz*dz; thinning compares d2 <= dst*dst (rangesearch is inclusive),
the nearest search compares d2 < max_dist*max_dist and takes the square root of the minimum afterwards.

Two things are stated differently from MATLAB, neither visible in a statistic:
  - reducePts_haa.m:9 draws an unseeded randperm; here the visiting order is an argument.
  - MaxDistCP.m reports distances up to and beyond MaxDist = 60; ComputeStat_web.m:40,43 drops everything
    >= 20, so nearest_distance reports min(distance, max_dist) for max_dist <= block.
"""
import numpy as np


def dist2(a, b):
    """Squared distances of a [N,3] (or [3]) to b [M,3] -> [N,M], in the fixed order."""
    a = np.asarray(a, np.float32).astype(np.float64).reshape(-1, 3)
    b = np.asarray(b, np.float32).astype(np.float64).reshape(-1, 3)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def thin_points(xyz, dst, perm, candidates=None):
    """reducePts_haa.m:7-31: visit the points in the order perm; a visited point that is still kept
    removes every other point within dst (:25-28). candidates(i) -> indices that contain every point
    within dst of point i (a spatial pre-filter; the exact test is applied to them); None = all points."""
    xyz = np.asarray(xyz, np.float32)
    n = len(xyz)
    keep = np.ones(n, bool)  # :7
    r2 = np.float64(dst) * np.float64(dst)
    for i in np.asarray(perm).reshape(-1):  # :24
        if not keep[i]:  # :25
            continue
        cand = np.arange(n) if candidates is None else np.asarray(candidates(i), np.int64)
        near = cand[dist2(xyz[i], xyz[cand])[0] <= r2]  # rangesearch(NS, pts, dst), :21
        keep[near] = False  # :26
        keep[i] = True  # :27
    return keep


def block_range(bb, block):
    """MaxDistCP.m:5,10-14: the from-points that fall into a block lie in [BB1, BB1 + (Range + 1) * block)."""
    bb = np.asarray(bb, np.float64).reshape(2, 3)
    return bb[0], bb[0] + (np.floor((bb[1] - bb[0]) / block) + 1.0) * block


def min_d2(q_from, q_to, chunk=512):
    """Brute force: every from-point's smallest squared distance to a to-point (knnsearch, MaxDistCP.m:33)."""
    q_from = np.asarray(q_from, np.float32).reshape(-1, 3)
    out = np.empty(len(q_from), np.float64)
    for s in range(0, len(q_from), chunk):
        out[s:s + chunk] = dist2(q_from[s:s + chunk], q_to).min(axis=1)
    return out


def nearest_d2(q_from, q_to, bb, max_dist=20.0, block=60.0, raw=None):
    """The squared distance behind nearest_distance: the minimum d2 where it is < max_dist^2 and the
    from-point lies in a block, else max_dist^2. With max_dist <= block every to-point nearer than max_dist
    lies in the 3x3x3 blocks MaxDistCP.m:22-26 searches, so the minimum over all to-points serves
    (raw = min_d2(q_from, q_to), when the caller has it already)."""
    assert 0 < max_dist <= block
    q_from = np.asarray(q_from, np.float32).reshape(-1, 3)
    md2 = np.float64(max_dist) * np.float64(max_dist)
    lo, hi = block_range(bb, block)
    f64 = q_from.astype(np.float64)
    inside = ((f64 >= lo) & (f64 < hi)).all(axis=1)  # :16-17
    m = min_d2(q_from, q_to) if raw is None else np.asarray(raw, np.float64)
    return np.where(inside & (m < md2), m, md2)  # :3, and the cap


def nearest_distance(q_from, q_to, bb, max_dist=20.0, block=60.0, raw=None):
    d2 = nearest_d2(q_from, q_to, bb, max_dist, block, raw)
    md2 = np.float64(max_dist) * np.float64(max_dist)
    return np.where(d2 < md2, np.sqrt(d2), np.float64(max_dist))


def matlab_round(x):
    """MATLAB round: half away from zero."""
    x = np.asarray(x, np.float64)
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def in_obs_mask(xyz, mask, bb, res):
    """PointCompareMain.m:37-45. mask is [X, Y, Z] as MATLAB indexes it."""
    q = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    bb = np.asarray(bb, np.float64).reshape(2, 3)
    mask = np.asarray(mask) != 0
    qv = matlab_round((q - bb[0]) / np.float64(res) + 1.0)  # :38-39
    size = np.array(mask.shape, np.float64)
    inside = ((qv > 0) & (qv <= size)).all(axis=1)  # :41
    out = np.zeros(len(q), bool)
    iv = qv[inside].astype(np.int64) - 1
    out[np.flatnonzero(inside)] = mask[iv[:, 0], iv[:, 1], iv[:, 2]]  # :42-46
    return out


def above_plane(xyz, plane):
    """PointCompareMain.m:57: P' * [Qstl; 1] > 0, the four products added left to right."""
    q = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    p = np.asarray(plane, np.float64).reshape(4)
    return ((p[0] * q[:, 0] + p[1] * q[:, 1]) + p[2] * q[:, 2]) + p[3] > 0


def matlab_median(d):
    """MATLAB median of a vector: the middle value, or for an even count the mean of the two middle
    values a <= b formed as a + (b - a) / 2, and as (a + b) / 2 when their signs differ."""
    s = np.sort(np.asarray(d, np.float64).reshape(-1))
    n = len(s)
    if n == 0:
        return np.nan
    if n % 2:
        return float(s[n // 2])
    a, b = s[n // 2 - 1], s[n // 2]
    if np.sign(a) != np.sign(b) or np.isinf(a) or np.isinf(b):
        return float((a + b) / 2)
    return float(a + (b - a) / 2)


def stats(d):
    """ComputeStat_web.m:44-54: (mean, median, var, n); var is MATLAB's default, normalised by n - 1
    (0 for a single value)."""
    d = np.asarray(d, np.float64).reshape(-1)
    n = len(d)
    if n == 0:
        return np.nan, np.nan, np.nan, 0
    var = float(((d - d.mean()) ** 2).sum() / (n - 1)) if n > 1 else 0.0
    return float(d.mean()), matlab_median(d), var, n


def evaluate_cloud(data_xyz, stl_xyz, mask, bb, res, plane, perm, dst=0.2, max_dist=20.0, candidates=None):
    """PointCompareMain.m then ComputeStat_web.m:38-54 for one scan, visiting order given."""
    data_xyz = np.asarray(data_xyz, np.float32)
    keep = thin_points(data_xyz, dst, perm, candidates)  # PointCompareMain.m:7
    thin = data_xyz[keep]
    d_data = nearest_distance(thin, stl_xyz, bb, max_dist)  # :24
    d_stl = nearest_distance(stl_xyz, thin, bb, max_dist)  # :28
    a = d_data[in_obs_mask(thin, mask, bb, res)]
    s = d_stl[above_plane(stl_xyz, plane)]
    acc, comp = stats(a[a < max_dist]), stats(s[s < max_dist])  # ComputeStat_web.m:38-43
    return {"acc_mean": acc[0], "acc_median": acc[1], "acc_var": acc[2], "n_data": acc[3],
            "comp_mean": comp[0], "comp_median": comp[1], "comp_var": comp[2], "n_stl": comp[3],
            "overall": (acc[0] + comp[0]) / 2, "n_input": len(data_xyz), "n_thinned": int(keep.sum())}
