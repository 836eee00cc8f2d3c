"""View selection and depth ranges of a COLMAP model, restated in numpy float64 with dense loops: a boolean
[V, P] visibility table instead of bit sets, a Python loop over the pairs of views, a Python loop over the views
for the depth ranges and the ranking. The tests compare transmvsnet_amd.view_select / colmap_scene with it; the
package never imports it.

  score of views i < j   sum over the points both see of exp(-(theta - theta0)^2 / (2 sigma^2)), theta =
                         atan2(|a x b|, a . b) in degrees, a = C_i - X, b = C_j - X, sigma = sigma1 when theta <=
                         theta0 else sigma2 (MVSNet, Yao et al. 2018, section 4.1)
  depth of (v, p)        ((r0 x + r1 y) + r2 z) + tz, (r0, r1, r2) the third row of R_v
  depth range of v       z ascending over the view's depths > 0, n of them: 0.75 z[(n 1) // 100], 1.25 z[(n 99) // 100]
  sources of v           the other views by descending score, ties to the lower number, the first min(n_src, V - 1)
"""
import numpy as np


def visibility(obs, n_views, n_points):
    vis = np.zeros((n_views, n_points), bool)
    vis[obs[:, 0], obs[:, 1]] = True
    return vis


def angles_deg(ci, cj, xyz):
    """theta per point [N] for centres ci, cj [3] and points xyz [N, 3]."""
    a, b = ci[None] - xyz, cj[None] - xyz
    c = np.cross(a, b)
    n = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    d = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    return np.arctan2(n, d) * (180.0 / np.pi)


def terms(theta, theta0=5.0, sigma1=1.0, sigma2=10.0):
    sigma = np.where(theta <= theta0, sigma1, sigma2)
    diff = theta - theta0
    return np.exp(-(diff * diff) / ((2.0 * sigma) * sigma))


def pair_scores(obs, n_views, centres, xyz, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """(scores [V, V] float64, counts [V, V] int32), symmetric, zero diagonal."""
    vis = visibility(obs, n_views, len(xyz))
    scores, counts = np.zeros((n_views, n_views)), np.zeros((n_views, n_views), np.int32)
    for i in range(n_views):
        for j in range(i + 1, n_views):
            both = np.nonzero(vis[i] & vis[j])[0]
            counts[i, j] = counts[j, i] = both.size
            if both.size:
                t = terms(angles_deg(centres[i], centres[j], xyz[both]), theta0, sigma1, sigma2)
                scores[i, j] = scores[j, i] = float(np.sum(t))
    return scores, counts


def obs_depth(obs, R, t, xyz):
    r, x = R[obs[:, 0], 2, :], xyz[obs[:, 1]]
    return ((r[:, 0] * x[:, 0] + r[:, 1] * x[:, 1]) + r[:, 2] * x[:, 2]) + t[obs[:, 0], 2]


def depth_range(z):
    """(depth_min, depth_max) of one view's observation depths."""
    z = np.sort(z[z > 0])
    n = len(z)
    if n == 0:
        raise ValueError("no observation in front of the camera")
    return 0.75 * z[(n * 1) // 100], 1.25 * z[(n * 99) // 100]


def depth_ranges(obs, z, n_views):
    out = np.zeros((n_views, 2))
    for v in range(n_views):
        out[v] = depth_range(z[obs[:, 0] == v])
    return out[:, 0], out[:, 1]


def rank_sources(scores, n_src=10):
    v = len(scores)
    return np.array([sorted((j for j in range(v) if j != i), key=lambda j: (-scores[i, j], j))[:min(n_src, v - 1)]
                     for i in range(v)], np.int64).reshape(v, -1)


def select(model, n_src=10, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """colmap_scene.select for a dictionary with "obs", "R", "t", "centres", "xyz"."""
    v = len(model["R"])
    scores, counts = pair_scores(model["obs"], v, model["centres"], model["xyz"], theta0, sigma1, sigma2)
    dmin, dmax = depth_ranges(model["obs"], obs_depth(model["obs"], model["R"], model["t"], model["xyz"]), v)
    return {"scores": scores, "counts": counts, "depth_min": dmin, "depth_max": dmax,
            "pairs": rank_sources(scores, n_src)}
