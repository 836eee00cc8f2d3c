"""Lattice scene for the depth-fusion tests: a scene on which float32 arithmetic is EXACT, so the
HIP kernel must equal the float64 oracle in every decision and, after the one final division, in
every bit.

Cameras: R = I, K = [[256, 0, 32], [0, 256, 8], [0, 0, 1]], centres at multiples of 1/2 with z = 0,
every depth 512 or 1024. Then RK_inv = [[1/256, 0, -1/8], [0, 1/256, -1/32], [0, 0, 1]], a pixel
(x, y) of view i at depth 512 is the world point (2 (x - 32) + cx_i, 2 (y - 8) + cy_i, 512), and it
projects into view j at (x + (cx_i - cx_j) / 2, y + (cy_i - cy_j) / 2): a disparity of half the
centre difference, so integer, half- and quarter-pixel disparities (filter weights 0, 128, 64 and
192 of 256) come from even, odd and half-odd centre differences. Everything is a small dyadic.

Colours (B, G, R): channel 0 is the view index / 16 (the fused value times n is the sum of the
contributing views' indices, which names the set of views summed); channels 1 and 2 are
(2 X mod 16) / 16 and (2 Y mod 8) / 8 of the pixel's world point on the 512 plane.
"""
import numpy as np

from oracle import fusion_ref
from transmvsnet_amd import fusion

K = np.array([[256.0, 0, 32.0], [0, 256.0, 8.0], [0, 0, 1.0]])
H, W = 21, 70  # ragged against the kernel's 64 x 4 block in both axes

# Views 1-6 have an even y offset from view 0 (integer disparity in y), so on row 8 of reference 0,
# where Y = 0, the fused Y stays exactly 0 for any of them; 7 and 8 are the half- and quarter-pixel
# views in y. (3, 4) from view 0 and (1.5, 2) give baselines 5 and 2.5, exact under sqrtf.
CENTRES = [(0, 0), (2, 0), (1, 0), (0.5, 0), (-2, 2), (-4, 0), (3, 4), (0, 1), (0, -0.5), (1.5, 2), (2, -2)]
PAIR = [(0, 0), (1, 0)]  # one unit apart: f b / 512 - f b / 1024 = 0.25 exactly

# The largest float32 the reference's `depth <= 425.001` (a double literal) still rejects, and the
# smallest it lets through: float32(425.001) rounds UP, so that value itself is a live depth.
FLOOR_DEAD = np.nextafter(np.float32(425.001), np.float32(0))
FLOOR_LIVE = np.float32(425.001)


def make_lattice(centres=CENTRES[:9], h=H, w=W, plane=512.0, plant=True):
    """Returns (rgbd [V,H,W,4] float32, cams_packed [V,32], cam_dicts). `plane` is one depth or one
    per view. plant=True needs >= 9 views and h >= 21, w >= 64."""
    v = len(centres)
    plane = np.broadcast_to(np.asarray(plane, np.float32), (v,))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    rgbd = np.empty((v, h, w, 4), np.float32)
    packs, dicts = [], []
    for i, (cx, cy) in enumerate(centres):
        p = K @ np.concatenate([np.eye(3), -np.array([[cx], [cy], [0.0]])], 1)
        pk, d = fusion.camera_params(p)
        packs.append(pk)
        dicts.append(d)
        rgbd[i, ..., 0] = i / 16.0
        rgbd[i, ..., 1] = np.mod(2 * (2 * (xs - 32) + cx), 16) / 16.0
        rgbd[i, ..., 2] = np.mod(2 * (2 * (ys - 8) + cy), 8) / 8.0
        rgbd[i, ..., 3] = plane[i]
    if plant:
        d = rgbd[..., 3]
        d[2, 3:7, 10:16] = 1024.0  # a patch that disagrees with the plane
        d[3, 0, :] = 1024.0  # first row and column differ from the last ones: a fetch that wrapped
        d[3, :, 0] = 1024.0  # or ran past the row blends in another depth where the clamp is hit
        for view, y in ((1, 12), (7, 15)):  # holes, in views that are sources and references
            d[view, y - 1:y + 2, 42:45] = 0.0  # zeros around FLOOR_DEAD: no blend of it is a live depth
            d[view, y, [38, 40, 43, 46, 48]] = [0.0, 425.0, FLOOR_DEAD, np.nan, np.inf]
        # one world point missing from most views, so few views agree around it
        for view in (1, 2, 4, 5, 6, 7):
            cx, cy = centres[view]
            x, y = 20 - cx / 2, 11 - cy / 2
            d[view, int(np.floor(y)):int(np.ceil(y)) + 1, int(np.floor(x)):int(np.ceil(x)) + 1] = 0.0
    return rgbd, np.stack(packs), dicts


def fusibile_f32(rgbd, dicts, ref, consistent_threshold, depth_threshold=0.25):
    """The oracle's (written, coord, tex) with the final division done in float32, as the kernel
    does it: exact sums (checked by the precondition test), then one IEEE float32 quotient."""
    with np.errstate(all="ignore"):
        wr, _, _, count, sx, st = fusion_ref.fusibile_ref(rgbd, dicts, ref, consistent_threshold, depth_threshold,
                                                          return_sums=True)
        n = (count + 1).astype(np.float32)[..., None]
        return wr, sx.astype(np.float32) / n, st.astype(np.float32) / n, count


def trace(rgbd, dicts, ref, consistent_threshold, depth_threshold=0.25):
    """Replays fusibile_ref's loop with its own building blocks and records, per source view, what
    happened to every pixel. Returns a dict of [V, H, W] bool arrays (tried, left, right, top,
    bottom, hole, mismatch, agree, clamp_x, clamp_y, nan_src), `count`, `avail` (views that would
    agree without the cap), the sums accumulated in float32 in the kernel's order (sum32_x, sum32_t), and
    the values the exactness preconditions are about."""
    v, h, w, _ = rgbd.shape
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    depth = rgbd[ref, ..., 3].astype(np.float64)
    alive = depth > fusion_ref.DEPTH_FLOOR
    f = dicts[ref]["fx"]
    names = ("tried", "left", "right", "top", "bottom", "hole", "mismatch", "agree", "clamp_x", "clamp_y", "nan_src")
    t = {k: np.zeros((v, h, w), bool) for k in names}
    count = np.zeros((h, w), np.int64)
    avail = np.zeros((h, w), np.int64)
    values, diffs = [], []
    with np.errstate(all="ignore"):
        X = fusion_ref.get_3dpoint(dicts[ref], xs, ys, depth)
        values.append(X[alive])
        s32x, s32t = X.astype(np.float32), rgbd[ref, ..., :3].copy()  # the kernel's running float32 sums
        for i in range(v):
            if i == ref:
                continue
            px, py, d = fusion_ref.project(dicts[i], X)
            fin = alive & np.isfinite(px) & np.isfinite(py)
            inside = fin & (px >= 0) & (px < w) & (py >= 0) & (py < h)
            tt = fusion_ref.tex_linear(rgbd[i], np.where(inside, px, 0.0) + 0.5, np.where(inside, py, 0.0) + 0.5)
            live = inside & (tt[..., 3] > fusion_ref.DEPTH_FLOOR)
            base = np.linalg.norm(dicts[ref]["C4"].astype(np.float64) - dicts[i]["C4"].astype(np.float64))
            dd, td = f * base / d, f * base / tt[..., 3]
            ok = live & (np.abs(dd - td) < depth_threshold)
            tx = fusion_ref.get_3dpoint(dicts[i], np.floor(px), np.floor(py), tt[..., 3])
            tried = alive & (count < 2 * consistent_threshold)
            t["tried"][i] = tried
            t["left"][i] = tried & fin & (px < 0)
            t["right"][i] = tried & fin & (px >= w)
            t["top"][i] = tried & fin & (py < 0)
            t["bottom"][i] = tried & fin & (py >= h)
            t["hole"][i] = tried & inside & ~live
            t["nan_src"][i] = tried & inside & np.isnan(tt[..., 3])
            t["mismatch"][i] = tried & live & ~ok
            t["agree"][i] = tried & ok
            t["clamp_x"][i] = tried & inside & (px > w - 1) & (px != np.floor(px))
            t["clamp_y"][i] = tried & inside & (py > h - 1) & (py != np.floor(py))
            count += tried & ok
            s32x = np.where((tried & ok)[..., None], s32x + tx.astype(np.float32), s32x)
            s32t = np.where((tried & ok)[..., None], s32t + tt[..., :3].astype(np.float32), s32t)
            avail += ok
            values += [px[fin], py[fin], d[fin], tt[inside], tx[ok]]
            diffs.append((dd[live], td[live], np.full(live.sum(), base)))
    t["count"], t["avail"], t["alive"] = count, avail, alive
    t["values"] = np.concatenate([a.reshape(-1) for a in values])
    t["sum32_x"], t["sum32_t"] = s32x, s32t
    t["dd"], t["td"], t["base"] = (np.concatenate(a) for a in zip(*diffs)) if diffs else (np.zeros(0),) * 3
    return t
