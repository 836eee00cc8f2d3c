"""CPU restatement of the reference's dynamic geometric-consistency filter (dynamic_fusion.py:
reproject_with_depth 78-115, check_geometric_consistency 117-140, filter_depth 142-280), written to
keep numpy's dtypes where the reference has them: float32 matrices, float64 per-pixel products
(int64 pixel grid x float32), float32 casts of the sampling coordinates, the reprojected depth /
pixel and the relative depth difference, a float32 depth sum divided in float64.

cv2 is absent, so ``remap_linear`` restates cv2.remap(INTER_LINEAR, constant border 0) for float
maps: subpixel_bits=5 is OpenCV's fixed-point path (coordinates rounded half-to-even to 1/32 pixel,
float32 weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy, taps summed left to right); subpixel_bits=0
uses the exact fractions from floor. That restatement is not pinned against cv2 itself.

Every function also reports which pixels sit too close to a threshold to assert on (``ambiguous``).
"""
import numpy as np

LEVELS = tuple(range(2, 11))  # dynamic_fusion.py:134
DIST_EPS = 1e-6
REL_EPS = 1e-7


def remap_linear(img, x, y, subpixel_bits=5):
    """cv2.remap(img, x, y, INTER_LINEAR) for float32 img [H, W] and float32 maps (:98)."""
    img = np.asarray(img, np.float32)
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    h, w = img.shape
    lim = np.float32(2.0 ** 30)
    with np.errstate(invalid="ignore", over="ignore"):
        if subpixel_bits:
            one = np.float32(1 << subpixel_bits)
            xs, ys = x * one, y * one
            ok = (xs > -lim) & (xs < lim) & (ys > -lim) & (ys < lim)
            sx = np.rint(np.where(ok, xs, 0)).astype(np.int64)  # cvRound: half to even
            sy = np.rint(np.where(ok, ys, 0)).astype(np.int64)
            ix, iy = sx >> subpixel_bits, sy >> subpixel_bits
            m = (1 << subpixel_bits) - 1
            fx = (sx & m).astype(np.float32) * (np.float32(1) / one)
            fy = (sy & m).astype(np.float32) * (np.float32(1) / one)
        else:
            ok = (x > -lim) & (x < lim) & (y > -lim) & (y < lim)
            xf, yf = np.floor(np.where(ok, x, 0)), np.floor(np.where(ok, y, 0))
            ix, iy = xf.astype(np.int64), yf.astype(np.int64)
            fx = (np.where(ok, x, 0) - xf).astype(np.float32)
            fy = (np.where(ok, y, 0) - yf).astype(np.float32)

    def tap(px, py):
        inside = (px >= 0) & (px < w) & (py >= 0) & (py < h)
        return np.where(inside, img[np.clip(py, 0, h - 1), np.clip(px, 0, w - 1)], np.float32(0))

    one = np.float32(1)
    out = tap(ix, iy) * ((one - fx) * (one - fy))
    out = out + tap(ix + 1, iy) * (fx * (one - fy))
    out = out + tap(ix, iy + 1) * ((one - fx) * fy)
    out = out + tap(ix + 1, iy + 1) * (fx * fy)
    return np.where(ok, out, np.float32(0)).astype(np.float32)


def _grid(h, w):
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))  # int64, as :82
    return xs, ys


def reproject_ref(depth_ref, k_ref, e_ref, depth_src, k_src, e_src, subpixel_bits=5):
    """reproject_with_depth (:78-115): (depth_reprojected, x_reprojected, y_reprojected) float32 [H, W]."""
    h, w = depth_ref.shape
    xs, ys = _grid(h, w)
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    ones = np.ones_like(xs)
    # reference pixel -> reference camera -> source camera -> source pixel (:85-92)
    cam_ref = np.linalg.inv(k_ref) @ (np.stack([xs, ys, ones]) * depth_ref.reshape(-1))
    cam_src = ((e_src @ np.linalg.inv(e_ref)) @ np.concatenate([cam_ref, ones[None]]))[:3]
    pix = k_src @ cam_src
    xy_src = pix[:2] / pix[2:3]
    # the source depth at the float32 coordinates (:96-98)
    sampled = remap_linear(depth_src, xy_src[0].reshape(h, w).astype(np.float32),
                           xy_src[1].reshape(h, w).astype(np.float32), subpixel_bits)
    # back with the float64 coordinates and the sampled depth (:103-113)
    cam_src = np.linalg.inv(k_src) @ (np.concatenate([xy_src, ones[None]]) * sampled.reshape(-1))
    cam_back = ((e_ref @ np.linalg.inv(e_src)) @ np.concatenate([cam_src, ones[None]]))[:3]
    d_rep = cam_back[2].reshape(h, w).astype(np.float32)
    pix = k_ref @ cam_back
    xy = pix[:2] / pix[2:3]
    return d_rep, xy[0].reshape(h, w).astype(np.float32), xy[1].reshape(h, w).astype(np.float32)


def check_pair_ref(depth_ref, k_ref, e_ref, depth_src, k_src, e_src, subpixel_bits=5):
    """check_geometric_consistency (:117-140) without the unused vis_mask: (masks for i = 2..10,
    depth_reprojected zeroed outside the i = 10 mask, ambiguous)."""
    h, w = depth_ref.shape
    xs, ys = _grid(h, w)
    d_rep, x_rep, y_rep = reproject_ref(depth_ref, k_ref, e_ref, depth_src, k_src, e_src, subpixel_bits)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dist = np.sqrt((x_rep - xs) ** 2 + (y_rep - ys) ** 2)  # float64 (:128)
        rel = np.abs(d_rep - depth_ref) / depth_ref  # float32 (:131-132)
        assert dist.dtype == np.float64 and rel.dtype == np.float32
        masks, amb = [], np.zeros((h, w), bool)
        for i in LEVELS:
            thr = np.float32(i / 1300)
            masks.append((dist < i / 4) & (rel < thr))
            amb |= (np.abs(dist - i / 4) < DIST_EPS) | (np.abs(rel.astype(np.float64) - np.float64(thr)) < REL_EPS)
    d_rep = d_rep.copy()
    d_rep[~masks[-1]] = 0
    return masks, d_rep, amb


def filter_view_ref(depths, confidence, ks, es, ref, srcs, photo_threshold=0.3, thres_view=3, subpixel_bits=5):
    """filter_depth (:182-262) for one reference view. depths [V, H, W] float32, ks [V, 3, 3] and
    es [V, 4, 4] float32. Returns a dict: geo_count, photo, geo, geo_thres (the thres_view term
    alone), final, depth_avg (float32), xyz [H, W, 3] float32 (0 outside final), ambiguous."""
    depths = np.asarray(depths, np.float32)
    ks, es = np.asarray(ks, np.float32), np.asarray(es, np.float32)
    s = len(srcs)
    if not 1 <= s <= 10:
        raise ValueError("1..10 source views (nine tolerance levels)")
    d_ref = depths[ref]
    h, w = d_ref.shape
    count10 = np.zeros((h, w), np.int32)
    counts = [np.zeros((h, w), np.int32) for _ in range(2, s + 1)]  # range(2, n), n = S + 1 (:210-214)
    amb = np.zeros((h, w), bool)
    dsum = 0
    for sv in srcs:
        masks, d_rep, a = check_pair_ref(d_ref, ks[ref], es[ref], depths[sv], ks[sv], es[sv], subpixel_bits)
        for j in range(len(counts)):
            counts[j] += masks[j].astype(np.int32)
        count10 += masks[-1].astype(np.int32)
        dsum = dsum + d_rep  # float32, source order (:228)
        amb |= a
    geo_thres = count10 >= thres_view
    geo = geo_thres.copy()
    for j, i in enumerate(range(2, s + 1)):
        geo |= counts[j] >= i
    depth_avg = (dsum + d_ref) / (count10 + 1)  # float32 / int32 -> float64
    assert (dsum + d_ref).dtype == np.float32 and depth_avg.dtype == np.float64
    photo = np.asarray(confidence, np.float32) > photo_threshold
    final = photo & geo
    xs, ys = _grid(h, w)
    x, y, d = xs[final], ys[final], depth_avg[final]
    cam = np.linalg.inv(ks[ref]) @ (np.stack([x, y, np.ones_like(x)]) * d)
    world = (np.linalg.inv(es[ref]) @ np.concatenate([cam, np.ones_like(x)[None]]))[:3]
    xyz = np.zeros((h, w, 3), np.float32)
    xyz[final] = world.T.astype(np.float32)
    return {"geo_count": count10, "photo": photo, "geo": geo, "geo_thres": geo_thres, "final": final,
            "depth_avg": depth_avg.astype(np.float32), "xyz": xyz, "ambiguous": amb}


def fuse_scene_ref(depths, confidences, images, ks, es, pairs, photo_threshold=0.3, thres_view=3, subpixel_bits=5):
    """filter_depth's whole-scan loop (:152-268): points [N, 3] float32 and colours [N, 3] uint8 in pair
    order, pixel order within a view; also the number of ambiguous pixels over all views."""
    pts, cols, n_amb = [], [], 0
    for ref, srcs in pairs:
        r = filter_view_ref(depths, confidences[ref], ks, es, ref, srcs, photo_threshold, thres_view, subpixel_bits)
        pts.append(r["xyz"][r["final"]])
        cols.append((np.asarray(images[ref], np.float32)[r["final"]] * 255).astype(np.uint8))
        n_amb += int(r["ambiguous"].sum())
    return np.concatenate(pts), np.concatenate(cols), n_amb
