"""Deterministic synthetic inputs and weights for the TransMVSNet hot path.

There is no network here (no DTU download, no Google-Drive checkpoint), so every
benchmark, smoke run and parity test feeds the same seeded data:

* ``synthetic_state_dict`` -- key-name-seeded weights for the reference state_dict
  layout (465 keys, ``models/TransMVSNet.py:112-139``), randomised BN statistics and
  an optional sharpening factor on ``cost_regularization.{s}.prob.weight`` so that the
  probability volumes are peaked (random-init volumes are nearly uniform, which
  makes winner-take-all parity meaningless).
* ``synthetic_cameras`` -- DTU-like ``proj_matrix`` dict (``datasets/general_eval.py:
  182-210``): extrinsic in ``[:, :, 0]``, 1/4-resolution intrinsics in
  ``[:, :, 1, :3, :3]``, scaled x2 / x4 for stages 2 / 3.
* ``synthetic_depth_values`` -- ``np.arange(425, 2.5*(192-0.5)+425, 2.5)``
  (``datasets/general_eval.py:190-192``).
* ``synthetic_features`` -- stand-in for FeatureNet's per-view pyramid
  (``models/module.py:399-422``): stage1 [B,32,H/4,W/4], stage2 [B,16,H/2,W/2],
  stage3 [B,8,H,W].
"""
from __future__ import annotations

import math
import zlib

import numpy as np
import torch

DTU_DEPTH_MIN = 425.0
DTU_DEPTH_INTERVAL = 2.5
DTU_NDEPTH = 192


def _rng(seed: int, key: str) -> np.random.Generator:
    return np.random.default_rng([int(seed) & 0xFFFFFFFF, zlib.crc32(key.encode("utf-8"))])


def synthetic_state_dict(shapes, seed: int = 0, sharpen: float = 100.0):
    """Fill every key of ``shapes`` ({key: (shape, dtype)}) deterministically.

    The generator depends only on (seed, key name, shape), so the reference model,
    the CPU oracle and the HIP model all receive bit-identical weights.
    """
    out = {}
    for key, (shape, dtype) in shapes.items():
        rng = _rng(seed, key)
        leaf = key.rsplit(".", 1)[-1]
        shape = tuple(int(s) for s in shape)
        if leaf == "num_batches_tracked":
            out[key] = torch.zeros(shape, dtype=torch.long)
            continue
        if "conv_offset_mask" in key:
            # the reference zero-initialises the DCN offset/mask conv (models/dcn.py:62-64)
            arr = np.zeros(shape, np.float32)
        elif leaf == "running_mean":
            arr = rng.uniform(-0.1, 0.1, shape)
        elif leaf == "running_var":
            arr = rng.uniform(0.5, 1.5, shape)
        elif len(shape) == 1 and leaf == "weight":  # BatchNorm / LayerNorm affine
            arr = rng.uniform(0.8, 1.2, shape)
        elif len(shape) == 1:  # biases
            arr = rng.uniform(-0.1, 0.1, shape)
        else:
            fan_in = int(np.prod(shape[1:]))
            b = math.sqrt(3.0 / fan_in)
            arr = rng.uniform(-b, b, shape)
            if sharpen != 1.0 and key.startswith("cost_regularization.") and key.endswith("prob.weight"):
                arr = arr * sharpen
        out[key] = torch.from_numpy(np.asarray(arr, dtype=np.float32))
    return out


def state_dict_shapes(module: torch.nn.Module):
    return {k: (tuple(v.shape), v.dtype) for k, v in module.state_dict().items()}


def synthetic_depth_values(batch: int = 1) -> torch.Tensor:
    dv = np.arange(DTU_DEPTH_MIN, DTU_DEPTH_INTERVAL * (DTU_NDEPTH - 0.5) + DTU_DEPTH_MIN,
                   DTU_DEPTH_INTERVAL, dtype=np.float32)
    return torch.from_numpy(np.tile(dv[None], (batch, 1)))


def _rodrigues(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * k + (1 - math.cos(angle)) * (k @ k)


def _look_at(center, target, up_jitter):
    z = target - center
    z = z / np.linalg.norm(z)
    up = np.array([0.0, 1.0, 0.0]) + up_jitter
    x = np.cross(up, z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z])  # rows: camera axes in world frame -> R (world->cam)


def synthetic_cameras(n_views: int, height: int, width: int, batch: int = 1, seed: int = 1):
    """DTU-like multi-view rig looking at a scene centred ~650 mm in front of the ref camera.

    Returns {"stage1","stage2","stage3": float32 tensor [B, N, 2, 4, 4]} in the layout
    of ``datasets/general_eval.py:182-210``.
    """
    rng = np.random.default_rng(seed)
    # 1/4-resolution intrinsics: DTU 2892.33/2883.18/823.205/619.071 /4 x0.72 at 864x1152
    sx = (width / 4.0) / 288.0
    sy = (height / 4.0) / 216.0
    K = np.array([[520.6 * sx, 0.0, 148.2 * sx], [0.0, 519.0 * sy, 111.4 * sy], [0.0, 0.0, 1.0]])
    target = np.array([0.0, 0.0, 650.0])
    mats = np.zeros((batch, n_views, 2, 4, 4), np.float32)
    for b in range(batch):
        for v in range(n_views):
            if v == 0:
                R = np.eye(3)
                C = np.zeros(3)
            else:
                ang = rng.uniform(0, 2 * math.pi)
                rad = rng.uniform(50.0, 150.0)
                C = np.array([rad * math.cos(ang), rad * math.sin(ang), rng.uniform(-20.0, 20.0)])
                R = _look_at(C, target + rng.uniform(-15, 15, 3), rng.uniform(-0.03, 0.03, 3))
                R = _rodrigues(rng.normal(size=3), math.radians(rng.uniform(0, 1.5))) @ R
            t = -R @ C
            E = np.eye(4)
            E[:3, :3] = R
            E[:3, 3] = t
            mats[b, v, 0] = E.astype(np.float32)
            mats[b, v, 1, :3, :3] = K.astype(np.float32)
    s2 = mats.copy()
    s2[:, :, 1, :2, :] = mats[:, :, 1, :2, :] * 2
    s3 = mats.copy()
    s3[:, :, 1, :2, :] = mats[:, :, 1, :2, :] * 4
    return {"stage1": torch.from_numpy(mats), "stage2": torch.from_numpy(s2), "stage3": torch.from_numpy(s3)}


def synthetic_images(n_views: int, height: int, width: int, batch: int = 1, seed: int = 0):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.random((batch, n_views, 3, height, width), dtype=np.float32))


def synthetic_features(n_views: int, height: int, width: int, batch: int = 1, seed: int = 2):
    """Per-view FeatureNet-shaped pyramids, ~N(0,1), NCHW float32 (CPU)."""
    rng = np.random.default_rng(seed)
    feats = []
    for _ in range(n_views):
        f = {}
        for name, c, s in (("stage1", 32, 4), ("stage2", 16, 2), ("stage3", 8, 1)):
            f[name] = torch.from_numpy(rng.standard_normal((batch, c, height // s, width // s), dtype=np.float32))
        feats.append(f)
    return feats


def stacked_features(n_views: int, height: int, width: int, seed: int = 2):
    """FeatureNet-shaped pyramids already stacked as forward_features takes them:
    {stage: [1, N, C, h, w]} ~N(0,1) from torch's CPU generator (bench.py's inputs)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return {name: torch.randn(1, n_views, c, height // s, width // s, generator=g)
            for name, c, s in (("stage1", 32, 4), ("stage2", 16, 2), ("stage3", 8, 1))}


# ------------------------------------------------------------------ training scans on disk
def _plane_view(K, E, height, width, plane=(0.02, -0.03, 1.0, 650.0)):
    """A textured plane n . X = c (world frame) seen by the camera (K 3x3 at this pixel scale, E 4x4
    world -> camera): (depth [h,w] float32, image [h,w,3] uint8)."""
    n, c = np.asarray(plane[:3], np.float64), float(plane[3])
    R, t = E[:3, :3].astype(np.float64), E[:3, 3].astype(np.float64)
    y, x = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    rays = np.linalg.inv(K.astype(np.float64)) @ np.stack([x.ravel(), y.ravel(), np.ones(x.size)])
    centre = -R.T @ t
    dirs = R.T @ rays
    s = (c - n @ centre) / (n @ dirs)  # camera-frame rays have z = 1, so the ray parameter is the depth
    pts = centre[:, None] + dirs * s
    tex = np.stack([0.5 + 0.5 * np.sin(pts[0] / f + p) * np.cos(pts[1] / g) for f, g, p in
                    ((9.0, 13.0, 0.0), (17.0, 7.0, 1.0), (5.0, 23.0, 2.0))], axis=-1)
    return (s.reshape(height, width).astype(np.float32),
            np.clip(tex.reshape(height, width, 3) * 255.0, 0, 255).astype(np.uint8))


def _write_cam(filename, extrinsic, intrinsic, depth_line):
    with open(filename, "w") as f:
        f.write("extrinsic\n")
        for row in extrinsic:
            f.write(" ".join("{:.9g}".format(float(v)) for v in row) + "\n")
        f.write("\nintrinsic\n")
        for row in intrinsic:
            f.write(" ".join("{:.9g}".format(float(v)) for v in row) + "\n")
        f.write("\n" + depth_line + "\n")


def _write_pairs(filename, n_views):
    with open(filename, "w") as f:
        f.write(f"{n_views}\n")
        for v in range(n_views):
            others = [(v + k) % n_views for k in range(1, n_views)]
            f.write(f"{v}\n{len(others)} " + " ".join(f"{o} {100.0 - i:.1f}" for i, o in enumerate(others)) + "\n")


def write_blended_scan(root, scan="scan0", n_views=3, height=128, width=160, seed=1):
    """A BlendedMVS-format scan as datasets/bld_train.py reads it, under root/scan: blended_images/*.jpg,
    cams/*_cam.txt (full-size intrinsics = synthetic_cameras' x 4; depth line 'min interval n max'),
    cams/pair.txt (every view with all others as sources) and rendered_depth_maps/*.pfm of a textured plane.
    Writes root/list.txt and returns its path."""
    import os

    from PIL import Image

    from .data import save_pfm
    cams = synthetic_cameras(n_views, height, width, seed=seed)["stage1"][0].numpy()
    for sub in ("blended_images", "cams", "rendered_depth_maps"):
        os.makedirs(os.path.join(root, scan, sub), exist_ok=True)
    for v in range(n_views):
        K = cams[v, 1, :3, :3].copy()
        K[:2] *= 4.0
        depth, img = _plane_view(K, cams[v, 0], height, width)
        Image.fromarray(img).save(os.path.join(root, scan, "blended_images", "{:0>8}.jpg".format(v)), quality=95)
        save_pfm(os.path.join(root, scan, "rendered_depth_maps", "{:0>8}.pfm".format(v)), depth)
        _write_cam(os.path.join(root, scan, "cams", "{:0>8}_cam.txt".format(v)), cams[v, 0], K,
                   "{} {} {} {}".format(DTU_DEPTH_MIN, DTU_DEPTH_INTERVAL, DTU_NDEPTH, 935.0))
    _write_pairs(os.path.join(root, scan, "cams", "pair.txt"), n_views)
    listfile = os.path.join(root, "list.txt")
    with open(listfile, "w") as f:
        f.write(scan + "\n")
    return listfile


def write_dtu_train_scan(root, scan="scan1", n_views=3, height=128, width=160, margin=(12, 12), seed=1):
    """A dtu_yao-format training set (datasets/dtu_yao.py) with one scan: Rectified/{scan}_train/
    rect_{vid+1:03}_{light}_r5000.png at height x width (7 lights), Cameras/train/*_cam.txt (intrinsics as
    stored), Cameras/pair.txt, and Depths_raw/{scan}/depth_map_*.pfm + depth_visual_*.png at the raw size
    2 * (height + margin[0]) x 2 * (width + margin[1]), whose halved centre crop is height x width. Writes
    root/list.txt and returns its path."""
    import os

    from PIL import Image

    from .data import save_pfm
    cams = synthetic_cameras(n_views, height, width, seed=seed)["stage1"][0].numpy()
    for sub in (f"Rectified/{scan}_train", "Cameras/train", f"Depths_raw/{scan}"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    rh, rw = 2 * (height + margin[0]), 2 * (width + margin[1])
    for v in range(n_views):
        K3 = cams[v, 1, :3, :3].copy()
        K3[:2] *= 4.0  # the image's own scale
        _, img = _plane_view(K3, cams[v, 0], height, width)
        for light in range(7):
            lit = np.clip(img.astype(np.float32) * (0.7 + 0.05 * light), 0, 255).astype(np.uint8)
            Image.fromarray(lit).save(os.path.join(root, f"Rectified/{scan}_train",
                                                   "rect_{:0>3}_{}_r5000.png".format(v + 1, light)))
        # the raw map: twice the image's scale, its centre moved by the crop's start
        Kr = K3.copy()
        Kr[:2] *= 2.0
        Kr[0, 2] += 2.0 * (margin[1] // 2)
        Kr[1, 2] += 2.0 * (margin[0] // 2)
        depth, _ = _plane_view(Kr, cams[v, 0], rh, rw)
        save_pfm(os.path.join(root, f"Depths_raw/{scan}", "depth_map_{:0>4}.pfm".format(v)), depth)
        visual = np.full((rh, rw), 128, np.uint8)
        visual[:rh // 8], visual[:, :rw // 8] = 0, 10  # a border outside the mask (0 and exactly 10: not > 10)
        Image.fromarray(visual).save(os.path.join(root, f"Depths_raw/{scan}", "depth_visual_{:0>4}.png".format(v)))
        _write_cam(os.path.join(root, "Cameras/train", "{:0>8}_cam.txt".format(v)), cams[v, 0], cams[v, 1, :3, :3],
                   "{} {}".format(DTU_DEPTH_MIN, DTU_DEPTH_INTERVAL))
    _write_pairs(os.path.join(root, "Cameras/pair.txt"), n_views)
    listfile = os.path.join(root, "list.txt")
    with open(listfile, "w") as f:
        f.write(scan + "\n")
    return listfile


# ------------------------------------------------------------------ COLMAP sparse models on disk
def _rot_to_quat(R):
    """The Hamilton quaternion (w, x, y, z), w >= 0, of a rotation matrix (Shepperd's branches)."""
    R = np.asarray(R, np.float64)
    tr = np.trace(R)
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = [0.0] * 4
        q[0], q[1 + i], q[1 + j], q[1 + k] = (R[k, j] - R[j, k]) / s, 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    q = np.array(q, np.float64)
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def write_colmap_model(root, n_views=6, n_points=300, height=128, width=160, seed=1, binary=True, spread=220.0):
    """A small COLMAP sparse model under `root` (cameras / images / points3D as .bin or .txt, colmap.write_raw):
    synthetic_cameras' rig with full-size PINHOLE intrinsics, image ids 2 v + 1 named view_{v:03}.png, and
    n_points random points round the rig's target (x, y within +-spread, z in 600..700; ids 10 + 3 p), each
    observed by the views it projects into (0 <= u < width, 0 <= v < height, z > 0). Returns what it wrote: the
    three dictionaries of colmap.read_raw under "cameras", "images", "points3D", and the arrays colmap.read_model
    gives for them: "image_ids", "names", "K", "R", "t", "centres", "point_ids", "xyz", "obs"."""
    from . import colmap
    rng = np.random.default_rng([int(seed), 77])
    cams = synthetic_cameras(n_views, height, width, seed=seed)["stage1"][0].numpy().astype(np.float64)
    xyz = np.stack([rng.uniform(-spread, spread, n_points), rng.uniform(-spread, spread, n_points),
                    rng.uniform(600.0, 700.0, n_points)], 1)
    point_ids = 10 + 3 * np.arange(n_points)
    cameras, images, tracks, obs = {}, {}, [[] for _ in range(n_points)], []
    K_all, R_all, t_all = [], [], []
    for v in range(n_views):
        K = cams[v, 1, :3, :3].copy()
        K[:2] *= 4.0
        q = _rot_to_quat(cams[v, 0, :3, :3])
        R, t = colmap.quat_to_rot(q), cams[v, 0, :3, 3].copy()
        cameras[v + 1] = ("PINHOLE", width, height, np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]))
        pc = xyz @ R.T + t
        uv = pc[:, :2] / pc[:, 2:3] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
        seen = np.nonzero((pc[:, 2] > 0) & (uv[:, 0] >= 0) & (uv[:, 0] < width) & (uv[:, 1] >= 0) & (uv[:, 1] < height))[0]
        # one 2-D point without a 3-D point in front, as COLMAP's images carry
        xy = np.concatenate([[[0.5, 0.5]], uv[seen]])
        ids = np.concatenate([[-1], point_ids[seen]]).astype(np.int64)
        for k, p in enumerate(seen):
            tracks[p].append((2 * v + 1, k + 1))
        images[2 * v + 1] = (q, t, v + 1, "view_{:03}.png".format(v), xy, ids)
        obs.append(np.stack([np.full(seen.size, v), seen], 1))
        K_all.append(K), R_all.append(R), t_all.append(t)
    points3D = {int(point_ids[p]): (xyz[p], rng.integers(0, 256, 3).astype(np.uint8), float(rng.uniform(0.1, 1.0)),
                                    np.array(tracks[p], np.int32).reshape(-1, 2)) for p in range(n_points)}
    colmap.write_raw(root, cameras, images, points3D, binary)
    R_all, t_all = np.stack(R_all), np.stack(t_all)
    return {"cameras": cameras, "images": images, "points3D": points3D, "image_ids": 2 * np.arange(n_views) + 1,
            "names": [images[2 * v + 1][3] for v in range(n_views)], "K": np.stack(K_all), "R": R_all, "t": t_all,
            "centres": np.stack([-R.T @ t for R, t in zip(R_all, t_all)]), "point_ids": point_ids, "xyz": xyz,
            "obs": np.concatenate(obs).astype(np.int32)}
