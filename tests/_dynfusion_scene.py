"""Synthetic multi-view scene for the dynamic-fusion tests: the plane-and-cameras construction of
tests/_fusion_scene.make_scene (V cameras with small rotations and ~100 mm baselines looking at the
tilted plane n . X = 650), rendered to what the Tanks & Temples output path reads: per view a
float32 depth map, float32 intrinsics K [3, 3] and extrinsics E [4, 4], a confidence map and an RGB
image in [0, 1]. Depth maps carry multiplicative Gaussian noise (sigma 2e-3, so the nine tolerance
levels i/1300 all see traffic), a 6 x 9 patch of depth 0 and a 5 x 7 patch 5 % too far.
Deterministic (numpy PCG64)."""
import numpy as np

from tests._fusion_scene import _rot

PLANE_N = np.array([0.05, -0.03, 1.0])
PLANE_D = 650.0


def make_scene(v=5, h=48, w=64, seed=0, noise=2e-3, patches=True):
    """Returns (depths [V,H,W] f32, confidences [V,H,W] f32, images [V,H,W,3] f32, Ks [V,3,3] f32,
    Es [V,4,4] f32)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    fx = 1.8 * w
    k = np.array([[fx, 0, w / 2 - 0.3], [0, fx * 0.997, h / 2 + 0.2], [0, 0, 1.0]])
    depths, confs, imgs, ks, es = [], [], [], [], []
    for _ in range(v):
        r = _rot(*rng.uniform(-0.04, 0.04, 3))
        c = np.array([rng.uniform(-60, 60), rng.uniform(-40, 40), rng.uniform(-10, 10)])
        e = np.eye(4)
        e[:3, :3], e[:3, 3] = r, -r @ c
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
        rays_c = np.stack([(xs - k[0, 2]) / k[0, 0], (ys - k[1, 2]) / k[1, 1], np.ones_like(xs)], -1)
        rays_w = rays_c @ r  # R^T applied to row vectors
        depth = (PLANE_D - PLANE_N @ c) / (rays_w @ PLANE_N)  # camera-frame z of the intersection
        pts = c + depth[..., None] * rays_w
        if noise:
            depth = depth * (1.0 + noise * rng.standard_normal((h, w)))
        depth = depth.astype(np.float32)
        if patches:
            depth[h // 3:h // 3 + 6, w // 4:w // 4 + 9] = 0
            depth[h // 2:h // 2 + 5, w // 2:w // 2 + 7] *= np.float32(1.05)
        rgb = np.stack([0.5 + 0.45 * np.sin(pts[..., 0] / 7.0), 0.5 + 0.45 * np.cos(pts[..., 1] / 5.0),
                        0.5 + 0.45 * np.sin((pts[..., 0] + pts[..., 1]) / 11.0)], -1)
        depths.append(depth)
        confs.append(rng.uniform(0.0, 1.0, (h, w)).astype(np.float32))
        imgs.append(rgb.astype(np.float32))
        ks.append(k.astype(np.float32))
        es.append(e.astype(np.float32))
    return np.stack(depths), np.stack(confs), np.stack(imgs), np.stack(ks), np.stack(es)
