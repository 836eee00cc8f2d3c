"""Restatement of what sits between the network and the fusion kernels, composed from the package's host
functions: test.py:127-157 (cv2.resize of the coarse confidences = data.resize_bilinear, the confidence
product, the 0.01 mask, utils.depth_normal = fusion.depth_normal, the clipped 8-bit image) and fusibile's
decode of the PNG (main.cpp:126-138 = fusion.rgbd_from_images). tmvs_depth_postprocess must equal it
bitwise. Also the seeded inputs and the planted scan folders the reconstruct tests share."""
import os

import numpy as np

from transmvsnet_amd import data, fusion

CONF_THRESHOLD = np.float32(0.01)


def postprocess_ref(depth, conf3, conf2, conf1, image=None, conf_threshold=CONF_THRESHOLD, depth_min=425.0,
                    depth_max=935.0):
    """depth, conf3 [H, W], conf2 [H/2, W/2], conf1 [H/4, W/4] float32, image [3, H, W] or None ->
    {"conf_final", "depth"} and, with an image, {"rgba_u8" [H, W, 4], "rgbd" [H, W, 4]}."""
    h, w = conf3.shape
    up1 = data.resize_bilinear(conf1, w, h)
    up2 = data.resize_bilinear(conf2, w, h)
    conf_final = conf3 * up1 * up2
    assert conf_final.dtype == np.float32
    d = np.array(depth, np.float32)
    with np.errstate(invalid="ignore"):
        d[conf_final < np.float32(conf_threshold)] = 0.0
    out = {"conf_final": conf_final, "depth": d}
    if image is not None:
        rgb = np.clip(np.transpose(image, (1, 2, 0)) * 255, 0, 255).astype(np.uint8)
        alpha = fusion.depth_normal(d, depth_min, depth_max)
        out["rgba_u8"] = np.concatenate([rgb, alpha[..., None]], axis=2)
        out["rgbd"] = fusion.rgbd_from_images(rgb[..., ::-1], alpha)
    return out


def seeded_inputs(h, w, seed=0):
    """Inputs that reach every branch: confidences whose product falls on both sides of 0.01, the pixels
    (0..1, 0..1) with both resized confidences exactly 1 and conf3 = float32(0.01), its two float32
    neighbours and a NaN; depths below 425, above 935, at both ends and at 425 + 2k, where the scaled alpha
    lands on an integer; colours outside [0, 1] and at k / 255."""
    rng = np.random.Generator(np.random.PCG64(seed + 131 * h + w))
    conf3 = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    conf2 = rng.uniform(0.0, 0.4, (h // 2, w // 2)).astype(np.float32)
    conf1 = rng.uniform(0.0, 0.4, (h // 4, w // 4)).astype(np.float32)
    conf1[0, 0] = 1.0
    conf2[:2, :2] = 1.0
    t = np.float32(0.01)
    conf3[0, 0], conf3[0, 1] = t, np.nextafter(t, np.float32(0))
    conf3[1, 0], conf3[1, 1] = np.nextafter(t, np.float32(1)), np.nan
    depth = rng.uniform(300.0, 1100.0, (h, w)).astype(np.float32)
    special = np.concatenate([np.float32([425.0, 935.0, 424.99997, 935.00006, 0.0]),
                              (425.0 + 2.0 * np.arange(1, 255)).astype(np.float32)])
    idx = rng.permutation(h * w)[:min(len(special), h * w // 2)]
    depth.reshape(-1)[idx] = special[:len(idx)]
    image = rng.uniform(-0.1, 1.1, (3, h, w)).astype(np.float32)
    ks = (np.arange(256) / 255.0).astype(np.float32)
    idx = rng.permutation(3 * h * w)[:min(256, 3 * h * w // 2)]
    image.reshape(-1)[idx] = ks[:len(idx)]
    return depth, conf3, conf2, conf1, image


# ------------------------------------------------------------------ planted scans for the driver
def planted_scene(v=5, h=64, w=96, seed=7):
    """tests/_dynfusion_scene cameras and depth maps (the construction of tests/_fusion_scene) plus the
    three stage confidences a stub model returns: conf3 uniform in [0, 1], the coarse ones in [0.8, 1]."""
    from tests._dynfusion_scene import make_scene
    depths, conf3, images, ks, es = make_scene(v, h, w, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    conf2 = rng.uniform(0.8, 1.0, (v, h // 2, w // 2)).astype(np.float32)
    conf1 = rng.uniform(0.8, 1.0, (v, h // 4, w // 4)).astype(np.float32)
    return {"depths": depths, "conf3": conf3, "conf2": conf2, "conf1": conf1, "images": images, "Ks": ks, "Es": es}


def write_planted_scan(root, scan, scene, cams_dir):
    """The scene as a scan folder of the dataset readers: images/{:0>8}.jpg at the depth maps' size,
    <cams_dir>/{:0>8}_cam.txt (the readers divide the intrinsics by 4 and stage 3 multiplies them back,
    exactly), pair.txt with every other view as a source."""
    from PIL import Image

    from transmvsnet_amd import reconstruct
    v = len(scene["depths"])
    os.makedirs(os.path.join(root, scan, "images"))
    os.makedirs(os.path.join(root, scan, cams_dir))
    for i in range(v):
        Image.fromarray((scene["images"][i] * 255).astype(np.uint8)).save(
            os.path.join(root, scan, "images", "{:0>8}.jpg".format(i)), quality=95)
        reconstruct.write_cam_tnt(os.path.join(root, scan, cams_dir, "{:0>8}_cam.txt".format(i)), scene["Ks"][i],
                                  scene["Es"][i], 425.0, 935.0 if cams_dir == "cams_1" else 2.5)
    with open(os.path.join(root, scan, "pair.txt"), "w") as f:
        f.write(f"{v}\n")
        for i in range(v):
            src = [u for u in range(v) if u != i]
            f.write(f"{i}\n{len(src)} " + " ".join(f"{u} {10.0 - u:.1f}" for u in src) + "\n")


class StubModel:
    """A callable with TransMVSNet.forward's signature that returns the planted depth and stage confidences
    of the reference view it recognises by the extrinsics in proj_matrix."""

    def __init__(self, scene, device="cuda"):
        import torch
        self.es = scene["Es"]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.t = {k: up(scene[k]) for k in ("depths", "conf3", "conf2", "conf1")}
        self.calls = []

    def __call__(self, imgs, proj_matrix, depth_values):
        e = proj_matrix["stage3"][0, 0, 0].numpy()
        i = [j for j in range(len(self.es)) if np.array_equal(self.es[j], e)]
        assert len(i) == 1, "reference view not recognised"
        i = i[0]
        self.calls.append((i, tuple(imgs.shape)))
        t = self.t
        out = {"depth": t["depths"][i:i + 1], "photo_confidence": t["conf3"][i:i + 1]}
        out["stage1"] = {"photo_confidence": t["conf1"][i:i + 1]}
        out["stage2"] = {"photo_confidence": t["conf2"][i:i + 1]}
        out["stage3"] = {"photo_confidence": t["conf3"][i:i + 1], "depth": t["depths"][i:i + 1]}
        return out
