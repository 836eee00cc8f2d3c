"""A COLMAP sparse model and its images -> a scan folder `reconstruct --dataset tnt` runs on.

    python -m transmvsnet_amd.colmap_scene --model sparse/0 --images images --out DATA/<scan>
    python -m transmvsnet_amd.reconstruct --dataset tnt --testpath DATA --image_size W H --loadckpt ...

  select    per view its depth range and its ranked source views, on the GPU (view_select.py):
            depth range   the depths z > 0 of the view's observations in ascending order (one torch.sort over all
                          observations, then a stable sort by view): depth_min = 0.75 z[(n 1) // 100], depth_max =
                          1.25 z[(n 99) // 100], n the view's count, integer indices
            pairs         MVSNet's view-selection score (Yao et al. 2018) of every pair of views, summed over the
                          points both see; per view the others by descending score, ties to the lower view number,
                          the first min(n_src, V - 1) kept
  convert   select, then the folder: images/{:0>8}.jpg (a JPEG is copied byte for byte, anything else re-encoded at
            quality 95), cams_1/{:0>8}_cam.txt (line 11 = depth_min depth_max, what data.read_cam_file(tnt=True)
            reads), cams/{:0>8}_cam.txt (line 11 = depth_min interval 192 depth_max, interval = (depth_max -
            depth_min) / 191) and pair.txt as data.read_pair_file reads it. Camera numbers carry the digits that read
            back the same float32, intrinsics at full resolution (the readers divide by 4).

Views are numbered 0..V-1 in ascending COLMAP IMAGE_ID. Only undistorted (PINHOLE / SIMPLE_PINHOLE) models.
"""
from __future__ import annotations

import argparse
import os
import shutil

import numpy as np
import torch

from . import colmap, view_select
from .reconstruct import write_cam_tnt

NDEPTHS = 192  # the planes the cams/ files announce; the readers' ndepths


def depth_ranges(z, view, n_views):
    """(depth_min [V], depth_max [V], n [V]) on z's device from the observation depths z [M] float64 and their
    views [M]: per view the 1st and 99th percentile by integer index of its ascending positive depths, widened
    to 0.75 / 1.25. A view without a positive depth gets NaN and n = 0."""
    keep = z > 0
    z, view = z[keep], view[keep].long()
    z, by_z = torch.sort(z)
    view, by_view = torch.sort(view[by_z], stable=True)
    z = z[by_view]
    n = torch.bincount(view, minlength=n_views)
    start = torch.cumsum(n, 0) - n
    some = n > 0
    last = max(z.numel() - 1, 0)
    lo = torch.clamp(start + n // 100, max=last)
    hi = torch.clamp(start + (n * 99) // 100, max=last)
    nan = torch.full((n_views,), float("nan"), dtype=torch.float64, device=z.device)
    if z.numel() == 0:
        return nan, nan.clone(), n
    return torch.where(some, 0.75 * z[lo], nan), torch.where(some, 1.25 * z[hi], nan), n


def rank_sources(scores, n_src):
    """[V, min(n_src, V - 1)] int64: per view the other views by descending score, ties to the lower number."""
    v = scores.shape[0]
    s = scores.clone()
    s.fill_diagonal_(float("-inf"))
    order = torch.sort(s, dim=1, descending=True, stable=True).indices
    return order[:, :min(int(n_src), v - 1)]


def select(model, n_src=10, theta0=5.0, sigma1=1.0, sigma2=10.0, device="cuda"):
    """View selection and depth ranges of a colmap.read_model dictionary, computed on `device`. Returns numpy
    arrays: {"scores" [V, V] float64, "counts" [V, V] int32, "depth_min" [V], "depth_max" [V], "pairs" [V, k]}."""
    if not torch.cuda.is_available():
        raise RuntimeError("colmap_scene.select: needs a GPU (HIP kernels; no CPU fallback)")
    v, p = len(model["image_ids"]), len(model["point_ids"])
    view_select.check_sizes(v, p)
    obs = np.ascontiguousarray(model["obs"], np.int32)
    if obs.shape[0] == 0:
        raise ValueError(f"image {model['names'][0]!r} has no observation of a 3-D point: no depth range")
    dev = torch.device(device)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    obs_view, obs_point = up(obs[:, 0], np.int32), up(obs[:, 1], np.int32)
    xyz, centres = up(model["xyz"], np.float64), up(model["centres"], np.float64)
    z = view_select.obs_depth(obs_view, obs_point, up(model["R"][:, 2, :], np.float64), up(model["t"][:, 2], np.float64), xyz)
    dmin, dmax, n = depth_ranges(z, obs_view, v)
    empty = torch.nonzero(n == 0).flatten().tolist()
    if empty:
        raise ValueError(f"image {model['names'][empty[0]]!r} has no observation in front of the camera: no depth "
                         f"range ({len(empty)} such images)")
    bits = view_select.set_bits(obs_view, obs_point, v, p)
    scores, counts = view_select.pair_scores(bits, p, centres, xyz, theta0, sigma1, sigma2)
    pairs = rank_sources(scores, n_src)
    return {"scores": scores.cpu().numpy(), "counts": counts.cpu().numpy(), "depth_min": dmin.cpu().numpy(),
            "depth_max": dmax.cpu().numpy(), "pairs": pairs.cpu().numpy()}


# ------------------------------------------------------------------ the folder
def _write_cam_dtu(filename, intrinsics, extrinsics, depth_min, depth_max):
    """write_cam_tnt's file with line 11 = depth_min interval 192 depth_max."""
    write_cam_tnt(filename, intrinsics, extrinsics)
    with open(filename) as f:
        lines = f.readlines()
    interval = (float(depth_max) - float(depth_min)) / (NDEPTHS - 1)
    lines[11] = "{} {} {} {}\n".format(repr(float(depth_min)), repr(interval), NDEPTHS, repr(float(depth_max)))
    with open(filename, "w") as f:
        f.writelines(lines)


def _copy_image(src, dst):
    from PIL import Image
    with Image.open(src) as im:
        if im.format == "JPEG":
            shutil.copyfile(src, dst)
        else:
            im.convert("RGB").save(dst, format="JPEG", quality=95)


def write_scan(out_scan_dir, K, R, t, depth_min, depth_max, pairs, scores):
    """cams_1/, cams/ and pair.txt of a scan folder for V views: K [V, 3, 3] at full resolution, R [V, 3, 3],
    t [V, 3], the depth ranges [V], pairs [V, k] and the score matrix the pair lines quote."""
    for sub in ("cams_1", "cams"):
        os.makedirs(os.path.join(out_scan_dir, sub), exist_ok=True)
    for i in range(len(K)):
        extr = np.eye(4)
        extr[:3, :3], extr[:3, 3] = R[i], t[i]
        write_cam_tnt(os.path.join(out_scan_dir, "cams_1", "{:0>8}_cam.txt".format(i)), K[i], extr, depth_min[i],
                      depth_max[i])
        _write_cam_dtu(os.path.join(out_scan_dir, "cams", "{:0>8}_cam.txt".format(i)), K[i], extr, depth_min[i],
                       depth_max[i])
    with open(os.path.join(out_scan_dir, "pair.txt"), "w") as f:
        f.write("{}\n".format(len(K)))
        for i, srcs in enumerate(pairs):
            f.write("{}\n{} ".format(i, len(srcs)) + " ".join("{} {}".format(int(s), repr(float(scores[i][s])))
                                                              for s in srcs) + "\n")


def convert(model_dir, image_dir, out_scan_dir, n_src=10, theta0=5.0, sigma1=1.0, sigma2=10.0, device="cuda",
            copy_images=True):
    """The COLMAP model folder `model_dir` and its images under `image_dir` -> the scan folder `out_scan_dir`.
    Returns select's arrays plus "names" and "image_ids" (view i is image_ids[i], written as {i:0>8})."""
    model = colmap.read_model(model_dir)
    res = select(model, n_src, theta0, sigma1, sigma2, device)
    write_scan(out_scan_dir, model["K"], model["R"], model["t"], res["depth_min"], res["depth_max"], res["pairs"],
               res["scores"])
    if copy_images:
        os.makedirs(os.path.join(out_scan_dir, "images"), exist_ok=True)
        for i, name in enumerate(model["names"]):
            _copy_image(os.path.join(image_dir, name), os.path.join(out_scan_dir, "images", "{:0>8}.jpg".format(i)))
    res.update(names=model["names"], image_ids=model["image_ids"], sizes=model["sizes"])
    return res


def make_parser():
    p = argparse.ArgumentParser(description="COLMAP sparse model + images -> a scan folder for reconstruct --dataset tnt")
    p.add_argument("--model", required=True, help="folder with cameras / images / points3D as .bin or .txt")
    p.add_argument("--images", required=True, help="folder the model's image names are relative to")
    p.add_argument("--out", required=True, help="the scan folder to write: DATA/<scan>")
    p.add_argument("--n_src", type=int, default=10, help="source views kept per view")
    p.add_argument("--theta0", type=float, default=5.0, help="the score's preferred baseline angle, degrees")
    p.add_argument("--sigma1", type=float, default=1.0, help="the score's width below theta0")
    p.add_argument("--sigma2", type=float, default=10.0, help="the score's width above theta0")
    return p


def main(argv=None):
    a = make_parser().parse_args(argv)
    res = convert(a.model, a.images, a.out, a.n_src, a.theta0, a.sigma1, a.sigma2)
    w, h = res["sizes"].max(0)
    print("{}: {} views, depth {:.4g} .. {:.4g}; run reconstruct --dataset tnt --image_size {} {}".format(
        a.out, len(res["names"]), res["depth_min"].min(), res["depth_max"].max(), int(w), int(h)))


if __name__ == "__main__":
    main()
