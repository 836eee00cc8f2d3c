"""A numpy restatement of the two training dataset classes (datasets/bld_train.py:30-172,
datasets/dtu_yao.py:26-193), written from their behaviour and independent of transmvsnet_amd.data /
transmvsnet_amd.finetune: what tests/test_finetune_host.py and tests/test_gpu_finetune.py compare against.

cv2 is not available, so `nearest` stands in for cv2.resize(..., interpolation=cv2.INTER_NEAREST): output
index x reads source index min(floor(x * (1.0 / (dst / src))), src - 1) computed in float64, with no
half-pixel offset. For a source size divisible by the factor that is [::2] / [::4]; the tests assert that
identity separately.
"""
import os
import re

import numpy as np
from PIL import Image


def nearest(img, new_w, new_h):
    h, w = img.shape
    out = np.empty((new_h, new_w), img.dtype)
    fy, fx = 1.0 / (new_h / h), 1.0 / (new_w / w)
    for y in range(new_h):
        sy = min(int(np.floor(y * fy)), h - 1)
        for x in range(new_w):
            out[y, x] = img[sy, min(int(np.floor(x * fx)), w - 1)]
    return out


def nearest_fast(img, new_w, new_h):
    """`nearest` with the two index vectors built first (the same double arithmetic per index)."""
    h, w = img.shape
    ys = [min(int(np.floor(y * (1.0 / (new_h / h)))), h - 1) for y in range(new_h)]
    xs = [min(int(np.floor(x * (1.0 / (new_w / w)))), w - 1) for x in range(new_w)]
    return img[np.array(ys)][:, np.array(xs)]


def read_pfm(filename):
    with open(filename, "rb") as f:
        kind = f.readline().decode().rstrip()
        assert kind == "Pf"
        w, h = map(int, re.match(r"^(\d+)\s(\d+)\s$", f.readline().decode()).groups())
        scale = float(f.readline().rstrip())
        d = np.fromfile(f, "<f" if scale < 0 else ">f")
    return np.array(np.flipud(d.reshape(h, w)), dtype=np.float32)


def _cam_lines(filename):
    with open(filename) as f:
        return [ln.rstrip() for ln in f.readlines()]


def _matrix(lines, n):
    return np.array([float(v) for ln in lines for v in ln.split()], dtype=np.float64).astype(np.float32).reshape(n, n)


def _pairs(filename):
    with open(filename) as f:
        out = []
        for _ in range(int(f.readline())):
            ref = int(f.readline().rstrip())
            out.append((ref, [int(x) for x in f.readline().rstrip().split()[1::2]]))
    return out


def _scans(listfile):
    with open(listfile) as f:
        return [ln.rstrip() for ln in f.readlines()]


def _stages(proj):
    s2, s3 = proj.copy(), proj.copy()
    s2[:, 1, :2, :] = proj[:, 1, :2, :] * 2
    s3[:, 1, :2, :] = proj[:, 1, :2, :] * 4
    return {"stage1": proj, "stage2": s2, "stage3": s3}


def _pyramid(full):
    h, w = full.shape
    return {"stage1": nearest_fast(full, w // 4, h // 4), "stage2": nearest_fast(full, w // 2, h // 2), "stage3": full}


class BldRef:
    def __init__(self, datapath, listfile, nviews, ndepths=192):
        self.datapath, self.nviews, self.ndepths = datapath, nviews, ndepths
        self.metas = []
        for scan in _scans(listfile):
            for ref, src in _pairs(os.path.join(datapath, scan, "cams", "pair.txt")):
                if len(src) < nviews - 1:
                    continue
                self.metas.append((scan, ref, src))

    def __len__(self):
        return len(self.metas)

    def cam(self, filename):
        lines = _cam_lines(filename)
        extr, intr = _matrix(lines[1:5], 4), _matrix(lines[7:10], 3)
        intr[:2, :] /= 4.0
        dmin, dmax = float(lines[11].split()[0]), float(lines[11].split()[-1])
        return intr, extr, dmin, float(dmax - dmin) / self.ndepths

    def __getitem__(self, idx):
        scan, ref, src = self.metas[idx]
        imgs, projs = [], []
        for i, vid in enumerate([ref] + src[:self.nviews - 1]):
            imgs.append(np.array(Image.open(os.path.join(self.datapath, scan, "blended_images", "%08d.jpg" % vid)),
                                 dtype=np.float32) / 255.)
            intr, extr, dmin, dint = self.cam(os.path.join(self.datapath, scan, "cams", "%08d_cam.txt" % vid))
            p = np.zeros((2, 4, 4), np.float32)
            p[0, :4, :4] = extr
            p[1, :3, :3] = intr
            projs.append(p)
            if i == 0:
                depth = read_pfm(os.path.join(self.datapath, scan, "rendered_depth_maps", "%08d.pfm" % vid))
                dend = dint * (self.ndepths - 1) + dmin
                mask = np.array((depth >= np.float32(dmin)) & (depth <= np.float32(dend)), dtype=np.float32)
                values = np.arange(dmin, dint * self.ndepths + dmin, dint, dtype=np.float32)
        # the class returns the interval left in its loop variable: the last view's
        return {"imgs": np.stack(imgs).transpose([0, 3, 1, 2]), "proj_matrix": _stages(np.stack(projs)),
                "depth": _pyramid(depth), "mask": _pyramid(mask), "depth_values": values, "depth_interval": dint}


class DtuRef:
    def __init__(self, datapath, listfile, nviews, ndepths=192, interval_scale=1.06, target_hw=(512, 640)):
        self.datapath, self.nviews, self.ndepths = datapath, nviews, ndepths
        self.interval_scale, self.target_hw = interval_scale, target_hw
        self.metas = []
        for scan in _scans(listfile):
            for ref, src in _pairs(os.path.join(datapath, "Cameras", "pair.txt")):
                for light in range(7):
                    self.metas.append((scan, light, ref, src))

    def __len__(self):
        return len(self.metas)

    def prepare(self, hr):
        h, w = hr.shape
        ds = nearest_fast(hr, w // 2, h // 2)
        h, w = ds.shape
        th, tw = self.target_hw
        sh, sw = (h - th) // 2, (w - tw) // 2
        return ds[sh:sh + th, sw:sw + tw]

    def __getitem__(self, idx):
        scan, light, ref, src = self.metas[idx]
        imgs, projs = [], []
        for i, vid in enumerate([ref] + src[:self.nviews - 1]):
            fn = os.path.join(self.datapath, "Rectified", scan + "_train", "rect_%03d_%d_r5000.png" % (vid + 1, light))
            imgs.append(np.array(Image.open(fn), dtype=np.float32) / 255.)
            lines = _cam_lines(os.path.join(self.datapath, "Cameras", "train", "%08d_cam.txt" % vid))
            extr, intr = _matrix(lines[1:5], 4), _matrix(lines[7:10], 3)
            dmin, dint = float(lines[11].split()[0]), float(lines[11].split()[1]) * self.interval_scale
            p = np.zeros((2, 4, 4), np.float32)
            p[0, :4, :4] = extr
            p[1, :3, :3] = intr
            projs.append(p)
            if i == 0:
                png = np.array(Image.open(os.path.join(self.datapath, "Depths_raw", scan, "depth_visual_%04d.png" % vid)),
                               dtype=np.float32)
                mask = _pyramid(self.prepare((png > 10).astype(np.float32)))
                depth = _pyramid(self.prepare(read_pfm(os.path.join(self.datapath, "Depths_raw", scan,
                                                                    "depth_map_%04d.pfm" % vid))))
                values = np.arange(dmin, dint * self.ndepths + dmin, dint, dtype=np.float32)
        return {"imgs": np.stack(imgs).transpose([0, 3, 1, 2]), "proj_matrix": _stages(np.stack(projs)),
                "depth": depth, "mask": mask, "depth_values": values, "depth_interval": dint}


def gt_pyramid_bld(depth, dmin, dend):
    """(depth pyramid, mask pyramid) of bld_train for a raw map; dmin / dend Python floats. numpy 2 compares a
    float32 array with a Python float in float32: the bounds are rounded first, spelled out here so that the
    rule does not depend on the numpy at hand."""
    mask = np.array((depth >= np.float32(dmin)) & (depth <= np.float32(dend)), dtype=np.float32)
    return _pyramid(depth), _pyramid(mask)


def gt_pyramid_dtu(depth, png, target_hw):
    ref = DtuRef.__new__(DtuRef)
    ref.target_hw = target_hw
    return _pyramid(ref.prepare(depth)), _pyramid(ref.prepare((png.astype(np.float32) > 10).astype(np.float32)))


def depth_eval_metrics(est, gt, mask):
    """train.py:216-228 in float64 on the float32 errors |est - gt|: the twelve scalars, in order."""
    valid = mask > 0.5
    err = np.abs(est.astype(np.float32) - gt.astype(np.float32))[valid]  # float32, as the kernel and torch
    e64 = err.astype(np.float64)
    n = err.size
    out = [e64.sum() / n if n else np.nan]
    for t in (2, 4, 8, 14, 20):
        out.append((err > np.float32(t)).sum() / n if n else np.nan)
    for lo, hi in ((0, 2), (2, 4), (4, 8), (8, 14), (14, 20), (20, 1e5)):
        sel = e64[(err >= np.float32(lo)) & (err <= np.float32(hi))]
        out.append(sel.sum() / sel.size if sel.size else 0.0)
    return np.array(out, np.float64)
