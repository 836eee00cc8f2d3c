"""Scan folder(s) -> fused point cloud(s): the reference's test.py (save_scene_depth :74-160, then
gipuma_filter) for DTU and test.py + dynamic_fusion.py (scripts/test_tnt.sh) for Tanks & Temples, in one
process and without the files in between. Depth maps never leave the device between the network and the
fusion kernel.

  postprocess_view     test.py:119-158 + fusibile's decode (main.cpp:126-138) as one tmvs_depth_postprocess
                       launch: conf_final, the masked depth, the PNG's RGBA bytes, fusibile's (B, G, R, depth)
  ViewCache            the dataset readers (general_eval.py:126-210, tnt_eval.py:120-210) with every image
                       decoded, uploaded and resized (tmvs_resize_bilinear_u8) once per scan instead of once
                       per sample; samples equal data.load_sample / load_sample_tnt bitwise
  reconstruct_scan     pair.txt loop -> forward -> postprocess_view into per-scan device slabs ->
                       fusion.fuse (dtu) / dynamic_fusion.fuse_scene (tnt) -> PLY
  python -m transmvsnet_amd.reconstruct   the reference's command line

With save_outputs the files the reference leaves on disk are written too (dtu: camera/*.txt, image/*.png;
tnt: depth_est/, confidence/, cams/, images/ as dynamic_fusion.load_scan reads them), so the from-files
tools (fusibile's inputs read with fusion.read_cam / rgbd_from_images, python -m
transmvsnet_amd.dynamic_fusion) give the same cloud. Scans run one after another, B = 1 per forward.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import data, dynamic_fusion, fusion, ops

CONF_THRESHOLD = 0.01  # test.py:144
DEPTH_MIN, DEPTH_MAX = 425.0, 935.0  # test.py:156


# ------------------------------------------------------------------ the kernel's wrapper
def _dev_f32(t, name, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"postprocess_view: {name} must be a CUDA tensor (HIP kernel; no CPU fallback)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"postprocess_view: {name} must be contiguous float32")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"postprocess_view: {name} must be {list(shape)}, got {list(t.shape)}")
    return t


def _one(t, name):
    """[1, h, w] (a B = 1 forward's output) or [h, w] -> [h, w]."""
    if isinstance(t, torch.Tensor) and t.dim() == 3:
        if t.shape[0] != 1:
            raise ValueError(f"postprocess_view: {name} has batch {t.shape[0]}; one view per call")
        t = t[0]
    return t


def alloc_outputs(h, w, device, image=True):
    """The output buffers of tmvs_depth_postprocess for an H x W view."""
    out = {"conf_final": torch.empty(h, w, device=device), "depth": torch.empty(h, w, device=device)}
    if image:
        out["rgba_u8"] = torch.empty(h, w, 4, dtype=torch.uint8, device=device)
        out["rgbd"] = torch.empty(h, w, 4, device=device)
    return out


def postprocess_view(outputs, image=None, conf_threshold=CONF_THRESHOLD, depth_min=DEPTH_MIN, depth_max=DEPTH_MAX,
                     out=None):
    """test.py:119-158 for one B = 1 forward's output dict, one tmvs_depth_postprocess launch.

    outputs: the dict TransMVSNet.forward returns (depth, photo_confidence and the stage1 / stage2
    photo_confidence at 1/4 and 1/2 size; float32 CUDA tensors, [1, h, w] or [h, w]). image: the reference
    view [3, H, W] RGB in [0, 1] as the network read it, or None. Returns {"conf_final", "depth"} (the
    depth masked to 0 where conf_final < conf_threshold) and, with an image, "rgba_u8" [H, W, 4] uint8 (the
    channels of the reference's PNG) and "rgbd" [H, W, 4] (what fusibile decodes from it: one slot of the
    slab fusion.fuse takes). `out` may hold preallocated tensors under the same keys (alloc_outputs, or
    slots of per-scan slabs); with it the call allocates nothing."""
    depth = _one(outputs["depth"], "depth")
    _dev_f32(depth, "depth")
    if depth.dim() != 2:
        raise ValueError("postprocess_view: depth must be [1, H, W] or [H, W]")
    h, w = depth.shape
    if h % 4 or w % 4:
        raise ValueError(f"postprocess_view: H and W must be multiples of 4, got {h} x {w}")
    conf3 = _dev_f32(_one(outputs["photo_confidence"], "photo_confidence"), "photo_confidence", (h, w))
    conf2 = _dev_f32(_one(outputs["stage2"]["photo_confidence"], "stage2 photo_confidence"),
                     "stage2 photo_confidence", (h // 2, w // 2))
    conf1 = _dev_f32(_one(outputs["stage1"]["photo_confidence"], "stage1 photo_confidence"),
                     "stage1 photo_confidence", (h // 4, w // 4))
    if image is not None:
        _dev_f32(image, "image", (3, h, w))
    if not float(depth_max) > float(depth_min):
        raise ValueError("postprocess_view: depth_max must exceed depth_min")
    given = out if out is not None else {}
    if image is None and ("rgba_u8" in given or "rgbd" in given):
        raise ValueError("postprocess_view: rgba_u8 / rgbd outputs need an image")
    res = dict(alloc_outputs(h, w, depth.device, image is not None), **given)
    _dev_f32(res["conf_final"], "out conf_final", (h, w))
    _dev_f32(res["depth"], "out depth", (h, w))
    rgba = rgbd = None
    if image is not None:
        rgba, rgbd = res["rgba_u8"], _dev_f32(res["rgbd"], "out rgbd", (h, w, 4))
        if not rgba.is_cuda or rgba.dtype != torch.uint8 or not rgba.is_contiguous() or tuple(rgba.shape) != (h, w, 4):
            raise RuntimeError("postprocess_view: out rgba_u8 must be a contiguous uint8 CUDA tensor [H, W, 4]")
    with torch.cuda.device(depth.device):  # the outputs' device and stream
        ops._launch("tmvs_depth_postprocess", depth, conf3, conf2, conf1, image, h, w, float(conf_threshold),
                    float(depth_min), float(depth_max), res["conf_final"], res["depth"], rgba, rgbd)
    return res


# ------------------------------------------------------------------ the GPU resize
class _AxisTables:
    """data.resize_axis tables on the device, one upload per (n_out, n_in)."""

    def __init__(self, device):
        self.device, self.tables = device, {}

    def get(self, n_out, n_in):
        key = (int(n_out), int(n_in))
        if key not in self.tables:
            i0, i1, t = data.resize_axis(*key)
            self.tables[key] = tuple(torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.device)
                                     for a, dt in ((i0, np.int32), (i1, np.int32), (t, np.float32)))
        return self.tables[key]


@ops._on_tensor_device
def resize_image(src, new_w, new_h, tables=None):
    """data.resize_bilinear on the GPU, CHW out. src: a decoded image [h, w, 3] uint8 (CUDA) -- then this
    is resize_bilinear(read_img(file), new_w, new_h) transposed to [3, new_h, new_w], bitwise -- or an
    already loaded float32 image [C, h, w] (the readers' second resize)."""
    if not isinstance(src, torch.Tensor) or not src.is_cuda or not src.is_contiguous():
        raise RuntimeError("resize_image: src must be a contiguous CUDA tensor (HIP kernel; no CPU fallback)")
    new_w, new_h = int(new_w), int(new_h)
    if new_w <= 0 or new_h <= 0:
        raise ValueError("resize_image: the new size must be positive")
    tables = tables if tables is not None else _AxisTables(src.device)
    if src.dtype == torch.uint8:
        if src.dim() != 3 or src.shape[2] != 3:
            raise ValueError("resize_image: a uint8 source must be [h, w, 3]")
        h, w = src.shape[:2]
        x0, x1, tx = tables.get(new_w, w)
        y0, y1, ty = tables.get(new_h, h)
        dst = torch.empty(3, new_h, new_w, device=src.device)
        ops._launch("tmvs_resize_bilinear_u8", src, h, w, x0, x1, tx, y0, y1, ty, new_h, new_w, dst)
        return dst
    if src.dtype != torch.float32 or src.dim() != 3:
        raise ValueError("resize_image: src must be uint8 [h, w, 3] or float32 [C, h, w]")
    c, h, w = src.shape
    x0, x1, tx = tables.get(new_w, w)
    y0, y1, ty = tables.get(new_h, h)
    dst = torch.empty(c, new_h, new_w, device=src.device)
    ops._launch("tmvs_resize_bilinear_f32", src, c, h, w, x0, x1, tx, y0, y1, ty, new_h, new_w, dst)
    return dst


def read_img_u8(filename):
    """The decoded image behind general_eval.read_img: [h, w, 3] uint8 (read_img is this / 255)."""
    from PIL import Image
    a = np.array(Image.open(filename))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{filename}: expected an 8-bit RGB image, got {a.dtype} {a.shape}")
    return a


# ------------------------------------------------------------------ one scan's views
class ViewCache:
    """The views of one scan as the dataset readers prepare them, each read once.

    Per view id: the camera file's extrinsics, the intrinsics scaled as scale_mvs_input scales them
    (data.scale_mvs_camera), the depth range, and -- on first use -- the image decoded once, uploaded as
    uint8 and resized on the GPU to a device [3, h, w] tensor. ``sample(ref, srcs)`` assembles what
    data.load_sample (dataset "dtu") or data.load_sample_tnt ("tnt") returns for the same arguments,
    bitwise: imgs (a device tensor), the three proj_matrix stages and depth_values (host arrays), including
    the second resize of a view whose size differs from the first view's (dtu) or from the run's fixed
    resolution (tnt: `fixed_hw`, set by the first sample when not given and kept, as the reference's
    fix_res; pass one scan's cache.fixed_hw to the next scan's cache)."""

    def __init__(self, datapath, scan, dataset="dtu", device="cuda", nviews=None, ndepths=192, interval_scale=1.0,
                 max_h=864, max_w=1152, image_size=None, fixed_hw=None, inverse_depth=False):
        if dataset not in ("dtu", "tnt"):
            raise ValueError(f"ViewCache: dataset must be 'dtu' or 'tnt', got {dataset!r}")
        self.datapath, self.scan, self.dataset, self.device = datapath, scan, dataset, torch.device(device)
        self.nviews = int(nviews) if nviews is not None else (5 if dataset == "dtu" else 11)
        self.ndepths, self.interval_scale, self.inverse_depth = ndepths, interval_scale, inverse_depth
        if dataset == "tnt":
            max_w, max_h = image_size if image_size is not None else data.TNT_IMAGE_SIZES[scan]
        self.max_w, self.max_h = max_w, max_h
        self.fixed_hw = tuple(fixed_hw) if fixed_hw is not None else None
        self.cams, self.images, self.resized = {}, {}, {}
        self.tables = _AxisTables(self.device)
        self.decoded = 0  # images decoded so far (each view once)

    def _image_file(self, vid):
        if self.dataset == "dtu":
            fn = os.path.join(self.datapath, "{}/images_post/{:0>8}.jpg".format(self.scan, vid))
            if os.path.exists(fn):
                return fn
        return os.path.join(self.datapath, "{}/images/{:0>8}.jpg".format(self.scan, vid))

    def camera(self, vid):
        """{"intr", "extr", "dmin", "dint", "dmax", "hw"}: the view's camera after scale_mvs_input, and the
        (h, w) its image is resized to. Reads the camera file and the image's header only."""
        if vid not in self.cams:
            from PIL import Image
            with Image.open(self._image_file(vid)) as im:
                w, h = im.size
            if self.dataset == "dtu":
                fn = os.path.join(self.datapath, "{}/cams/{:0>8}_cam.txt".format(self.scan, vid))
                intr, extr, dmin, dint = data.read_cam_file(fn, self.ndepths, self.interval_scale)
                dmax = None
            else:
                fn = os.path.join(self.datapath, "{}/cams_1/{:0>8}_cam.txt".format(self.scan, vid))
                intr, extr, dmin, dint, dmax = data.read_cam_file(fn, self.ndepths, tnt=True)
            new_w, new_h, intr = data.scale_mvs_camera(h, w, intr, self.max_w, self.max_h)
            self.cams[vid] = {"intr": intr, "extr": extr, "dmin": dmin, "dint": dint, "dmax": dmax,
                              "hw": (new_h, new_w)}
        return self.cams[vid]

    def image(self, vid, hw=None):
        """The view's image [3, h, w] on the device at its own scaled size, or resized again to `hw`."""
        cam = self.camera(vid)
        if vid not in self.images:
            src = torch.from_numpy(read_img_u8(self._image_file(vid))).to(self.device)
            self.decoded += 1
            self.images[vid] = resize_image(src, cam["hw"][1], cam["hw"][0], self.tables)
        if hw is None or tuple(hw) == cam["hw"]:
            return self.images[vid]
        key = (vid, tuple(hw))
        if key not in self.resized:
            self.resized[key] = resize_image(self.images[vid], hw[1], hw[0], self.tables)
        return self.resized[key]

    def sample(self, ref_view, src_views, images=True):
        """data.load_sample / load_sample_tnt for (ref_view, src_views) from the cache. images=False leaves
        "imgs" out (cameras and depth values only: no decode, no GPU)."""
        nviews = self.nviews if self.dataset == "dtu" else min(self.nviews, len(src_views) + 1)
        view_ids = [ref_view] + list(src_views[:nviews - 1])
        s_hw = self.fixed_hw if self.dataset == "tnt" else None
        imgs, projs, depth_values = [], [], None
        for i, vid in enumerate(view_ids):
            cam = self.camera(vid)
            if s_hw is None:
                s_hw = cam["hw"]
            intr = cam["intr"].copy()
            (c_h, c_w), (s_h, s_w) = cam["hw"], s_hw
            if (c_h, c_w) != (s_h, s_w):
                intr[0, :] *= 1.0 * s_w / c_w
                intr[1, :] *= 1.0 * s_h / c_h
            if images:
                imgs.append(self.image(vid, s_hw))
            p = np.zeros((2, 4, 4), np.float32)
            p[0] = cam["extr"]
            p[1, :3, :3] = intr
            projs.append(p)
            if i == 0:
                dmin, dint, nd = cam["dmin"], cam["dint"], self.ndepths
                if self.dataset == "dtu":
                    depth_values = np.arange(dmin, dint * (nd - 0.5) + dmin, dint, dtype=np.float32)
                elif not self.inverse_depth:
                    depth_values = np.arange(dmin, dint * nd + dmin, dint, dtype=np.float32)
                else:  # tnt_eval.py:181-185
                    depth_end = cam["dmax"] - dint / self.interval_scale
                    depth_values = (1.0 / np.linspace(1.0 / depth_end, 1.0 / dmin, nd, endpoint=False)).astype(
                        np.float32)
        if self.dataset == "tnt" and self.fixed_hw is None:
            self.fixed_hw = s_hw
        proj = np.stack(projs)
        s2, s3 = proj.copy(), proj.copy()
        s2[:, 1, :2, :] = proj[:, 1, :2, :] * 2
        s3[:, 1, :2, :] = proj[:, 1, :2, :] * 4
        out = {"proj_matrix": {"stage1": proj, "stage2": s2, "stage3": s3}, "depth_values": depth_values,
               "filename": self.scan + "/{}/" + "{:0>8}".format(ref_view) + "{}", "hw": tuple(s_hw)}
        if images:
            out["imgs"] = torch.stack(imgs)
        if self.dataset == "tnt":
            out["fixed_hw"] = tuple(s_hw)
        return out


# ------------------------------------------------------------------ writers
def write_cam_tnt(filename, intrinsics, extrinsics, depth_min=0.0, depth_interval=0.0):
    """A camera file in the layout dynamic_fusion.read_camera_parameters reads (extrinsic on lines 1-4,
    intrinsic on lines 7-9), every number with the digits that read back the same float32."""
    with open(filename, "w") as f:
        f.write("extrinsic\n")
        for row in np.asarray(extrinsics, np.float32):
            f.write(" ".join(repr(float(x)) for x in row) + "\n")
        f.write("\nintrinsic\n")
        for row in np.asarray(intrinsics, np.float32)[:3, :3]:
            f.write(" ".join(repr(float(x)) for x in row) + "\n")
        f.write("\n{} {}\n".format(repr(float(depth_min)), repr(float(depth_interval))))


def save_rgba_png(filename, rgba_u8):
    """The reference's image/{:0>8}.png (test.py:153-158): cv2.imwrite of the BGRA array stores the PNG
    channels (R, G, B, alpha = 8-bit depth), which is the rgba_u8 buffer."""
    from PIL import Image
    if isinstance(rgba_u8, torch.Tensor):
        rgba_u8 = rgba_u8.cpu().numpy()
    rgba_u8 = np.ascontiguousarray(rgba_u8, np.uint8)
    if rgba_u8.ndim != 3 or rgba_u8.shape[2] != 4:
        raise ValueError("save_rgba_png: rgba_u8 must be [H, W, 4]")
    Image.fromarray(rgba_u8).save(filename)


def read_rgba_png(filename):
    """What fusibile reads from that PNG (main.cpp:126-138): (BGR uint8 [H, W, 3], depth alpha [H, W])."""
    from PIL import Image
    a = np.array(Image.open(filename))
    return np.ascontiguousarray(a[..., [2, 1, 0]]), np.ascontiguousarray(a[..., 3])


def _save_rgb_jpg(filename, image_chw):
    from PIL import Image
    rgb = (image_chw.permute(1, 2, 0) * 255).clamp(0, 255).to(torch.uint8).cpu().numpy()
    Image.fromarray(rgb).save(filename, quality=95)


class _RefColours:
    """images[slot] for dynamic_fusion.fuse_scene: the reference view [H, W, 3] of slot's sample."""

    def __init__(self, chw):
        self.chw = chw

    def __getitem__(self, slot):
        return self.chw[slot].permute(1, 2, 0)


# ------------------------------------------------------------------ the driver
def reconstruct_scan(model, datapath, scan, dataset="dtu", outdir=None, nviews=None, ndepths=192, interval_scale=1.0,
                     max_h=864, max_w=1152, conf_threshold=CONF_THRESHOLD, consistent_threshold=3,
                     depth_threshold=0.25, photo_threshold=0.3, thres_view=3, subpixel_bits=5, save_outputs=False,
                     image_size=None, fixed_hw=None, device="cuda", on_view=None, verbose=False):
    """One scan folder -> fused point cloud, everything between the forward and the PLY on the device.

    model: any callable with TransMVSNet.forward's signature (imgs [1, N, 3, H, W] on the device,
    proj_matrix {stage: [1, N, 2, 4, 4]} host tensors, depth_values [1, D] on the device) returning its
    output dict. For each reference view of <datapath>/<scan>/pair.txt (sources filled to nviews as
    read_pair_file for dtu, unpadded for tnt) one forward and one postprocess_view into per-scan slabs;
    then dtu: fusion.fuse over the (B, G, R, depth) slab with fusibile's camera parameters of the written
    projection matrices, cloud to <outdir>/<scan>/3d_model.ply; tnt: dynamic_fusion.fuse_scene over the
    depth and confidence slabs with the stage-3 cameras, cloud to <outdir>/<scan>.ply. on_view(slot,
    ref_view, sample, post) is called after each view. Returns {"points", "colors" (tnt) / "textures"
    (dtu), "ply", "views", "depth", "conf", "fixed_hw"}."""
    if not torch.cuda.is_available():
        raise RuntimeError("reconstruct_scan: needs a GPU (HIP kernels; no CPU fallback)")
    if dataset not in ("dtu", "tnt"):
        raise ValueError(f"reconstruct_scan: dataset must be 'dtu' or 'tnt', got {dataset!r}")
    cache = ViewCache(datapath, scan, dataset, device, nviews, ndepths, interval_scale, max_h, max_w, image_size,
                      fixed_hw)
    pair_path = os.path.join(datapath, scan, "pair.txt")
    pairs = data.read_pair_file(pair_path, cache.nviews, pad=dataset == "dtu")
    if not pairs:
        raise ValueError(f"reconstruct_scan: {pair_path} names no reference view with sources")
    views = [ref for ref, _ in pairs]
    slot = {vid: i for i, vid in enumerate(views)}
    if dataset == "tnt":
        for ref, srcs in pairs:
            missing = [s for s in srcs if s not in slot]
            if missing:
                raise ValueError(f"reconstruct_scan: source views {missing} of view {ref} are never reference "
                                 "views, so they get no depth map to check against")
    scan_out = os.path.join(outdir, scan) if outdir is not None else None
    if save_outputs:
        if scan_out is None:
            raise ValueError("reconstruct_scan: save_outputs needs an outdir")
        for sub in (("camera", "image") if dataset == "dtu" else ("depth_est", "confidence", "cams", "images")):
            os.makedirs(os.path.join(scan_out, sub), exist_ok=True)
    name = lambda sub, vid, ext: os.path.join(scan_out, "{}/{:0>8}{}".format(sub, vid, ext))

    dev = cache.device
    depth_slab = conf_slab = rgbd_slab = rgba = None
    ref_cams, ref_imgs = [], []
    with torch.no_grad():
        for i, (ref, srcs) in enumerate(pairs):
            sample = cache.sample(ref, srcs)
            imgs = sample["imgs"]
            h, w = imgs.shape[2:]
            if depth_slab is None:
                v = len(pairs)
                depth_slab, conf_slab = torch.empty(v, h, w, device=dev), torch.empty(v, h, w, device=dev)
                rgbd_slab = torch.empty(v, h, w, 4, device=dev) if dataset == "dtu" else torch.empty(h, w, 4, device=dev)
                rgba = torch.empty(h, w, 4, dtype=torch.uint8, device=dev)
            elif (h, w) != tuple(depth_slab.shape[1:]):
                raise ValueError(f"reconstruct_scan: view {ref} is {h} x {w}, the scan's first view "
                                 f"{tuple(depth_slab.shape[1:])}; the fusion needs one resolution per scan")
            proj = {k: torch.from_numpy(p)[None] for k, p in sample["proj_matrix"].items()}
            dv = torch.from_numpy(sample["depth_values"])[None].to(dev)
            outputs = model(imgs[None], proj, dv)
            post = postprocess_view(outputs, imgs[0], conf_threshold, out={
                "conf_final": conf_slab[i], "depth": depth_slab[i], "rgba_u8": rgba,
                "rgbd": rgbd_slab[i] if dataset == "dtu" else rgbd_slab})
            cam = sample["proj_matrix"]["stage3"][0]
            ref_cams.append(cam)
            ref_imgs.append(imgs[0])
            if save_outputs and dataset == "dtu":
                fusion.write_cam(name("camera", ref, ".txt"), cam)
                save_rgba_png(name("image", ref, ".png"), rgba)
            elif save_outputs:
                data.save_pfm(name("depth_est", ref, ".pfm"), depth_slab[i].cpu().numpy())
                data.save_pfm(name("confidence", ref, ".pfm"), conf_slab[i].cpu().numpy())
                write_cam_tnt(name("cams", ref, "_cam.txt"), cam[1, :3, :3], cam[0],
                              cache.camera(ref)["dmin"], cache.camera(ref)["dint"])
                _save_rgb_jpg(name("images", ref, ".jpg"), imgs[0])
            if on_view is not None:
                on_view(i, ref, sample, post)
            if verbose:
                print("{} view {:0>8} ({}/{}) {}x{}".format(scan, ref, i + 1, len(pairs), h, w), flush=True)

        res = {"views": views, "depth": depth_slab, "conf": conf_slab, "fixed_hw": cache.fixed_hw,
               "decoded": cache.decoded, "ply": None}
        if dataset == "dtu":
            packed = np.stack([fusion.camera_params(fusion.projection_matrix(c).astype(np.float32))[0]
                               for c in ref_cams])
            pts, tex = fusion.fuse(rgbd_slab, packed, consistent_threshold, depth_threshold)
            res.update(points=pts, textures=tex, rgbd=rgbd_slab, cams_packed=packed)
            if scan_out is not None:
                os.makedirs(scan_out, exist_ok=True)
                res["ply"] = os.path.join(scan_out, "3d_model.ply")
                fusion.save_point_cloud(res["ply"], pts.cpu().numpy(), tex.cpu().numpy())
        else:
            ks = np.stack([np.ascontiguousarray(c[1, :3, :3], np.float32) for c in ref_cams])
            es = np.stack([np.ascontiguousarray(c[0], np.float32) for c in ref_cams])
            slot_pairs = [(slot[r], [slot[s] for s in srcs]) for r, srcs in pairs]
            pts, cols = dynamic_fusion.fuse_scene(depth_slab, conf_slab, _RefColours(ref_imgs), ks, es, slot_pairs,
                                                  photo_threshold, thres_view, subpixel_bits)
            res.update(points=pts, colors=cols, Ks=ks, Es=es, pairs=slot_pairs)
            if outdir is not None:
                os.makedirs(outdir, exist_ok=True)
                res["ply"] = os.path.join(outdir, f"{scan}.ply")
                dynamic_fusion.save_ply(res["ply"], pts, cols)
    if verbose and res["ply"]:
        print("saving the final model to", res["ply"], "({} points)".format(len(res["points"])), flush=True)
    return res


# ------------------------------------------------------------------ command line
def make_parser():
    p = argparse.ArgumentParser(description="Predict depth, filter and fuse on the GPU: scan folders to point clouds")
    p.add_argument("--dataset", choices=["dtu", "tnt"], default="dtu",
                   help="dtu: general_eval reader + gipuma fusion; tnt: tnt_eval reader + dynamic fusion")
    p.add_argument("--testpath", help="testing data dir for some scenes")
    p.add_argument("--testpath_single_scene", help="testing data path for single scene")
    p.add_argument("--testlist", default="all", help="testing scene list file, or 'all'")
    p.add_argument("--loadckpt", required=True, help="load a specific checkpoint")
    p.add_argument("--outdir", default="./outputs", help="output dir")
    p.add_argument("--max_h", type=int, default=864, help="testing max h")
    p.add_argument("--max_w", type=int, default=1152, help="testing max w")
    p.add_argument("--num_view", type=int, default=None, help="views per forward (default 5 for dtu, 11 for tnt)")
    p.add_argument("--photo_threshold", type=float, default=0.3, help="tnt: photo threshold for filter confidence")
    p.add_argument("--thres_view", type=int, default=3, help="tnt: threshold of num view")
    p.add_argument("--image_size", type=int, nargs=2, default=None, metavar=("W", "H"),
                   help="tnt: the (max_w, max_h) images are fitted into, for a scan outside data.TNT_IMAGE_SIZES "
                        "(a folder written by transmvsnet_amd.colmap_scene)")
    p.add_argument("--save_outputs", action="store_true",
                   help="also write the per-view files the reference leaves on disk")
    return p


def scan_list(args):
    """test.py:36-37, 166-172: the scans to run."""
    if args.testpath_single_scene:
        args.testpath = os.path.dirname(args.testpath_single_scene)
    if not args.testpath:
        raise SystemExit("reconstruct: --testpath or --testpath_single_scene is required")
    if args.testlist != "all":
        with open(args.testlist) as f:
            return [ln.rstrip() for ln in f.readlines() if ln.strip()]
    if args.testpath_single_scene:
        return [os.path.basename(args.testpath_single_scene)]
    return sorted(e for e in os.listdir(args.testpath) if os.path.isdir(os.path.join(args.testpath, e)))


def load_model(ckpt, device="cuda"):
    """test.py:83-91: TransMVSNet with state_dict['model'], strict."""
    from .model import TransMVSNet
    model = TransMVSNet().eval()
    state = torch.load(ckpt, map_location=torch.device("cpu"))
    model.load_state_dict(state["model"], strict=True)
    return model.to(device)


def main(argv=None):
    args = make_parser().parse_args(argv)
    scans = scan_list(args)
    model = load_model(args.loadckpt)
    fixed_hw = None
    for scan in scans:  # sequentially: one process holds the GPU
        res = reconstruct_scan(model, args.testpath, scan, args.dataset, args.outdir, nviews=args.num_view,
                               max_h=args.max_h, max_w=args.max_w, photo_threshold=args.photo_threshold,
                               thres_view=args.thres_view, save_outputs=args.save_outputs, fixed_hw=fixed_hw,
                               image_size=tuple(args.image_size) if args.image_size else None, verbose=True)
        fixed_hw = res["fixed_hw"]


if __name__ == "__main__":
    main()
