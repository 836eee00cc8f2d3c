"""The Tanks & Temples output path: the reference's dynamic_fusion.py (run by scripts/test_tnt.sh with
--photo_threshold 0.18 --thres_view 5) with its per-view filter as the HIP kernel
``tmvs_dynamic_fusion`` (csrc/dynamic_fusion.hip), one launch per reference view.

  pair_constants / ref_constants   the float32 matrices of reproject_with_depth (:85-106) and of the
                                   final back-projection (:259-262), composed with numpy as the reference
  filter_view                      filter_depth's per-view body (:182-262) on the GPU
  fuse_scene                       filter_depth's loop over the pair list (:152-268), from arrays
  read_camera_parameters           :33-49      align_image  :162-176      save_ply  :269-279
  fuse_scan                        filter_depth from a scan folder, plus the three mask PNGs (:234-238)
  python -m transmvsnet_amd.dynamic_fusion   the reference's command line, minus --display

The reference's worker (:282-289) does nothing unless --test_dataset is dtu; here both datasets run:
dtu writes <outdir>/mvsnet_{id:03d}_l3.ply as the reference, tnt writes <outdir>/<scan>.ply, and
--photo_threshold applies to both (the reference hard-codes 0.3 for dtu, which is the default).
Scans run one after another in this process (no multiprocessing.Pool: one process holds the GPU).

The reference samples the source depth with cv2.remap(INTER_LINEAR); cv2 is absent here, so
``subpixel_bits=5`` restates OpenCV's fixed-point path from its documentation (coordinates rounded
to 1/32 pixel) and is not pinned against cv2 itself; ``subpixel_bits=0`` uses exact fractions.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import data, ops
from ._lib import (DYNFUSE_FINAL, DYNFUSE_GEO, DYNFUSE_MAX_SRC, DYNFUSE_PAIR_FLOATS, DYNFUSE_PHOTO,
                   DYNFUSE_REF_FLOATS)


# ------------------------------------------------------------------ host-side matrices
def pair_constants(K_ref, E_ref, K_src, E_src):
    """The packed float32 block of one (reference, source) pair (include/transmvs.h
    TMVS_DYNFUSE_PAIR_FLOATS): inv(K_ref), rows 0-2 of E_src @ inv(E_ref), K_src, inv(K_src), rows 0-2
    of E_ref @ inv(E_src), K_ref -- np.linalg.inv and @ on float32, as reproject_with_depth."""
    K_ref, E_ref = np.asarray(K_ref, np.float32), np.asarray(E_ref, np.float32)
    K_src, E_src = np.asarray(K_src, np.float32), np.asarray(E_src, np.float32)
    pk = np.zeros(DYNFUSE_PAIR_FLOATS, np.float32)
    pk[0:9] = np.linalg.inv(K_ref).reshape(-1)
    pk[9:21] = np.matmul(E_src, np.linalg.inv(E_ref))[:3].reshape(-1)
    pk[21:30] = K_src.reshape(-1)
    pk[30:39] = np.linalg.inv(K_src).reshape(-1)
    pk[39:51] = np.matmul(E_ref, np.linalg.inv(E_src))[:3].reshape(-1)
    pk[51:60] = K_ref.reshape(-1)
    return pk


def ref_constants(K_ref, E_ref):
    """The reference camera block (TMVS_DYNFUSE_REF_FLOATS): inv(K_ref), rows 0-2 of inv(E_ref)."""
    pk = np.zeros(DYNFUSE_REF_FLOATS, np.float32)
    pk[0:9] = np.linalg.inv(np.asarray(K_ref, np.float32)).reshape(-1)
    pk[9:21] = np.linalg.inv(np.asarray(E_ref, np.float32))[:3].reshape(-1)
    return pk


def _check_views(n_views, ref, srcs):
    srcs = [int(s) for s in srcs]
    if not 0 <= int(ref) < n_views:
        raise ValueError(f"dynamic fusion: reference view {ref} outside [0, {n_views})")
    if not 1 <= len(srcs) <= DYNFUSE_MAX_SRC:
        raise ValueError(f"dynamic fusion: {len(srcs)} source views; the reference's nine tolerance levels "
                         f"allow 1..{DYNFUSE_MAX_SRC}")
    for s in srcs:
        if not 0 <= s < n_views or s == int(ref):
            raise ValueError(f"dynamic fusion: source view {s} must be in [0, {n_views}) and differ from the "
                             f"reference view {ref}")
    return srcs


def view_constants(Ks, Es, ref, srcs, device):
    """Device-side constants of one reference view: (src_views int32 [S], pair blocks [S, 64], reference
    block [24]). Validates the view indices (the C entry point cannot read the device index array)."""
    srcs = _check_views(len(Ks), ref, srcs)
    pairs = np.stack([pair_constants(Ks[ref], Es[ref], Ks[s], Es[s]) for s in srcs])
    return (torch.tensor(srcs, dtype=torch.int32, device=device), torch.from_numpy(pairs).to(device),
            torch.from_numpy(ref_constants(Ks[ref], Es[ref])).to(device))


def alloc_outputs(h, w, device):
    """The four output buffers of tmvs_dynamic_fusion for an H x W view."""
    return {"geo_count": torch.empty(h, w, dtype=torch.uint8, device=device),
            "mask": torch.empty(h, w, dtype=torch.uint8, device=device),
            "depth_avg": torch.empty(h, w, dtype=torch.float32, device=device),
            "xyz": torch.empty(h, w, 3, dtype=torch.float32, device=device)}


# ------------------------------------------------------------------ the GPU filter
@ops._on_tensor_device
def filter_view(depths, confidence, Ks, Es, ref, srcs, photo_threshold=0.3, thres_view=3, subpixel_bits=5,
                consts=None, out=None):
    """filter_depth's body for one reference view (:182-262) as one tmvs_dynamic_fusion launch.

    depths [V, H, W] and confidence [H, W]: float32 CUDA tensors; Ks [V, 3, 3], Es [V, 4, 4]: host
    arrays; srcs: 1..10 view indices in pair-file order. Returns device tensors geo_count (uint8, sources
    passing the loosest level), photo / geo / final (bool), depth_avg, xyz [H, W, 3] (world point where
    final, 0 elsewhere) and the raw bit mask. `consts` (view_constants) and `out` (alloc_outputs) may
    be passed in; with both the call allocates no kernel argument and copies nothing from the host."""
    for t, name in ((depths, "depths"), (confidence, "confidence")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"filter_view: {name} must be a CUDA tensor (HIP kernel; no CPU fallback)")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"filter_view: {name} must be contiguous float32")
    if depths.dim() != 3 or confidence.shape != depths.shape[1:]:
        raise ValueError("filter_view: depths must be [V, H, W] and confidence [H, W]")
    v, h, w = depths.shape
    srcs = _check_views(v, ref, srcs)
    if int(thres_view) < 1 or subpixel_bits not in (0, 5):
        raise ValueError("filter_view: thres_view >= 1 and subpixel_bits in {0, 5}")
    idx, pairs, rblk = consts if consts is not None else view_constants(Ks, Es, ref, srcs, depths.device)
    if idx.numel() != len(srcs) or pairs.numel() != len(srcs) * DYNFUSE_PAIR_FLOATS:
        raise ValueError("filter_view: consts do not match srcs")
    if out is None:
        out = alloc_outputs(h, w, depths.device)
    ops._launch("tmvs_dynamic_fusion", depths, v, h, w, int(ref), idx, len(srcs), pairs, rblk, confidence,
                float(photo_threshold), int(thres_view), int(subpixel_bits), out["geo_count"], out["mask"],
                out["depth_avg"], out["xyz"])
    m = out["mask"]
    return {"geo_count": out["geo_count"], "photo": (m & DYNFUSE_PHOTO) != 0, "geo": (m & DYNFUSE_GEO) != 0,
            "final": (m & DYNFUSE_FINAL) != 0, "depth_avg": out["depth_avg"], "xyz": out["xyz"], "mask": m}


def fuse_scene(depths, confidences, images, Ks, Es, pairs, photo_threshold=0.3, thres_view=3, subpixel_bits=5,
               on_view=None):
    """filter_depth's loop (:152-268) from arrays: depths / confidences [V, H, W] and images [V, H, W, 3]
    (RGB in [0, 1], aligned to the depth maps) as CUDA tensors or arrays, Ks / Es per view (a sequence
    indexed by view, or a callable ref -> (Ks, Es) when the cameras depend on the reference view as in
    fuse_scan), pairs [(ref, [src...])]. Views are concatenated in pair order, pixels within a view in
    pixel order. Returns (points [N, 3] float32, colors [N, 3] uint8) as device tensors.
    on_view(ref, result) is called after each view (fuse_scan writes the mask images from it)."""
    if not torch.cuda.is_available():
        raise RuntimeError("fuse_scene: needs a GPU (HIP kernel; no CPU fallback)")
    dev = depths.device if isinstance(depths, torch.Tensor) and depths.is_cuda else torch.device("cuda")
    up = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float32))
                    ).to(dev).float().contiguous()
    depths, confidences = up(depths), up(confidences)
    h, w = depths.shape[1:]
    pts, cols = [], []
    for ref, srcs in pairs:
        ks, es = (Ks(ref), Es(ref)) if callable(Ks) else (Ks, Es)
        r = filter_view(depths, confidences[ref], ks, es, ref, srcs, photo_threshold, thres_view, subpixel_bits)
        keep = r["final"]
        img = images[ref]
        img = up(img) if not (isinstance(img, torch.Tensor) and img.is_cuda) else img.float()
        pts.append(r["xyz"][keep])
        cols.append((img[keep] * 255).to(torch.uint8))  # (img * 255).astype(uint8) (:264): truncation
        if on_view is not None:
            on_view(ref, r)
    if not pts:
        return (torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.uint8, device=dev))
    return torch.cat(pts), torch.cat(cols)


# ------------------------------------------------------------------ host readers / writers
def read_camera_parameters(filename, scale, index, flag):
    """dynamic_fusion.read_camera_parameters (:33-49): extrinsics from lines [1, 5), intrinsics from lines
    [7, 10), float32; K[:2] *= scale, then the crop offset `index` leaves cx (flag 0) or cy (flag 1)."""
    with open(filename) as f:
        lines = [ln.rstrip() for ln in f.readlines()]
    extrinsics = np.array(" ".join(lines[1:5]).split(), np.float32).reshape(4, 4)
    intrinsics = np.array(" ".join(lines[7:10]).split(), np.float32).reshape(3, 3)
    intrinsics[:2, :] *= scale
    if flag == 0:
        intrinsics[0, 2] -= index
    else:
        intrinsics[1, 2] -= index
    return intrinsics, extrinsics


def align_image(img, depth_shape):
    """filter_depth's image alignment (:162-176): scale the image to the depth map's height (or, when
    that leaves it too narrow, to its width), then crop the other axis centrally to the depth map.
    Returns (img, scale, index, flag) -- the arguments read_camera_parameters takes."""
    dh, dw = int(depth_shape[0]), int(depth_shape[1])
    ih, iw = img.shape[:2]
    scale = float(dh) / ih
    index = int((int(iw * scale) - dw) / 2)
    index_p = (int(iw * scale) - dw) - index
    flag = 0
    if dw / iw > scale:
        scale = float(dw) / iw
        index = int((int(ih * scale) - dh) / 2)
        index_p = (int(ih * scale) - dh) - index
        flag = 1
    img = data.resize_bilinear(img, int(iw * scale), int(ih * scale))
    if flag == 0:
        img = img[:, index:img.shape[1] - index_p]
    else:
        img = img[index:img.shape[0] - index_p]
    return img, scale, index, flag


def read_pair_file(filename):
    """dynamic_fusion.read_pair_file (:65-75): views without sources are skipped, nothing is padded."""
    return data.read_pair_file(filename, pad=False)


def save_ply(filename, points, colors):
    """The PLY plyfile writes for filter_depth's vertex element (:269-279): binary little-endian, float
    x y z and uchar red green blue, 15 bytes per vertex."""
    if isinstance(points, torch.Tensor):
        points = points.detach().cpu().numpy()
    if isinstance(colors, torch.Tensor):
        colors = colors.detach().cpu().numpy()
    x = np.asarray(points, np.float32).reshape(-1, 3)
    c = np.asarray(colors, np.uint8).reshape(-1, 3)
    if len(x) != len(c):
        raise ValueError("save_ply: points and colors differ in length")
    rec = np.empty(len(x), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"),
                                  ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = x[:, 0], x[:, 1], x[:, 2]
    rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    with open(filename, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                 "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
                 % len(x)).encode("ascii"))
        f.write(rec.tobytes())


def _save_mask(filename, mask):
    from PIL import Image
    Image.fromarray(mask.to(torch.uint8).mul(255).cpu().numpy()).save(filename)


def load_scan(scan_folder, pairs):
    """Read what filter_depth reads for the views `pairs` names: depth_est/, confidence/, images/ and
    cams/ of the scan folder. Returns (view ids, depths [V, H, W], confidences {slot: [H, W]}, images
    {slot: aligned [H, W, 3]}, cams(ref slot) -> (Ks, Es), pairs in slot indices). As in the reference,
    the cameras of every view of a pair are scaled and shifted by the REFERENCE view's image alignment."""
    ids = []
    for ref, srcs in pairs:
        for vid in [ref] + list(srcs):
            if vid not in ids:
                ids.append(vid)
    slot = {vid: i for i, vid in enumerate(ids)}
    name = lambda sub, vid, ext: os.path.join(scan_folder, "{}/{:0>8}{}".format(sub, vid, ext))
    depths = np.stack([np.ascontiguousarray(data.read_pfm(name("depth_est", vid, ".pfm"))[0], np.float32)
                       for vid in ids])
    confs, imgs, align = {}, {}, {}
    for ref, _ in pairs:
        conf = np.ascontiguousarray(data.read_pfm(name("confidence", ref, ".pfm"))[0], np.float32)
        img, scale, index, flag = align_image(data.read_img(name("images", ref, ".jpg")), conf.shape)
        confs[slot[ref]], imgs[slot[ref]], align[slot[ref]] = conf, np.ascontiguousarray(img), (scale, index, flag)
    cache = {}

    def cams(ref_slot):
        key = align[ref_slot]
        if key not in cache:
            ke = [read_camera_parameters(name("cams", vid, "_cam.txt"), *key) for vid in ids]
            cache[key] = (np.stack([k for k, _ in ke]), np.stack([e for _, e in ke]))
        return cache[key]

    return ids, depths, confs, imgs, cams, [(slot[r], [slot[s] for s in srcs]) for r, srcs in pairs]


def fuse_scan(scan_folder, pair_path, ply_path, out_folder=None, photo_threshold=0.3, thres_view=3, subpixel_bits=5,
              verbose=False):
    """filter_depth (:142-280) from files: every depth map is uploaded once, every reference view of the
    pair file is filtered on the GPU, the fused cloud goes to `ply_path` and, with `out_folder`, the
    photo / geo / final masks to <out_folder>/mask/{view:0>8}_{photo,geo,final}.png. Returns
    (points, colors) as device tensors."""
    if not torch.cuda.is_available():
        raise RuntimeError("fuse_scan: needs a GPU (HIP kernel; no CPU fallback)")
    pairs = read_pair_file(pair_path)
    ids, depths, confs, imgs, cams, slot_pairs = load_scan(scan_folder, pairs)
    dev = torch.device("cuda")
    depths_d = torch.from_numpy(depths).to(dev)
    conf_d = torch.zeros_like(depths_d)
    for s, c in confs.items():
        conf_d[s] = torch.from_numpy(c).to(dev)
    if out_folder is not None:
        os.makedirs(os.path.join(out_folder, "mask"), exist_ok=True)

    def on_view(ref_slot, r):
        if out_folder is not None:
            for kind in ("photo", "geo", "final"):
                _save_mask(os.path.join(out_folder, "mask/{:0>8}_{}.png".format(ids[ref_slot], kind)), r[kind])
        if verbose:
            print("processing {}, ref-view{:0>2}, photo/geo/final-mask:{}/{}/{}".format(
                scan_folder, ids[ref_slot], *(r[k].float().mean().item() for k in ("photo", "geo", "final"))))

    pts, cols = fuse_scene(depths_d, conf_d, imgs, lambda r: cams(r)[0], lambda r: cams(r)[1], slot_pairs,
                           photo_threshold, thres_view, subpixel_bits, on_view=on_view)
    os.makedirs(os.path.dirname(os.path.abspath(ply_path)), exist_ok=True)
    save_ply(ply_path, pts, cols)
    if verbose:
        print("saving the final model to", ply_path)
    return pts, cols


# ------------------------------------------------------------------ command line
def worker(scan, args):
    """dynamic_fusion.worker (:282-289) for one scan, both datasets. Returns the PLY's path."""
    scan_folder = os.path.join(args.testpath, scan)
    out_folder = os.path.join(args.outdir, scan)
    pair_path = os.path.join(args.tntpath, f"{scan}/pair.txt")
    if args.test_dataset == "dtu":
        ply = os.path.join(args.outdir, "mvsnet_{:0>3}_l3.ply".format(int(scan[4:])))
    else:
        ply = os.path.join(args.outdir, f"{scan}.ply")
    fuse_scan(scan_folder, pair_path, ply, out_folder, args.photo_threshold, args.thres_view,
              getattr(args, "subpixel_bits", 5), verbose=getattr(args, "verbose", False))
    return ply


def make_parser():
    p = argparse.ArgumentParser(description="Filter and fuse depth maps (dynamic geometric consistency) on the GPU")
    p.add_argument("--testpath", required=True, help="testing data path (the scans' depth_est/, confidence/, ...)")
    p.add_argument("--tntpath", required=True, help="data path holding <scan>/pair.txt")
    p.add_argument("--testlist", required=True, help="testing scan list")
    p.add_argument("--outdir", required=True, help="output dir")
    p.add_argument("--photo_threshold", type=float, default=0.3, help="photo threshold for filter confidence")
    p.add_argument("--test_dataset", choices=["dtu", "tnt"], required=True, help="which dataset to evaluate")
    p.add_argument("--thres_view", type=int, default=3, help="threshold of num view")
    p.add_argument("--subpixel_bits", type=int, choices=[0, 5], default=5,
                   help="5: cv2.remap's 1/32-pixel sampling (the reference); 0: exact bilinear fractions")
    return p


def main(argv=None):
    args = make_parser().parse_args(argv)
    args.verbose = True
    with open(args.testlist) as f:
        scans = [ln.rstrip() for ln in f.readlines() if ln.strip()]
    for scan in scans:  # sequentially: one process holds the GPU
        worker(scan, args)


if __name__ == "__main__":
    main()
