"""COLMAP sparse models on the host: cameras / images / points3D as .bin or .txt in, plain numpy arrays out.

  read_raw(path)     the three files as dictionaries keyed by COLMAP's ids, .bin preferred over .txt
  read_model(path)   what view selection needs: views 0..V-1 in ascending IMAGE_ID, points 0..P-1 in ascending
                     POINT3D_ID, fp64 poses (R maps world to camera: X_cam = R X + t, centre C = -R^T t), 3 x 3
                     intrinsics, and the observations as unique int32 (view, point) pairs
  write_raw(...)     the writer of both formats (synthetic.write_colmap_model and the tests use it)

Only undistorted models are accepted (PINHOLE, SIMPLE_PINHOLE). Every problem with a file -- truncated, an unknown
camera model id, an image whose camera is missing -- is a ValueError that names the file.

Formats. Text: '#' lines are comments; cameras.txt 'CAMERA_ID MODEL WIDTH HEIGHT PARAMS...'; images.txt two lines
per image, 'IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME' then 'X Y POINT3D_ID' triples (possibly none; -1 = no
3-D point); points3D.txt 'POINT3D_ID X Y Z R G B ERROR (IMAGE_ID POINT2D_IDX)...'. Binary: little-endian, packed;
cameras.bin uint64 n, then int32 id, int32 model, uint64 width, uint64 height, double params[k]; images.bin uint64
n, then int32 id, double q[4], double t[3], int32 camera, the name up to a NUL, uint64 m, m x (double x, double y,
int64 point3D); points3D.bin uint64 n, then uint64 id, double xyz[3], uint8 rgb[3], double error, uint64 k,
k x (int32 image, int32 point2D).
"""
from __future__ import annotations

import os
import struct

import numpy as np

# model id -> (name, number of parameters)
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5),
                 4: ("OPENCV", 8), 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5),
                 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
MODEL_IDS = {name: (mid, n) for mid, (name, n) in CAMERA_MODELS.items()}


# ------------------------------------------------------------------ binary
class _Bin:
    """A little-endian cursor over one file's bytes; reading past the end is a ValueError naming the file."""

    def __init__(self, filename):
        self.filename = filename
        with open(filename, "rb") as f:
            self.data = f.read()
        self.pos = 0

    def take(self, fmt):
        size = struct.calcsize("<" + fmt)
        if self.pos + size > len(self.data):
            raise ValueError(f"{self.filename}: truncated (needs {size} bytes at offset {self.pos}, has "
                             f"{len(self.data) - self.pos})")
        out = struct.unpack_from("<" + fmt, self.data, self.pos)
        self.pos += size
        return out

    def array(self, dtype, count):
        dtype = np.dtype(dtype)
        size = dtype.itemsize * count
        if count < 0 or self.pos + size > len(self.data):
            raise ValueError(f"{self.filename}: truncated (needs {size} bytes at offset {self.pos}, has "
                             f"{len(self.data) - self.pos})")
        out = np.frombuffer(self.data, dtype, count, self.pos).copy()
        self.pos += size
        return out

    def name(self):
        end = self.data.find(b"\0", self.pos)
        if end < 0:
            raise ValueError(f"{self.filename}: truncated (an image name without its NUL at offset {self.pos})")
        out = self.data[self.pos:end].decode("utf-8")
        self.pos = end + 1
        return out


_OBS2D = np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")])


def _read_cameras_bin(filename):
    b, cams = _Bin(filename), {}
    for _ in range(b.take("Q")[0]):
        cid, model, width, height = b.take("iiQQ")
        if model not in CAMERA_MODELS:
            raise ValueError(f"{filename}: camera {cid} has the unknown model id {model}")
        name, k = CAMERA_MODELS[model]
        cams[cid] = (name, int(width), int(height), b.array("<f8", k))
    return cams


def _read_images_bin(filename):
    b, images = _Bin(filename), {}
    for _ in range(b.take("Q")[0]):
        iid, = b.take("i")
        q, t = b.array("<f8", 4), b.array("<f8", 3)
        cam, = b.take("i")
        name = b.name()
        obs = b.array(_OBS2D, b.take("Q")[0])
        images[iid] = (q, t, cam, name, np.stack([obs["x"], obs["y"]], 1).reshape(-1, 2), obs["id"].astype(np.int64))
    return images


def _read_points_bin(filename):
    b, points = _Bin(filename), {}
    for _ in range(b.take("Q")[0]):  # one unpack per record: models hold millions of points
        pid, x, y, z, r, g, bl, err, k = b.take("Q3d3BdQ")
        points[pid] = (np.array([x, y, z], np.float64), np.array([r, g, bl], np.uint8), err,
                       b.array("<i4", 2 * k).reshape(-1, 2))
    return points


# ------------------------------------------------------------------ text
def _data_lines(filename):
    with open(filename) as f:
        return [ln.rstrip("\r\n") for ln in f if not ln.lstrip().startswith("#")]


def _read_cameras_txt(filename):
    cams = {}
    for ln in _data_lines(filename):
        f = ln.split()
        if not f:
            continue
        try:
            cid, name, width, height = int(f[0]), f[1], int(f[2]), int(f[3])
            params = np.array([float(x) for x in f[4:]], np.float64)
        except (ValueError, IndexError):
            raise ValueError(f"{filename}: malformed camera line {ln!r}") from None
        if name not in MODEL_IDS:
            raise ValueError(f"{filename}: camera {cid} has the unknown model {name}")
        if params.size != MODEL_IDS[name][1]:
            raise ValueError(f"{filename}: truncated (camera {cid}, {name}, has {params.size} parameters, needs "
                             f"{MODEL_IDS[name][1]})")
        cams[cid] = (name, width, height, params)
    return cams


def _read_images_txt(filename):
    lines, images, i = _data_lines(filename), {}, 0
    while i < len(lines):
        f = lines[i].split()
        i += 1
        if not f:
            continue  # blank lines between images; an image's (possibly empty) second line is consumed below
        try:
            if len(f) < 10:
                raise IndexError
            iid, cam = int(f[0]), int(f[8])
            q, t = np.array([float(x) for x in f[1:5]], np.float64), np.array([float(x) for x in f[5:8]], np.float64)
            name = lines[i - 1].split(None, 9)[9].strip()
            g = lines[i].split() if i < len(lines) else []
            i += 1
            if len(g) % 3:
                raise IndexError
            xy = np.array([float(x) for k, x in enumerate(g) if k % 3 != 2], np.float64).reshape(-1, 2)
            ids = np.array([int(x) for x in g[2::3]], np.int64)
        except (ValueError, IndexError):
            raise ValueError(f"{filename}: truncated or malformed entry at line {lines[i - 1]!r}") from None
        images[iid] = (q, t, cam, name, xy, ids)
    return images


def _read_points_txt(filename):
    points = {}
    for ln in _data_lines(filename):
        f = ln.split()
        if not f:
            continue
        try:
            if len(f) < 8 or len(f) % 2:
                raise IndexError
            pid = int(f[0])
            xyz = np.array([float(x) for x in f[1:4]], np.float64)
            rgb = np.array([int(x) for x in f[4:7]], np.uint8)
            err = float(f[7])
            track = np.array([int(x) for x in f[8:]], np.int32).reshape(-1, 2)
        except (ValueError, IndexError, OverflowError):
            raise ValueError(f"{filename}: truncated or malformed point line {ln[:80]!r}") from None
        points[pid] = (xyz, rgb, err, track)
    return points


_READERS = {"cameras": (_read_cameras_bin, _read_cameras_txt), "images": (_read_images_bin, _read_images_txt),
            "points3D": (_read_points_bin, _read_points_txt)}


def read_raw(path):
    """(cameras, images, points3D) of the model folder `path`, each a dictionary by COLMAP id:
    cameras[id] = (model name, width, height, params float64); images[id] = (q [4] (w, x, y, z), t [3],
    camera id, name, xy [m, 2], point3D ids [m] int64); points3D[id] = (xyz [3], rgb [3] uint8, error,
    track [k, 2] int32). For each file .bin is read when it exists, else .txt."""
    out = []
    for stem, (read_bin, read_txt) in _READERS.items():
        fb, ft = os.path.join(path, stem + ".bin"), os.path.join(path, stem + ".txt")
        if os.path.exists(fb):
            out.append(read_bin(fb))
        elif os.path.exists(ft):
            out.append(read_txt(ft))
        else:
            raise ValueError(f"{path}: neither {stem}.bin nor {stem}.txt")
    return tuple(out)


def _images_file(path):
    fb = os.path.join(path, "images.bin")
    return fb if os.path.exists(fb) else os.path.join(path, "images.txt")


def quat_to_rot(q):
    """R of the Hamilton unit quaternion q = (w, x, y, z), fp64 (q is normalised first)."""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)


def intrinsics(model, params, image="", filename=""):
    """The 3 x 3 fp64 K of a PINHOLE (fx, fy, cx, cy) or SIMPLE_PINHOLE (f, cx, cy) camera."""
    if model == "PINHOLE":
        fx, fy, cx, cy = params
    elif model == "SIMPLE_PINHOLE":
        (fx, cx, cy), fy = params, params[0]
    else:
        raise ValueError(f"{filename}: image {image!r} uses a {model} camera; only PINHOLE and SIMPLE_PINHOLE are "
                         "accepted -- run COLMAP's image undistorter (colmap image_undistorter) first")
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], np.float64)


def read_model(path):
    """The model folder `path` as arrays: {"image_ids" [V] int64 ascending, "names" (list of V), "camera_ids" [V],
    "sizes" [V, 2] (width, height), "K" [V, 3, 3], "q" [V, 4], "t" [V, 3], "R" [V, 3, 3], "centres" [V, 3] (all
    float64), "point_ids" [P] int64 ascending, "xyz" [P, 3] float64, "rgb" [P, 3] uint8, "error" [P], "obs"
    [M, 2] int32 unique (view, point) pairs in lexicographic order}. Observations come from the images' 2-D points
    whose POINT3D_ID is not -1 and is present in points3D."""
    cameras, images, points = read_raw(path)
    fn = _images_file(path)
    image_ids = np.array(sorted(images), np.int64)
    point_ids = np.array(sorted(points), np.int64)
    v, p = len(image_ids), len(point_ids)
    out = {"image_ids": image_ids, "names": [], "camera_ids": np.zeros(v, np.int64), "sizes": np.zeros((v, 2), np.int64),
           "K": np.zeros((v, 3, 3)), "q": np.zeros((v, 4)), "t": np.zeros((v, 3)), "R": np.zeros((v, 3, 3)),
           "centres": np.zeros((v, 3)), "point_ids": point_ids,
           "xyz": np.array([points[i][0] for i in point_ids], np.float64).reshape(p, 3),
           "rgb": np.array([points[i][1] for i in point_ids], np.uint8).reshape(p, 3),
           "error": np.array([points[i][2] for i in point_ids], np.float64)}
    obs = []
    for k, iid in enumerate(image_ids):
        q, t, cam, name, _, ids = images[int(iid)]
        if cam not in cameras:
            raise ValueError(f"{fn}: image {name!r} (id {iid}) names camera {cam}, which the cameras file lacks")
        model, width, height, params = cameras[cam]
        out["K"][k] = intrinsics(model, params, name, fn)
        out["names"].append(name)
        out["camera_ids"][k], out["sizes"][k] = cam, (width, height)
        out["q"][k], out["t"][k] = q, t
        out["R"][k] = quat_to_rot(q)
        out["centres"][k] = -out["R"][k].T @ t
        ids = np.unique(ids[ids != -1])
        if p and ids.size:
            at = np.minimum(np.searchsorted(point_ids, ids), p - 1)
            at = at[point_ids[at] == ids]
            obs.append(np.stack([np.full(at.size, k, np.int64), at], 1))
    out["obs"] = (np.concatenate(obs) if obs else np.zeros((0, 2), np.int64)).astype(np.int32)
    return out


# ------------------------------------------------------------------ writer
def write_raw(path, cameras, images, points3D, binary, image_order=None):
    """Write the three dictionaries of read_raw under `path` as .bin (binary=True) or .txt. Text numbers carry
    the digits that read back the same float64. `image_order` lists the image ids in file order (default: the
    dictionary's)."""
    os.makedirs(path, exist_ok=True)
    order = list(images) if image_order is None else list(image_order)
    num = lambda x: repr(float(x))  # noqa: E731
    if binary:
        with open(os.path.join(path, "cameras.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(cameras)))
            for cid, (name, width, height, params) in cameras.items():
                f.write(struct.pack("<iiQQ", cid, MODEL_IDS[name][0], width, height))
                f.write(np.asarray(params, "<f8").tobytes())
        with open(os.path.join(path, "images.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(order)))
            for iid in order:
                q, t, cam, name, xy, ids = images[iid]
                f.write(struct.pack("<i", iid) + np.asarray(q, "<f8").tobytes() + np.asarray(t, "<f8").tobytes())
                f.write(struct.pack("<i", cam) + name.encode("utf-8") + b"\0" + struct.pack("<Q", len(ids)))
                rec = np.zeros(len(ids), _OBS2D)
                rec["x"], rec["y"], rec["id"] = np.asarray(xy).reshape(-1, 2)[:, 0], np.asarray(xy).reshape(-1, 2)[:, 1], ids
                f.write(rec.tobytes())
        with open(os.path.join(path, "points3D.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(points3D)))
            for pid, (xyz, rgb, err, track) in points3D.items():
                f.write(struct.pack("<Q", pid) + np.asarray(xyz, "<f8").tobytes() + np.asarray(rgb, "u1").tobytes())
                f.write(struct.pack("<dQ", err, len(track)) + np.asarray(track, "<i4").tobytes())
        return
    with open(os.path.join(path, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for cid, (name, width, height, params) in cameras.items():
            f.write(" ".join([str(cid), name, str(width), str(height), *map(num, params)]) + "\n")
    with open(os.path.join(path, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, "
                "NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for iid in order:
            q, t, cam, name, xy, ids = images[iid]
            f.write(" ".join([str(iid), *map(num, q), *map(num, t), str(cam), name]) + "\n")
            f.write(" ".join(f"{num(x)} {num(y)} {int(i)}" for (x, y), i in zip(np.asarray(xy).reshape(-1, 2), ids)) + "\n")
    with open(os.path.join(path, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, "
                "TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for pid, (xyz, rgb, err, track) in points3D.items():
            f.write(" ".join([str(pid), *map(num, xyz), *(str(int(c)) for c in rgb), num(err),
                              *(str(int(x)) for x in np.asarray(track).reshape(-1))]) + "\n")
