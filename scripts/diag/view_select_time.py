"""COLMAP scene import at the size of a Tanks-and-Temples model: V = 300 views on a ring, P = 10^6 points, each seen
by a run of neighbouring views (track length 2 + Poisson(6), mean about 8). Timed on the GPU, after warm-up, as the
median of the repeats: tmvs_vs_pair_scores alone (device events), colmap_scene.select (uploads, depths, sorts, bit
matrix, scores, ranking, downloads; host clock round a synchronise), and once colmap_scene.convert from .bin files
without image copying, with the share colmap.read_model takes. The numpy restatement (tests/_view_select_ref.py)
is timed on a model of the same construction with --ref-points points (default: the same 10^6, where it takes well
under a minute because it is vectorised over the points and skips the pairs without a common point) and compared
with the GPU's answer there. A record, not a test.
Usage: view_select_time.py [--out profiles/view_select_time.json] [--views 300] [--points 1000000] [--ref-points 1000000]"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from tests import _view_select_ref as ref
from transmvsnet_amd import colmap, colmap_scene, synthetic, view_select


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def ring_model(v, p, seed=0):
    """Arrays of colmap.read_model's layout: cameras on a ring of radius 30 looking at the origin, points in a
    ball of radius 8, each seen by 2 + Poisson(6) neighbouring views round a random one."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(v) / v
    centres = np.stack([30 * np.cos(ang), 30 * np.sin(ang), rng.uniform(-2, 2, v)], 1)
    R = np.stack([synthetic._look_at(c, np.zeros(3), np.zeros(3)) for c in centres])
    t = np.stack([-r @ c for r, c in zip(R, centres)])
    xyz = rng.normal(size=(p, 3))
    xyz *= 8 * rng.uniform(0, 1, (p, 1)) ** (1 / 3) / np.linalg.norm(xyz, axis=1, keepdims=True)
    length = 2 + rng.poisson(6.0, p)
    first = rng.integers(0, v, p)
    point = np.repeat(np.arange(p), length)
    view = (np.repeat(first, length) + np.arange(length.sum()) - np.repeat(np.cumsum(length) - length, length)) % v
    key = np.unique(view.astype(np.int64) * p + point)  # a run longer than the ring wraps onto itself
    obs = np.stack([key // p, key % p], 1).astype(np.int32)
    K = np.tile(np.array([[1000.0, 0, 960], [0, 1000.0, 540], [0, 0, 1]]), (v, 1, 1))
    return {"image_ids": np.arange(1, v + 1), "names": ["{:04}.jpg".format(i) for i in range(v)], "K": K, "R": R, "t": t,
            "centres": centres, "point_ids": np.arange(1, p + 1), "xyz": xyz, "obs": obs}


def write_bin(path, m):
    """The model as .bin files through colmap.write_raw (poses as quaternions, so R is re-derived on reading)."""
    v, p, obs = len(m["R"]), len(m["xyz"]), m["obs"]
    cameras = {1: ("PINHOLE", 1920, 1080, np.array([1000.0, 1000.0, 960.0, 540.0]))}
    by_view = np.split(obs[:, 1], np.cumsum(np.bincount(obs[:, 0], minlength=v))[:-1])
    images = {i + 1: (synthetic._rot_to_quat(m["R"][i]), m["t"][i], 1, m["names"][i], np.zeros((len(by_view[i]), 2)),
                      by_view[i].astype(np.int64) + 1) for i in range(v)}
    order = np.argsort(obs[:, 1], kind="stable")
    tracks = np.split(obs[order, 0] + 1, np.cumsum(np.bincount(obs[:, 1], minlength=p))[:-1])
    rgb = np.zeros(3, np.uint8)
    points = {i + 1: (m["xyz"][i], rgb, 0.5, np.stack([tracks[i], np.zeros_like(tracks[i])], 1)) for i in range(p)}
    colmap.write_raw(path, cameras, images, points, True)


def median_ms(fn, warmup, repeats, events):
    times = []
    for k in range(warmup + repeats):
        torch.cuda.synchronize()
        if events:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
        else:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            times.append(ms)
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "warmup": warmup,
            "repeats": repeats}


out_path = arg("--out", "profiles/view_select_time.json")
V, P, P_REF = arg("--views", 300), arg("--points", 1_000_000), arg("--ref-points", 1_000_000)
assert torch.cuda.is_available(), "view_select_time needs a GPU: nothing here is measured on the CPU but the restatement"
dev = "cuda:0"
model = ring_model(V, P)
obs = model["obs"]
up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
ov, op_, xyz, centres = up(obs[:, 0], np.int32), up(obs[:, 1], np.int32), up(model["xyz"], np.float64), up(model["centres"], np.float64)
bits = view_select.set_bits(ov, op_, V, P)
scores, counts = view_select.pair_scores(bits, P, centres, xyz)
common = int(counts.sum().item()) // 2
record = {"workload": f"ring of {V} views, {P} points, {len(obs)} observations (mean track {len(obs) / P:.2f}), "
                      f"{V * (V - 1) // 2} pairs, {common} common points over all pairs, bit matrix {bits.numel() * 8} bytes",
          "pair_scores": median_ms(lambda: view_select.pair_scores(bits, P, centres, xyz), 2, 7, True),
          "set_bits": median_ms(lambda: view_select.set_bits(ov, op_, V, P), 2, 7, True),
          "select": median_ms(lambda: colmap_scene.select(model), 1, 5, False)}
record["pair_scores"]["bit_matrix_gbytes_per_s"] = V * (V - 1) * view_select.words(P) * 8 / record["pair_scores"]["median_ms"] / 1e6
print(json.dumps(record), flush=True)

with tempfile.TemporaryDirectory() as tmp:  # the whole convert, once: parsing a million points is host work
    t0 = time.perf_counter()
    write_bin(os.path.join(tmp, "sparse"), model)
    t1 = time.perf_counter()
    colmap.read_model(os.path.join(tmp, "sparse"))
    t2 = time.perf_counter()
    res = colmap_scene.convert(os.path.join(tmp, "sparse"), None, os.path.join(tmp, "scan"), copy_images=False)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    record["convert_from_bin_once"] = {"write_model_s": t1 - t0, "read_model_alone_s": t2 - t1, "convert_s": t3 - t2,
                                       "bin_bytes": sum(os.path.getsize(os.path.join(tmp, "sparse", f))
                                                        for f in os.listdir(os.path.join(tmp, "sparse")))}
    record["convert_from_bin_once"]["counts_equal_arrays_run"] = bool(np.array_equal(res["counts"], counts.cpu().numpy()))
print(json.dumps(record["convert_from_bin_once"]), flush=True)

small = model if P_REF == P else ring_model(V, P_REF)
t0 = time.perf_counter()
want = ref.select(small)
ref_s = time.perf_counter() - t0
got = colmap_scene.select(small)
gpu_small = median_ms(lambda: colmap_scene.select(small), 1, 5, False)
nz = want["scores"] > 0
record["numpy_restatement"] = {
    "workload": f"{V} views, {P_REF} points, {len(small['obs'])} observations", "select_s": ref_s,
    "gpu_select_same_model": gpu_small, "counts_equal": bool(np.array_equal(got["counts"], want["counts"])),
    "pairs_equal": bool(np.array_equal(got["pairs"], want["pairs"])),
    "depth_ranges_equal": bool(np.array_equal(got["depth_min"], want["depth_min"]) and np.array_equal(got["depth_max"], want["depth_max"])),
    "worst_relative_score_difference": float((np.abs(got["scores"] - want["scores"])[nz] / want["scores"][nz]).max())}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(record, f, indent=1)
    f.write("\n")
print(json.dumps(record["numpy_restatement"]), flush=True)
print("wrote", out_path)
