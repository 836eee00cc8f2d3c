"""transmvsnet_amd.dtu_eval.evaluate_cloud at the size of a DTU scan: a synthetic fused cloud of about 20 M
points (a curved surface inside a 400 mm box with 0.15 mm noise along z and 1 % outliers anywhere in the box)
against about 3 M ground-truth points on the same surface, 0.2 mm apart. Per step in ms: the thinning with
its number of rounds, the two nearest passes, mask + plane, the statistics; the two nearest passes for a few
grid cell sizes; and on the same inputs scipy's cKDTree.query(workers=16) for the two nearest passes (tree
build and query) as the CPU yardstick. A record, not a test.
Usage: dtu_eval_time.py [--out profiles/dtu_eval_time.json] [--cloud 20000000] [--no-cpu]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from transmvsnet_amd import dtu_eval


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path = arg("--out", "profiles/dtu_eval_time.json")
n_cloud = arg("--cloud", 20_000_000)
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(0)


def height(x, y):
    return 200.0 + 60.0 * torch.sin(x / 70.0) * torch.cos(y / 90.0)


# ground truth: a 0.2 mm lattice over 346 x 346 mm = 3.0 M points
k = 1730
ix, iy = torch.meshgrid(torch.arange(k, device=dev), torch.arange(k, device=dev), indexing="ij")
sx, sy = 27.0 + 0.2 * ix.reshape(-1).float(), 27.0 + 0.2 * iy.reshape(-1).float()
stl = torch.stack([sx, sy, height(sx, sy)], 1).contiguous()
n_out = n_cloud // 100
cx, cy = (27.0 + 346.0 * torch.rand(n_cloud - n_out, device=dev, generator=g) for _ in range(2))
cloud = torch.stack([cx, cy, height(cx, cy) + 0.15 * torch.randn(n_cloud - n_out, device=dev, generator=g)], 1)
cloud = torch.cat([cloud, 400.0 * torch.rand(n_out, 3, device=dev, generator=g)])
cloud = cloud[torch.randperm(n_cloud, device=dev, generator=g)].contiguous()
del ix, iy, sx, sy, cx, cy
bb = np.array([[0.0, 0.0, 0.0], [400.0, 400.0, 400.0]])
mask = np.ones((51, 51, 51), np.uint8)
mask[:, :, 40:] = 0
res, plane = 8.0, np.array([0.0, 0.0, 1.0, -150.0])
print(f"cloud {tuple(cloud.shape)}, stl {tuple(stl.shape)}", flush=True)

dtu_eval.evaluate_cloud(cloud[:200000], stl[:200000], mask, bb, res, plane)  # warm-up: library load, allocator
torch.cuda.synchronize()
timings = {}
t0 = time.perf_counter()
result = dtu_eval.evaluate_cloud(cloud, stl, mask, bb, res, plane, timings=timings)
torch.cuda.synchronize()
total_s = time.perf_counter() - t0
print(json.dumps(timings), flush=True)
print(json.dumps(result), flush=True)

thin = cloud[dtu_eval.thin_points(cloud, 0.2, seed=0)]


def gpu_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


cells = {}
for cell in (0.5, 1.0, 2.0):
    a, _ = gpu_ms(lambda: dtu_eval.nearest_distance(thin, stl, bb, 20.0, 60.0, cell=cell))
    b, _ = gpu_ms(lambda: dtu_eval.nearest_distance(stl, thin, bb, 20.0, 60.0, cell=cell))
    cells[str(cell)] = {"data_to_stl_ms": a, "stl_to_data_ms": b}
    print(f"cell {cell}: data->stl {a:.1f} ms, stl->data {b:.1f} ms", flush=True)

cpu = None
if "--no-cpu" not in sys.argv:
    from scipy.spatial import cKDTree
    d_data = dtu_eval.nearest_distance(thin, stl, bb, 20.0, 60.0).cpu().numpy()
    d_stl = dtu_eval.nearest_distance(stl, thin, bb, 20.0, 60.0).cpu().numpy()
    tn, sn = thin.cpu().numpy().astype(np.float64), stl.cpu().numpy().astype(np.float64)
    cpu = {}
    for name, frm, to, got in (("data_to_stl", tn, sn, d_data), ("stl_to_data", sn, tn, d_stl)):
        t0 = time.perf_counter()
        tree = cKDTree(to)
        t1 = time.perf_counter()
        d, _ = tree.query(frm, k=1, distance_upper_bound=20.0, workers=16)
        t2 = time.perf_counter()
        d = np.minimum(d, 20.0)  # inf where nothing is within 20
        cpu[name] = {"build_ms": (t1 - t0) * 1e3, "query_ms": (t2 - t1) * 1e3,
                     "max_abs_diff_vs_gpu": float(np.abs(d - got).max())}
        print(name, json.dumps(cpu[name]), flush=True)

rec = {"workload": f"synthetic scan: {n_cloud} cloud points (1 % outliers), {stl.shape[0]} ground-truth points, "
                   "curved surface in a 400 mm box; dst 0.2, max_dist 20, nearest cell 1.0 / 5.0",
       "n_thinned": result["n_thinned"], "steps_ms": timings, "evaluate_cloud_wall_s": total_s,
       "nearest_ms_by_fine_cell": cells, "ckdtree_workers16": cpu,
       "gpu_nearest_faster_than_ckdtree": None if cpu is None else bool(
           timings["nearest_data_to_stl_ms"] < cpu["data_to_stl"]["query_ms"]
           and timings["nearest_stl_to_data_ms"] < cpu["stl_to_data"]["query_ms"]),
       "result": result}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
