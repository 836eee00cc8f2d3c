"""python -m transmvsnet_amd.finetune at config C5's size: a synthetic BlendedMVS-format scan (768 x 576, 4
views, so N = 4 and 4 samples per epoch) written to a temporary directory, the driver run on it for a few
dozen steps (48/32/8, focal_loss_bld, one log record per step), and from its train.jsonl the steps per second
and the share of the wall time the loop spent waiting for data (decode on the host threads, upload, the uint8
conversion and tmvs_gt_pyramid). On the same box and in the same process afterwards: the eager training step
of bench.py --full (bench.train_steps: synthetic device tensors, no loader, no per-step host sync of the loss),
wall time per step. The driver runs that same step eagerly plus the loader, the NaN check's host sync and the
log line; bench.py's headline training figure is a HIP-graph replay of it. A record, not a test.
Usage: finetune_time.py [--out profiles/finetune_time.json] [--epochs 10] [--workers 2]"""
import json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from transmvsnet_amd import TransMVSNet, finetune, synthetic


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path = arg("--out", "profiles/finetune_time.json")
epochs, workers = arg("--epochs", 10), arg("--workers", 2)
H, W, N = 576, 768, 4

with tempfile.TemporaryDirectory(prefix="tmvs_finetune_time_") as tmp:
    listfile = synthetic.write_blended_scan(tmp, n_views=N, height=H, width=W)
    ckpt = os.path.join(tmp, "init.ckpt")
    torch.save({"model": synthetic.synthetic_state_dict(synthetic.state_dict_shapes(TransMVSNet()), seed=0)}, ckpt)
    logdir = os.path.join(tmp, "log")
    t0 = time.perf_counter()
    finetune.main(["--mode", "train", "--dataset", "bld_train", "--trainpath", tmp, "--trainlist", listfile,
                   "--nviews", str(N), "--epochs", str(epochs), "--summary_freq", "1", "--save_freq", str(10 ** 6),
                   "--loadckpt", ckpt, "--logdir", logdir, "--workers", str(workers)])
    wall = time.perf_counter() - t0
    with open(os.path.join(logdir, "train.jsonl")) as f:
        recs = [json.loads(ln) for ln in f]
recs = [r for r in recs if r["mode"] == "train"][N:]  # the first epoch warms the caches and the allocator
step = np.array([r["step_seconds"] for r in recs])
wait = np.array([r["data_wait_seconds"] for r in recs])
driver = {"steps_timed": len(recs), "steps_per_s": float(len(recs) / (step.sum() + wait.sum())),
          "step_ms_median": float(np.median(step) * 1e3), "data_wait_ms_median": float(np.median(wait) * 1e3),
          "data_wait_ms_first_of_epoch_median": float(np.median(wait[::N]) * 1e3),
          "data_wait_share": float(wait.sum() / (step.sum() + wait.sum())),
          "all_steps_applied": bool(all(r["applied"] for r in recs)), "wall_s_whole_run": wall}
print(json.dumps(driver), flush=True)

import bench  # noqa: E402 -- the repository's benchmark: its C5 training closures
full_step, _, _ = bench.train_steps(torch.device("cuda:0"))
for _ in range(2):
    full_step()
torch.cuda.synchronize()
ts = []
for _ in range(10):
    t0 = time.perf_counter()
    full_step()
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
eager_ms = float(np.median(ts) * 1e3)
rec = {"workload": f"synthetic BlendedMVS-format scan {W}x{H}, N={N}, 48/32/8, focal_loss_bld, {epochs} epochs of "
                   f"{N} samples, {workers} decode threads, summary_freq 1",
       "driver": driver,
       "bench_eager_step_ms": eager_ms,
       "driver_step_over_bench_eager": driver["step_ms_median"] / eager_ms,
       "driver_wall_per_step_over_bench_eager": 1e3 / driver["steps_per_s"] / eager_ms,
       "loader_starves_step": bool(driver["data_wait_share"] > 0.05)}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
