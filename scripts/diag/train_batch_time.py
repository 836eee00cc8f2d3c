"""The eager training step per sample at batch 1 and at batch 2, in one process, at the DTU training size
(train.py / scripts/train.sh: 512 x 640 crop, N = 5, 48/32/8, trans_mvsnet_loss with dlossw 0.5, 1, 2): the
reference's train_sample body on the drop-in model over resident synthetic tensors (no loader, no per-step host
sync of the loss) -- model.train(); zero_grad; outputs = model(imgs, proj, depth_values); loss; backward;
FlatAdam.step. After a warm-up of both batch sizes, `rounds` alternations of (`steps` steps at B = 1, `steps`
steps at B = 2), each block timed by a host clock around work that ends in a device synchronise; per batch size
the median over the rounds of the block's time per sample, the spread between the rounds, and the peak device
memory of a step. The expectation it checks: a sample costs no more in a batch of two than alone (the per-sample
kernels run the same work; the joint BatchNorm passes replace two launches by one). A record, not a test.
Usage: train_batch_time.py [--out profiles/train_batch_time.json] [--rounds 6] [--steps 8]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from transmvsnet_amd import TransMVSNet, loss, synthetic
from transmvsnet_amd.train import FlatAdam


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path = arg("--out", "profiles/train_batch_time.json")
rounds, steps = arg("--rounds", 6), arg("--steps", 8)
H, W, N, ND, BMAX = arg("--height", 512), arg("--width", 640), 5, [48, 32, 8], 2
if not torch.cuda.is_available():
    raise SystemExit("train_batch_time.py measures on the GPU; there is none here (not measured)")
dev = torch.device("cuda:0")

model = TransMVSNet(ndepths=ND)
model.load_state_dict(synthetic.synthetic_state_dict(synthetic.state_dict_shapes(model), seed=0), strict=True)
model = model.to(dev)
opt = FlatAdam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-6, betas=(0.9, 0.999), weight_decay=1e-4)
imgs = synthetic.synthetic_images(N, H, W, batch=BMAX, seed=0).to(dev)
proj = synthetic.synthetic_cameras(N, H, W, batch=BMAX, seed=1)
dv = synthetic.synthetic_depth_values(BMAX).to(dev)
g = torch.Generator().manual_seed(11)
gt3 = torch.nn.functional.interpolate(520.0 + 300.0 * torch.rand(BMAX, 1, 8, 10, generator=g), size=(H, W),
                                      mode="bilinear", align_corners=False)[:, 0]
m3 = (torch.rand(BMAX, H, W, generator=g) > 0.2).float()
gt = {f"stage{s}": gt3[:, ::k, ::k].contiguous().to(dev) for s, k in ((1, 4), (2, 2), (3, 1))}
mask = {f"stage{s}": m3[:, ::k, ::k].contiguous().to(dev) for s, k in ((1, 4), (2, 2), (3, 1))}


def step(b):
    model.train()
    opt.zero_grad()
    outputs = model(imgs[:b], {k: v[:b] for k, v in proj.items()}, dv[:b])
    total = loss.trans_mvsnet_loss(outputs, {k: v[:b] for k, v in gt.items()}, {k: v[:b] for k, v in mask.items()},
                                   dlossw=[0.5, 1.0, 2.0])[0]
    total.backward()
    opt.step()
    return total


peak, last = {}, {}
for b in (1, 2):  # warm-up: every shape the timed window uses, the allocator's pools, the pack caches
    for _ in range(3):
        step(b)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    last[b] = float(step(b).detach())
    torch.cuda.synchronize()
    peak[b] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
block = {1: [], 2: []}
for _ in range(rounds):
    for b in (1, 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(b)
        torch.cuda.synchronize()
        block[b].append((time.perf_counter() - t0) / (steps * b) * 1e3)
per = {b: {"ms_per_sample_median": float(np.median(v)), "ms_per_sample_min": float(min(v)),
           "ms_per_sample_max": float(max(v)), "ms_per_sample_rounds": [float(x) for x in v],
           "spread_over_median": float((max(v) - min(v)) / np.median(v)), "peak_memory_mib": float(peak[b]),
           "loss_of_a_warm_step": last[b]} for b, v in block.items()}
ratio = per[2]["ms_per_sample_median"] / per[1]["ms_per_sample_median"]
ratios = [y / x for x, y in zip(block[1], block[2])]
rec = {"workload": f"resident synthetic tensors {W}x{H}, N={N}, 48/32/8, trans_mvsnet_loss 0.5,1,2, eager step, "
                   f"{rounds} alternations of {steps} steps per batch size after 3 warm-up steps each",
       "device": torch.cuda.get_device_name(dev),
       "batch_1": per[1], "batch_2": per[2],
       "batch_2_over_batch_1_per_sample": ratio,
       "batch_2_over_batch_1_per_sample_by_round": [float(r) for r in ratios],
       "batch_2_costs_more_per_sample_beyond_spread": bool(min(ratios) > 1.0 + per[1]["spread_over_median"])}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
