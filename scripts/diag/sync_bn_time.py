"""What synchronised BatchNorm statistics cost per eager training step on one GPU, at the DTU training size
(train.py / scripts/train.sh: 512 x 640 crop, N = 5, 48/32/8, B = 1 per rank, trans_mvsnet_loss 0.5, 1, 2): the
reference's train_sample body on the drop-in model over resident synthetic tensors, three ways, alternated:

    off     this tree, sync off (today's calls)
    sync    this tree, model.sync_batchnorm(always=True) on a one-rank RCCL group: every collective of the
            synchronised path is issued (slot fill, all_reduce, tmvs_rank_sum), with nobody to wait for
    parent  another checkout (--parent DIR, built there), e.g. the parent commit: sync off must cost what it costs

Each way runs in a worker process of its own (this file with --worker; a second package of the same name cannot be
imported next to the first). After every worker's warm-up, `rounds` alternations of one block of `steps` steps per
worker, each block timed by a host clock around work that ends in a device synchronise. Reported: per way the
median over the rounds of the block's time per step and the spread between the rounds; the collectives of one
synchronised step (count and bytes); whether `off` is within the alternation spread of `parent`. Multi-rank
latency (xGMI) is not in these figures: one rank has nobody to wait for. A record, not a test.
Usage: sync_bn_time.py [--out profiles/sync_bn_time.json] [--parent DIR] [--rounds 6] [--steps 6] [--order off,sync,parent]"""
import json, os, subprocess, sys, tempfile, time
HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


H, W, N, ND = arg("--height", 512), arg("--width", 640), 5, [48, 32, 8]


def worker(mode, root):
    sys.path.insert(0, root)
    import torch
    from transmvsnet_amd import TransMVSNet, loss, synthetic
    from transmvsnet_amd.train import FlatAdam
    if not torch.cuda.is_available():
        raise SystemExit("sync_bn_time.py measures on the GPU; there is none here (not measured)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    model = TransMVSNet(ndepths=ND)
    model.load_state_dict(synthetic.synthetic_state_dict(synthetic.state_dict_shapes(model), seed=0), strict=True)
    model = model.to(dev)
    if mode == "sync":
        import torch.distributed as dist
        store = "file://" + os.path.join(tempfile.mkdtemp(prefix="tmvs_sync_bn_time_"), "store")
        dist.init_process_group("nccl", init_method=store, rank=0, world_size=1, device_id=dev)
        model.sync_batchnorm(always=True)
    opt = FlatAdam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-6, betas=(0.9, 0.999), weight_decay=1e-4)
    imgs = synthetic.synthetic_images(N, H, W, batch=1, seed=0).to(dev)
    proj = synthetic.synthetic_cameras(N, H, W, batch=1, seed=1)
    dv = synthetic.synthetic_depth_values(1).to(dev)
    g = torch.Generator().manual_seed(11)
    gt3 = torch.nn.functional.interpolate(520.0 + 300.0 * torch.rand(1, 1, 8, 10, generator=g), size=(H, W),
                                          mode="bilinear", align_corners=False)[:, 0]
    m3 = (torch.rand(1, H, W, generator=g) > 0.2).float()
    gt = {f"stage{s}": gt3[:, ::k, ::k].contiguous().to(dev) for s, k in ((1, 4), (2, 2), (3, 1))}
    mask = {f"stage{s}": m3[:, ::k, ::k].contiguous().to(dev) for s, k in ((1, 4), (2, 2), (3, 1))}

    def step():
        model.train()
        opt.zero_grad()
        total = loss.trans_mvsnet_loss(model(imgs, proj, dv), gt, mask, dlossw=[0.5, 1.0, 2.0])[0]
        total.backward()
        opt.allreduce()
        opt.step()
        return total

    for _ in range(3):  # the allocator's pools, the pack caches, the communicator
        last = step()
    torch.cuda.synchronize()
    sync = getattr(model, "sync_bn", None)
    print(json.dumps({"ready": mode, "device": torch.cuda.get_device_name(dev), "loss_of_a_warm_step": float(last.detach()),
                      "collectives_per_step": sync.record() if sync is not None else None}), flush=True)
    for line in sys.stdin:
        k = int(line)
        if k <= 0:
            break
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            step()
        torch.cuda.synchronize()
        print(json.dumps({"ms_per_step": (time.perf_counter() - t0) / k * 1e3}), flush=True)
    if mode == "sync":
        import torch.distributed as dist
        dist.destroy_process_group()


def read_record(proc, mode):
    """the worker's next JSON line (libraries may print lines of their own in between)"""
    while True:
        line = proc.stdout.readline()
        if not line:
            raise SystemExit(f"sync_bn_time.py: the `{mode}` worker ended early")
        if line.startswith("{"):
            return json.loads(line)


def main():
    import numpy as np
    out_path = arg("--out", "profiles/sync_bn_time.json")
    rounds, steps, parent = arg("--rounds", 6), arg("--steps", 6), arg("--parent", "")
    ways = [("off", ROOT), ("sync", ROOT)] + ([("parent", os.path.abspath(parent))] if parent else [])
    order = arg("--order", ",".join(m for m, _ in ways)).split(",")  # the order the workers start and take turns in
    ways = sorted(ways, key=lambda w: order.index(w[0]))
    procs, ready = {}, {}
    try:
        for mode, root in ways:  # one at a time: a warm-up never runs against another's
            procs[mode] = subprocess.Popen([sys.executable, HERE, "--worker", "off" if mode == "parent" else mode, "--root",
                                            root, "--height", str(H), "--width", str(W)], stdin=subprocess.PIPE,
                                           stdout=subprocess.PIPE, text=True, cwd=root)
            ready[mode] = read_record(procs[mode], mode)
        block = {mode: [] for mode, _ in ways}
        for r in range(rounds):
            for mode, _ in (ways if r % 2 == 0 else ways[::-1]):  # back and forth: no way always follows the same one
                procs[mode].stdin.write(f"{steps}\n")
                procs[mode].stdin.flush()
                block[mode].append(read_record(procs[mode], mode)["ms_per_step"])
    finally:
        for p in procs.values():
            if p.poll() is None:
                try:
                    p.stdin.write("0\n")
                    p.stdin.flush()
                except OSError:
                    pass
                p.wait(timeout=60)
    per = {mode: {"ms_per_step_median": float(np.median(v)), "ms_per_step_min": float(min(v)),
                  "ms_per_step_max": float(max(v)), "ms_per_step_rounds": [float(x) for x in v],
                  "spread_over_median": float((max(v) - min(v)) / np.median(v)),
                  "loss_of_a_warm_step": ready[mode]["loss_of_a_warm_step"]} for mode, v in block.items()}
    rec = {"workload": f"resident synthetic tensors {W}x{H}, N={N}, 48/32/8, B=1, trans_mvsnet_loss 0.5,1,2, eager "
                       f"step, {rounds} alternations of {steps} steps per way (order {','.join(m for m, _ in ways)}, reversed "
                       "every other round) after 3 warm-up steps each, one worker process per way",
           "device": ready["off"]["device"], **per,
           "collectives_per_synchronised_step": ready["sync"]["collectives_per_step"],
           "sync_over_off": per["sync"]["ms_per_step_median"] / per["off"]["ms_per_step_median"],
           "multi_rank_latency": "not measured (one rank: the all-reduce has nobody to wait for)"}
    if parent:
        ratios = [x / y for x, y in zip(block["off"], block["parent"])]
        spread = max(per["off"]["spread_over_median"], per["parent"]["spread_over_median"])
        ratio = per["off"]["ms_per_step_median"] / per["parent"]["ms_per_step_median"]
        rec.update({"off_over_parent": ratio, "off_over_parent_by_round": [float(r) for r in ratios],
                    "off_within_alternation_spread_of_parent": bool(abs(ratio - 1.0) <= spread)})
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker(arg("--worker", "off"), arg("--root", ROOT))
    else:
        main()
