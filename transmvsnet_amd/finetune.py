"""Scan folders -> checkpoints: the reference's training entry points (finetune.py for BlendedMVS, train.py
for DTU) as one driver over this package's HIP training step.

  warmup_multistep_lr   utils.WarmupMultiStepLR.get_lr (utils.py:253-268) as a pure function of the iteration
  BldTrainSet           datasets/bld_train.py:30-172 (blended_images/, cams/, rendered_depth_maps/)
  DtuTrainSet           datasets/dtu_yao.py:26-193 (Rectified/, Cameras/train/, Depths_raw/, 7 lights per view)
  Prefetcher            the DataLoader's role: files decoded on a few host threads ahead of the step
  train_sample          finetune.py:144-195 / train.py:137-189
  test_sample           finetune.py:198-236 / train.py:192-241 (dtu_yao: the twelve validation scalars, one
                        tmvs_depth_eval_metrics launch, no host sync per sample)
  train / test          finetune.py:55-141: LR schedule, checkpoints, evaluation, the JSON-lines log
  python -m transmvsnet_amd.finetune   the reference's command line

A sample's images are decoded once on the host, uploaded as uint8 and converted on the GPU
(tmvs_resize_bilinear_u8 at the image's own size: every fraction is 0, so each value is exactly
float32(u8) / 255); the raw depth map (and DTU's depth_visual PNG) is uploaded once and the depth / mask
pyramid comes out of one tmvs_gt_pyramid launch. --batch_size B samples per rank and step (finetune.py runs 1,
train.py's DTU recipe 2): the training order is cut into batches of B with the remainder dropped (the
reference's train loader has drop_last=True), evaluation runs batches of B with a smaller last one, and every
train-mode BatchNorm takes its statistics over the batch (train.forward_train). focal_bld takes B = 1 only.
--sync_bn under torchrun takes every train-mode BatchNorm statistic over the samples of all ranks (sync_bn.py), as
the reference always does under torch.distributed. Not built: apex, tensorboard summaries, DataParallel,
--mode profile.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import gc
import json
import os
import random
import time
from bisect import bisect_right

import numpy as np
import torch

from . import data, ops
from .reconstruct import _AxisTables, read_img_u8, resize_image

MAX_WORKERS = 4  # host decode threads: a small fixed bound, never sized from the machine's CPU count
BLD_METRICS = ("epe", "less1", "less3")


# ------------------------------------------------------------------ LR schedule
def warmup_multistep_lr(base_lr, it, milestones, gamma, warmup_factor=1.0 / 3, warmup_iters=500):
    """The learning rate iteration `it` of the run trains with: WarmupMultiStepLR.get_lr (utils.py:253-268) at
    last_epoch = it, linear warm-up. finetune.py:56-59 builds the scheduler at last_epoch = len(loader) *
    start_epoch - 1 and its constructor steps once, so the first iteration after a resume is len(loader) *
    start_epoch; it steps once after every train_sample (:72)."""
    factor = 1
    if it < warmup_iters:
        alpha = float(it) / warmup_iters
        factor = warmup_factor * (1 - alpha) + alpha
    return base_lr * factor * gamma ** bisect_right(milestones, it)


def parse_lrepochs(lrepochs, iters_per_epoch):
    """'10,12,14:2' -> (milestones in iterations, gamma = 1 / rate) (finetune.py:56-57)."""
    epochs, rate = lrepochs.split(":")
    return [iters_per_epoch * int(e) for e in epochs.split(",")], 1 / float(rate)


# ------------------------------------------------------------------ training sets
class _TrainSet:
    """What the two dataset classes share: a sample is read in two halves, `load_host` (files -> host
    arrays; runs on the Prefetcher's threads, touches no GPU) and `upload` (host arrays -> the sample dict,
    on the caller's thread and stream); `sample(idx)` is both."""

    gt_mode = None

    def __init__(self, datapath, listfile, mode, nviews, ndepths=192, device="cuda", **kwargs):
        if mode not in ("train", "val", "test"):
            raise ValueError(f"mode must be train, val or test, got {mode!r}")
        self.datapath, self.listfile, self.mode = datapath, listfile, mode
        self.nviews, self.ndepths, self.device = int(nviews), int(ndepths), torch.device(device)
        self.target_hw = (512, 640)
        self.metas = self.build_list()
        self._axes = _AxisTables(self.device)
        self._gt_tables = {}

    def __len__(self):
        return len(self.metas)

    def _pyramid_tables(self, h, w):
        """tmvs_gt_pyramid's index tables on the device, one upload per raw size."""
        if (h, w) not in self._gt_tables:
            rows, cols, _ = data.gt_pyramid_tables(h, w, self.gt_mode, self.target_hw)
            self._gt_tables[(h, w)] = (torch.from_numpy(rows).to(self.device), torch.from_numpy(cols).to(self.device))
        return self._gt_tables[(h, w)]

    def _stack(self, host):
        proj = np.stack(host["proj"])
        s2, s3 = proj.copy(), proj.copy()
        s2[:, 1, :2, :] = proj[:, 1, :2, :] * 2
        s3[:, 1, :2, :] = proj[:, 1, :2, :] * 4
        return {"stage1": proj, "stage2": s2, "stage3": s3}

    def upload(self, host):
        """The reference's sample dict: imgs [N,3,H,W], depth {stage: [h,w]} and mask {stage: [h,w]} on the
        device; proj_matrix {stage: [N,2,4,4]} and depth_values [D] host float32 arrays; depth_interval a
        float."""
        imgs = []
        for u8 in host["imgs_u8"]:
            src = torch.from_numpy(u8).to(self.device)
            imgs.append(resize_image(src, u8.shape[1], u8.shape[0], self._axes))  # float32(u8) / 255, CHW
        depth_raw = torch.from_numpy(host["depth_raw"]).to(self.device)
        rows, cols = self._pyramid_tables(*host["depth_raw"].shape)
        png = torch.from_numpy(host["mask_png"]).to(self.device) if host.get("mask_png") is not None else None
        depth, mask = ops.gt_pyramid(depth_raw, rows, cols, self.gt_mode, host.get("depth_min", 0.0),
                                     host.get("depth_end", 0.0), png, self.target_hw)
        out = {"imgs": torch.stack(imgs), "proj_matrix": self._stack(host), "depth": depth, "mask": mask,
               "depth_values": host["depth_values"], "depth_interval": host["depth_interval"]}
        if "name" in host:
            out["name"] = host["name"]
        return out

    def sample(self, idx):
        return self.upload(self.load_host(idx))


class BldTrainSet(_TrainSet):
    """bld_train.MVSDataset (datasets/bld_train.py:30-172). Intrinsics / 4; depth_interval = (max - min) /
    ndepths from the last field of the camera file's line 11; depth_values = arange(min, interval * ndepths +
    min, interval); mask = depth_min <= depth <= interval * (ndepths - 1) + min of the reference view. As in
    the reference, the returned depth_interval is the LAST view's (its loop variable outlives the loop,
    :119 / :171); the depth range and the mask are the reference view's."""

    gt_mode = "bld"

    def build_list(self):
        return data.build_list_bld(self.datapath, self.listfile, self.nviews)

    def load_host(self, idx):
        scan, ref_view, src_views = self.metas[idx]
        view_ids = [ref_view] + src_views[:self.nviews - 1]
        host = {"imgs_u8": [], "proj": []}
        for i, vid in enumerate(view_ids):
            host["imgs_u8"].append(read_img_u8(os.path.join(self.datapath,
                                                            "{}/blended_images/{:0>8}.jpg".format(scan, vid))))
            intr, extr, dmin, dint = data.read_cam_file_bld(
                os.path.join(self.datapath, "{}/cams/{:0>8}_cam.txt".format(scan, vid)), self.ndepths)
            p = np.zeros((2, 4, 4), np.float32)
            p[0] = extr
            p[1, :3, :3] = intr
            host["proj"].append(p)
            if i == 0:
                name = os.path.join(self.datapath, "{}/rendered_depth_maps/{:0>8}.pfm".format(scan, vid))
                host["name"] = name
                host["depth_raw"] = np.ascontiguousarray(data.read_pfm(name)[0], np.float32)
                host["depth_min"], host["depth_end"] = dmin, dint * (self.ndepths - 1) + dmin
                host["depth_values"] = np.arange(dmin, dint * self.ndepths + dmin, dint, dtype=np.float32)
            host["depth_interval"] = dint
        return host


class DtuTrainSet(_TrainSet):
    """dtu_yao.MVSDataset (datasets/dtu_yao.py:26-193): 7 light conditions per viewpoint, image files numbered
    vid + 1, Cameras/train intrinsics as stored, depth_interval = the file's x interval_scale (1.06), the
    raw depth map and depth_visual PNG halved (nearest) and centre-cropped to 512 x 640 (prepare_img)."""

    gt_mode = "dtu"

    def __init__(self, datapath, listfile, mode, nviews, ndepths=192, interval_scale=1.06, device="cuda",
                 target_hw=(512, 640), **kwargs):
        self.interval_scale = interval_scale
        super().__init__(datapath, listfile, mode, nviews, ndepths, device)
        self.target_hw = tuple(target_hw)

    def build_list(self):
        return data.build_list_dtu_train(self.datapath, self.listfile)

    def load_host(self, idx):
        from PIL import Image
        scan, light_idx, ref_view, src_views = self.metas[idx]
        view_ids = [ref_view] + src_views[:self.nviews - 1]
        host = {"imgs_u8": [], "proj": []}
        for i, vid in enumerate(view_ids):
            host["imgs_u8"].append(read_img_u8(os.path.join(
                self.datapath, "Rectified/{}_train/rect_{:0>3}_{}_r5000.png".format(scan, vid + 1, light_idx))))
            intr, extr, dmin, dint = data.read_cam_file_dtu_train(
                os.path.join(self.datapath, "Cameras/train/{:0>8}_cam.txt".format(vid)), self.interval_scale)
            p = np.zeros((2, 4, 4), np.float32)
            p[0] = extr
            p[1, :3, :3] = intr
            host["proj"].append(p)
            if i == 0:
                fn = os.path.join(self.datapath, "Depths_raw/{}/depth_visual_{:0>4}.png".format(scan, vid))
                png = np.array(Image.open(fn))
                if png.dtype != np.uint8 or png.ndim != 2:
                    raise ValueError(f"{fn}: expected an 8-bit single-channel image, got {png.dtype} {png.shape}")
                host["mask_png"] = np.ascontiguousarray(png)
                host["depth_raw"] = np.ascontiguousarray(data.read_pfm(os.path.join(
                    self.datapath, "Depths_raw/{}/depth_map_{:0>4}.pfm".format(scan, vid)))[0], np.float32)
                host["depth_values"] = np.arange(dmin, dint * self.ndepths + dmin, dint, dtype=np.float32)
            host["depth_interval"] = dint
        return host


DATASETS = {"bld_train": BldTrainSet, "dtu_yao": DtuTrainSet}


def find_dataset_def(name):
    if name not in DATASETS:
        raise ValueError(f"unknown dataset {name!r}; one of {sorted(DATASETS)}")
    return DATASETS[name]


class Prefetcher:
    """Iterates `dataset` in `order`: load_host runs on up to `workers` (<= MAX_WORKERS) host threads, `depth`
    samples ahead of the consumer; upload runs on the consumer's thread. `wait_s` is the time the consumer
    spent inside next() (blocked on a decode, plus the uploads and the two kinds of launches)."""

    def __init__(self, dataset, order, workers=2, depth=3):
        self.dataset, self.order = dataset, list(order)
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.depth = max(1, int(depth))
        self.wait_s = 0.0

    def __len__(self):
        return len(self.order)

    def __iter__(self):
        pool = cf.ThreadPoolExecutor(max_workers=self.workers)
        pending = []
        try:
            nxt = 0
            t0 = time.perf_counter()
            while nxt < len(self.order) or pending:
                while nxt < len(self.order) and len(pending) < self.depth:
                    pending.append(pool.submit(self.dataset.load_host, self.order[nxt]))
                    nxt += 1
                sample = self.dataset.upload(pending.pop(0).result())
                self.wait_s = time.perf_counter() - t0
                yield sample
                t0 = time.perf_counter()
        finally:
            for f in pending:
                f.cancel()
            pool.shutdown(wait=True)


def epoch_order(n, seed, epoch, shuffle=True):
    """The sample order of one epoch on one process: a function of (seed, epoch) only."""
    if not shuffle:
        return list(range(n))
    g = torch.Generator()
    g.manual_seed(int(seed) + int(epoch))
    return torch.randperm(n, generator=g).tolist()


def _is_distributed():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if _is_distributed() else 0


def rank_order(dataset, seed, epoch, shuffle=True, drop_last=False):
    """epoch_order, or under torch.distributed this rank's share through DistributedSampler.set_epoch."""
    if not _is_distributed():
        return epoch_order(len(dataset), seed, epoch, shuffle)
    import torch.distributed as dist
    from torch.utils.data import DistributedSampler
    sampler = DistributedSampler(dataset, num_replicas=dist.get_world_size(), rank=dist.get_rank(), shuffle=shuffle,
                                 seed=int(seed), drop_last=drop_last)
    sampler.set_epoch(epoch)
    return list(iter(sampler))


def batches(order, batch_size, drop_last):
    """`order` cut into consecutive batches of batch_size, as the DataLoader's BatchSampler does: the
    remainder is dropped (the reference's train loader, drop_last=True) or kept as a smaller last batch
    (its test loader)."""
    b = int(batch_size)
    if b < 1:
        raise ValueError(f"batch_size must be at least 1, got {batch_size}")
    order = list(order)
    out = [order[i:i + b] for i in range(0, len(order), b)]
    if drop_last and out and len(out[-1]) < b:
        out.pop()
    return out


def iters_per_epoch(n_samples, batch_size):
    """Training iterations per epoch of a rank whose share is n_samples: len(loader) with drop_last=True. The
    LR milestones (parse_lrepochs) and the first iteration after --resume count in these."""
    return len(batches(range(n_samples), batch_size, True))


class BatchLoader:
    """A Prefetcher over the flattened `batch_list`, yielding each batch as the list of its uploaded samples
    (decoded per sample on the host threads, uploaded on the consumer's thread). `wait_s`: the consumer's
    time inside next() for the whole batch."""

    def __init__(self, dataset, batch_list, workers=2):
        self.batch_list = [list(b) for b in batch_list]
        self.samples = Prefetcher(dataset, [i for b in self.batch_list for i in b], workers)
        self.wait_s = 0.0

    def __len__(self):
        return len(self.batch_list)

    def __iter__(self):
        it = iter(self.samples)
        for b in self.batch_list:
            group, wait = [], 0.0
            for _ in b:
                group.append(next(it))
                wait += self.samples.wait_s
            self.wait_s = wait
            yield group
        it.close()


# ------------------------------------------------------------------ one step
def collate(samples, device):
    """The DataLoader's collation: a leading batch axis on everything the model reads. `samples`: one
    sample dict (batch 1) or a list of them, which must agree in their image size and view count."""
    if isinstance(samples, dict):
        samples = [samples]
    first = samples[0]
    for i, s in enumerate(samples[1:], 1):
        if s["imgs"].shape != first["imgs"].shape:
            raise ValueError(f"a batch needs samples of one image size and view count: sample 0 "
                             f"({first.get('name', '?')}) has imgs {list(first['imgs'].shape)}, sample {i} "
                             f"({s.get('name', '?')}) {list(s['imgs'].shape)}; use --batch_size 1 or one --crop")
    if len(samples) == 1:
        stack, interval = (lambda ts: ts[0][None]), float(first["depth_interval"])
    else:
        stack, interval = torch.stack, torch.tensor([float(s["depth_interval"]) for s in samples])
    return {"imgs": stack([s["imgs"] for s in samples]),
            "proj_matrix": {k: stack([torch.from_numpy(s["proj_matrix"][k]) for s in samples])
                            for k in first["proj_matrix"]},
            "depth_values": stack([torch.from_numpy(s["depth_values"]) for s in samples]).to(device),
            "depth": {k: stack([s["depth"][k] for s in samples]) for k in first["depth"]},
            "mask": {k: stack([s["mask"][k] for s in samples]) for k in first["mask"]},
            "depth_interval": interval}


def _loss_outputs(loss_name, outputs, s, dlossw):
    from . import loss as loss_mod
    if loss_name == "focal_bld":
        total, depth_loss, epe, less1, less3 = loss_mod.focal_loss_bld(outputs, s["depth"], s["mask"],
                                                                       s["depth_interval"], dlossw=dlossw)
        return total, {"loss": total, "depth_loss": depth_loss, "epe": epe, "less1": less1, "less3": less3}
    total, depth_loss, entropy, _ = loss_mod.trans_mvsnet_loss(outputs, s["depth"], s["mask"], dlossw=dlossw)
    return total, {"loss": total, "depth_loss": depth_loss, "entropy_loss": entropy}


def reduce_scalar_outputs(scalars):
    """utils.reduce_scalar_outputs (utils.py:199-217): the scalars summed onto rank 0 and divided by the world
    size there (the other ranks keep what the reduce leaves them, as in the reference)."""
    if not _is_distributed():
        return scalars
    import torch.distributed as dist
    with torch.no_grad():
        names = sorted(scalars.keys())
        stacked = torch.stack([scalars[k].detach().float().reshape(()) for k in names], dim=0)
        dist.reduce(stacked, dst=0)
        if dist.get_rank() == 0:
            stacked /= dist.get_world_size()
        return {k: v for k, v in zip(names, stacked)}


def tensor2float(scalars):
    """One device-to-host copy for all of a step's scalars."""
    names = list(scalars)
    vals = torch.stack([scalars[k].detach().float().reshape(()) for k in names]).cpu().tolist()
    return dict(zip(names, vals))


def train_sample(model, opt, sample, loss_name, dlossw):
    """finetune.py:144-195's body for one batch (`sample`: a sample dict, or a list of them): train-mode
    forward, loss, the NaN check that skips the step, backward, the gradient all-reduce, the Adam step.
    Returns the step's scalars as device tensors (averaged onto rank 0 under torch.distributed) and whether
    the step was applied."""
    model.train()
    opt.zero_grad()
    s = collate(sample, (sample if isinstance(sample, dict) else sample[0])["imgs"].device)
    outputs = model(s["imgs"], s["proj_matrix"], s["depth_values"])
    total, scalars = _loss_outputs(loss_name, outputs, s, dlossw)
    applied = not np.isnan(total.item())
    if _is_distributed():  # every rank steps or none does: the all-reduce below is collective
        import torch.distributed as dist
        ok = torch.tensor([1 if applied else 0], device=total.device)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        applied = bool(ok.item())
    if applied:
        total.backward()
        opt.allreduce()
        opt.step()
    else:
        print("nan error occurred: step skipped", flush=True)
        gc.collect()
    return reduce_scalar_outputs({k: v.detach() for k, v in scalars.items()}), applied


@torch.no_grad()
def test_sample(model, sample, loss_name, dlossw, eval_metrics):
    """The eval-mode forward, the loss and the metrics of one batch (`sample`: a sample dict, or a list of
    them) as device tensors (no host sync). eval_metrics (dtu_yao): train.py:216-228's twelve scalars on the
    stage-3 depth, per image and then averaged over the batch (utils.compute_metrics_for_each_image)."""
    model.eval()
    s = collate(sample, (sample if isinstance(sample, dict) else sample[0])["imgs"].device)
    outputs = model(s["imgs"], s["proj_matrix"], s["depth_values"])
    _, scalars = _loss_outputs(loss_name, outputs, s, dlossw)
    if eval_metrics:
        est, gt, mask = outputs["depth"].float().contiguous(), s["depth"]["stage3"], s["mask"]["stage3"]
        if est.shape[0] == 1:
            m = ops.depth_eval_metrics(est, gt, mask)
        else:
            m = torch.stack([ops.depth_eval_metrics(est[i], gt[i].contiguous(), mask[i].contiguous())
                             for i in range(est.shape[0])]).mean(0)
        scalars.update({name: m[i] for i, name in enumerate(ops.EVAL_METRIC_NAMES)})
    return scalars


def evaluate(model, dataset, args, loss_name, dlossw, verbose=True):
    """finetune.test / the testing half of finetune.train (:98-141): the mean of every scalar over the test
    set (DictAverageMeter): batches of --batch_size with a smaller last one, the mean over the batches. The
    per-batch scalars stay on the device; they are summed there and read once."""
    import torch.distributed as dist
    order = rank_order(dataset, args.seed, 0, shuffle=False)
    loader = BatchLoader(dataset, batches(order, getattr(args, "batch_size", 1), False), args.workers)
    names, total, t0 = None, None, time.time()
    for i, sample in enumerate(loader):
        scalars = test_sample(model, sample, loss_name, dlossw, args.dataset == "dtu_yao")
        names = names or list(scalars)
        vec = torch.stack([scalars[k].detach().float().reshape(()) for k in names])
        total = vec.clone() if total is None else total + vec
        if verbose and _rank() == 0 and i % args.summary_freq == 0:
            print("Iter {}/{}, test loss = {:.3f}, time = {:.3f}".format(i, len(loader), float(scalars["loss"]),
                                                                      time.time() - t0), flush=True)
            t0 = time.time()
    if total is None:
        return {}
    count = torch.tensor([float(len(loader))], device=total.device)
    if _is_distributed():
        dist.all_reduce(total)
        dist.all_reduce(count)
    return dict(zip(names, (total / count).cpu().tolist()))


# ------------------------------------------------------------------ checkpoints and the loop
def latest_checkpoint(logdir):
    """train.py:333-342: the *.ckpt with the largest epoch number in its name."""
    saved = [fn for fn in os.listdir(logdir) if fn.endswith(".ckpt")]
    if not saved:
        raise FileNotFoundError(f"--resume: no *.ckpt in {logdir}")
    return os.path.join(logdir, sorted(saved, key=lambda x: int(x.split("_")[-1].split(".")[0]))[-1])


def save_checkpoint(path, epoch, model, opt):
    """{'epoch', 'model', 'optimizer'} as finetune.py:91-95 writes it (host copies, written through a
    temporary name so that a reader never sees half a file)."""
    state = {"epoch": epoch, "model": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
             "optimizer": opt.state_dict()}
    state["optimizer"]["state"] = {i: {k: v.cpu() for k, v in st.items()}
                                   for i, st in state["optimizer"]["state"].items()}
    torch.save(state, path + ".tmp")
    os.replace(path + ".tmp", path)


def _log(logdir, record):
    with open(os.path.join(logdir, "train.jsonl"), "a") as f:
        f.write(json.dumps(record) + "\n")


def train(model, opt, train_set, test_set, start_epoch, args, loss_name, dlossw):
    """finetune.train (:55-125). The learning rate of global iteration len(loader) * epoch + batch is
    warmup_multistep_lr's, set on the optimizer before the step."""
    bsz = getattr(args, "batch_size", 1)
    iters = iters_per_epoch(len(rank_order(train_set, args.seed, 0, drop_last=True)), bsz)
    milestones, gamma = parse_lrepochs(args.lrepochs, iters)
    main_rank = _rank() == 0
    for epoch in range(start_epoch, args.epochs):
        loader = BatchLoader(train_set, batches(rank_order(train_set, args.seed, epoch, drop_last=True), bsz, True),
                             args.workers)
        for batch, sample in enumerate(loader):
            t0 = time.perf_counter()
            step = iters * epoch + batch
            opt.lr = warmup_multistep_lr(args.lr, step, milestones, gamma)
            scalars, applied = train_sample(model, opt, sample, loss_name, dlossw)
            if main_rank and step % args.summary_freq == 0:
                vals = tensor2float(scalars)  # the host sync of the logging interval
                rec = {"mode": "train", "epoch": epoch, "iteration": step, "batch": batch, "lr": opt.lr,
                       "applied": applied, **vals, "step_seconds": time.perf_counter() - t0,
                       "data_wait_seconds": loader.wait_s}
                _log(args.logdir, rec)
                print("Epoch {}/{}, Iter {}/{}, lr {:.6f}, ".format(epoch, args.epochs, batch, len(loader), opt.lr) +
                      ", ".join("{} = {:.3f}".format(k, v) for k, v in vals.items()) +
                      ", time = {:.3f}, data wait = {:.3f}".format(rec["step_seconds"], loader.wait_s), flush=True)
        if main_rank and (epoch + 1) % args.save_freq == 0:
            save_checkpoint("{}/model_{:0>6}.ckpt".format(args.logdir, epoch), epoch, model, opt)
        gc.collect()
        if test_set is not None and (epoch % args.eval_freq == 0 or epoch == args.epochs - 1):
            means = evaluate(model, test_set, args, loss_name, dlossw, verbose=False)
            if main_rank:
                _log(args.logdir, {"mode": "fulltest", "epoch": epoch, "iteration": iters * (epoch + 1) - 1, **means})
                print("avg_test_scalars:", means, flush=True)


# ------------------------------------------------------------------ command line
def make_parser():
    p = argparse.ArgumentParser(
        description="Train / fine-tune TransMVSNet on BlendedMVS or DTU scan folders (HIP training step, "
                    "--batch_size samples per rank and step with BatchNorm statistics over the batch; "
                    "--loss focal_bld takes --batch_size 1 only; --sync_bn: those statistics over all ranks). "
                    "Not built: apex (--using_apex), tensorboard summaries, DataParallel and --mode "
                    "profile; start one process per GPU with torchrun for DDP.")
    p.add_argument("--mode", default="train", choices=["train", "test"], help="train or test")
    p.add_argument("--dataset", default="dtu_yao", choices=sorted(DATASETS), help="select dataset")
    p.add_argument("--trainpath", help="train datapath")
    p.add_argument("--testpath", help="test datapath (default: --trainpath)")
    p.add_argument("--trainlist", help="train list")
    p.add_argument("--testlist", help="test list")
    p.add_argument("--epochs", type=int, default=16, help="number of epochs to train")
    p.add_argument("--lr", type=float, default=0.001, help="learning rate")
    p.add_argument("--lrepochs", type=str, default="10,12,14:2", help="epoch ids to downscale lr and the downscale rate")
    p.add_argument("--wd", type=float, default=0.0001, help="weight decay")
    p.add_argument("--nviews", type=int, default=5, help="total number of views")
    p.add_argument("--batch_size", type=int, default=1,
                   help="samples per rank and step (train.py's DTU recipe: 2; focal_bld: 1 only)")
    p.add_argument("--numdepth", type=int, default=192, help="the number of depth values")
    p.add_argument("--interval_scale", type=float, default=1.06, help="the depth interval scale (dtu_yao)")
    p.add_argument("--loadckpt", default=None, help="load a specific checkpoint ('model' only, strict)")
    p.add_argument("--logdir", default="./checkpoints", help="the directory to save checkpoints/logs")
    p.add_argument("--resume", action="store_true", help="continue from the newest *.ckpt in --logdir")
    p.add_argument("--summary_freq", type=int, default=50, help="print and log frequency (iterations)")
    p.add_argument("--save_freq", type=int, default=1, help="save checkpoint frequency (epochs)")
    p.add_argument("--eval_freq", type=int, default=1, help="eval frequency (epochs)")
    p.add_argument("--seed", type=int, default=1, metavar="S", help="random seed")
    p.add_argument("--local_rank", type=int, default=0, help="the GPU of this process (LOCAL_RANK overrides)")
    p.add_argument("--ndepths", type=str, default="48,32,8", help="ndepths")
    p.add_argument("--dlossw", type=str, default=None,
                   help="depth loss weight per stage (default 1.0,1.0,1.0 for focal_bld, 0.5,1.0,2.0 for trans_mvsnet)")
    p.add_argument("--loss", default="auto", choices=["auto", "focal_bld", "trans_mvsnet"],
                   help="auto: focal_bld for bld_train, trans_mvsnet for dtu_yao")
    p.add_argument("--crop", type=str, default="512,640",
                   help="dtu_yao: target_h,target_w of prepare_img's centre crop (the image size)")
    p.add_argument("--sync_bn", action="store_true",
                   help="BatchNorm batch statistics over the samples of all ranks (SyncBN). The reference always "
                        "does this under torch.distributed (convert_sync_batchnorm before DDP); here it is off by "
                        "default, so runs without the flag keep their bits. A logged no-op with one process")
    p.add_argument("--workers", type=int, default=2, help=f"host decode threads (at most {MAX_WORKERS})")
    return p


def parse_args(argv=None):
    """The parsed arguments with finetune.py:285-289's checks: --resume only trains and excludes --loadckpt;
    --testpath defaults to --trainpath."""
    parser = make_parser()
    args = parser.parse_args(argv)
    if args.resume and args.mode != "train":
        parser.error("--resume needs --mode train")
    if args.resume and args.loadckpt is not None:
        parser.error("--resume and --loadckpt exclude each other")
    if args.batch_size < 1:
        parser.error(f"--batch_size must be at least 1, got {args.batch_size}")
    if args.batch_size > 1 and resolve_loss(args)[0] == "focal_bld":
        from .loss import FOCAL_BLD_BATCH_MSG
        parser.error(f"--batch_size {args.batch_size} with --loss focal_bld: {FOCAL_BLD_BATCH_MSG}")
    if args.testpath is None:
        args.testpath = args.trainpath
    return args


def resolve_loss(args):
    """(loss name, dlossw): --loss auto picks focal_bld for bld_train (finetune.py) and trans_mvsnet for
    dtu_yao (train.py), each with its script's default stage weights unless --dlossw is given."""
    name = args.loss
    if name == "auto":
        name = "focal_bld" if args.dataset == "bld_train" else "trans_mvsnet"
    if args.dlossw is not None:
        dlossw = [float(e) for e in args.dlossw.split(",") if e]
    else:
        dlossw = [1.0, 1.0, 1.0] if name == "focal_bld" else [0.5, 1.0, 2.0]
    if len(dlossw) != 3:
        raise ValueError(f"--dlossw needs three weights, got {dlossw}")
    return name, dlossw


def set_random_seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def _make_set(args, path, listfile, mode, device):
    return find_dataset_def(args.dataset)(path, listfile, mode, args.nviews, args.numdepth,
                                          interval_scale=args.interval_scale, device=device,
                                          target_hw=tuple(int(v) for v in args.crop.split(",")))


def main(argv=None):
    """Runs the command line; returns {"model", "optimizer", "metrics"} (metrics: --mode test's means)."""
    import torch.distributed as dist
    from .model import TransMVSNet
    from .train import FlatAdam
    args = parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", args.local_rank))
    if not torch.cuda.is_available():
        raise RuntimeError("transmvsnet_amd.finetune needs a GPU (the HIP path has no CPU fallback)")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    own_group = False
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(backend="nccl", init_method="env://", device_id=device)
        own_group = True
    try:
        set_random_seed(args.seed)
        main_rank = _rank() == 0
        if main_rank and args.mode == "train":
            os.makedirs(args.logdir, exist_ok=True)
        loss_name, dlossw = resolve_loss(args)
        model = TransMVSNet(ndepths=[int(n) for n in args.ndepths.split(",") if n])
        start_epoch, opt_state = 0, None
        if args.resume:
            ckpt = latest_checkpoint(args.logdir)
            print("resuming", ckpt, flush=True)
            state = torch.load(ckpt, map_location=torch.device("cpu"))
            model.load_state_dict(state["model"], strict=True)
            opt_state, start_epoch = state["optimizer"], state["epoch"] + 1
        elif args.loadckpt:
            print("loading model {}".format(args.loadckpt), flush=True)
            state = torch.load(args.loadckpt, map_location=torch.device("cpu"))
            model.load_state_dict(state["model"], strict=True)
        model = model.to(device)
        opt = FlatAdam(filter(lambda p: p.requires_grad, model.parameters()), lr=args.lr, betas=(0.9, 0.999),
                       weight_decay=args.wd)
        if opt_state is not None:
            opt.load_state_dict(opt_state)
        if args.sync_bn and _is_distributed():
            model.sync_batchnorm()  # train.py:361-366: convert_sync_batchnorm(model) whenever distributed
            if main_rank:
                print("BatchNorm statistics synchronised over {} ranks".format(dist.get_world_size()), flush=True)
        elif args.sync_bn:
            print("--sync_bn: one process, nothing to synchronise (statistics are this process's batch)", flush=True)
        if main_rank:
            print("start at epoch {}".format(start_epoch))
            print("Number of model parameters: {}".format(sum(p.numel() for p in model.parameters())), flush=True)
        test_set = None
        if args.testlist:
            test_set = _make_set(args, args.testpath, args.testlist, "test", device)
        metrics = None
        if args.mode == "train":
            train_set = _make_set(args, args.trainpath, args.trainlist, "train", device)
            train(model, opt, train_set, test_set, start_epoch, args, loss_name, dlossw)
        else:
            if test_set is None:
                raise SystemExit("finetune: --mode test needs --testlist")
            metrics = evaluate(model, test_set, args, loss_name, dlossw)
            if main_rank:
                print("final", metrics, flush=True)
        torch.cuda.synchronize(device)
        return {"model": model, "optimizer": opt, "metrics": metrics}
    finally:
        if own_group:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
