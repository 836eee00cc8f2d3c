"""A training step with BatchNorm statistics synchronised across ranks, two ranks on one card (needs an MI355X;
-m gpu): spawned processes, gloo over a file store, both ranks on cuda:0 with device tensors, as
tests/test_gpu_distributed.py runs its ranks -- the collective is the production one (SyncBN.reduce: one
all_reduce of zero-filled slots, then tmvs_rank_sum on the device).

(1) Two ranks x one sample with synchronised statistics and the gradient mean are, in exact arithmetic, the
    one-process batch of two that tests/golden/train_c1_b2*.npz records from the reference's own run. Rank r
    takes sample r: model.sync_batchnorm(group), the train-mode forward, trans_mvsnet_loss, backward, one
    all-reduce mean of the gradients. Every buffer (running statistics) is bitwise equal across the ranks and
    within the fixture's bar (_check_buffers); the 318 mean gradients pass _judge against the float64 oracle
    (tests/test_gpu_train_batch.py's bars and its `exact`, imported). Per-rank statistics cannot pass:
    test_statistics_are_the_batch_s_not_a_sample_s shows a single sample's running means more than twice the
    buffer bar away. The distance of the two-rank mean gradients from the one-process B = 2 GPU step is printed
    per tensor, not asserted (the two differ in summation order only).
(2) The driver: each worker initialises gloo itself (finetune.main skips its own init when a group exists), sets
    WORLD_SIZE=2, its RANK and LOCAL_RANK=0, and runs finetune.main([... "--sync_bn"]) on a written BlendedMVS
    scan (4 views, 128x160, one epoch: two steps per rank). Both ranks end with bitwise-equal parameters, Adam
    moments and BatchNorm buffers, only rank 0 writes the checkpoint, and a second identical run reproduces the
    checkpoint bitwise.
"""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _train_b2 as b2
from tests._util import golden_rot, golden_state_dict
from tests.test_gpu_finetune import _ckpt_diff, _records, _train_args
from tests.test_gpu_train_batch import _inputs, _model, exact, gold  # noqa: F401  (module-scoped fixtures)
from tests.test_gpu_train_ref import _check_buffers, _judge, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORLD = 2


def _store():
    return "file://" + os.path.join(tempfile.mkdtemp(prefix="tmvs_sync_bn_step_"), "store")


def _run_ranks(target, *args, timeout=300):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    store = _store()
    procs = [ctx.Process(target=target, args=(r, WORLD, store, q, *args)) for r in range(WORLD)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(WORLD):
        out = q.get(timeout=timeout)
        res[out[0]] = out[1:]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def _np_dict(named):
    return {n: t.detach().cpu().numpy().copy() for n, t in named}


# ------------------------------------------------------------------ (1) the step against the reference's B = 2 run
def _step_worker(rank, world, store, q):
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=store, rank=rank, world_size=world)
    try:
        from transmvsnet_amd import loss as hip_loss
        from transmvsnet_amd.train import allreduce_gradients
        fixture = b2.load_parts()
        model = _model()
        assert model.sync_batchnorm(dist.group.WORLD) is model
        imgs, proj, dv = _inputs()
        gt, mask = b2.targets(fixture, DEV)
        one = slice(rank, rank + 1)  # rank r takes sample r
        with golden_rot(model):
            model.train()
            outputs = model(imgs[one], {k: v[one] for k, v in proj.items()}, dv[one])
            loss = hip_loss.trans_mvsnet_loss(outputs, {k: v[one] for k, v in gt.items()},
                                              {k: v[one] for k, v in mask.items()}, dlossw=list(b2.DLOSSW))[0]
            loss.backward()
        record = model.sync_bn.record()
        allreduce_gradients(list(model.parameters()))
        torch.cuda.synchronize()
        q.put((rank, _np_dict((n, p.grad) for n, p in model.named_parameters() if p.grad is not None),
               _np_dict(model.named_buffers()), record))
    finally:
        dist.destroy_process_group()


def test_two_ranks_of_one_sample_are_the_reference_s_batch_of_two(gold, exact):  # noqa: F811
    res = _run_ranks(_step_worker, timeout=600)
    (grads0, bufs0, rec0), (grads1, bufs1, rec1) = res[0], res[1]
    print("collectives per step (count, bytes):", rec0)
    assert rec0 == rec1 and rec0["collectives"] > 0
    # the running statistics are identical on every rank, bit for bit, and the reference's batch-of-two's
    assert bufs0.keys() == bufs1.keys() and len(bufs0) > 0
    for n in bufs0:
        assert np.array_equal(bufs0[n], bufs1[n]), n
    from transmvsnet_amd import TransMVSNet
    holder = TransMVSNet(ndepths=list(b2.ND))
    holder.load_state_dict({**golden_state_dict(sharpen=b2.TRAIN_SHARPEN), **{n: torch.from_numpy(v) for n, v in bufs0.items()}},
                           strict=True)
    _check_buffers(gold, "i", holder)
    # the mean gradients: identical on both ranks, and within the project's bar of the float64 batch-of-two step
    assert len(grads0) == 318
    for n in grads0:
        assert np.array_equal(grads0[n], grads1[n]), n
    _judge(gold, exact, "i", grads0)

    # not asserted: how far the two-rank step is from the one-process B = 2 step on this GPU
    from transmvsnet_amd import loss as hip_loss
    model = _model()
    imgs, proj, dv = _inputs()
    gt, mask = b2.targets(gold, DEV)
    with golden_rot(model):
        model.train()
        hip_loss.trans_mvsnet_loss(model(imgs, proj, dv), gt, mask, dlossw=list(b2.DLOSSW))[0].backward()
    torch.cuda.synchronize()
    scale = float(np.median([np.abs(g).max() for g in exact[0].values()]))
    zero = {n for n, g in exact[0].items() if float(np.abs(g).max()) < 1e-7 * scale}  # _judge's exactly-zero gradients
    dist_b2 = sorted(((_rel(grads0[n], p.grad.cpu().numpy()), n) for n, p in model.named_parameters() if n not in zero),
                     reverse=True)
    print(f"two-rank mean gradients vs the one-process B = 2 GPU step, worst relative distances over {len(dist_b2)} "
          f"tensors (the {len(zero)} gradients that are exactly zero in fp64 left out):",
          [(f"{e:.2e}", n) for e, n in dist_b2[:6]])
    bdist = max(float(np.abs(bufs0[n].astype(np.float64) - b.cpu().numpy()).max()) for n, b in model.named_buffers())
    print(f"running statistics vs the one-process B = 2 GPU step, worst absolute distance: {bdist:.2e}")


# ------------------------------------------------------------------ (2) the driver
def _driver_worker(rank, world, store, q, argv):
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=store, rank=rank, world_size=world)
    try:
        os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK="0")
        from transmvsnet_amd import finetune as ft
        saves = []
        save = ft.save_checkpoint
        ft.save_checkpoint = lambda path, *a: (saves.append(path), save(path, *a))
        res = ft.main(argv)
        opt, model = res["optimizer"], res["model"]
        assert model.sync_bn is not None and model.sync_bn.world == world
        q.put((rank, opt.flat.cpu().numpy().copy(), opt.exp_avg.cpu().numpy().copy(),
               opt.exp_avg_sq.cpu().numpy().copy(), _np_dict(model.named_buffers()), saves, model.sync_bn.record()))
    finally:
        dist.destroy_process_group()


def test_driver_two_ranks_sync_bn(tmp_path):
    from transmvsnet_amd import synthetic
    ckpt = str(tmp_path / "golden.ckpt")
    torch.save({"model": golden_state_dict()}, ckpt)
    root = str(tmp_path / "scan")
    listfile = synthetic.write_blended_scan(root, n_views=4, height=128, width=160)
    logs = [str(tmp_path / "log_a"), str(tmp_path / "log_b")]
    for logdir in logs:
        res = _run_ranks(_driver_worker, _train_args(root, listfile, ckpt, logdir, 1, "--sync_bn"), timeout=600)
        (flat0, m0, v0, bufs0, saves0, rec0), (flat1, m1, v1, bufs1, saves1, _) = res[0], res[1]
        np.testing.assert_array_equal(flat0, flat1)
        np.testing.assert_array_equal(m0, m1)
        np.testing.assert_array_equal(v0, v1)
        for n in bufs0:
            assert np.array_equal(bufs0[n], bufs1[n]), n
        assert saves0 == [os.path.join(logdir, "model_000000.ckpt")] and saves1 == []  # only rank 0 writes
        assert len(_records(logdir)) == 2  # 4 samples over 2 ranks: two steps each
        assert rec0["collectives"] > 0
    equal, worst = _ckpt_diff(os.path.join(logs[0], "model_000000.ckpt"), os.path.join(logs[1], "model_000000.ckpt"))
    print("two identical synchronised runs: bitwise", equal, "largest relative difference", worst)
    assert equal, worst


def _nccl_worker(rank, world, store, q, argv):
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", init_method=store, rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    try:
        os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank))
        from transmvsnet_amd import finetune as ft
        res = ft.main(argv)
        opt, model = res["optimizer"], res["model"]
        q.put((rank, opt.flat.cpu().numpy().copy(), opt.exp_avg.cpu().numpy().copy(), _np_dict(model.named_buffers())))
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_driver_two_gpus_sync_bn_nccl(tmp_path):
    """The same over RCCL, one process per GPU: bitwise-equal parameters, moments and buffers on both ranks."""
    from transmvsnet_amd import synthetic
    ckpt = str(tmp_path / "golden.ckpt")
    torch.save({"model": golden_state_dict()}, ckpt)
    root = str(tmp_path / "scan")
    listfile = synthetic.write_blended_scan(root, n_views=4, height=128, width=160)
    res = _run_ranks(_nccl_worker, _train_args(root, listfile, ckpt, str(tmp_path / "log"), 1, "--sync_bn"), timeout=600)
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    for n in res[0][2]:
        assert np.array_equal(res[0][2][n], res[1][2][n]), n
