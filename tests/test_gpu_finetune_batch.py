"""python -m transmvsnet_amd.finetune --batch_size 2 on the GPU (needs an MI355X; -m gpu): four dtu_yao
samples of a small synthetic scan (128 x 160, N = 3, ndepths 8/8/8), two training steps per epoch.

  * one epoch writes its checkpoint and the JSON-lines records, with the iterations counted in batches;
  * two identical runs end bitwise equal (parameters, BatchNorm buffers, Adam moments), and one epoch followed
    by --resume equals two epochs uninterrupted, bitwise;
  * the first step is, bit for bit, a step made by hand: the same two samples stacked, model(...),
    trans_mvsnet_loss (dlossw 0.5, 1, 2), backward, FlatAdam at the driver's first learning rate;
  * evaluation runs batches of two and logs the mean over the batches.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests._util import golden_state_dict
from tests.test_gpu_finetune import _ckpt_diff
from transmvsnet_amd import data, finetune, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
PICK = (0, 8, 15, 20)  # four of the scan's 21 (viewpoint, light) samples: every viewpoint, four lights


@pytest.fixture(scope="module")
def four_samples(tmp_path_factory):
    """(root, listfile) of a dtu_yao scan whose sample list is cut to PICK for this module."""
    root = str(tmp_path_factory.mktemp("dtu4"))
    listfile = synthetic.write_dtu_train_scan(root, n_views=3, height=128, width=160)
    full = data.build_list_dtu_train
    mp = pytest.MonkeyPatch()
    mp.setattr(data, "build_list_dtu_train", lambda datapath, lf: [full(datapath, lf)[i] for i in PICK])
    yield root, listfile
    mp.undo()


@pytest.fixture(scope="module")
def golden_ckpt(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ckpt") / "golden.ckpt")
    torch.save({"model": golden_state_dict()}, path)
    return path


def _args(root, listfile, ckpt, logdir, epochs, *more):
    return ["--mode", "train", "--dataset", "dtu_yao", "--batch_size", "2", "--trainpath", root, "--trainlist",
            listfile, "--ndepths", "8,8,8", "--nviews", "3", "--crop", "128,160", "--epochs", str(epochs),
            "--summary_freq", "1", "--logdir", logdir, *(("--loadckpt", ckpt) if ckpt else ()), *more]


def _records(logdir, mode="train"):
    with open(os.path.join(logdir, "train.jsonl")) as f:
        return [r for r in map(json.loads, f) if r["mode"] == mode]


@pytest.fixture(scope="module")
def two_epochs(four_samples, golden_ckpt, tmp_path_factory):
    """The uninterrupted run, with the flat parameters as they stand after its first step."""
    root, listfile = four_samples
    logdir = str(tmp_path_factory.mktemp("run2"))
    after_first = []
    step = finetune.train_sample

    def spy(model, opt, sample, *a):
        out = step(model, opt, sample, *a)
        if not after_first:
            assert isinstance(sample, list) and len(sample) == 2
            after_first.append(opt.flat.clone())
        return out

    mp = pytest.MonkeyPatch()
    mp.setattr(finetune, "train_sample", spy)
    try:
        res = finetune.main(_args(root, listfile, golden_ckpt, logdir, 2, "--testlist", listfile))
    finally:
        mp.undo()
    return logdir, res, after_first[0]


def test_driver_batch_of_two_trains_and_logs(two_epochs):
    logdir, res, _ = two_epochs
    assert sorted(f for f in os.listdir(logdir) if f.endswith(".ckpt")) == ["model_000000.ckpt", "model_000001.ckpt"]
    state = torch.load(os.path.join(logdir, "model_000000.ckpt"), map_location="cpu")
    assert set(state) == {"epoch", "model", "optimizer"} and state["epoch"] == 0 and len(state["model"]) == 465
    assert float(state["optimizer"]["state"][0]["step"]) == 2.0  # 4 samples at B = 2: two steps per epoch
    assert res["optimizer"].step_count == 4
    recs = _records(logdir)
    milestones, gamma = finetune.parse_lrepochs("10,12,14:2", 2)
    assert [(r["epoch"], r["iteration"], r["batch"]) for r in recs] == [(0, 0, 0), (0, 1, 1), (1, 2, 0), (1, 3, 1)]
    for it, r in enumerate(recs):
        assert r["applied"] and r["lr"] == finetune.warmup_multistep_lr(0.001, it, milestones, gamma)
        for k in ("loss", "depth_loss", "entropy_loss", "step_seconds", "data_wait_seconds"):
            assert np.isfinite(r[k]), (it, k)
    # a FeatureNet BatchNorm has seen N = 3 calls per step, the PixelwiseNet's N - 1, a CostRegNet's one
    assert int(state["model"]["feature.conv0.0.bn.num_batches_tracked"]) == 6
    assert int(state["model"]["DepthNet.pixel_wise_net.conv0.bn.num_batches_tracked"]) == 4
    assert int(state["model"]["cost_regularization.0.conv0.bn.num_batches_tracked"]) == 2
    # evaluation after each epoch: two batches of two, the twelve dtu_yao scalars and the loss terms
    tests = _records(logdir, "fulltest")
    assert [r["epoch"] for r in tests] == [0, 1] and [r["iteration"] for r in tests] == [1, 3]
    for r in tests:
        assert set(ops.EVAL_METRIC_NAMES) <= set(r) and {"loss", "depth_loss", "entropy_loss"} <= set(r)
        assert all(np.isfinite(r[k]) for k in ops.EVAL_METRIC_NAMES)
        assert 0 <= r["thres20mm_error"] <= r["thres2mm_error"] <= 1


def test_driver_batch_runs_repeat_and_resume_bitwise(two_epochs, four_samples, golden_ckpt, tmp_path):
    root, listfile = four_samples
    first = os.path.join(two_epochs[0], "model_000001.ckpt")
    again = str(tmp_path / "again")
    finetune.main(_args(root, listfile, golden_ckpt, again, 2))
    equal, worst = _ckpt_diff(os.path.join(again, "model_000001.ckpt"), first)
    print("two identical runs at batch 2: bitwise", equal, "largest relative difference", worst)
    assert equal, worst
    split = str(tmp_path / "split")
    finetune.main(_args(root, listfile, golden_ckpt, split, 1))
    assert os.listdir(split).count("model_000000.ckpt") == 1
    res = finetune.main(_args(root, listfile, None, split, 2, "--resume"))
    assert res["optimizer"].step_count == 4
    equal, worst = _ckpt_diff(os.path.join(split, "model_000001.ckpt"), first)
    print("one epoch + --resume vs uninterrupted at batch 2: bitwise", equal, "largest relative difference", worst)
    assert equal, worst
    assert [r["iteration"] for r in _records(split)] == [0, 1, 2, 3]
    assert [r["lr"] for r in _records(split)] == [r["lr"] for r in _records(two_epochs[0])]


def test_first_step_is_the_hand_made_step(two_epochs, four_samples):
    """train.py:137-161's body written out on the first batch of the driver's order."""
    from transmvsnet_amd import TransMVSNet
    from transmvsnet_amd import loss as hip_loss
    from transmvsnet_amd.train import FlatAdam
    root, listfile = four_samples
    ds = finetune.DtuTrainSet(root, listfile, "train", 3, 192, 1.06, device=DEV, target_hw=(128, 160))
    assert len(ds) == 4
    first = finetune.batches(finetune.epoch_order(len(ds), 1, 0), 2, True)[0]
    samples = [ds.sample(i) for i in first]
    assert not torch.equal(samples[0]["imgs"], samples[1]["imgs"])
    model = TransMVSNet(ndepths=[8, 8, 8])
    model.load_state_dict(golden_state_dict(), strict=True)
    model = model.to(DEV)
    opt = FlatAdam(filter(lambda p: p.requires_grad, model.parameters()), lr=0.001, betas=(0.9, 0.999),
                   weight_decay=0.0001)
    opt.lr = finetune.warmup_multistep_lr(0.001, 0, *finetune.parse_lrepochs("10,12,14:2", 2))
    imgs = torch.stack([s["imgs"] for s in samples])
    proj = {k: torch.stack([torch.from_numpy(s["proj_matrix"][k]) for s in samples]) for k in samples[0]["proj_matrix"]}
    dv = torch.stack([torch.from_numpy(s["depth_values"]) for s in samples]).to(DEV)
    depth = {k: torch.stack([s["depth"][k] for s in samples]) for k in samples[0]["depth"]}
    mask = {k: torch.stack([s["mask"][k] for s in samples]) for k in samples[0]["mask"]}
    model.train()
    opt.zero_grad()
    outputs = model(imgs, proj, dv)
    assert outputs["depth"].shape == (2, 128, 160) and outputs["stage1"]["prob_volume"].shape == (2, 8, 32, 40)
    total = hip_loss.trans_mvsnet_loss(outputs, depth, mask, dlossw=[0.5, 1.0, 2.0])[0]
    total.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(opt.flat, two_epochs[2]), float((opt.flat - two_epochs[2]).abs().max())
    total = float(total.detach())
    assert abs(total - _records(two_epochs[0])[0]["loss"]) <= 1e-6 * abs(total)
