"""The oracle's TRAIN mode on a batch of two against the reference's own training step
(tests/golden/train_c1_b2*.npz, made by tests/golden/make_golden_train_b2.py: train.py:137-161's train_sample
body with trans_mvsnet_loss, dlossw 0.5, 1, 2, at C1 size, B = 2, from images). CPU only.

Pins at B = 2 what tests/test_train_oracle.py pins at B = 1, to the same bar: oracle.forward(training=True)
-- the BatchNorm batch statistics over the batch (FeatureNet per view over B*h*w, PixelwiseNet per view
over B*D*h*w, the CostRegNets over B*D*h*w), their running-statistic updates, the autograd of every block
-- and oracle/loss_ref.trans_mvsnet_loss (the mean over the batch of the per-sample masked means). Every
quantity within 1e-6 relative of the reference's, the WTA depths identical, num_batches_tracked exact.
The GPU tests of the batched step (tests/test_gpu_train_batch.py) are judged against this oracle in float64.
"""
import numpy as np
import pytest

from tests import _train_b2 as b2


@pytest.fixture(scope="module")
def gold():
    return b2.load_parts()


def test_fixture_is_a_batch_of_two_different_samples(gold):
    imgs, proj, dv = b2.inputs()
    assert imgs.shape == (b2.B, b2.N, 3, b2.H, b2.W) and dv.shape[0] == b2.B
    assert not np.array_equal(imgs[0].numpy(), imgs[1].numpy())
    assert all(not np.array_equal(p[0].numpy(), p[1].numpy()) for p in proj.values())
    for s in b2.STAGES:
        assert gold[f"gt_{s}"].shape[0] == b2.B and not np.array_equal(gold[f"gt_{s}"][0], gold[f"gt_{s}"][1])
        assert not np.array_equal(gold[f"mask_{s}"][0], gold[f"mask_{s}"][1])
    assert sum(1 for k in gold if k.startswith("i_grad.")) == 318
    for s in (1, 2, 3):
        assert gold[f"i_stage{s}_prob"].shape[0] == b2.B == gold[f"i_stage{s}_depth"].shape[0]


def test_oracle_train_step_batch_of_two(gold):
    res, out, sd = b2.train_step_oracle(gold)
    worst = {}
    for name, v in zip(("loss", "depth_loss", "entropy_loss"), res):
        ref = float(gold[f"i_{name}"])
        worst[name] = abs(float(v.detach()) - ref) / max(abs(ref), 1e-30)
    for s in (1, 2, 3):
        o = out[f"stage{s}"]
        assert np.array_equal(o["depth"].detach().numpy(), gold[f"i_stage{s}_depth"]), s
        assert np.array_equal(o["depth_values"].detach().numpy(), gold[f"i_stage{s}_hyp"]), s
        worst[f"stage{s}_prob"] = float(np.abs(o["prob_volume"].detach().numpy() - gold[f"i_stage{s}_prob"]).max())
    names = [k[len("i_grad."):] for k in gold if k.startswith("i_grad.")]
    grads = [k for k, v in sd.items() if v.requires_grad and v.grad is not None]
    assert sorted(names) == sorted(grads), set(names) ^ set(grads)
    gmax = 0.0
    for n in names:
        ref = gold["i_grad." + n]
        gmax = max(gmax, float(np.abs(sd[n].grad.numpy() - ref).max()) / max(float(np.abs(ref).max()), 1e-30))
    worst["param_grads"] = gmax
    bmax, tracked = 0.0, 0
    for k in gold:
        if k.startswith("i_buf."):
            n = k[len("i_buf."):]
            if n.endswith("num_batches_tracked"):
                assert int(sd[n]) == int(gold[k]), n
                tracked += 1
            else:
                bmax = max(bmax, float(np.abs(sd[n].detach().numpy() - gold[k]).max()))
    assert tracked == 49  # 17 FeatureNet (+N each), 30 CostRegNet (+1), 2 PixelwiseNet (+N-1)
    worst["running_stats"] = bmax
    print(worst)
    assert all(v <= 1e-6 for v in worst.values()), worst
