"""The reference's train_sample body on a batch of two, on the drop-in model (needs an MI355X; -m gpu):

    model.train(); outputs = model(imgs, proj_matrix, depth_values)          # imgs [2, N, 3, H, W]
    loss, depth_loss, entropy_loss, depth_entropy = trans_mvsnet_loss(outputs, depth_gt_ms, mask_ms,
                                                                      dlossw=[0.5, 1.0, 2.0])
    loss.backward()

against tests/golden/train_c1_b2*.npz (the reference's own run of train.py:137-161 at C1 size, B = 2) and the
float64 oracle that tests/test_train_oracle_batch.py pins to it. The bars are those of
tests/test_gpu_train_ref.py, computed the same way: every one of the 318 gradients within max(1e-4, 2x the fp32
spread) of the float64 evaluation, the spread being the worst distance from float64 over the fixture's own fp32
run and 4 fp32 oracle runs whose images are jittered by ~1 ulp (exactly-zero gradients judged absolutely, as
there); loss terms within 1e-5 relative; prob volumes within max(1e-4, 3x the reference's fp32 distance from
float64); WTA depths identical outside the 1e-4 near-tie margin; running statistics within 1e-5 and
num_batches_tracked exact. Both backward routes: transmvsnet_amd.loss (the `_tmvs_logits` shortcut) and the
reference's torch-op loss through prob_volume.

Also: the statistics are the batch's (each sample alone leaves a FeatureNet, a PixelwiseNet and a CostRegNet
running mean elsewhere, by far more than the bar), and a batch of one is today's single-sample path bit for bit.
"""
import numpy as np
import pytest
import torch

from tests import _train_b2 as b2
from tests._util import golden_rot, golden_state_dict
from tests.test_gpu_train_ref import ENSEMBLE, _check_buffers, _judge, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, N = b2.H, b2.W, b2.N


@pytest.fixture(scope="module")
def gold():
    return b2.load_parts()


@pytest.fixture(scope="module")
def exact(gold):
    """(float64 gradients, {}, float64 prob volumes, per-gradient fp32 spread), as tests/test_gpu_train_ref.exact"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _, o, sd = b2.train_step_oracle(gold, dtype=torch.float64)
    grads = {k: v.grad.detach().numpy() for k, v in sd.items() if v.requires_grad and v.grad is not None}
    prob = {s: o[f"stage{s}"]["prob_volume"].detach().numpy() for s in (1, 2, 3)}
    spread = {n: _rel(gold[f"i_grad.{n}"], grads[n]) for n in grads}
    for e in range(ENSEMBLE):
        sd_e = b2.train_step_oracle(gold, perturb_seed=1000 + e)[2]
        for n in grads:
            spread[n] = max(spread[n], _rel(sd_e[n].grad.detach().numpy(), grads[n]))
    return grads, {}, prob, spread


def _model():
    from transmvsnet_amd import TransMVSNet
    m = TransMVSNet(ndepths=list(b2.ND))
    m.load_state_dict(golden_state_dict(sharpen=b2.TRAIN_SHARPEN), strict=True)
    return m.to(DEV)


def _inputs():
    imgs, proj, dv = b2.inputs()
    return imgs.to(DEV), proj, dv.to(DEV)


def _check_outputs(gold, outputs, loss_terms, exact_prob):
    for name, v in zip(("loss", "depth_loss", "entropy_loss"), loss_terms):
        ref = float(gold[f"i_{name}"])
        v = float(v.detach())
        print(name, v, "reference", ref)
        assert abs(v - ref) <= 1e-5 * max(abs(ref), 1.0), (name, v, ref)
    rep = {}
    for s in (1, 2, 3):
        o = outputs[f"stage{s}"]
        for k in ("depth", "photo_confidence"):
            assert o[k].shape[0] == b2.B, (s, k, tuple(o[k].shape))
        np.testing.assert_array_equal(o["depth_values"].detach().cpu().numpy(), gold[f"i_stage{s}_hyp"])
        ref = gold[f"i_stage{s}_prob"].astype(np.float64)
        assert tuple(o["prob_volume"].shape) == ref.shape
        srt = np.sort(ref, axis=1)  # WTA depth identical except at the reference's near ties
        near = (np.log(np.maximum(srt[:, -1], 1e-30)) - np.log(np.maximum(srt[:, -2], 1e-30))) < 1e-4
        diff = o["depth"].detach().cpu().numpy() != gold[f"i_stage{s}_depth"]
        assert not (diff & ~near).any(), (s, int(diff.sum()), int((diff & ~near).sum()))
        ex = exact_prob[s]
        e_gpu = float(np.abs(o["prob_volume"].detach().cpu().numpy() - ex).max())
        e_ref = float(np.abs(ref - ex).max())
        rep[s] = (e_gpu, e_ref)
        assert e_gpu <= max(1e-4, 3.0 * e_ref), (s, e_gpu, e_ref)
    for k in ("depth", "photo_confidence", "prob_volume", "depth_values"):  # the top-level keys are stage 3's
        assert outputs[k] is outputs["stage3"][k]
    print("prob vs fp64 per stage (gpu, fp32 reference):", rep)


@pytest.mark.parametrize("loss_impl", ["hip", "reference_torch_ops"])
def test_train_sample_body_batch_of_two_vs_reference(gold, exact, loss_impl):
    from oracle import loss_ref
    from transmvsnet_amd import loss as hip_loss
    loss_fn = hip_loss.trans_mvsnet_loss if loss_impl == "hip" else loss_ref.trans_mvsnet_loss
    model = _model()
    imgs, proj, dv = _inputs()
    gt, mask = b2.targets(gold, DEV)
    with golden_rot(model):
        model.train()
        outputs = model(imgs, proj, dv)
        loss, depth_loss, entropy, _ = loss_fn(outputs, gt, mask, dlossw=list(b2.DLOSSW))
        loss.backward()
    torch.cuda.synchronize()
    _check_outputs(gold, outputs, (loss, depth_loss, entropy), exact[2])
    grads = {n: p.grad.detach().cpu().numpy() for n, p in model.named_parameters() if p.grad is not None}
    assert len(grads) == 318
    _judge(gold, exact, "i", grads)
    _check_buffers(gold, "i", model)


def test_statistics_are_the_batch_s_not_a_sample_s(gold):
    """Sample 0 alone and sample 1 alone leave the running means elsewhere than the batch of two does."""
    imgs, proj, dv = _inputs()
    names = ("feature.conv0.0.bn.running_mean", "feature.out1.2.running_mean",
             "DepthNet.pixel_wise_net.conv0.bn.running_mean", "DepthNet.pixel_wise_net.conv1.bn.running_mean",
             "cost_regularization.0.conv0.bn.running_mean", "cost_regularization.2.conv6.bn.running_mean")
    for b in range(b2.B):
        model = _model()
        model.train()
        with golden_rot(model), torch.no_grad():
            out = model(imgs[b:b + 1], {k: v[b:b + 1] for k, v in proj.items()}, dv[b:b + 1])
        assert out["depth"].shape == (1, H, W)
        bufs = dict(model.named_buffers())
        for n in names:
            away = float(np.abs(bufs[n].cpu().numpy() - gold["i_buf." + n]).max())
            print(f"sample {b} alone, {n}: {away:.3e} from the batch's")
            # the batched run is within the 1e-5 bar of the fixture (_check_buffers): twice the bar away from the
            # fixture is more than the bar away from the batched run
            assert away > 2e-5, (b, n, away)


def test_batch_of_one_is_the_single_sample_path_bitwise():
    """model(imgs[:1], ...) against featurenet_train / fmt_train / pathway_train / depth_stages_forward_train
    called the single-sample way, outputs, gradients and BatchNorm buffers bit for bit."""
    from transmvsnet_amd import loss as hip_loss
    from transmvsnet_amd.featurenet_train import featurenet_train
    from transmvsnet_amd.train import depth_stages_forward_train, fmt_train, pathway_train
    imgs, proj, dv = _inputs()
    imgs, proj, dv = imgs[:1], {k: v[:1] for k, v in proj.items()}, dv[:1]
    g = torch.Generator().manual_seed(3)
    gt = {s: (520.0 + 300.0 * torch.rand(1, H >> k, W >> k, generator=g)).to(DEV)
          for s, k in zip(b2.STAGES, (2, 1, 0))}
    mask = {s: torch.ones_like(v) for s, v in gt.items()}
    runs = []
    for whole in (True, False):
        model = _model()
        model.train()
        with golden_rot(model):
            if whole:
                out = model(imgs, proj, dv)
            else:
                s1, s2, s3 = featurenet_train(model.feature, imgs[0])
                assert s1.dim() == 4
                st1 = fmt_train(model, s1)
                st2, st3 = pathway_train(model, st1, s2, s3)
                out = depth_stages_forward_train(model, {"stage1": st1, "stage2": st2, "stage3": st3}, proj, dv, (H, W))
            hip_loss.trans_mvsnet_loss(out, gt, mask, dlossw=list(b2.DLOSSW))[0].backward()
        torch.cuda.synchronize()
        runs.append(({f"stage{s}.{k}": out[f"stage{s}"][k].detach().clone() for s in (1, 2, 3)
                      for k in ("depth", "photo_confidence", "prob_volume", "depth_values")},
                     {n: p.grad.detach().clone() for n, p in model.named_parameters()},
                     {n: b.detach().clone() for n, b in model.named_buffers()}))
    for a, b in zip(runs[0], runs[1]):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k
    # featurenet_train's two call forms: [1, N, 3, H, W] is [N, 3, H, W] with a leading axis, bit for bit
    m1, m2 = _model(), _model()
    with torch.no_grad():
        a = featurenet_train(m1.feature, imgs[0])
        b = featurenet_train(m2.feature, imgs)
    for x, y in zip(a, b):
        assert y.shape == (1, *x.shape) and torch.equal(x, y[0])
    assert all(torch.equal(p, q) for p, q in zip(m1.feature.buffers(), m2.feature.buffers()))
