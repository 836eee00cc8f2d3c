"""Golden vectors for a TRAINING step on a batch of two, from the REAL reference (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_b2.py

Imports the reference's models as make_golden_train.py does (load_reference) and runs train.py's
train_sample body (train.py:137-161) at C1 size (128x160, N=3, ndepths 8/8/8, the TRAIN_SHARPEN weights of
make_golden_train.py) on B = 2 samples, from images (FeatureNet + DCN included):

    model.train(); outputs = model(imgs, proj_matrix, depth_values)
    loss, depth_loss, entropy_loss, depth_entropy = trans_mvsnet_loss(outputs, depth_gt_ms, mask_ms,
                                                                      dlossw=[0.5, 1.0, 2.0])
    loss.backward()

A batch of two is not two steps of one: every train-mode BatchNorm takes its statistics over the batch
(FeatureNet's per view over B*h*w, PixelwiseNet's per view over B*D*h*w, the CostRegNets' over B*D*h*w) and
the loss is the mean over the batch. The two samples differ in images, cameras and ground truth (checked).
Stores the loss terms, the train-mode outputs (depth, prob volume, hypotheses per stage), every parameter
gradient and every BatchNorm buffer after the step, under the keys of train_c1.npz's case "i". Writes
tests/golden/train_c1_b2.npz and its parts train_c1_b2.pNN.npz (tests/_train_b2.py: each part below the
size limit for a committed file): data only.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(os.path.dirname(HERE)))

from make_golden import load_reference  # noqa: E402
from tests import _train_b2 as b2  # noqa: E402
from transmvsnet_amd import synthetic  # noqa: E402


def ground_truth(seed):
    """make_golden_train.ground_truth with its seed as an argument (11 there)."""
    h, w = b2.H, b2.W
    g = torch.Generator().manual_seed(seed)
    coarse = 520.0 + 300.0 * torch.rand(1, 1, 8, 10, generator=g)
    d3 = F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=False)[:, 0]
    d3 = d3 + 2.0 * torch.randn(1, h, w, generator=g)
    m3 = (torch.rand(1, h, w, generator=g) > 0.2).float()
    gt, mask = {"stage3": d3.contiguous()}, {"stage3": m3}
    for s, f in (("stage2", 2), ("stage1", 4)):
        gt[s] = d3[:, ::f, ::f].contiguous()
        mask[s] = m3[:, ::f, ::f].contiguous()
    return gt, mask


def main():
    TransMVSNet, ref_module, _ = load_reference()
    torch.manual_seed(0)
    shapes = synthetic.state_dict_shapes(TransMVSNet())
    sd = synthetic.synthetic_state_dict(shapes, seed=0, sharpen=b2.TRAIN_SHARPEN)
    imgs, proj, dv = b2.inputs()
    per = [ground_truth(s) for s in b2.GT_SEEDS]
    gt = {s: torch.cat([g[s] for g, _ in per]) for s in b2.STAGES}
    mask = {s: torch.cat([m[s] for _, m in per]) for s in b2.STAGES}
    assert imgs.shape[0] == b2.B and not torch.equal(imgs[0], imgs[1])
    assert all(not torch.equal(p[0], p[1]) for p in proj.values())
    assert all(not torch.equal(gt[s][0], gt[s][1]) and not torch.equal(mask[s][0], mask[s][1]) for s in b2.STAGES)
    out = {}
    for s in b2.STAGES:
        out[f"gt_{s}"] = gt[s].numpy()
        out[f"mask_{s}"] = mask[s].numpy()
    model = TransMVSNet(ndepths=list(b2.ND))
    model.load_state_dict(sd, strict=True)
    model.train()
    outputs = model(imgs, proj, dv)
    loss, depth_loss, entropy, _ = ref_module.trans_mvsnet_loss(outputs, gt, mask, dlossw=list(b2.DLOSSW))
    loss.backward()
    out.update({"i_loss": loss.detach().numpy(), "i_depth_loss": depth_loss.detach().numpy(),
                "i_entropy_loss": entropy.detach().numpy()})
    for s in (1, 2, 3):
        o = outputs[f"stage{s}"]
        out[f"i_stage{s}_depth"] = o["depth"].detach().numpy()
        out[f"i_stage{s}_prob"] = o["prob_volume"].detach().numpy()
        out[f"i_stage{s}_hyp"] = o["depth_values"].detach().numpy()
    for n, p in model.named_parameters():
        if p.grad is not None:
            out[f"i_grad.{n}"] = p.grad.numpy()
    for n, b in model.named_buffers():
        if "running" in n or "num_batches_tracked" in n:
            out[f"i_buf.{n}"] = b.numpy()
    names = b2.save_parts(b2.GOLD, out)
    sizes = [os.path.getsize(n) for n in names]
    print("wrote", len(names), "parts,", sum(sizes), "bytes, largest", max(sizes),
          {k: float(v) for k, v in out.items() if v.ndim == 0})
    print("grads:", sum(1 for k in out if k.startswith("i_grad.")))


if __name__ == "__main__":
    main()
