"""What the batch-of-two training tests share: the fixture tests/golden/train_c1_b2*.npz (made by
tests/golden/make_golden_train_b2.py from the reference: train.py:137-161's train_sample body with
trans_mvsnet_loss, dlossw 0.5, 1, 2, at C1 size and B = 2), its inputs, and the same step through the oracle.

The fixture is several .npz parts, each below the size limit for a committed file: `save_parts` cuts an
array that is too large for one part along its first axis (keys "name#0", "name#1", ...), and `load_parts`
puts them together again. Data only.
"""
import glob
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden", "train_c1_b2.npz")
H, W, N, ND, B = 128, 160, 3, (8, 8, 8), 2
TRAIN_SHARPEN = 10.0  # tests/golden/make_golden_train.py
DLOSSW = [0.5, 1.0, 2.0]  # train.py's default
STAGES = ("stage1", "stage2", "stage3")
GT_SEEDS = (11, 12)  # sample 0's is make_golden_train.ground_truth's
PART_BYTES = 900 << 10  # uncompressed payload per part (compression only shrinks it)


def save_parts(path, arrays):
    """arrays {key: ndarray} -> path (part 0) and path[:-4] + '.pNN.npz', each at most PART_BYTES of payload."""
    items = []
    for k in sorted(arrays):
        a = np.asarray(arrays[k])
        a = a if a.flags.c_contiguous else a.copy()  # (ascontiguousarray would make a scalar 1-D)
        if a.nbytes <= PART_BYTES // 2:
            items.append((k, a))
            continue
        n = -(-a.nbytes // (PART_BYTES // 2))
        assert a.ndim and a.shape[0] >= 1
        chunks = np.array_split(a, min(n, a.shape[0]), axis=0)
        assert all(c.nbytes <= PART_BYTES for c in chunks), (k, a.shape)
        items += [(f"{k}#{i}", c) for i, c in enumerate(chunks)]
    parts, cur, size = [], {}, 0
    for k, a in items:
        if cur and size + a.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += a.nbytes
    parts.append(cur)
    for old in glob.glob(path[:-4] + ".p[0-9][0-9].npz"):
        os.remove(old)
    names = [path] + [f"{path[:-4]}.p{i:02d}.npz" for i in range(1, len(parts))]
    for name, part in zip(names, parts):
        np.savez_compressed(name, **part)
    return names


def load_parts(path=GOLD):
    raw = {}
    for name in [path] + sorted(glob.glob(path[:-4] + ".p[0-9][0-9].npz")):
        with np.load(name) as z:
            raw.update({k: z[k] for k in z.files})
    out, cut = {}, {}
    for k, v in raw.items():
        if "#" in k:
            base, i = k.rsplit("#", 1)
            cut.setdefault(base, {})[int(i)] = v
        else:
            out[k] = v
    for base, chunks in cut.items():
        out[base] = np.concatenate([chunks[i] for i in range(len(chunks))], axis=0)
    return out


def inputs():
    """(imgs [B,N,3,H,W], proj {stage: [B,N,2,4,4]}, depth_values [B,192]) of the fixture, float32 on the host."""
    from transmvsnet_amd import synthetic
    return (synthetic.synthetic_images(N, H, W, batch=B, seed=0), synthetic.synthetic_cameras(N, H, W, batch=B, seed=1),
            synthetic.synthetic_depth_values(B))


def targets(gold, device="cpu", dtype=torch.float32):
    gt = {s: torch.from_numpy(gold[f"gt_{s}"]).to(device, dtype) for s in STAGES}
    mask = {s: torch.from_numpy(gold[f"mask_{s}"]).to(device, dtype) for s in STAGES}
    return gt, mask


def _is_buffer(k):
    return k.endswith(("running_mean", "running_var", "num_batches_tracked"))


def train_step_oracle(gold, dtype=torch.float32, perturb_seed=None, samples=None):
    """train.py:137-161's train_sample body at B = 2 through the oracle -> (loss terms, outputs, sd); the
    parameters are autograd leaves of sd (their .grad set), the buffers are updated in place. dtype and
    perturb_seed as tests/test_train_oracle.train_step_oracle (float64: the exact value; a ~1-ulp jitter of
    the images: how far fp32 rounding alone moves a gradient). samples: a slice of the batch to run alone."""
    from oracle import loss_ref
    from oracle import transmvs_ref as oracle
    from tests._util import golden_state_dict
    cast = (lambda t: t.to(dtype) if t.is_floating_point() else t)  # noqa: E731
    sd = {k: cast(v.clone()) for k, v in golden_state_dict(sharpen=TRAIN_SHARPEN).items()}
    for k, v in sd.items():
        if v.is_floating_point() and not _is_buffer(k):
            v.requires_grad_(True)
    imgs, proj, dv = inputs()
    if perturb_seed is not None:
        gen = torch.Generator().manual_seed(int(perturb_seed))
        imgs = (imgs * (1 + 2e-7 * torch.randn(imgs.shape, generator=gen, dtype=torch.float64))).to(imgs.dtype)
    gt, mask = targets(gold, dtype=dtype)
    sl = slice(None) if samples is None else samples
    out = oracle.forward(sd, cast(imgs)[sl], {k: cast(v)[sl] for k, v in proj.items()}, cast(dv)[sl], ndepths=ND,
                         training=True)
    res = loss_ref.trans_mvsnet_loss(out, {k: v[sl] for k, v in gt.items()}, {k: v[sl] for k, v in mask.items()},
                                     dlossw=DLOSSW)
    res[0].backward()
    return res, out, sd
