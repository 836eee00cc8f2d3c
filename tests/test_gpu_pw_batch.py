"""The PixelwiseNet training kernels on a batch (csrc/pw_train.hip: tmvs_pixelwise_train_forward_batched /
_backward_batched through their transmvsnet_amd.ops wrappers), at the smallest shapes where the batch indexing
can go wrong.

The reference calls PixelwiseNet per source view on [B,1,D,h,w] (models/TransMVSNet.py:71-77), so a view's two
BatchNorm3d layers take their statistics over the B*D*h*w elements of that view in all samples. The yardstick
is the one of tests/test_gpu_train_loss_pw.py (its helpers are imported, the file is not changed): the chain
written out in plain torch with the statistics joint over the batch, in fp64 (the truth) and in fp32 (the
yardstick), err_gpu <= max(2 x err_fp32ref, 1e-5) (_judge / _hold print both errors). The ReLU-kink margin >= 1
is a condition on the input, asserted; PWB_SEEDS records the first seed of each case that meets it (found on
the CPU). A kernel that took its statistics per sample cannot pass: the joint statistics are asserted to differ
from every single sample's by far more than the bar.

The three parameter sets of tests/test_gpu_train_loss_pw.py (PW_KINDS) run at the two larger shapes. At
(2, 1, 1, 1, 1) only "random" does: a BatchNorm over N = 2 elements outputs +-1 whatever its input, so the
gradient through it exists only through eps -- dz = g / 2 * eps / (var + eps) -- and the fp32-rounded statistics
(the [V][48] float ABI) alone move it by 2^-24 (var + eps) / eps relative, 1e-4 to 1e-2 here, in ANY fp32
evaluation, the yardstick's included. Each such comparison is one draw against another, so further parameter
sets at that shape add coin flips and no coverage; the shape is there for its indexing (one element per sample,
statistics only through the batch), which one parameter set shows. Measured on an MI355X (err_gpu,
err_fp32ref), backward at (2, 1, 1, 1, 1): random dsims (3.5e-03, 2.6e-03), w0 (2.2e-04, 1.6e-04), g0 (2.8e-04,
3.9e-04), b0 (3.0e-04, 4.0e-04), W1 (3.8e-04, 3.3e-04), layer-1 groups below 1e-07; the two sets not run:
zero_w0 dsims (3.6e-02, 3.6e-02), g0 (4.3e-04, 7.3e-04); negative_gamma dsims (3.8e-03, 2.2e-03), w0 (2.7e-04,
1.9e-03), g0 (1.8e-03, 6.3e-04) -- the last one above 2x its yardstick's draw. The B = 1 test below runs all
three sets at every shape bit for bit.

Layouts: sims / dsims [B][V][D][P], stats [V][48] (one row per view, shared by the batch), view_w / dstar /
dview_w [B][V][P], dpwp [201].
"""
import pytest
import torch

from oracle import transmvs_ref as oracle
from transmvsnet_amd import ops

from tests._primitives import DEV, _assert_guard, _bits, _gen, _hold, _judge, _rel
from tests.test_gpu_train_loss_pw import (F32, F64, PW_GROUPS, PW_KINDS, PW_SHAPES, _flat_guarded, _pw_chain,
                                          _pw_inputs, _pw_kink_margin, _pw_oracle_sd, _pw_split)

pytestmark = pytest.mark.gpu

# (B, V, D, H, W)
PWB_SHAPES = [(3, 2, 5, 9, 13),    # D*P = 585, B*D*P = 1755: sample boundaries inside a 1024-element reduction
                                   # block, a block's range ending mid-sample; B*P = 351 pixels, two blocks
              (2, 3, 8, 1, 257),   # P one past a 256-pixel block, B*P = 514
              (2, 1, 1, 1, 1)]     # one element per sample: the statistics exist only through the batch
# The seed of each (shape, kind): the first for which no layer-0 / layer-1 pre-activation of the fp64 reference
# lies within the fp32 chain's own rounding of a ReLU kink (asserted by the backward test; an input property).
PWB_SEEDS = {((3, 2, 5, 9, 13), "zero_w0"): 1, ((3, 2, 5, 9, 13), "negative_gamma"): 1,
             ((2, 3, 8, 1, 257), "random"): 124, ((2, 3, 8, 1, 257), "zero_w0"): 1686,
             ((2, 3, 8, 1, 257), "negative_gamma"): 490}
PWB_CASES = [(s, k) for s in PWB_SHAPES for k in PW_KINDS if s != (2, 1, 1, 1, 1) or k == "random"]
STAT_NAMES = (("mean0", 0, 16), ("var0", 16, 32), ("mean1", 32, 40), ("var1", 40, 48))


def _ids(s):
    return "x".join(map(str, s))


def _case_id(c):
    return _ids(c[0]) + "-" + c[1]


def _pwb_inputs(shape, kind, seed=None):
    """sims [B,V,D,H,W] whose samples differ in scale and offset (so that each sample's own statistics are far
    from the batch's), pwp as tests/test_gpu_train_loss_pw._pw_inputs draws it, dview_w [B,V,H,W], a preload"""
    B, V, D, H, W = shape
    seed = PWB_SEEDS.get((shape, kind), 0) if seed is None else seed
    _, pwp, _, _ = _pw_inputs((V, D, H, W), kind, seed=seed)
    g = _gen(B, V, D, H, W, PW_KINDS.index(kind) + 1, seed, 77)
    sims = 0.3 * torch.randn(B, V, D, H, W, generator=g)
    for b in range(B):
        sims[b] = sims[b] * (1.0 + 0.5 * b) + 0.2 * b
    dview_w = torch.randn(B, V, H, W, generator=g)
    preload = torch.randn(B, V, D, H, W, generator=g)
    return sims, pwp, dview_w, preload


def _chains(prm, sims):
    """one joint chain per view: _pw_chain flattens whatever it is given, so sims[:, v] [B,D,H,W] gives the
    statistics over B*D*H*W and the sigmoid volume [B,D,H,W]"""
    return [_pw_chain(prm, sims[:, v]) for v in range(sims.shape[1])]


def _forward_ref(dt, sims, pwp):
    """(stats [V,48] joint over the batch, view_w [B,V,H,W] by the oracle's train-mode pixelwise_net on
    [B,1,D,H,W] per view, sigmoid volumes [B,V,D,H,W])"""
    prm = _pw_split(pwp.to(dt))
    s = sims.to(dt)
    chains = _chains(prm, s)
    vw = torch.stack([oracle.pixelwise_net(_pw_oracle_sd(prm), s[:, v][:, None], training=True)[:, 0]
                      for v in range(s.shape[1])], 1)
    return torch.stack([c["stats"] for c in chains]), vw, torch.stack([c["sig"] for c in chains], 1)


def _backward_ref(dt, sims, pwp, dview_w, dstar):
    """autograd of sum_{b,v} <dview_w[b,v], sigmoid(net(s))[b,v] gathered at dstar[b,v]> with the statistics
    joint over the batch -> (d sims, d pwp, the chains)"""
    leaf = pwp.to(dt).clone().requires_grad_()
    s = sims.to(dt).clone().requires_grad_()
    chains = _chains(_pw_split(leaf), s)
    total = 0
    for v, c in enumerate(chains):
        at = torch.gather(c["sig"], 1, dstar[:, v].long()[:, None])[:, 0]  # [B,H,W]
        total = total + (dview_w[:, v].to(dt) * at).sum()
    total.backward()
    return s.grad, leaf.grad, chains


def _judge_forward(tag, sims, pwp, stats, vw, dstar):
    B, V, D, H, W = sims.shape
    (st32, vw32, _), (st64, vw64, sig64) = (_forward_ref(dt, sims, pwp) for dt in (F32, F64))
    assert tuple(stats.shape) == (V, 48) and tuple(vw.shape) == (B, V, H, W) and tuple(dstar.shape) == (B, V, H, W)
    assert dstar.dtype == torch.int32
    prm64 = _pw_split(pwp.to(F64))
    for v in range(V):
        for name, a, b in STAT_NAMES:
            _judge(f"{tag} stats[{v}] {name}", stats[v, a:b], st32[v, a:b], st64[v, a:b])
        # ... and they are not any single sample's: a per-sample kernel (or a batch stride that reads one
        # sample B times) would land on one of these
        for b in range(B):
            alone = _pw_chain(prm64, sims[b, v].to(F64))["stats"]
            assert _rel(stats[v], alone) > 1e-2, (tag, v, b, _rel(stats[v], alone))
    assert _rel(sig64.max(2)[0], vw64) < 1e-12  # the oracle's max_d sigmoid and the chain above are one function
    _judge(f"{tag} view_w", vw, vw32, vw64)
    ds = dstar.cpu().long()
    assert int(ds.min()) >= 0 and int(ds.max()) < D, (int(ds.min()), int(ds.max()))
    at = torch.gather(sig64, 2, ds[:, :, None])[:, :, 0]  # every pixel of every sample
    _hold(f"{tag} dstar (reference sigmoid at dstar vs its maximum)", _rel(at, vw64), _rel(vw32, vw64))
    return sig64


@pytest.mark.parametrize("shape,kind", PWB_CASES, ids=[_case_id(c) for c in PWB_CASES])
def test_pixelwise_forward_batched(shape, kind):
    """stats rows against the fp64 statistics joint over the batch (and away from each sample's own), view_w
    against the oracle's train-mode PixelwiseNet on [B,1,D,H,W], dstar at every pixel of every sample; a
    repeat call repeats every bit."""
    sims, pwp, _, _ = _pwb_inputs(shape, kind)
    sd, pd = sims.to(DEV), pwp.to(DEV)
    stats, vw, dstar = ops.pixelwise_train_forward_batched(sd, pd)
    _judge_forward(f"pw fwd batched {shape} {kind}", sims, pwp, stats, vw, dstar)
    if kind == "zero_w0":
        assert float(stats[:, 5].abs().max()) == 0.0 and float(stats[:, 16 + 5].abs().max()) == 0.0
    stats2, vw2, dstar2 = ops.pixelwise_train_forward_batched(sd, pd)
    assert torch.equal(_bits(stats), _bits(stats2)) and torch.equal(_bits(vw), _bits(vw2))
    assert torch.equal(dstar.cpu(), dstar2.cpu())


def test_pixelwise_forward_batched_first_argmax():
    """Plane 3 is a copy of plane 1 in sample 1 only (D = 5), so the chain is bitwise equal on both there: in
    sample 1 the first argmax never answers 3 and answers 1 wherever the fp64 argmax is plane 1 or 3, while
    samples 0 and 2, with no tie, do answer 3 somewhere (the tie handling is per sample and pixel)."""
    shape = (3, 2, 5, 9, 13)
    sims, pwp, _, _ = _pwb_inputs(shape, "random", seed=101)
    sims[1, :, 3] = sims[1, :, 1]
    stats, vw, dstar = ops.pixelwise_train_forward_batched(sims.to(DEV), pwp.to(DEV))
    sig64 = _judge_forward("pw fwd batched first argmax", sims, pwp, stats, vw, dstar)
    assert torch.equal(sig64[1, :, 1], sig64[1, :, 3])
    ds = dstar.cpu().long()
    best = sig64.argmax(2)
    tied = (best[1] == 1) | (best[1] == 3)
    assert int(tied.sum()) >= 20  # the planted tie is the maximum at a good share of sample 1's 234 pixels
    assert not bool((ds[1] == 3).any())
    assert bool((ds[1][tied] == 1).all())
    assert bool((ds[0] == 3).any()) and bool((ds[2] == 3).any())


@pytest.mark.parametrize("shape,kind", PWB_CASES, ids=[_case_id(c) for c in PWB_CASES])
def test_pixelwise_backward_batched(shape, kind):
    """dsims - preload (in a guarded buffer) and the eight parameter-gradient groups of dpwp against fp64
    autograd of the chain with joint statistics, gathered at the kernel's own dstar (the forward test judges
    dstar at every pixel). The BatchNorm backward's sums and its 1/N run over the view's whole batch, so a
    gradient reaches every sample's elements from every other sample's. A repeat call repeats every bit."""
    B, V, D, H, W = shape
    tag = f"pw bwd batched {shape} {kind}"
    sims, pwp, dview_w, preload = _pwb_inputs(shape, kind)
    sd, pd, dvd = sims.to(DEV), pwp.to(DEV), dview_w.to(DEV)
    stats, vw, dstar = ops.pixelwise_train_forward_batched(sd, pd)
    buf, dsims, nrows = _flat_guarded(shape, preload)
    dpwp = ops.pixelwise_train_backward_batched(sd, pd, stats, vw, dstar, dvd, dsims)
    _assert_guard(buf, 2, nrows, f"{tag} dsims")
    (ds32, dp32, _), (ds64, dp64, chains) = (_backward_ref(dt, sims, pwp, dview_w, dstar.cpu()) for dt in (F32, F64))
    margin = _pw_kink_margin(chains)  # ReLU kinks are a condition on the input, not a tolerance
    print(f"{tag}: kink margin {margin:.3g} (>= 1 required)")
    assert margin >= 1.0, (tag, margin)
    _judge(f"{tag} dsims - preload", dsims.cpu().double() - preload.double(), (preload + ds32) - preload, ds64)
    assert tuple(dpwp.shape) == (201,)
    for name, a, b in PW_GROUPS:
        _judge(f"{tag} dpwp {name}", dpwp[a:b], dp32[a:b], dp64[a:b])
    buf2, dsims2, _ = _flat_guarded(shape, preload)
    dpwp2 = ops.pixelwise_train_backward_batched(sd, pd, stats, vw, dstar, dvd, dsims2)
    assert torch.equal(_bits(dsims), _bits(dsims2)) and torch.equal(_bits(dpwp), _bits(dpwp2))
    assert torch.equal(_bits(buf), _bits(buf2))


@pytest.mark.parametrize("kind", PW_KINDS)
@pytest.mark.parametrize("shape", PW_SHAPES, ids=_ids)
def test_batch_of_one_is_the_single_sample_entry_point_bitwise(shape, kind):
    """With B = 1 the batched entry points return what ops.pixelwise_train_forward / _backward return, bit for
    bit, at the shapes and parameter sets of tests/test_gpu_train_loss_pw.py."""
    sims, pwp, dview_w, preload = _pw_inputs(shape, kind)
    sd, pd, dvd = sims.to(DEV), pwp.to(DEV), dview_w.to(DEV)
    stats, vw, dstar = ops.pixelwise_train_forward(sd, pd)
    stats_b, vw_b, dstar_b = ops.pixelwise_train_forward_batched(sd[None], pd)
    assert torch.equal(_bits(stats), _bits(stats_b)) and torch.equal(_bits(vw), _bits(vw_b[0]))
    assert torch.equal(dstar.cpu(), dstar_b[0].cpu())
    dsims, dsims_b = preload.to(DEV), preload.to(DEV)[None].contiguous()
    dpwp = ops.pixelwise_train_backward(sd, pd, stats, vw, dstar, dvd, dsims)
    dpwp_b = ops.pixelwise_train_backward_batched(sd[None], pd, stats_b, vw_b, dstar_b, dvd[None], dsims_b)
    assert torch.equal(_bits(dsims), _bits(dsims_b[0])) and torch.equal(_bits(dpwp), _bits(dpwp_b))


def test_batched_wrappers_refuse_what_the_entry_points_would_misread():
    """The entry points take one B, V, D, H, W for all their tensors: a non-contiguous, wrong-device, wrong-dtype
    or mis-shaped tensor is refused by the wrapper before any launch."""
    B, V, D, H, W = 2, 2, 3, 4, 6
    sims = torch.randn(B, V, D, H, W, device=DEV)
    pwp = torch.randn(201, device=DEV)
    stats, vw, dstar = ops.pixelwise_train_forward_batched(sims, pwp)
    dvw, dsims = torch.randn(B, V, H, W, device=DEV), torch.zeros(B, V, D, H, W, device=DEV)
    ops.pixelwise_train_backward_batched(sims, pwp, stats, vw, dstar, dvw, dsims)  # the good call
    with pytest.raises(ValueError, match=r"sims must be \[B, V, D, H, W\]"):
        ops.pixelwise_train_forward_batched(sims[0], pwp)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.pixelwise_train_forward_batched(sims.transpose(0, 1), pwp)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.pixelwise_train_forward_batched(sims.cpu(), pwp)
    with pytest.raises(ValueError, match="pwp"):
        ops.pixelwise_train_forward_batched(sims, pwp.cpu())
    with pytest.raises(ValueError, match="pwp"):
        ops.pixelwise_train_forward_batched(sims, pwp[:200])

    def bwd(**kw):
        a = dict(sims=sims, pwp=pwp, stats=stats, view_w=vw, dstar=dstar, dview_w=dvw, dsims=dsims)
        a.update(kw)
        return ops.pixelwise_train_backward_batched(a["sims"], a["pwp"], a["stats"], a["view_w"], a["dstar"],
                                                    a["dview_w"], a["dsims"])

    with pytest.raises(RuntimeError, match="contiguous"):
        bwd(sims=sims.transpose(3, 4).contiguous().transpose(3, 4))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        bwd(sims=sims.cpu())
    for name, bad in (("view_w", vw[0]), ("view_w", vw[:, :1]), ("view_w", vw.transpose(2, 3)), ("view_w", vw.cpu()),
                      ("dstar", dstar[0]), ("dstar", dstar.float()), ("dstar", dstar.cpu()),
                      ("dstar", dstar.transpose(0, 1)),
                      ("dview_w", dvw[:1]), ("dview_w", dvw.cpu()),
                      ("dsims", dsims[0]), ("dsims", dsims[:, :, :2]), ("dsims", dsims.cpu()),
                      ("dsims", torch.zeros(B, V, D, H, W + 1, device=DEV)),
                      ("stats", stats[:1]), ("stats", torch.zeros(B, V, 48, device=DEV))):
        with pytest.raises(ValueError, match=name):
            bwd(**{name: bad})
