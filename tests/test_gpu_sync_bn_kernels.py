"""The split BatchNorm and staged PixelwiseNet entries of include/transmvs_sync.h (BatchNorm statistics
synchronised across ranks), through their transmvsnet_amd.sync_bn wrappers, with the ranks emulated in one
process: the rows (or samples) are sharded, the local entries run per shard, the shards' fp64 sums are stacked
as the slots the all-reduce would deliver, and tmvs_rank_sum adds them in rank order.

* world = 1: the split path is the fused one bit for bit (mean, var, y, dz, dgamma, dbeta; PixelwiseNet stats,
  view_w, dstar, dsims, dpwp) -- the same kernels with the same arguments.
* world = 2 and 3, grouped BatchNorm, C in {8, 32, 256} x groups in {1, 3} x per-shard rows in {1, 4 rs + 1,
  4099} (rs = 256 / C rows per step: below one step, one past the 4-row unroll, several blocks of the partial
  pass), and one case with shards of 5 and 3 rows (n_total, not the shard's own count, is the divisor).
  Statistics against float64 torch on the concatenation within 2^-23 relative, per element: the sums are
  accumulated in fp64 (relative error ~1e-16 times the cancellation factor 1 + mean^2 / var <= 17 of
  sum z^2 / N - mean^2, the inputs having |mean| <= 4 std), then rounded once to fp32 (2^-24). dz per shard, and
  the shards' dgamma / dbeta added over the ranks, against float64 autograd of batch_norm + relu over the
  concatenation at the bar of tests/test_gpu_train_conv_bn.py (err <= max(2 x err of the fp32 torch reference,
  1e-5)), with its conditioning (_bn_condition, imported) keeping every pre-activation off the ReLU edge. The
  shards differ in offset, and each shard's own mean is asserted to miss the concatenation's by more than the
  bar: the statistics are joint, not local.
* PixelwiseNet: two emulated ranks x B = 1 against the batched entries at B = 2 on the same two samples: stats
  within 2^-23 relative (two fp32 roundings of fp64 values that agree to ~1e-16), view_w / dstar / dsims / the
  rank-summed dpwp by the references and bars of tests/test_gpu_pw_batch.py (imported).
"""
import pytest
import torch
import torch.nn.functional as F

from tests._primitives import DEV, _bits, _gen, _judge
from tests.test_gpu_pw_batch import _backward_ref, _judge_forward, _pwb_inputs
from tests.test_gpu_train_conv_bn import EPS, _bn_condition
from tests.test_gpu_train_loss_pw import F32, F64, PW_GROUPS, PW_KINDS, _pw_kink_margin
from transmvsnet_amd import ops, sync_bn

pytestmark = pytest.mark.gpu
REL = 2.0 ** -23


# --------------------------------------------------------------------------------------------- rank sum
@pytest.mark.parametrize("world,count", [(1, 1), (1, 300), (2, 257), (3, 16), (3, 1025), (8, 513)])
def test_rank_sum_adds_the_slots_in_rank_order(world, count):
    """tmvs_rank_sum against the same fp64 additions on the host, bit for bit, with values whose sum depends on
    the order (1, 2^60, -2^60 rotated over the ranks and elements); world 1 is a copy."""
    g = _gen(world, count)
    slots = torch.randn(world, count, generator=g, dtype=F64)
    big = torch.tensor([1.0, 2.0 ** 60, -2.0 ** 60], dtype=F64)
    for r in range(world):
        slots[r, ::3] = big[(r + torch.arange(slots[r, ::3].numel())) % 3]
    want = slots[0].clone()
    for r in range(1, world):
        want += slots[r]
    got = sync_bn.rank_sum(slots.to(DEV))
    assert got.dtype == F64 and tuple(got.shape) == (count,)
    assert torch.equal(got.cpu().view(torch.int64), want.view(torch.int64))
    assert torch.equal(sync_bn.rank_sum(slots).view(torch.int64), want.view(torch.int64))  # the host form, CPU tensors


# --------------------------------------------------------------------------------------------- BatchNorm
def _draw(G, rows, C, *seed):
    """z [G][sum(rows)][C] whose shards (consecutive row ranges) differ in offset by 0.75 std per rank, with
    |mean| <= 4 std per channel over the concatenation; gamma in +-[0.5, 1.5), |beta| in [0.3, 1.3); conditioned
    per group on the concatenation (the statistics are joint) until no pre-activation is within tau of 0."""
    g = _gen(G, sum(rows), C, len(rows), *seed)
    n = sum(rows)
    std = torch.rand(C, generator=g) * 1.5 + 0.5
    mu = (torch.rand(C, generator=g) * 2.0 + 0.25) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0) * std
    z = torch.randn(G, n, C, generator=g) * std + mu
    r0 = 0
    for r, k in enumerate(rows):
        z[:, r0:r0 + k] += 0.75 * std * r
        r0 += k
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    beta = (torch.rand(C, generator=g) + 0.3) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    dy = torch.randn(G, n, C, generator=g)
    for gi in range(G):
        assert _bn_condition(z[gi], gamma, beta) >= 1.0  # on the CPU, before any GPU call
    return z, dy, gamma, beta


def _autograd_ref(dt, z, dy, gamma, beta):
    """autograd of relu(batch_norm(z_g)) per group over all rows -> (y, dz, dgamma, dbeta), gamma / beta shared"""
    zz = z.to(dt).clone().requires_grad_()
    ga, be = gamma.to(dt).clone().requires_grad_(), beta.to(dt).clone().requires_grad_()
    y = torch.stack([torch.relu(F.batch_norm(zz[gi], None, None, ga, be, True, 0.1, EPS)) for gi in range(z.shape[0])])
    y.backward(dy.to(dt))
    return y.detach(), zz.grad, ga.grad, be.grad


def _shards(t, rows):
    out, r0 = [], 0
    for k in rows:
        out.append(t[:, r0:r0 + k].contiguous().to(DEV))
        r0 += k
    return out


def _within(tag, got, ref64):
    err = (got.double().cpu() - ref64).abs()
    worst = float((err / ref64.abs().clamp_min(1e-300)).max())
    print(f"{tag}: worst relative error {worst:.3e} (bound {REL:.3e})")
    assert bool((err <= REL * ref64.abs()).all()), (tag, worst)


def _emulated_bn(rows, G, C, seed):
    world, n_total = len(rows), sum(rows)
    z, dy, gamma, beta = _draw(G, rows, C, seed)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    zs, dys = _shards(z, rows), _shards(dy, rows)
    tag = f"sync bn world={world} G={G} C={C} rows={rows}"

    # forward: local moments -> slots -> rank sum -> statistics over n_total
    slots = torch.stack([sync_bn.bn_moments_grouped(zr).reshape(-1) for zr in zs])
    assert slots.dtype == F64 and tuple(slots.shape) == (world, G * 2 * C)
    mean, var = sync_bn.bn_stats_from_sums(sync_bn.rank_sum(slots).view(G, 2, C), n_total)
    z64 = z.double()
    m64 = z64.mean(1)
    v64 = ((z64 - m64[:, None]) ** 2).mean(1)
    _within(tag + " mean", mean, m64)
    _within(tag + " var", var, v64)
    for r, zr in enumerate(zs):  # joint, not local: every shard's own mean is far off
        own_mean, _ = sync_bn.bn_stats_from_sums(sync_bn.bn_moments_grouped(zr), rows[r])
        assert bool(((own_mean.double().cpu() - m64).abs() > REL * m64.abs()).all()), (tag, r)

    (y32, dz32, dg32, db32), (y64, dz64, dg64, db64) = (_autograd_ref(dt, z, dy, gamma, beta) for dt in (F32, F64))
    ys = [ops.bn_relu_train_grouped(zr, mean, var, gd, bd, EPS) for zr in zs]
    _judge(tag + " y", torch.cat(ys, 1), y32, y64)

    # backward: local sums + local dgamma / dbeta -> rank sum -> dz with the global sums and n_total
    local = [sync_bn.bn_relu_backward_sums_grouped(dyr, zr, mean, var, gd, bd, EPS) for dyr, zr in zip(dys, zs)]
    gsums = sync_bn.rank_sum(torch.stack([s.reshape(-1) for s, _, _ in local])).view(G, 2, C)
    dzs = [sync_bn.bn_relu_backward_apply_grouped(dyr, zr, mean, var, gd, bd, EPS, gsums, n_total)
           for dyr, zr in zip(dys, zs)]
    _judge(tag + " dz", torch.cat(dzs, 1), dz32, dz64)
    r0 = 0
    for r, k in enumerate(rows):  # and every shard on its own scale
        _judge(f"{tag} dz [rank {r}]", dzs[r], dz32[:, r0:r0 + k], dz64[:, r0:r0 + k])
        r0 += k
    dg = sum(g.cpu() for _, g, _ in local)
    db = sum(b.cpu() for _, _, b in local)
    _judge(tag + " dgamma (added over ranks)", dg, dg32, dg64)
    _judge(tag + " dbeta (added over ranks)", db, db32, db64)


def _nvox(C, kind):
    return {"1": 1, "4rs+1": 4 * (256 // C) + 1, "4099": 4099}[kind]


@pytest.mark.parametrize("kind", ["1", "4rs+1", "4099"])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("C", [8, 32, 256])
@pytest.mark.parametrize("world", [2, 3])
def test_bn_statistics_and_gradients_are_joint_over_emulated_ranks(world, C, G, kind):
    _emulated_bn((_nvox(C, kind),) * world, G, C, 1)


@pytest.mark.parametrize("G,C", [(1, 8), (3, 32)])
def test_bn_unequal_shards_divide_by_n_total(G, C):
    """Shards of 5 and 3 rows: the kernels take n_total = 8 as the divisor, not either shard's own count."""
    _emulated_bn((5, 3), G, C, 2)


@pytest.mark.parametrize("kind", ["1", "4rs+1", "4099"])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("C", [8, 32, 256])
def test_bn_split_path_at_world_one_is_the_fused_path_bitwise(C, G, kind):
    nvox = _nvox(C, kind)
    z, dy, gamma, beta = _draw(G, (nvox,), C, 3) if nvox > 1 else \
        (torch.randn(G, 1, C), torch.randn(G, 1, C), torch.rand(C) + 0.5, torch.rand(C) + 0.3)
    zd, dyd, gd, bd = (t.to(DEV) for t in (z, dy, gamma, beta))
    mean, var = ops.bn_stats_grouped(zd)
    dz, dg, db = ops.bn_relu_backward_grouped(dyd, zd, mean, var, gd, bd, EPS)
    sums = sync_bn.bn_moments_grouped(zd)
    mean_s, var_s = sync_bn.bn_stats_from_sums(sync_bn.rank_sum(sums.view(1, -1)).view(G, 2, C), nvox)
    bsums, dg_s, db_s = sync_bn.bn_relu_backward_sums_grouped(dyd, zd, mean_s, var_s, gd, bd, EPS)
    dz_s = sync_bn.bn_relu_backward_apply_grouped(dyd, zd, mean_s, var_s, gd, bd, EPS,
                                                  sync_bn.rank_sum(bsums.view(1, -1)).view(G, 2, C), nvox)
    y = ops.bn_relu_train_grouped(zd, mean, var, gd, bd, EPS)
    y_s = ops.bn_relu_train_grouped(zd, mean_s, var_s, gd, bd, EPS)
    for name, a, b in (("mean", mean, mean_s), ("var", var, var_s), ("y", y, y_s), ("dz", dz, dz_s),
                       ("dgamma", dg, dg_s), ("dbeta", db, db_s)):
        assert torch.equal(_bits(a), _bits(b)), name
    if G == 1:  # the ungrouped entries are groups = 1
        m1, v1 = ops.bn_stats(zd[0])
        dz1, dg1, db1 = ops.bn_relu_backward(dyd[0], zd[0], m1, v1, gd, bd, EPS)
        for name, a, b in (("mean", m1, mean_s[0]), ("var", v1, var_s[0]), ("dz", dz1, dz_s[0]), ("dgamma", dg1, dg_s),
                           ("dbeta", db1, db_s)):
            assert torch.equal(_bits(a), _bits(b)), name


def test_bn_wrappers_refuse_what_the_entries_would_misread():
    z = torch.randn(2, 5, 8, device=DEV)
    c = torch.ones(8, device=DEV)
    gc = torch.ones(2, 8, device=DEV)
    sums = sync_bn.bn_moments_grouped(z)
    with pytest.raises(ValueError, match="float64"):
        sync_bn.bn_stats_from_sums(sums.float(), 5)
    with pytest.raises(ValueError, match=r"\[G, 2, C\]"):
        sync_bn.bn_stats_from_sums(sums.view(-1), 5)
    with pytest.raises(ValueError, match="mean"):
        sync_bn.bn_relu_backward_sums_grouped(z, z, c, gc, c, c, EPS)
    with pytest.raises(ValueError, match="global_sums"):
        sync_bn.bn_relu_backward_apply_grouped(z, z, gc, gc, c, c, EPS, sums[:1], 10)
    with pytest.raises(ValueError, match="n_total"):
        sync_bn.bn_relu_backward_apply_grouped(z, z, gc, gc, c, c, EPS, sums, 4)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sync_bn.bn_moments_grouped(z.cpu())


# ------------------------------------------------------------------------------------------ PixelwiseNet
# (B, V, D, H, W): 60 elements per sample and view; 2560 (more than one 1024-element block of the partial passes)
PWS_SHAPES = [(2, 2, 3, 4, 5), (2, 2, 8, 16, 20)]
# the first seed of each case with a ReLU-kink margin >= 1 in the fp64 reference (an input property; found on the CPU)
PWS_SEEDS = {((2, 2, 8, 16, 20), "random"): 8, ((2, 2, 8, 16, 20), "zero_w0"): 24,
             ((2, 2, 8, 16, 20), "negative_gamma"): 63}


def _staged(sims, pwp):
    """the staged forward of one process on its own sums (world 1)"""
    b, v, d, h, w = sims.shape
    n = b * d * h * w
    one = lambda t: sync_bn.rank_sum(t.reshape(1, -1)).view(t.shape)  # noqa: E731
    stats = torch.empty(v, 48, device=sims.device)
    z1 = sync_bn.pw_forward_z1(sims, pwp, one(sync_bn.pw_forward_sums(sims)), n, stats)
    vw, dstar = sync_bn.pw_forward_weights(sims, pwp, one(z1), n, stats)
    return stats, vw, dstar, n


@pytest.mark.parametrize("kind", PW_KINDS)
@pytest.mark.parametrize("shape", PWS_SHAPES + [(3, 2, 5, 9, 13)], ids=lambda s: "x".join(map(str, s)))
def test_pixelwise_staged_path_at_world_one_is_the_batched_path_bitwise(shape, kind):
    sims, pwp, dview_w, preload = _pwb_inputs(shape, kind, seed=PWS_SEEDS.get((shape, kind)))
    sd, pd, dvd = sims.to(DEV), pwp.to(DEV), dview_w.to(DEV)
    stats, vw, dstar = ops.pixelwise_train_forward_batched(sd, pd)
    stats_s, vw_s, dstar_s, n = _staged(sd, pd)
    assert torch.equal(_bits(stats), _bits(stats_s)) and torch.equal(_bits(vw), _bits(vw_s))
    assert torch.equal(dstar.cpu(), dstar_s.cpu())
    dsims, dsims_s = preload.to(DEV), preload.to(DEV)
    dpwp = ops.pixelwise_train_backward_batched(sd, pd, stats, vw, dstar, dvd, dsims)
    s1 = sync_bn.pw_backward_s1(sd, pd, stats, vw, dstar, dvd)
    s2 = sync_bn.pw_backward_s2(sd, pd, stats, vw, dstar, dvd, s1, n)
    dpwp_s = sync_bn.pw_backward_apply(sd, pd, stats, vw, dstar, dvd, s1, s2, n, s1, s2, dsims_s)
    assert torch.equal(_bits(dsims), _bits(dsims_s)) and torch.equal(_bits(dpwp), _bits(dpwp_s))


@pytest.mark.parametrize("kind", PW_KINDS)
@pytest.mark.parametrize("shape", PWS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pixelwise_two_emulated_ranks_equal_the_batch_of_two(shape, kind):
    B, V, D, H, W = shape
    tag = f"sync pw {shape} {kind}"
    sims, pwp, dview_w, preload = _pwb_inputs(shape, kind, seed=PWS_SEEDS.get((shape, kind)))
    sd, pd, dvd = sims.to(DEV), pwp.to(DEV), dview_w.to(DEV)
    ranks = [sd[r:r + 1].contiguous() for r in range(B)]  # rank r holds sample r: B = 1 each
    n_total = B * D * H * W
    rsum = lambda parts: sync_bn.rank_sum(torch.stack([p.reshape(-1) for p in parts])).view(parts[0].shape)  # noqa: E731

    # forward: two collectives for all views
    g0 = rsum([sync_bn.pw_forward_sums(s) for s in ranks])
    stats_r = [torch.empty(V, 48, device=DEV) for _ in ranks]
    g1 = rsum([sync_bn.pw_forward_z1(s, pd, g0, n_total, st) for s, st in zip(ranks, stats_r)])
    out = [sync_bn.pw_forward_weights(s, pd, g1, n_total, st) for s, st in zip(ranks, stats_r)]
    assert all(torch.equal(_bits(stats_r[0]), _bits(st)) for st in stats_r)  # the same bits on every rank
    stats, vw, dstar = stats_r[0], torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])

    stats_b, vw_b, dstar_b = ops.pixelwise_train_forward_batched(sd, pd)
    err = (stats.double() - stats_b.double()).abs()
    print(f"{tag}: stats vs batched, worst relative {float((err / stats_b.double().abs().clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= REL * stats_b.double().abs()).all()), tag
    _judge_forward(tag, sims, pwp, stats, vw, dstar)  # stats, view_w, and dstar outside its near-tie margin

    # backward: two collectives for all views; each rank's loss is its own sample's
    dvr = [dvd[r:r + 1].contiguous() for r in range(B)]
    saved = [(ranks[r], pd, stats, vw[r:r + 1].contiguous(), dstar[r:r + 1].contiguous(), dvr[r]) for r in range(B)]
    s1 = [sync_bn.pw_backward_s1(*a) for a in saved]
    gs1 = rsum(s1)
    s2 = [sync_bn.pw_backward_s2(*a, gs1, n_total) for a in saved]
    gs2 = rsum(s2)
    dsims = [preload[r:r + 1].to(DEV).contiguous() for r in range(B)]
    dpwp = [sync_bn.pw_backward_apply(*a, gs1, gs2, n_total, s1[r], s2[r], dsims[r]) for r, a in enumerate(saved)]
    (ds32, dp32, _), (ds64, dp64, chains) = (_backward_ref(dt, sims, pwp, dview_w, dstar.cpu()) for dt in (F32, F64))
    margin = _pw_kink_margin(chains)
    print(f"{tag}: kink margin {margin:.3g} (>= 1 required)")
    assert margin >= 1.0, (tag, margin)
    _judge(f"{tag} dsims - preload", torch.cat(dsims).cpu().double() - preload.double(), (preload + ds32) - preload, ds64)
    total = sum(d.cpu() for d in dpwp)
    for name, a, b in PW_GROUPS:
        _judge(f"{tag} dpwp {name} (added over ranks)", total[a:b], dp32[a:b], dp64[a:b])
    # the parameter-gradient slots stay local: one rank's dpwp alone is not the sum
    assert not torch.equal(_bits(dpwp[0]), _bits(total))
