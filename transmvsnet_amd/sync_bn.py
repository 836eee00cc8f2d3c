"""BatchNorm statistics synchronised across ranks: torch.nn.SyncBatchNorm's semantics under DDP, on HIP.

The reference converts its model whenever it runs on more than one process (train.py:361-366, finetune.py the
same lines: nn.SyncBatchNorm.convert_sync_batchnorm(model), then DistributedDataParallel), so every train-mode
BatchNorm takes its batch statistics over the samples of all ranks. Here every BatchNorm reduction is "fp64
block partials -> fixed-order sum -> finalize"; with sync on, the fixed-order sums leave the library before the
finalize (include/transmvs_sync.h), cross ranks through `SyncBN.reduce`, and come back with the count of all
ranks' elements:

    forward     (sum z, sum z^2)        -> mean, biased variance over N_total; running statistics with N_total
    backward    (sum g, sum g * xhat)   -> dz with the global sums and N_total; dgamma / dbeta stay local sums,
                                           the gradient all-reduce (FlatAdam.allreduce) averages them as DDP does

`reduce` is bit-identical on every rank and independent of the backend's reduction algorithm: each rank writes
its sums into slot `rank` of a zero-filled [world][K] fp64 buffer, one all_reduce(SUM) follows (adding zeros is
exact, so it acts as a gather; all_reduce because gloo offers device tensors nothing else but broadcast), and
tmvs_rank_sum adds the slots in rank order.

All ranks must hold equal counts (the driver guarantees it: same crop, drop_last); `check_counts` verifies it
on the host once per step. Not built: sync under a view-sharded forward, and inside HIP-graph capture.
"""
from __future__ import annotations

import contextlib

import torch

from . import _lib, ops

F64 = torch.float64
CAPTURE_MSG = ("synchronised BatchNorm inside HIP-graph capture (TrainStepGraph) is not built: run the step "
               "eagerly, or turn sync off with model.sync_batchnorm(None)")
VIEW_SHARD_MSG = ("synchronised BatchNorm together with a view-sharded forward (view_shard=...) is not built: "
                  "turn sync off with model.sync_batchnorm(None)")


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class SyncBN:
    """The process group of a synchronised BatchNorm and its one collective.

    group: a torch.distributed process group (None: the default group; without torch.distributed initialised, a
    world of one). always=True issues the collective on a one-rank group too (as ViewShard.always_reduce), for
    timing the synchronised path on one GPU and for one-rank tests. `comm_bytes` lists the bytes of every
    collective since `begin_step()` (the training forward calls it), `record()` sums them up."""

    def __init__(self, group=None, always=False):
        import torch.distributed as dist
        self.group, self.always = group, bool(always)
        if dist.is_available() and dist.is_initialized():
            self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        else:
            if group is not None:
                raise ValueError("SyncBN: a process group without torch.distributed initialised")
            if always:
                raise ValueError("SyncBN(always=True) needs torch.distributed initialised (a one-rank group will do)")
            self.world, self.rank = 1, 0
        self.comm_bytes = []
        self.timer = None  # optional begin(name) / end(token) around each collective, as ViewShard.timer

    @property
    def active(self):
        """whether `reduce` communicates (otherwise it is the identity)"""
        return self.world > 1 or self.always

    def begin_step(self):
        self.comm_bytes = []

    def record(self):
        """{"collectives", "bytes"} since begin_step(): one training step's, after its backward"""
        return {"collectives": len(self.comm_bytes), "bytes": int(sum(self.comm_bytes))}

    def n_total(self, n_local):
        """the count behind reduced sums: every rank holds n_local elements (check_counts verifies it)"""
        return self.world * int(n_local)

    def reduce(self, local_sums):
        """local_sums: contiguous float64 tensor (device, or CPU on a gloo group) -> the sum over ranks, added in
        rank order; the same bits on every rank. The identity at world 1 unless `always`."""
        if not self.active:
            return local_sums
        if local_sums.dtype != F64 or not local_sums.is_contiguous():
            raise ValueError("SyncBN.reduce: the sums must be a contiguous float64 tensor")
        if local_sums.is_cuda and _capturing():
            raise RuntimeError(CAPTURE_MSG)
        import torch.distributed as dist
        slots = torch.zeros(self.world, local_sums.numel(), dtype=F64, device=local_sums.device)
        slots[self.rank].copy_(local_sums.reshape(-1))
        tok = self.timer.begin("sync_bn_all_reduce") if self.timer is not None else None
        dist.all_reduce(slots, op=dist.ReduceOp.SUM, group=self.group)
        if tok is not None:
            self.timer.end(tok)
        self.comm_bytes.append(slots.numel() * 8)
        return rank_sum(slots).view(local_sums.shape)

    def check_counts(self, counts, device=None):
        """Raise unless every rank holds the same `counts` (a sequence of ints, e.g. the batch's shape): the sums
        of all ranks are divided by N_total = world * N_local. One collective and one host read; every rank
        raises or none does."""
        if not self.active:
            return
        local = torch.tensor([float(c) for c in counts], dtype=F64, device=device)
        total = self.reduce(local).cpu()
        if any(float(t) != self.world * float(c) for t, c in zip(total.tolist(), counts)):
            raise RuntimeError(
                f"synchronised BatchNorm needs equal counts on every rank (N_total == world * N_local): rank "
                f"{self.rank} of {self.world} holds {list(counts)}, all ranks together {[int(t) for t in total.tolist()]}")


# ------------------------------------------------------------------ the sync a training forward runs under
_CURRENT = [None]


def current():
    """the SyncBN of the training forward being built (None: statistics per rank)"""
    return _CURRENT[0]


@contextlib.contextmanager
def using(sync):
    """Run a training forward with `sync` (None: off); its autograd Functions keep it for their backward."""
    prev = _CURRENT[0]
    _CURRENT[0] = sync if sync is not None and sync.active else None
    try:
        yield _CURRENT[0]
    finally:
        _CURRENT[0] = prev


# ------------------------------------------------------------------ C-ABI wrappers (include/transmvs_sync.h)
def _f64(t, name, numel=None):
    if not isinstance(t, torch.Tensor) or t.dtype != F64 or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"{name} must be a contiguous float64 GPU tensor")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name} must hold {numel} doubles, not {t.numel()}")


def rank_sum(slots):
    """slots [world, K] float64 -> [K], the slots added in rank order (tmvs_rank_sum on the device; the same
    ordered fp64 additions on the host for CPU tensors of a gloo group, which the library cannot reach)."""
    if slots.dim() != 2 or slots.dtype != F64 or not slots.is_contiguous():
        raise ValueError("rank_sum: slots must be a contiguous float64 [world, K] tensor")
    if not slots.is_cuda:
        out = slots[0].clone()
        for r in range(1, slots.shape[0]):
            out += slots[r]
        return out
    return _rank_sum_device(slots)


@ops._on_tensor_device
def _rank_sum_device(slots):
    out = torch.empty(slots.shape[1], dtype=F64, device=slots.device)
    ops._launch("tmvs_rank_sum", slots, slots.shape[0], slots.shape[1], out)
    return out


def _bn_dims(what, z, per_group, per_channel, like_z):
    """z [G, ..., C] -> (G, voxels per group, C), after the size checks the entries cannot make"""
    ops._dev(z, "z")
    if z.dim() < 3:
        raise ValueError(f"{what}: z must be [G, ..., C], not {list(z.shape)}")
    g, c = z.shape[0], z.shape[-1]
    for name, t in (*per_group, *per_channel, *like_z):
        ops._dev(t, name)
    ops._bn_shapes(what, z, [(n, t, g) for n, t in per_group] + [(n, t, 1) for n, t in per_channel], like_z)
    return g, z.numel() // (g * c), c


def _bn_ws(g, nvox, c, device):
    return ops._workspace("tmvs_bn_train_workspace_grouped", g, nvox, c, device=device)


@ops._on_tensor_device
def bn_moments_grouped(z):
    """tmvs_bn_moments_grouped: z [G, ..., C] -> float64 [G, 2, C] = (sum z, sum z^2), this rank's."""
    g, nvox, c = _bn_dims("bn_moments_grouped", z, (), (), ())
    sums = torch.empty(g, 2, c, dtype=F64, device=z.device)
    ops._launch("tmvs_bn_moments_grouped", z, g, nvox, c, *_bn_ws(g, nvox, c, z.device), sums)
    return sums


@ops._on_tensor_device
def bn_stats_from_sums(sums, n_total):
    """tmvs_bn_stats_from_sums: float64 [G, 2, C] over n_total elements -> (mean [G, C], biased variance [G, C])."""
    _f64(sums, "sums")
    if sums.dim() != 3 or sums.shape[1] != 2:
        raise ValueError(f"bn_stats_from_sums: sums must be [G, 2, C], not {list(sums.shape)}")
    g, _, c = sums.shape
    mean = torch.empty(g, c, device=sums.device)
    var = torch.empty(g, c, device=sums.device)
    ops._launch("tmvs_bn_stats_from_sums", sums, g, c, int(n_total), mean, var)
    return mean, var


@ops._on_tensor_device
def bn_relu_backward_sums_grouped(dy, z, mean, var, gamma, beta, eps):
    """tmvs_bn_relu_backward_sums_grouped -> (float64 [G, 2, C] = (sum g, sum g * xhat), dgamma [C], dbeta [C]),
    all of this rank's elements."""
    g, nvox, c = _bn_dims("bn_relu_backward_sums_grouped", z, (("mean", mean), ("var", var)),
                          (("gamma", gamma), ("beta", beta)), (("dy", dy),))
    sums = torch.empty(g, 2, c, dtype=F64, device=z.device)
    dg = torch.empty(c, device=z.device)
    db = torch.empty(c, device=z.device)
    ops._launch("tmvs_bn_relu_backward_sums_grouped", dy, z, g, nvox, c, mean, var, gamma, beta, eps,
                *_bn_ws(g, nvox, c, z.device), sums, dg, db)
    return sums, dg, db


@ops._on_tensor_device
def bn_relu_backward_apply_grouped(dy, z, mean, var, gamma, beta, eps, global_sums, n_total):
    """tmvs_bn_relu_backward_apply_grouped: dz from the sums of all ranks over n_total elements."""
    g, nvox, c = _bn_dims("bn_relu_backward_apply_grouped", z, (("mean", mean), ("var", var)),
                          (("gamma", gamma), ("beta", beta)), (("dy", dy),))
    _f64(global_sums, "global_sums", g * 2 * c)
    if n_total < nvox:
        raise ValueError(f"bn_relu_backward_apply_grouped: n_total {n_total} below this rank's {nvox}")
    dz = torch.empty_like(z)
    ops._launch("tmvs_bn_relu_backward_apply_grouped", dy, z, g, nvox, c, mean, var, gamma, beta, eps, global_sums,
                int(n_total), dz)
    return dz


def _pw_ws(device):
    return ops._workspace("tmvs_pixelwise_train_workspace", device=device)


def _pw_dims(op, sims, pwp):
    b, v, d, h, w = ops._pw_sims(op, sims, batched=True)
    ops._pw_shaped(op, pwp, "pwp", (_lib.PW_NPARAMS,), sims)
    return b, v, d, h, w


@ops._on_tensor_device
def pw_forward_sums(sims):
    """tmvs_pw_sync_forward_sums: sims [B,V,D,H,W] -> float64 [V, 2] = (sum s, sum s^2) per view, this rank's."""
    b, v, d, h, w = ops._pw_sims("pw_forward_sums", sims, batched=True)
    s = torch.empty(v, 2, dtype=F64, device=sims.device)
    ops._launch("tmvs_pw_sync_forward_sums", sims, b, v, d, h, w, *_pw_ws(sims.device), s)
    return s


@ops._on_tensor_device
def pw_forward_z1(sims, pwp, s_sums, n_total, stats):
    """tmvs_pw_sync_forward_z1: the layer-0 statistics into stats [V,48] from the global s_sums -> float64 [V, 16]."""
    b, v, d, h, w = _pw_dims("pw_forward_z1", sims, pwp)
    _f64(s_sums, "s_sums", v * 2)
    ops._pw_shaped("pw_forward_z1", stats, "stats", (v, 48), sims)
    z1 = torch.empty(v, 16, dtype=F64, device=sims.device)
    ops._launch("tmvs_pw_sync_forward_z1", sims, b, v, d, h, w, pwp, s_sums, int(n_total), *_pw_ws(sims.device), stats, z1)
    return z1


@ops._on_tensor_device
def pw_forward_weights(sims, pwp, z1_sums, n_total, stats):
    """tmvs_pw_sync_forward_weights: the layer-1 statistics into stats -> (view_w [B,V,H,W], dstar int32)."""
    b, v, d, h, w = _pw_dims("pw_forward_weights", sims, pwp)
    _f64(z1_sums, "z1_sums", v * 16)
    ops._pw_shaped("pw_forward_weights", stats, "stats", (v, 48), sims)
    vw = torch.empty(b, v, h, w, device=sims.device)
    dstar = torch.empty(b, v, h, w, device=sims.device, dtype=torch.int32)
    ops._launch("tmvs_pw_sync_forward_weights", sims, b, v, d, h, w, pwp, z1_sums, int(n_total), stats, vw, dstar)
    return vw, dstar


def _pw_saved(op, sims, pwp, stats, view_w, dstar, dview_w):
    b, v, d, h, w = _pw_dims(op, sims, pwp)
    for t, n, shape in ((stats, "stats", (v, 48)), (view_w, "view_w", (b, v, h, w)), (dview_w, "dview_w", (b, v, h, w))):
        ops._pw_shaped(op, t, n, shape, sims)
    ops._pw_shaped(op, dstar, "dstar", (b, v, h, w), sims, torch.int32)
    return b, v, d, h, w


@ops._on_tensor_device
def pw_backward_s1(sims, pwp, stats, view_w, dstar, dview_w):
    """tmvs_pw_sync_backward_s1 -> float64 [V, 25], this rank's pass-1 sums."""
    b, v, d, h, w = _pw_saved("pw_backward_s1", sims, pwp, stats, view_w, dstar, dview_w)
    s1 = torch.empty(v, 25, dtype=F64, device=sims.device)
    ops._launch("tmvs_pw_sync_backward_s1", sims, b, v, d, h, w, pwp, stats, view_w, dstar, dview_w, *_pw_ws(sims.device),
                s1)
    return s1


@ops._on_tensor_device
def pw_backward_s2(sims, pwp, stats, view_w, dstar, dview_w, global_s1, n_total):
    """tmvs_pw_sync_backward_s2 -> float64 [V, 160], this rank's pass-2 sums."""
    b, v, d, h, w = _pw_saved("pw_backward_s2", sims, pwp, stats, view_w, dstar, dview_w)
    _f64(global_s1, "global_s1", v * 25)
    s2 = torch.empty(v, 160, dtype=F64, device=sims.device)
    ops._launch("tmvs_pw_sync_backward_s2", sims, b, v, d, h, w, pwp, stats, view_w, dstar, dview_w, global_s1,
                int(n_total), *_pw_ws(sims.device), s2)
    return s2


@ops._on_tensor_device
def pw_backward_apply(sims, pwp, stats, view_w, dstar, dview_w, global_s1, global_s2, n_total, local_s1, local_s2,
                      dsims):
    """tmvs_pw_sync_backward_apply: adds the PixelwiseNet path into dsims (in place) -> dpwp [201] (this rank's)."""
    op = "pw_backward_apply"
    b, v, d, h, w = _pw_saved(op, sims, pwp, stats, view_w, dstar, dview_w)
    ops._pw_shaped(op, dsims, "dsims", (b, v, d, h, w), sims)
    for t, n, k in ((global_s1, "global_s1", 25), (local_s1, "local_s1", 25), (global_s2, "global_s2", 160),
                    (local_s2, "local_s2", 160)):
        _f64(t, n, v * k)
    dpwp = torch.zeros(_lib.PW_NPARAMS, device=sims.device)
    ops._launch("tmvs_pw_sync_backward_apply", sims, b, v, d, h, w, pwp, stats, view_w, dstar, dview_w, global_s1,
                global_s2, int(n_total), local_s1, local_s2, *_pw_ws(sims.device), dsims, dpwp)
    return dpwp


# ------------------------------------------------------------------ what the training Functions call
def bn_stats_grouped(sync, z):
    """Batch statistics of z [G, ..., C] per group over all ranks -> (mean [G, C], var [G, C], N_total)."""
    n_total = sync.n_total(z.numel() // (z.shape[0] * z.shape[-1]))
    mean, var = bn_stats_from_sums(sync.reduce(bn_moments_grouped(z)), n_total)
    return mean, var, n_total


def bn_relu_backward_grouped(sync, dy, z, mean, var, gamma, beta, eps, n_total):
    """ops.bn_relu_backward_grouped with the sums of all ranks in dz; dgamma / dbeta stay this rank's."""
    sums, dg, db = bn_relu_backward_sums_grouped(dy, z, mean, var, gamma, beta, eps)
    dz = bn_relu_backward_apply_grouped(dy, z, mean, var, gamma, beta, eps, sync.reduce(sums), n_total)
    return dz, dg, db


def pixelwise_forward(sync, sims, pwp):
    """ops.pixelwise_train_forward_batched with statistics over all ranks: two collectives for all views ->
    (stats [V,48], view_w, dstar, N_total per view)."""
    b, v, d, h, w = sims.shape
    n_total = sync.n_total(b * d * h * w)
    stats = torch.empty(v, 48, device=sims.device)
    z1 = pw_forward_z1(sims, pwp, sync.reduce(pw_forward_sums(sims)), n_total, stats)
    vw, dstar = pw_forward_weights(sims, pwp, sync.reduce(z1), n_total, stats)
    return stats, vw, dstar, n_total


def pixelwise_backward(sync, sims, pwp, stats, view_w, dstar, dview_w, dsims, n_total):
    """ops.pixelwise_train_backward_batched with the BatchNorm sums of all ranks: two collectives for all views;
    the parameter gradients dpwp [201] are this rank's."""
    s1 = pw_backward_s1(sims, pwp, stats, view_w, dstar, dview_w)
    g1 = sync.reduce(s1)
    s2 = pw_backward_s2(sims, pwp, stats, view_w, dstar, dview_w, g1, n_total)
    g2 = sync.reduce(s2)
    return pw_backward_apply(sims, pwp, stats, view_w, dstar, dview_w, g1, g2, n_total, s1, s2, dsims)
