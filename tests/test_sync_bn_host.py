"""Synchronised BatchNorm without a GPU: the second header (include/transmvs_sync.h) against its signature table
and the library's exports, what every new entry refuses before any launch, the driver's flag, the three
refusals of the Python path, and SyncBN.reduce on gloo (world 2 and 3, CPU tensors): every rank gets, bit for
bit, the sum of the ranks' values added in rank order -- also where the fp64 sum depends on the order."""
import os
import re
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from transmvsnet_amd import _lib, build, sync_bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "transmvs_sync.h")
ARG, SHAPE = -1, -2


def _declarations():
    """name -> argument count of every function the header declares (the method of tests/test_abi.py)"""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    decls = {}
    for m in re.finditer(r"\b(?:int|size_t|const\s+char\s*\*)\s*\*?\s*(tmvs_\w+)\s*\(([^)]*)\)\s*;", src):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return decls


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_sync_header_declarations_match_binding():
    decls = _declarations()
    assert len(decls) == 11
    assert set(decls) == set(_lib.SYNC_SIGNATURES), set(decls) ^ set(_lib.SYNC_SIGNATURES)
    for name, n in decls.items():
        assert len(_lib.SYNC_SIGNATURES[name][1]) == n, name
    assert not set(decls) & set(_lib.SIGNATURES)  # the first header's table is left as it was


def test_library_exports_and_types_every_sync_entry(lib):
    for name, (res, args) in _lib.SYNC_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_sync_entries_refuse_before_any_launch(lib):
    """Null pointers, non-positive extents, world <= 0, n_total below the rank's own count and a short workspace
    are TMVS_ERR_ARG; a BatchNorm channel count that does not divide 256 is TMVS_ERR_SHAPE. The pointers are host
    memory that is never read, and every call has exactly one thing wrong with it."""
    backing = np.zeros(256, np.float64)
    p = (backing.ctypes.data + 63) & ~63
    big = 1 << 40
    not_dividing = (3, 5, 6, 12, 24, 48, 96, 100, 255, 257, 512)

    # ---- tmvs_rank_sum(slots, world, count, out, stream)
    rs = lib.tmvs_rank_sum
    assert rs(None, 2, 16, p, None) == ARG and rs(p, 2, 16, None, None) == ARG
    for world in (0, -1):
        assert rs(p, world, 16, p, None) == ARG
    for count in (0, -1):
        assert rs(p, 2, count, p, None) == ARG

    # ---- tmvs_bn_moments_grouped(z, groups, nvox, C, ws, ws_bytes, sums, stream)
    need = lib.tmvs_bn_train_workspace_grouped(2, 16, 8)
    mo = lib.tmvs_bn_moments_grouped
    for nul in range(3):
        a = [p, p, p]
        a[nul] = None
        assert mo(a[0], 2, 16, 8, a[1], big, a[2], None) == ARG, nul
    for groups, nvox in ((0, 16), (-1, 16), (2, 0), (2, -1)):
        assert mo(p, groups, nvox, 8, p, big, p, None) == ARG
    for c in (0, -8) + not_dividing:
        assert mo(p, 2, 16, c, p, big, p, None) == SHAPE, c
    assert mo(p, 2, 16, 8, p, need - 1, p, None) == ARG

    # ---- tmvs_bn_stats_from_sums(sums, groups, C, n_total, mean, var, stream)
    fs = lib.tmvs_bn_stats_from_sums
    for nul in range(3):
        a = [p, p, p]
        a[nul] = None
        assert fs(a[0], 2, 8, 32, a[1], a[2], None) == ARG, nul
    for groups, n_total in ((0, 32), (-1, 32), (2, 0), (2, -1)):
        assert fs(p, groups, 8, n_total, p, p, None) == ARG
    for c in (0, -8) + not_dividing:
        assert fs(p, 2, c, 32, p, p, None) == SHAPE, c

    # ---- tmvs_bn_relu_backward_sums_grouped(dy, z, groups, nvox, C, mean, var, gamma, beta, eps, ws, ws_bytes,
    #                                         sums, dgamma, dbeta, stream)
    bs = lib.tmvs_bn_relu_backward_sums_grouped
    for nul in range(10):
        a = [p] * 10
        a[nul] = None
        assert bs(a[0], a[1], 2, 16, 8, a[2], a[3], a[4], a[5], 1e-5, a[6], big, a[7], a[8], a[9], None) == ARG, nul
    for groups, nvox in ((0, 16), (-1, 16), (2, 0), (2, -1)):
        assert bs(p, p, groups, nvox, 8, p, p, p, p, 1e-5, p, big, p, p, p, None) == ARG
    for c in (0, -8) + not_dividing:
        assert bs(p, p, 2, 16, c, p, p, p, p, 1e-5, p, big, p, p, p, None) == SHAPE, c
    assert bs(p, p, 2, 16, 8, p, p, p, p, 1e-5, p, need - 1, p, p, p, None) == ARG

    # ---- tmvs_bn_relu_backward_apply_grouped(dy, z, groups, nvox, C, mean, var, gamma, beta, eps, global_sums,
    #                                          n_total, dz, stream)
    ba = lib.tmvs_bn_relu_backward_apply_grouped
    for nul in range(8):
        a = [p] * 8
        a[nul] = None
        assert ba(a[0], a[1], 2, 16, 8, a[2], a[3], a[4], a[5], 1e-5, a[6], 32, a[7], None) == ARG, nul
    for groups, nvox in ((0, 16), (-1, 16), (2, 0), (2, -1)):
        assert ba(p, p, groups, nvox, 8, p, p, p, p, 1e-5, p, 32, p, None) == ARG
    for n_total in (15, 0, -1):  # fewer elements than this rank's own
        assert ba(p, p, 2, 16, 8, p, p, p, p, 1e-5, p, n_total, p, None) == ARG
    for c in (0, -8) + not_dividing:
        assert ba(p, p, 2, 16, c, p, p, p, p, 1e-5, p, 32, p, None) == SHAPE, c

    # ---- the staged PixelwiseNet entries: (sims, batch, n_views, ndepth, height, width, ...)
    ws = lib.tmvs_pixelwise_train_workspace()
    dims, n = (1, 2, 4, 8, 8), 4 * 8 * 8
    bad_dims = [(0, 2, 4, 8, 8), (1, 0, 4, 8, 8), (1, 2, 0, 8, 8), (1, 2, 4, 0, 8), (1, 2, 4, 8, 0), (-1, 2, 4, 8, 8),
                (1, 2, 4, 8, -8)]

    def entry(name, pointers, d=dims, n_total=2 * n, nbytes=big):
        """the call of `name` with its pointers in order (None for a null), its dims, n_total and workspace size"""
        q = list(pointers)
        if name == "forward_sums":
            return lib.tmvs_pw_sync_forward_sums(q[0], *d, q[1], nbytes, q[2], None)
        if name == "forward_z1":
            return lib.tmvs_pw_sync_forward_z1(q[0], *d, q[1], q[2], n_total, q[3], nbytes, q[4], q[5], None)
        if name == "forward_weights":
            return lib.tmvs_pw_sync_forward_weights(q[0], *d, q[1], q[2], n_total, q[3], q[4], q[5], None)
        if name == "backward_s1":
            return lib.tmvs_pw_sync_backward_s1(q[0], *d, q[1], q[2], q[3], q[4], q[5], q[6], nbytes, q[7], None)
        if name == "backward_s2":
            return lib.tmvs_pw_sync_backward_s2(q[0], *d, q[1], q[2], q[3], q[4], q[5], q[6], n_total, q[7], nbytes,
                                                q[8], None)
        return lib.tmvs_pw_sync_backward_apply(q[0], *d, q[1], q[2], q[3], q[4], q[5], q[6], q[7], n_total, q[8], q[9],
                                               q[10], nbytes, q[11], q[12], None)

    # (pointer count, takes n_total, takes a workspace)
    table = {"forward_sums": (3, False, True), "forward_z1": (6, True, True), "forward_weights": (6, True, False),
             "backward_s1": (8, False, True), "backward_s2": (9, True, True), "backward_apply": (13, True, True)}
    for name, (nptr, has_n, has_ws) in table.items():
        for nul in range(nptr):
            a = [p] * nptr
            a[nul] = None
            assert entry(name, a) == ARG, (name, nul)
        for d in bad_dims:
            assert entry(name, [p] * nptr, d=d) == ARG, (name, d)
        if has_n:
            for n_total in (n - 1, 0, -1):
                assert entry(name, [p] * nptr, n_total=n_total) == ARG, (name, n_total)
        if has_ws:
            assert entry(name, [p] * nptr, nbytes=ws - 1) == ARG, name


def test_driver_flag_parses():
    from transmvsnet_amd import finetune
    base = ["--dataset", "bld_train", "--trainpath", "x", "--trainlist", "y"]
    assert finetune.parse_args(base).sync_bn is False  # off by default: runs without the flag keep their bits
    assert finetune.parse_args(base + ["--sync_bn"]).sync_bn is True
    text = finetune.make_parser().format_help()
    assert "--sync_bn" in text and "reference always" in " ".join(text.split())


def test_sync_off_without_distributed_and_the_refusals():
    from transmvsnet_amd import TransMVSNet, synthetic
    from transmvsnet_amd.distributed import ViewShard
    from transmvsnet_amd.train import TrainStepGraph
    m = TransMVSNet(ndepths=[8, 8, 8])
    assert m.sync_bn is None
    assert m.sync_batchnorm() is m and isinstance(m.sync_bn, sync_bn.SyncBN)
    assert (m.sync_bn.world, m.sync_bn.rank, m.sync_bn.active) == (1, 0, False)
    local = torch.arange(6, dtype=torch.float64)
    assert m.sync_bn.reduce(local) is local and m.sync_bn.record() == {"collectives": 0, "bytes": 0}  # the identity
    with sync_bn.using(m.sync_bn) as s:
        assert s is None and sync_bn.current() is None  # a one-rank group without `always`: today's calls
    with pytest.raises(ValueError, match="torch.distributed"):
        sync_bn.SyncBN(always=True)
    # sync together with a view-sharded forward
    feats = synthetic.synthetic_features(3, 64, 80)
    proj = synthetic.synthetic_cameras(3, 64, 80)
    with pytest.raises(RuntimeError, match="view-sharded"):
        m.eval().forward_features(feats, proj, synthetic.synthetic_depth_values(1), (64, 80), view_shard=ViewShard(0, 1, 2))
    # sync inside TrainStepGraph capture: refused before anything is captured
    with pytest.raises(RuntimeError, match="HIP-graph capture"):
        TrainStepGraph(lambda: None, m)
    assert m.sync_batchnorm(None) is m and m.sync_bn is None


def test_reduce_refuses_capture(monkeypatch):
    class Fake(sync_bn.SyncBN):
        def __init__(self):
            self.group, self.always, self.world, self.rank, self.comm_bytes, self.timer = None, True, 1, 0, [], None

    class CudaF64:
        dtype, is_cuda = torch.float64, True

        def is_contiguous(self):
            return True

    monkeypatch.setattr(sync_bn, "_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="HIP-graph capture"):
        Fake().reduce(CudaF64())


def _store():
    return "file://" + os.path.join(tempfile.mkdtemp(prefix="tmvs_sync_bn_"), "store")


def _values(rank, world):
    """[4 + world] doubles: three magnitudes 1, 2^60, -2^60 spread over the ranks (world 3, column 0: ranks 0, 1, 2
    hold 1, 2^60, -2^60, so rank order gives (1 + 2^60) - 2^60 = 0 and the reverse order 1: the fp64 sum depends
    on the order; two values alone commute, so at world 2 only the placement varies), plus random values"""
    g = torch.Generator().manual_seed(11 + rank)
    v = torch.randn(4 + world, generator=g, dtype=torch.float64)
    mags = [1.0, 2.0 ** 60, -2.0 ** 60]
    order = {2: [[0, 1, 1], [1, 0, 0], [0, 0, 1]], 3: [[0, 1, 2], [1, 0, 2], [1, 2, 0]]}[world]
    for col, ranks in enumerate(order):  # column `col`: rank ranks[i] adds magnitude i (two on one rank: their sum)
        v[col] = 0.0
        for i, r in enumerate(ranks):
            if r == rank:
                v[col] += mags[i]
    return v


def _reduce_worker(rank, world, store, q):
    dist.init_process_group("gloo", init_method=store, rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        s = sync_bn.SyncBN()
        assert (s.world, s.rank, s.active) == (world, rank, True)
        s.begin_step()
        out = s.reduce(_values(rank, world))
        out2 = s.reduce(_values(rank, world).view(-1, 1)).view(-1)  # shapes are kept, the bits repeat
        rec = s.record()
        s.check_counts((2, 5, 3, 64, 80))  # equal everywhere: passes (one more collective)
        refused = ""
        try:
            s.check_counts((2 + (rank == world - 1), 5, 3, 64, 80))
        except RuntimeError as e:
            refused = str(e)
        q.put((rank, out.numpy().copy(), out2.numpy().copy(), rec, s.record(), refused))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_reduce_is_the_rank_ordered_sum_on_every_rank_gloo(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    store = _store()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, store, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = _values(0, world).clone()
    for r in range(1, world):
        want += _values(r, world)
    # the order matters for these values: another order gives another sum
    back = _values(world - 1, world).clone()
    for r in range(world - 2, -1, -1):
        back += _values(r, world)
    if world > 2:
        assert want[0] == 0.0 and back[0] == 1.0
    k = want.numel()
    for rank, out, out2, rec, rec_after, refused in res:
        assert np.array_equal(out.view(np.int64), want.numpy().view(np.int64)), rank
        assert np.array_equal(out2.view(np.int64), want.numpy().view(np.int64)), rank
        assert rec == {"collectives": 2, "bytes": 2 * world * k * 8}
        assert rec_after == {"collectives": 4, "bytes": 2 * world * k * 8 + 2 * world * 5 * 8}
        assert "equal counts" in refused and "N_total == world * N_local" in refused, rank  # every rank raises
