"""The C-ABI boundary without a GPU: the library builds for gfx950, loads, exports every
function include/transmvs.h declares with the argument count the ctypes binding uses, and the
host-only entry points behave (version, status strings, BN fold, argument validation).
Also: the product path refuses CPU tensors (no fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from transmvsnet_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "transmvs.h")


def _declarations():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    decls = {}
    for m in re.finditer(r"\b(?:int|size_t|const\s+char\s*\*)\s*\*?\s*(tmvs_\w+)\s*\(([^)]*)\)\s*;", src):
        args = m.group(2).strip()
        n = 0 if args in ("", "void") else args.count(",") + 1
        decls[m.group(1)] = n
    return decls


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_header_declarations_match_binding():
    decls = _declarations()
    assert len(decls) >= 20
    assert set(decls) == set(_lib.SIGNATURES), set(decls) ^ set(_lib.SIGNATURES)
    for name, n in decls.items():
        assert len(_lib.SIGNATURES[name][1]) == n, name


def test_library_exports_every_symbol(lib):
    for name in _declarations():
        assert hasattr(lib, name), name
    assert lib.tmvs_abi_version() == _lib.ABI_VERSION


def test_header_constants_match_binding():
    src = open(HEADER).read()
    consts = dict(re.findall(r"#define\s+(TMVS_\w+)\s+(-?\d+)", src))
    assert int(consts["TMVS_ABI_VERSION"]) == _lib.ABI_VERSION
    assert int(consts["TMVS_PW_NPARAMS"]) == _lib.PW_NPARAMS
    assert int(consts["TMVS_ENC_NPARAMS"]) == _lib.ENC_NPARAMS
    assert int(consts["TMVS_KV_NFLOATS"]) == _lib.KV_NFLOATS
    assert int(consts["TMVS_WARP_PARTIAL"]) == _lib.WARP_PARTIAL
    assert int(consts["TMVS_WARP_ROT_PLAIN"]) == _lib.WARP_ROT_PLAIN


def test_status_strings(lib):
    for code in (0, -1, -2, -3):
        assert lib.tmvs_status_string(code)
    assert lib.tmvs_status_string(0) != lib.tmvs_status_string(-2)


def test_bn_fold_host(lib):
    """tmvs_bn_fold is host code: alpha = gamma/sqrt(var+eps) (reference op order), shift = beta - mean*alpha."""
    g = np.random.default_rng(0)
    gamma, beta, mean = (g.standard_normal(16).astype(np.float32) for _ in range(3))
    var = g.random(16).astype(np.float32) + 0.1
    alpha = np.empty(16, np.float32)
    shift = np.empty(16, np.float32)
    p = lambda a: a.ctypes.data
    assert lib.tmvs_bn_fold(p(gamma), p(beta), p(mean), p(var), 16, 1e-5, p(alpha), p(shift)) == 0
    ea = (np.float32(1) / np.sqrt(var + np.float32(1e-5))) * gamma
    np.testing.assert_array_equal(alpha, ea)
    np.testing.assert_allclose(shift, beta - mean * ea, rtol=0, atol=1e-6)


def test_argument_validation_without_gpu(lib):
    """Null pointers / unsupported shapes are rejected before any launch."""
    assert lib.tmvs_warp_corr(None, None, None, None, None, 0, 0, 4, None, 1, 4, 32, 48, 8, 8, 0,
                              None, None, None, None) == -1
    assert lib.tmvs_softmax_wta(None, None, 1, 48, 8, 8, 425.0, 935.0, None, None, None, None, None) == -1
    assert lib.tmvs_costregnet_workspace(1, 48, 216, 288, 8) > 0
    assert lib.tmvs_depth_stage_workspace(48, 216, 288, 8) > lib.tmvs_costregnet_workspace(1, 48, 216, 288, 8)
    # the grouped K/V: a view subset keeps the tiling of the larger launch, so its slab is the subset's share
    L = 216 * 288
    assert lib.tmvs_fmt_kv_grouped_workspace(5, 5, L) == lib.tmvs_fmt_kv_workspace(5, L)
    assert 5 * lib.tmvs_fmt_kv_grouped_workspace(1, 5, L) == lib.tmvs_fmt_kv_workspace(5, L)
    assert lib.tmvs_fmt_kv_grouped_workspace(1, 1, L) == lib.tmvs_fmt_kv_workspace(1, L)
    assert lib.tmvs_fmt_kv_grouped_workspace(0, 5, L) == 0
    assert lib.tmvs_fmt_kv_grouped(None, 1, 5, L, None, None, 0, None, None) == -1
    # the apply with an explicit tiling: declared, bound with its 8 arguments, and it validates like tmvs_fmt_apply
    # (the pointers are host memory that is never read; every call has exactly one thing wrong with it)
    assert _declarations()["tmvs_fmt_apply_tiled"] == len(_lib.SIGNATURES["tmvs_fmt_apply_tiled"][1]) == 8
    backing = np.zeros(64, np.float32)
    p = backing.ctypes.data
    for tiled in (lib.tmvs_fmt_apply_tiled, lambda *a: lib.tmvs_fmt_apply(*a[:6], a[7])):
        for tpw in (0, 1, 3):
            for nul in range(3):  # x, kv, enc_w
                a = [p, p, p]
                a[nul] = None
                assert tiled(a[0], 1, 16, a[1], 160, a[2], tpw, None) == -1, (nul, tpw)
            for nv, l, stride in ((0, 16, 160), (-1, 16, 160), (1, 0, 160), (1, -1, 160), (1, 16, -1)):
                assert tiled(p, nv, l, p, stride, p, tpw, None) == -1, (nv, l, stride, tpw)
    # the split FMT needs both K/V slabs; NULL side stream falls back to (and validates like) tmvs_fmt_forward
    assert lib.tmvs_fmt_forward_split_workspace(5, L) > lib.tmvs_fmt_forward_workspace(5, L)
    assert lib.tmvs_fmt_forward_split_workspace(1, L) == lib.tmvs_fmt_forward_workspace(1, L)
    assert lib.tmvs_fmt_forward_split(None, 0, None, 0, 0, 5, 216, 288, None, None, 0, None, None, None) == -1


def test_warp_corr_shape_validation_without_gpu(lib):
    """tmvs_warp_corr with given view weights reads them at (y >> vw_shift, x >> vw_shift) of an
    [H >> vw_shift][W >> vw_shift] map, so a height or width that is no multiple of 2^vw_shift would
    index column W >> vw_shift (and, on the last row, past the buffer): TMVS_ERR_SHAPE, as is a shift no
    size can satisfy. tmvs_warp_corr_backward refuses planes with D > 64 likewise. Both before anything
    is enqueued (the pointers are host memory that is never read; no device is needed to refuse)."""
    ARG, SHAPE = -1, -2
    backing = np.zeros(256, np.float32)
    p = (backing.ctypes.data + 63) & ~63

    def given(h, w, shift, c=8, d=8):
        return lib.tmvs_warp_corr(p, p, p, p, p, shift, 0, 2, None, 1, 2, c, d, h, w, 0, p, None, None, None)

    for h, w, shift in ((9, 28, 1), (8, 29, 1), (9, 29, 1), (10, 28, 2), (12, 30, 2), (4, 4, 3), (1, 8, 1),
                        (16, 16, 15), (16, 16, 31), (16, 16, 32), (16, 16, 1 << 20)):
        for c, d in ((8, 8), (16, 32), (32, 48)):
            assert given(h, w, shift, c, d) == SHAPE, (h, w, shift, c, d)
    assert given(8, 28, -1) == ARG
    # the PARTIAL (view-sharded) form validates the same way
    assert lib.tmvs_warp_corr(p, p, p, p, p, 1, 0, 2, None, 1, 2, 8, 8, 9, 29, _lib.WARP_PARTIAL, p, p, None,
                              None) == SHAPE
    # planes: D <= 64, refused before the workspace is cleared
    big = 1 << 40
    for c in (8, 16, 32):
        assert lib.tmvs_warp_corr_backward(p, p, p, p, p, 2, c, 65, 5, 5, _lib.WARP_BWD_PLANES, p, big, p, p,
                                           None) == SHAPE, c


def test_training_primitive_validation_without_gpu(lib):
    """The training-only token and glue entry points (fmt_train / pathway_train / featurenet_train / loss):
    null pointers and non-positive sizes are TMVS_ERR_ARG (one pinned exception: tmvs_depth_metrics, see its
    block below), shapes outside the dispatch tables TMVS_ERR_SHAPE, all before any launch (the pointers below are host memory that is never read);
    the workspace sizes follow the formulas in the sources, checked either side of each doubling point."""
    ARG, SHAPE = -1, -2
    backing = np.zeros(256, np.float32)
    p = (backing.ctypes.data + 63) & ~63  # 16-byte aligned, as the float4 entry points require
    q = p + 256
    big = 1 << 40

    # ---- tmvs_token_linear / tmvs_token_linear_res
    tl = lib.tmvs_token_linear
    assert tl(None, 16, 32, 32, p, p, 0, None, 0, p, None) == ARG
    assert tl(p, 16, 32, 32, None, p, 0, None, 0, p, None) == ARG
    assert tl(p, 16, 32, 32, p, p, 0, None, 0, None, None) == ARG
    for t in (0, -1):
        assert tl(p, t, 32, 32, p, p, 0, None, 0, p, None) == ARG
    for tr in (0, 1):
        assert tl(p, 16, 64, 64, p, p, tr, None, 0, p, None) == SHAPE
        assert tl(p, 16, 16, 32, p, p, tr, None, 0, p, None) == SHAPE
    tlr = lib.tmvs_token_linear_res
    assert tlr(p, 16, 32, 32, p, p, 0, None, None, q, None) == ARG
    assert tlr(p, 16, 32, 32, p, p, 0, None, q, q, None) == ARG  # residual == y: in place is refused
    assert tlr(p, 16, 32, 32, p, p, 0, None, q + 4, p, None) == ARG  # rows move as 16-byte quads
    assert tlr(None, 16, 32, 32, p, p, 0, None, p, q, None) == ARG
    assert tlr(p, 16, 32, 32, None, p, 0, None, p, q, None) == ARG
    assert tlr(p, 16, 32, 32, p, p, 0, None, p, None, None) == ARG
    assert tlr(p, 0, 32, 32, p, p, 0, None, p, q, None) == ARG
    assert tlr(p, 16, 64, 64, p, p, 0, None, p, q, None) == SHAPE

    # ---- tmvs_token_wgrad
    tw = lib.tmvs_token_wgrad
    for nul in range(5):
        a = [p, p, p, p, p]
        a[nul] = None
        assert tw(a[0], 32, a[1], 32, 16, a[2], big, a[3], a[4], 0, None) == ARG
    for t in (0, -1):
        assert tw(p, 32, p, 32, t, p, big, p, p, 0, None) == ARG
    assert tw(p, 32, p, 32, 16, p, lib.tmvs_token_wgrad_workspace(16, 32, 32) - 1, p, p, 0, None) == ARG
    assert tw(p, 64, p, 64, 16, p, big, p, p, 0, None) == SHAPE
    assert tw(p, 16, p, 32, 16, p, big, p, p, 0, None) == SHAPE

    def tok_chunk(t, maxblk, c):
        while (t + c - 1) // c > maxblk:
            c *= 2
        return c

    T0 = 512 * 256
    for t in (1, 77, 1961, T0 - 1, T0, T0 + 1, T0 + 77, 2 * T0 - 1, 2 * T0, 2 * T0 + 1):
        c = tok_chunk(t, 512, 256)
        for a, b in ((32, 32), (64, 32), (32, 64)):
            assert lib.tmvs_token_wgrad_workspace(t, a, b) == -(-t // c) * (a * b + a) * 8, (t, a, b)
    assert lib.tmvs_token_wgrad_workspace(T0, 64, 32) == 512 * 2112 * 8        # 256-token blocks
    assert lib.tmvs_token_wgrad_workspace(T0 + 1, 64, 32) == 257 * 2112 * 8    # 512-token blocks
    assert lib.tmvs_token_wgrad_workspace(2 * T0 + 1, 64, 32) == 257 * 2112 * 8  # 1024-token blocks

    # ---- tmvs_layer_norm_fwd / tmvs_layer_norm_bwd
    lf = lib.tmvs_layer_norm_fwd
    for nul in range(4):
        a = [p, p, p, q]
        a[nul] = None
        assert lf(a[0], 16, a[1], a[2], a[3], None) == ARG
    for t in (0, -1):
        assert lf(p, t, p, p, q, None) == ARG
    lb = lib.tmvs_layer_norm_bwd
    for nul in range(6):
        a = [p, p, p, p, q, p]
        a[nul] = None
        assert lb(a[0], a[1], 16, a[2], a[3], big, a[4], a[5], 0, None) == ARG
    for t in (0, -1):
        assert lb(p, p, t, p, p, big, q, p, 0, None) == ARG
    assert lb(p, p, 16, p, p, lib.tmvs_layer_norm_bwd_workspace(16) - 1, q, p, 0, None) == ARG
    T1 = 1024 * 256
    for t in (1, 255, 257, 1961, T1 - 1, T1, T1 + 1, T1 + 77, 2 * T1 - 1, 2 * T1, 2 * T1 + 1):
        assert lib.tmvs_layer_norm_bwd_workspace(t) == -(-t // tok_chunk(t, 1024, 256)) * 64 * 8, t
    assert lib.tmvs_layer_norm_bwd_workspace(T1) == 1024 * 64 * 8
    assert lib.tmvs_layer_norm_bwd_workspace(T1 + 1) == 513 * 64 * 8

    # ---- tmvs_linattn_fwd / tmvs_linattn_bwd_q / tmvs_linattn_bwd_kv
    af = lib.tmvs_linattn_fwd
    for nul in range(3):
        a = [p, p, q]
        a[nul] = None
        assert af(a[0], 16, 8, a[1], 0, a[2], None) == ARG
    for t, tpg in ((0, 8), (-1, 8), (16, 0), (16, -1)):
        assert af(p, t, tpg, p, 0, q, None) == ARG
    aq = lib.tmvs_linattn_bwd_q
    for nul in range(6):
        a = [p, p, p, p, q, q]
        a[nul] = None
        assert aq(a[0], a[1], 16, 8, a[2], 0, a[3], big, a[4], a[5], None) == ARG
    for t, tpg in ((0, 8), (-1, 8), (16, 0), (16, -1)):
        assert aq(p, p, t, tpg, p, 0, p, big, q, q, None) == ARG
    assert aq(p, p, 10, 4, p, 0, p, big, q, q, None) == SHAPE  # tokens % tokens_per_group != 0
    assert aq(p, p, 1961 * 3 + 1, 1961, p, 160, p, big, q, q, None) == SHAPE
    assert aq(p, p, 16, 8, p, 0, p, lib.tmvs_linattn_bwd_workspace(16, 8) - 1, q, q, None) == ARG
    ak = lib.tmvs_linattn_bwd_kv
    for nul in range(5):
        a = [p, p, p, q, q]
        a[nul] = None
        assert ak(a[0], a[1], 16, 8, a[2], a[3], a[4], None) == ARG
    for t, tpg in ((0, 8), (-1, 8), (16, 0), (16, -1)):
        assert ak(p, p, t, tpg, p, q, q, None) == ARG

    def group_chunk(tpg):
        c = 128
        while c > 1 and tpg % c:
            c >>= 1
        while tpg // c > 512 and tpg % (2 * c) == 0:
            c *= 2
        return c

    G0 = 128 * 512  # the largest group 128-token blocks cover with 512 of them
    want = {1: 1, 6: 2, 320: 64, 1961: 1, 2 * 1961: 2, G0 - 1: 1, G0: 128, G0 + 1: 1, 128 * 513: 128, 128 * 514: 256,
            131072: 256, 3 * 131072: 1024}
    for tpg, c in want.items():
        assert group_chunk(tpg) == c, tpg
        for groups in (1, 3):
            assert lib.tmvs_linattn_bwd_workspace(groups * tpg, tpg) == groups * tpg // c * 160 * 8, (tpg, groups)

    # ---- tmvs_upsample2_add_nhwc / tmvs_upsample2_backward_nhwc
    ua, ub = lib.tmvs_upsample2_add_nhwc, lib.tmvs_upsample2_backward_nhwc
    for nul in range(3):
        a = [p, p, q]
        a[nul] = None
        assert ua(a[0], a[1], 1, 2, 2, 8, a[2], None) == ARG
    assert ub(None, 1, 2, 2, 8, q, None) == ARG and ub(p, 1, 2, 2, 8, None, None) == ARG
    for n, h, w in ((0, 2, 2), (1, 0, 2), (1, 2, 0), (-1, 2, 2), (1, -1, 2), (1, 2, -1)):
        assert ua(p, p, n, h, w, 8, q, None) == ARG
        assert ub(p, n, h, w, 8, q, None) == ARG
    for c in (32, 4, 0):
        assert ua(p, p, 1, 2, 2, c, q, None) == SHAPE
        assert ub(p, 1, 2, 2, c, q, None) == SHAPE

    # ---- tmvs_colsum
    cs = lib.tmvs_colsum
    for nul in range(3):
        a = [p, p, q]
        a[nul] = None
        assert cs(a[0], 16, 8, a[1], big, a[2], None) == ARG
    for n, c in ((0, 8), (-1, 8), (16, 0), (16, -1), (16, 33)):
        assert cs(p, n, c, p, big, q, None) == ARG
    assert cs(p, 16, 8, p, lib.tmvs_colsum_workspace(16, 8) - 1, q, None) == ARG

    def ppb_for(n, maxblk):
        ppb = 1024
        while (n + ppb - 1) // ppb > maxblk:
            ppb *= 2
        return ppb

    N0 = 1024 * 1024
    for n in (1, 7, 1025, N0 - 1, N0, N0 + 1, N0 + 3, 2 * N0 - 1, 2 * N0, 2 * N0 + 1):
        for c in (1, 8, 27, 32):
            assert lib.tmvs_colsum_workspace(n, c) == -(-n // ppb_for(n, 1024)) * c * 8, (n, c)
    assert lib.tmvs_colsum_workspace(N0, 8) == 1024 * 8 * 8
    assert lib.tmvs_colsum_workspace(N0 + 1, 8) == 513 * 8 * 8

    # ---- tmvs_nearest_up2_backward_nhwc / tmvs_softmax_backward
    nu = lib.tmvs_nearest_up2_backward_nhwc
    assert nu(None, 1, 2, 2, 8, 0, q, None) == ARG and nu(p, 1, 2, 2, 8, 0, None, None) == ARG
    for dims in ((0, 2, 2, 8), (1, 0, 2, 8), (1, 2, 0, 8), (1, 2, 2, 0), (-1, 2, 2, 8), (1, 2, 2, -8)):
        assert nu(p, *dims, 0, q, None) == ARG
    sb = lib.tmvs_softmax_backward
    for nul in range(3):
        a = [p, p, q]
        a[nul] = None
        assert sb(a[0], a[1], 1, 8, 2, 2, a[2], None) == ARG
    for dims in ((0, 8, 2, 2), (1, 0, 2, 2), (1, 8, 0, 2), (1, 8, 2, 0), (-1, 8, 2, 2), (1, -8, 2, 2)):
        assert sb(p, p, *dims, q, None) == ARG

    # ---- tmvs_depth_metrics
    dm = lib.tmvs_depth_metrics
    for nul in range(5):
        a = [p, p, p, p, q]
        a[nul] = None
        assert dm(a[0], a[1], a[2], 16, 2.5, a[3], big, a[4], None) == ARG
    # KNOWN MISMATCH, pinned so it cannot drift unnoticed: include/transmvs.h documents TMVS_ERR_ARG for a
    # non-positive size, and every other entry point above returns it; tmvs_depth_metrics (csrc/loss.hip)
    # rejects n <= 0 before any launch too, but with TMVS_ERR_SHAPE. The fix is to fold `n <= 0` into its
    # first (TMVS_ERR_ARG) check; when it lands, this expectation becomes ARG.
    for n in (0, -1):
        assert dm(p, p, p, n, 2.5, p, big, q, None) == SHAPE
    assert dm(p, p, p, 16, 2.5, p, lib.tmvs_depth_metrics_workspace(16) - 1, q, None) == ARG


def test_view_aggregation_validation_without_gpu(lib):
    """tmvs_aggregate_train and tmvs_aggregate_train_backward read the view weights at (y >> vw_shift,
    x >> vw_shift) of an [H >> vw_shift][W >> vw_shift] map per view. A height or width with any of its low
    vw_shift bits set would read the next row's weight in the last column and the next view's map (past the
    buffer, for the last view) in the last row: TMVS_ERR_SHAPE, as is a shift above 4 (the model uses 0, 1, 2).
    Null pointers, non-positive sizes and a negative shift stay TMVS_ERR_ARG. All before any launch (the
    pointers are host memory that is never read), and every call has exactly one thing wrong with it."""
    ARG, SHAPE = -1, -2
    backing = np.zeros(256, np.float32)
    p = (backing.ctypes.data + 63) & ~63
    fwd, bwd = lib.tmvs_aggregate_train, lib.tmvs_aggregate_train_backward

    def both(v, d, h, w, shift):
        return (fwd(p, p, v, d, h, w, shift, p, p, None), bwd(p, p, p, p, p, v, d, h, w, shift, p, p, None),
                bwd(p, p, p, p, p, v, d, h, w, shift, p, None, None))

    for h, w, shift in ((9, 28, 1), (8, 29, 1), (9, 29, 1), (1, 8, 1), (8, 1, 1), (10, 28, 2), (12, 30, 2), (9, 12, 2),
                        (12, 13, 2), (4, 12, 3), (8, 4, 3), (16, 24, 4), (8, 16, 4), (1, 1, 1), (3, 3, 2)):
        for v, d in ((1, 1), (3, 8), (5, 48)):
            assert both(v, d, h, w, shift) == (SHAPE,) * 3, (v, d, h, w, shift)
    for shift in (5, 6, 15, 30, 31, 32, 33, 64, 1 << 20, (1 << 31) - 1):  # whatever the size, also one it divides
        assert both(2, 4, 1 << 12, 1 << 12, shift) == (SHAPE,) * 3, shift
        assert both(2, 4, 16, 16, shift) == (SHAPE,) * 3, shift
    for shift in (-1, -2, -(1 << 31)):
        assert both(2, 4, 16, 16, shift) == (ARG,) * 3, shift
    for dims in ((0, 4, 8, 8), (2, 0, 8, 8), (2, 4, 0, 8), (2, 4, 8, 0), (-1, 4, 8, 8), (2, -4, 8, 8), (2, 4, -8, 8),
                 (2, 4, 8, -8)):
        for shift in (0, 1, 2):
            assert both(*dims, shift) == (ARG,) * 3, (dims, shift)
    for shift in (0, 1, 2, 3, 4):
        for nul in range(4):
            a = [p, p, p, p]
            a[nul] = None
            assert fwd(a[0], a[1], 2, 4, 16, 32, shift, a[2], a[3], None) == ARG, (nul, shift)
        for nul in range(6):  # dview_w is optional: NULL there is no error
            a = [p, p, p, p, p, p]
            a[nul] = None
            assert bwd(a[0], a[1], a[2], a[3], a[4], 2, 4, 16, 32, shift, a[5], p, None) == ARG, (nul, shift)

    # ---- the PixelwiseNet entry points next to them (csrc/pw_train.hip): nulls, sizes and the workspace
    pf, pb = lib.tmvs_pixelwise_train_forward, lib.tmvs_pixelwise_train_backward
    big = 1 << 40
    need = lib.tmvs_pixelwise_train_workspace()
    assert need >= (1024 * 160 + 2 + 16 + 25 + 160 + 16) * 8
    for nul in range(6):
        a = [p, p, p, p, p, p]
        a[nul] = None
        assert pf(a[0], 2, 4, 8, 8, a[1], a[2], big, a[3], a[4], a[5], None) == ARG, nul
    for nul in range(9):
        a = [p] * 9
        a[nul] = None
        assert pb(a[0], 2, 4, 8, 8, a[1], a[2], a[3], a[4], a[5], a[6], big, a[7], a[8], None) == ARG, nul
    for dims in ((0, 4, 8, 8), (2, 0, 8, 8), (2, 4, 0, 8), (2, 4, 8, 0), (-1, 4, 8, 8), (2, 4, 8, -8)):
        assert pf(p, *dims, p, p, big, p, p, p, None) == ARG, dims
        assert pb(p, *dims, p, p, p, p, p, p, big, p, p, None) == ARG, dims
    assert pf(p, 2, 4, 8, 8, p, p, need - 1, p, p, p, None) == ARG
    assert pb(p, 2, 4, 8, 8, p, p, p, p, p, p, need - 1, p, p, None) == ARG


def test_loss_and_adam_validation_without_gpu(lib):
    """tmvs_entropy_loss and the two Adam steps (csrc/loss.hip, csrc/optim.hip): what they refuse before any
    launch, and the loss workspace formula either side of a 256-pixel block."""
    ARG, SHAPE = -1, -2
    backing = np.zeros(256, np.float32)
    p = (backing.ctypes.data + 63) & ~63
    big = 1 << 40
    el = lib.tmvs_entropy_loss
    for nul in range(6):  # prob, depth_values, depth_gt, mask, workspace, out; the three maps after out are optional
        a = [p] * 6
        a[nul] = None
        for per_pixel in (0, 1):
            assert el(a[0], a[1], per_pixel, a[2], a[3], 1, 4, 8, 8, 1.0, a[4], big, a[5], None, None, None,
                      None) == ARG, nul
    for dims in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (-1, 4, 8, 8), (1, 4, 8, -8)):
        assert el(p, p, 0, p, p, *dims, 1.0, p, big, p, p, p, p, None) == SHAPE, dims
    assert el(p, p, 0, p, p, 1, 4, 1 << 12, 1 << 11, 1.0, p, big, p, p, p, p, None) == SHAPE  # HW * 256 >= 2^31
    assert el(p, p, 0, p, p, 2, 4, 3, 171, 1.0, p, lib.tmvs_entropy_loss_workspace(2, 3, 171) - 1, p, p, p, p,
              None) == ARG
    for b, h, w in ((1, 1, 1), (2, 1, 255), (3, 1, 256), (3, 1, 257), (1, 3, 171), (2, 257, 257), (65, 363, 363)):
        want = -(-b * 4 // 256) * 256 + b * -(-h * w // 256) * 2 * 4
        assert lib.tmvs_entropy_loss_workspace(b, h, w) == want, (b, h, w)
    for dims in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        assert lib.tmvs_entropy_loss_workspace(*dims) == 0, dims

    ad, add = lib.tmvs_adam_step, lib.tmvs_adam_step_dev
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1e-4)
    for nul in range(4):
        a = [p] * 4
        a[nul] = None
        assert ad(*a, 16, *hyper, 1, None) == ARG, nul
    for n, step in ((0, 1), (-1, 1), (16, 0), (16, -1)):
        assert ad(p, p, p, p, n, *hyper, step, None) == ARG, (n, step)
    for nul in range(6):  # lr_dev is optional
        a = [p] * 6
        a[nul] = None
        assert add(a[0], a[1], a[2], a[3], 16, hyper[0], None, *hyper[1:], a[4], a[5], None) == ARG, nul
    for n in (0, -1):
        assert add(p, p, p, p, n, hyper[0], None, *hyper[1:], p, p, None) == ARG, n


def test_training_conv_bn_validation_without_gpu(lib):
    """The training convolution, weight-gradient and BatchNorm entry points (costreg_train / featurenet_train):
    null pointers and non-positive extents are TMVS_ERR_ARG, channel counts outside the dispatch tables,
    stride 3, k of 0 or 8 and a BN channel count that does not divide 256 TMVS_ERR_SHAPE, a workspace one
    byte short TMVS_ERR_ARG -- all before any launch (the pointers are host memory that is never read; every
    call below has exactly one thing wrong with it). Entry points that answer differently from their
    neighbours are pinned with a comment. The workspace formulas are spelled out here and checked either
    side of their doubling points."""
    ARG, SHAPE = -1, -2
    backing = np.zeros(256, np.float32)
    p = (backing.ctypes.data + 63) & ~63
    q = p + 256
    big = 1 << 40

    def blocks(n, per, maxblk):
        while (n + per - 1) // per > maxblk:
            per *= 2
        return -(-n // per)

    # ---- tmvs_conv3d_generic(x, batch, cin, d_in, h_in, w_in, w, cout, d_out, h_out, w_out, stride, flags, y, stream)
    cg = lib.tmvs_conv3d_generic
    for nul in range(3):
        a = [p, p, q]
        a[nul] = None
        assert cg(a[0], 1, 8, 2, 2, 2, a[1], 8, 2, 2, 2, 1, 0, a[2], None) == ARG
    for pos in range(7):  # batch, d_in, h_in, w_in, d_out, h_out, w_out
        for bad in (0, -1):
            e = [1, 2, 2, 2, 2, 2, 2]
            e[pos] = bad
            assert cg(p, e[0], 8, e[1], e[2], e[3], p, 8, e[4], e[5], e[6], 1, 0, q, None) == ARG, (pos, bad)
    for flags in (0, 1, 2, 3):
        for cin, cout in ((3, 8), (8, 3), (0, 8), (8, 0), (-8, 8), (8, -8), (128, 8), (8, 128), (4, 4), (8, 24)):
            assert cg(p, 1, cin, 2, 2, 2, p, cout, 2, 2, 2, 1, flags, q, None) == SHAPE, (cin, cout)
        for stride in (0, 3, -1, 4):
            assert cg(p, 1, 8, 2, 2, 2, p, 8, 2, 2, 2, stride, flags, q, None) == SHAPE

    # ---- tmvs_conv3d_wgrad(direct, a_ch, batch, pd, ph, pw, gathered, b_ch, gd, gh, gw, stride, ws, ws_bytes, dw, stream)
    wg = lib.tmvs_conv3d_wgrad
    for nul in range(4):
        a = [p, p, p, q]
        a[nul] = None
        assert wg(a[0], 8, 1, 2, 2, 2, a[1], 8, 2, 2, 2, 1, a[2], big, a[3], None) == ARG
    for pos in range(7):  # batch, pd, ph, pw, gd, gh, gw
        for bad in (0, -1):
            e = [1, 2, 2, 2, 2, 2, 2]
            e[pos] = bad
            assert wg(p, 8, e[0], e[1], e[2], e[3], p, 8, e[4], e[5], e[6], 1, p, big, q, None) == ARG, (pos, bad)
    for stride in (0, 3, -1):
        assert wg(p, 8, 1, 2, 2, 2, p, 8, 2, 2, 2, stride, p, big, q, None) == SHAPE
    # the 12 dispatched (direct, gathered) pairs; everything else is TMVS_ERR_SHAPE
    pairs = {(8, 1), (1, 8), (8, 8), (16, 8), (8, 16), (16, 16), (32, 16), (16, 32), (32, 32), (64, 32), (32, 64),
             (64, 64)}
    for a_ch in (0, 1, 3, 8, 16, 32, 64, 128):
        for b_ch in (0, 1, 3, 8, 16, 32, 64, 128):
            if (a_ch, b_ch) not in pairs:
                assert wg(p, a_ch, 1, 2, 2, 2, p, b_ch, 2, 2, 2, 1, p, big, q, None) == SHAPE, (a_ch, b_ch)
    for a_ch, b_ch in sorted(pairs):
        need = lib.tmvs_conv3d_wgrad_workspace(1, 2, 3, 5, a_ch, b_ch)
        assert need == 27 * a_ch * b_ch * 8
        assert wg(p, a_ch, 1, 2, 3, 5, p, b_ch, 2, 3, 5, 1, p, need - 1, q, None) == ARG
    V0 = 512 * 2048  # the most voxels 2048-voxel blocks cover with 512 of them
    for nvox in (1, 90, 2047, 2048, 2049, 2058, 18480, V0 - 1, V0, V0 + 1, 1052969, 2 * V0, 2 * V0 + 1):
        for a_ch, b_ch in ((8, 1), (8, 8), (64, 64)):
            want = blocks(nvox, 2048, 512) * 27 * a_ch * b_ch * 8
            assert lib.tmvs_conv3d_wgrad_workspace(1, 1, 1, nvox, a_ch, b_ch) == want, (nvox, a_ch, b_ch)
    assert lib.tmvs_conv3d_wgrad_workspace(1, 512, 2048, 1, 8, 8) == 512 * 27 * 64 * 8      # 2048-voxel blocks
    assert lib.tmvs_conv3d_wgrad_workspace(1, 1, 1, V0 + 1, 8, 8) == 257 * 27 * 64 * 8      # 4096-voxel blocks
    assert lib.tmvs_conv3d_wgrad_workspace(1, 17, 241, 257, 8, 8) == 258 * 27 * 64 * 8
    assert lib.tmvs_conv3d_wgrad_workspace(2, 3, 7, 49, 8, 8) == 2 * 27 * 64 * 8            # the batch counts

    # ---- tmvs_conv2d_generic(x, batch, cin, h_in, w_in, w, bias, cout, h_out, w_out, k, stride, pad, flags, y, stream)
    c2 = lib.tmvs_conv2d_generic
    for nul in range(3):  # (the bias may be NULL)
        a = [p, p, q]
        a[nul] = None
        assert c2(a[0], 1, 8, 4, 4, a[1], None, 8, 4, 4, 3, 1, 1, 0, a[2], None) == ARG
    for pos in range(5):  # batch, h_in, w_in, h_out, w_out
        for bad in (0, -1):
            e = [1, 4, 4, 4, 4]
            e[pos] = bad
            assert c2(p, e[0], 8, e[1], e[2], p, p, 8, e[3], e[4], 3, 1, 1, 0, q, None) == ARG, (pos, bad)
    for flags in (0, 1, 2, 3):
        for k in (0, 8, -1):
            assert c2(p, 1, 8, 4, 4, p, p, 8, 4, 4, k, 1, 1, flags, q, None) == SHAPE
        for stride in (0, 3, -1):
            assert c2(p, 1, 8, 4, 4, p, p, 8, 4, 4, 3, stride, 1, flags, q, None) == SHAPE
        assert c2(p, 1, 8, 4, 4, p, p, 8, 4, 4, 3, 1, -1, flags, q, None) == SHAPE  # pad < 0
        # cin in {3, 8, 16, 27, 32} with cout % 8 == 0; cin in {8, 16, 32} with cout % 9 == 0
        for cin, cout in ((4, 8), (0, 8), (-8, 8), (64, 8), (1, 8), (8, 7), (8, 10), (3, 9), (27, 27), (3, 27),
                          (8, 0), (8, -8), (8, -9)):
            assert c2(p, 1, cin, 4, 4, p, p, cout, 4, 4, 3, 1, 1, flags, q, None) == SHAPE, (cin, cout)

    # ---- tmvs_conv2d_wgrad(direct, a_ch, batch, ph, pw, gathered, b_ch, gh, gw, k, stride, pad, ws, ws_bytes, dw, stream)
    w2 = lib.tmvs_conv2d_wgrad
    for nul in range(4):
        a = [p, p, p, q]
        a[nul] = None
        assert w2(a[0], 8, 1, 4, 4, a[1], 8, 4, 4, 3, 1, 1, a[2], big, a[3], None) == ARG
    for pos in range(5):  # batch, ph, pw, gh, gw
        for bad in (0, -1):
            e = [1, 4, 4, 4, 4]
            e[pos] = bad
            assert w2(p, 8, e[0], e[1], e[2], p, 8, e[3], e[4], 3, 1, 1, p, big, q, None) == ARG, (pos, bad)
    for k in (0, 8, -1):
        assert w2(p, 8, 1, 4, 4, p, 8, 4, 4, k, 1, 1, p, big, q, None) == SHAPE
    for stride in (0, 3, -1):
        assert w2(p, 8, 1, 4, 4, p, 8, 4, 4, 3, stride, 1, p, big, q, None) == SHAPE
    # a_ch is padded to a multiple of 8: 1..32 with b_ch in {8, 16, 32}, and 8 x 3 (conv0)
    for a_ch, b_ch in ((0, 8), (33, 8), (64, 8), (8, 0), (8, 4), (8, 64), (16, 3), (8, 27), (9, 3)):
        assert w2(p, a_ch, 1, 4, 4, p, b_ch, 4, 4, 3, 1, 1, p, big, q, None) == SHAPE, (a_ch, b_ch)
    assert w2(p, 8, 1, 4, 4, p, 8, 4, 4, 3, 1, 1, p, lib.tmvs_conv2d_wgrad_workspace(1, 4, 4, 8, 8, 3) - 1, q, None) == ARG
    P0 = 512 * 1024
    for n in (1, 35, 1023, 1024, 1025, P0 - 1, P0, P0 + 1, 2 * P0, 2 * P0 + 1):
        for a_ch, b_ch, k in ((8, 3, 3), (27, 32, 3), (16, 8, 5), (9, 16, 1), (32, 32, 7)):
            want = blocks(n, 1024, 512) * k * k * (-(-a_ch // 8) * 8) * b_ch * 8
            assert lib.tmvs_conv2d_wgrad_workspace(1, 1, n, a_ch, b_ch, k) == want, (n, a_ch, b_ch, k)
    assert lib.tmvs_conv2d_wgrad_workspace(1, 512, 1024, 8, 8, 3) == 512 * 9 * 64 * 8
    assert lib.tmvs_conv2d_wgrad_workspace(1, 1, P0 + 1, 8, 8, 3) == 257 * 9 * 64 * 8

    # ---- BatchNorm: the workspace is [groups][blocks][2][C] partials and [groups][2][C] sums, fp64
    N0 = 4096 * 1024  # the most voxels 1024-voxel blocks cover with 4096 of them

    def bn_ws(nvox, c):
        return (blocks(nvox, 1024, 4096) + 1) * 2 * c * 8

    for nvox in (1, 1023, 1024, 1025, N0 - 1, N0, N0 + 1, 2 * N0, 2 * N0 + 1):
        for c in (1, 4, 8, 64, 256):
            assert lib.tmvs_bn_train_workspace(nvox, c) == bn_ws(nvox, c), (nvox, c)
            for groups in (1, 2, 5):
                assert lib.tmvs_bn_train_workspace_grouped(groups, nvox, c) == groups * bn_ws(nvox, c)
            for groups in (0, -1):
                assert lib.tmvs_bn_train_workspace_grouped(groups, nvox, c) == 0
    assert lib.tmvs_bn_train_workspace(N0, 8) == 4097 * 16 * 8        # 1024-voxel blocks
    assert lib.tmvs_bn_train_workspace(N0 + 1, 8) == 2050 * 16 * 8    # 2048-voxel blocks
    assert lib.tmvs_bn_train_workspace_grouped(3, N0 + 1, 8) == 3 * 2050 * 16 * 8
    not_dividing = (3, 5, 6, 12, 24, 48, 96, 100, 255, 257, 512)

    # ---- tmvs_bn_stats(z, nvox, C, ws, ws_bytes, mean, var, stream); _grouped: groups after z
    bs, bsg = lib.tmvs_bn_stats, lib.tmvs_bn_stats_grouped
    for nul in range(4):
        a = [p, p, q, q]
        a[nul] = None
        assert bs(a[0], 16, 8, a[1], big, a[2], a[3], None) == ARG
        assert bsg(a[0], 2, 16, 8, a[1], big, a[2], a[3], None) == ARG
    for nvox in (0, -1):
        assert bs(p, nvox, 8, p, big, q, q, None) == ARG
        assert bsg(p, 2, nvox, 8, p, big, q, q, None) == ARG
    for groups in (0, -1):
        assert bsg(p, groups, 16, 8, p, big, q, q, None) == ARG
    for c in (0, -8) + not_dividing:  # (a non-positive channel count is a shape here, an argument for the apply below)
        assert bs(p, 16, c, p, big, q, q, None) == SHAPE, c
        assert bsg(p, 2, 16, c, p, big, q, q, None) == SHAPE, c
    assert bs(p, 16, 8, p, bn_ws(16, 8) - 1, q, q, None) == ARG
    assert bsg(p, 3, 16, 8, p, 3 * bn_ws(16, 8) - 1, q, q, None) == ARG

    # ---- tmvs_bn_relu_train(z, nvox, C, mean, var, gamma, beta, eps, skip, out, stream); _grouped: groups after z
    bt, btg = lib.tmvs_bn_relu_train, lib.tmvs_bn_relu_train_grouped
    for nul in range(6):  # (skip may be NULL)
        a = [p, p, p, p, p, q]
        a[nul] = None
        assert bt(a[0], 16, 8, a[1], a[2], a[3], a[4], 1e-5, None, a[5], None) == ARG
        assert btg(a[0], 2, 16, 8, a[1], a[2], a[3], a[4], 1e-5, None, a[5], None) == ARG
    for nvox in (0, -1):
        assert bt(p, nvox, 8, p, p, p, p, 1e-5, None, q, None) == ARG
        assert btg(p, 2, nvox, 8, p, p, p, p, 1e-5, None, q, None) == ARG
    for groups in (0, -1):
        assert btg(p, groups, 16, 8, p, p, p, p, 1e-5, None, q, None) == ARG
    # PINNED DIFFERENCE: the apply has no workspace and folds `channels <= 0` into its first check, so a
    # non-positive channel count is TMVS_ERR_ARG here and TMVS_ERR_SHAPE for tmvs_bn_stats / tmvs_bn_relu_backward
    for c in (0, -8):
        assert bt(p, 16, c, p, p, p, p, 1e-5, None, q, None) == ARG
        assert btg(p, 2, 16, c, p, p, p, p, 1e-5, None, q, None) == ARG
    for c in not_dividing:
        assert bt(p, 16, c, p, p, p, p, 1e-5, None, q, None) == SHAPE, c
        assert btg(p, 2, 16, c, p, p, p, p, 1e-5, None, q, None) == SHAPE, c

    # ---- tmvs_bn_relu_backward(dy, z, nvox, C, mean, var, gamma, beta, eps, ws, ws_bytes, dz, dgamma, dbeta, stream)
    bb, bbg = lib.tmvs_bn_relu_backward, lib.tmvs_bn_relu_backward_grouped
    for nul in range(10):
        a = [p, p, p, p, p, p, p, q, q, q]
        a[nul] = None
        assert bb(a[0], a[1], 16, 8, a[2], a[3], a[4], a[5], 1e-5, a[6], big, a[7], a[8], a[9], None) == ARG
        assert bbg(a[0], a[1], 2, 16, 8, a[2], a[3], a[4], a[5], 1e-5, a[6], big, a[7], a[8], a[9], None) == ARG
    for nvox in (0, -1):
        assert bb(p, p, nvox, 8, p, p, p, p, 1e-5, p, big, q, q, q, None) == ARG
        assert bbg(p, p, 2, nvox, 8, p, p, p, p, 1e-5, p, big, q, q, q, None) == ARG
    for groups in (0, -1):
        assert bbg(p, p, groups, 16, 8, p, p, p, p, 1e-5, p, big, q, q, q, None) == ARG
    for c in (0, -8) + not_dividing:
        assert bb(p, p, 16, c, p, p, p, p, 1e-5, p, big, q, q, q, None) == SHAPE, c
        assert bbg(p, p, 2, 16, c, p, p, p, p, 1e-5, p, big, q, q, q, None) == SHAPE, c
    assert bb(p, p, 16, 8, p, p, p, p, 1e-5, p, bn_ws(16, 8) - 1, q, q, q, None) == ARG
    assert bbg(p, p, 3, 16, 8, p, p, p, p, 1e-5, p, 3 * bn_ws(16, 8) - 1, q, q, q, None) == ARG


def test_inference_costreg_validation_without_gpu(lib):
    """The inference CostRegNet and softmax / WTA entry points (costreg / glue): the status each returns before
    any launch, as the library answers today (the pointers are host memory that is never read; every call
    below has exactly one thing wrong with it). tmvs_conv3d_mfma asks for the device before it dispatches and
    is left out."""
    ARG, SHAPE = -1, -2
    backing = np.zeros(256, np.float32)
    p = (backing.ctypes.data + 63) & ~63
    q = p + 256

    # ---- tmvs_conv3d_bn_relu(x, batch, cin, d, h, w, wpk, alpha, shift, cout, stride, y, stream)
    cb = lib.tmvs_conv3d_bn_relu
    for nul in range(5):
        a = [p, p, p, p, q]
        a[nul] = None
        assert cb(a[0], 1, 16, 2, 2, 2, a[1], a[2], a[3], 16, 1, a[4], None) == ARG
    for pos in range(4):  # batch, d, h, w
        for bad in (0, -1):
            e = [1, 2, 2, 2]
            e[pos] = bad
            assert cb(p, e[0], 16, e[1], e[2], e[3], p, p, p, 16, 1, q, None) == ARG, (pos, bad)
    for stride in (0, 3, -1):  # a bad enum: TMVS_ERR_ARG (tmvs_conv3d_generic answers TMVS_ERR_SHAPE)
        assert cb(p, 1, 16, 2, 2, 2, p, p, p, 16, stride, q, None) == ARG
    conv_pairs = {(16, 16, 1), (32, 32, 1), (64, 64, 1), (8, 16, 2), (16, 32, 2), (32, 64, 2)}
    for cin in (0, 1, 8, 16, 32, 64, 128):
        for cout in (0, 1, 8, 16, 32, 64, 128):
            for stride in (1, 2):
                if (cin, cout, stride) not in conv_pairs:
                    assert cb(p, 1, cin, 2, 2, 2, p, p, p, cout, stride, q, None) == SHAPE, (cin, cout, stride)
    # one sample's input of 2 GiB or more (32-bit byte offsets): 16 channels x 4 bytes x 2^25 voxels
    assert cb(p, 1, 16, 32, 1024, 1024, p, p, p, 16, 1, q, None) == SHAPE
    assert cb(p, 1, 8, 64, 1024, 1024, p, p, p, 16, 2, q, None) == SHAPE

    # ---- tmvs_deconv3d_bn_relu_add(x, batch, cin, d, h, w, wpk, alpha, shift, cout, skip, y, stream)
    db = lib.tmvs_deconv3d_bn_relu_add
    for nul in range(6):  # (the skip is required here; tmvs_conv3d_mfma's is nullable)
        a = [p, p, p, p, p, q]
        a[nul] = None
        assert db(a[0], 1, 16, 2, 2, 2, a[1], a[2], a[3], 8, a[4], a[5], None) == ARG
    for pos in range(4):
        for bad in (0, -1):
            e = [1, 2, 2, 2]
            e[pos] = bad
            assert db(p, e[0], 16, e[1], e[2], e[3], p, p, p, 8, p, q, None) == ARG, (pos, bad)
    deconv_pairs = {(64, 32), (32, 16), (16, 8)}
    for cin in (0, 1, 8, 16, 32, 64, 128):
        for cout in (0, 1, 8, 16, 32, 64, 128):
            if (cin, cout) not in deconv_pairs:
                assert db(p, 1, cin, 2, 2, 2, p, p, p, cout, p, q, None) == SHAPE, (cin, cout)

    # ---- tmvs_costregnet_workspace: conv0, conv1, conv2, ..., x7, x9, x11, each rounded up to 256 bytes
    def ws_bytes(b, d, h, w, c=8):
        up = lambda n: (n + 255) & ~255
        v0 = b * d * h * w
        v1, v2, v3 = v0 // 8, v0 // 64, v0 // 512
        return (2 * up(v0 * c * 4) + 3 * up(v1 * 2 * c * 4) + 3 * up(v2 * 4 * c * 4) + 2 * up(v3 * 8 * c * 4))

    assert lib.tmvs_costregnet_workspace(2, 8, 24, 40, 8) == ws_bytes(2, 8, 24, 40) == 1459200
    assert lib.tmvs_costregnet_workspace(1, 4, 4, 4, 8) == ws_bytes(1, 4, 4, 4) == 6400  # the 256-byte rounding

    # ---- tmvs_costregnet(x, batch, depth, height, width, weights, workspace, workspace_bytes, logits, stream)
    #      tmvs_costregnet_wta(x, hyp, batch, depth, height, width, weights, workspace, workspace_bytes,
    #                          clamp_lo, clamp_hi, prob, depth_out, depth_raw, conf, stream)
    def weights(base_ch=8, null=None):
        st = _lib.CostRegWeights()
        for i in range(11):
            st.w[i] = p
        for i in range(10):
            st.alpha[i] = p
            st.shift[i] = p
        if null is not None:
            getattr(st, null[0])[null[1]] = None
        st.base_ch = base_ch
        return st

    cr, cw = lib.tmvs_costregnet, lib.tmvs_costregnet_wta
    good = weights()
    need = ws_bytes(1, 8, 8, 8)

    def both(x=p, hyp=p, b=1, d=8, h=8, w=8, st=good, ws=p, nbytes=need, out=q):
        """(tmvs_costregnet, tmvs_costregnet_wta) on the same arguments"""
        ref = None if st is None else ctypes.byref(st)
        return (cr(x, b, d, h, w, ref, ws, nbytes, out, None),
                cw(x, hyp, b, d, h, w, ref, ws, nbytes, 425.0, 935.0, out, q, q, q, None))

    assert both(x=None) == (ARG, ARG) and both(st=None) == (ARG, ARG) and both(ws=None) == (ARG, ARG)
    assert both(out=None) == (ARG, ARG)
    assert cw(p, None, 1, 8, 8, 8, ctypes.byref(good), p, need, 425.0, 935.0, q, q, q, q, None) == ARG
    for nul in range(3):  # depth_out, depth_raw, conf
        a = [q, q, q]
        a[nul] = None
        assert cw(p, p, 1, 8, 8, 8, ctypes.byref(good), p, need, 425.0, 935.0, q, a[0], a[1], a[2], None) == ARG
    for b in (0, -1):
        assert both(b=b) == (ARG, ARG)
    for null in (("w", 0), ("w", 10), ("alpha", 0), ("alpha", 9), ("shift", 0), ("shift", 9)):
        assert both(st=weights(null=null)) == (ARG, ARG), null
    for bad in (4, 12, 20, 7):  # a depth, height or width that is no multiple of 8
        assert both(h=bad) == (SHAPE, SHAPE) and both(w=bad) == (SHAPE, SHAPE)
    for bad in (4, 12, 20, 7):
        assert both(d=bad) == (SHAPE, SHAPE)
    for base_ch in (0, 4, 16, -8):
        assert both(st=weights(base_ch)) == (SHAPE, SHAPE), base_ch
    # one sample's 8-channel full-resolution volume of 2 GiB or more
    assert both(d=64, h=1024, w=1024, nbytes=1 << 40) == (SHAPE, SHAPE)
    assert both(nbytes=need - 1) == (ARG, ARG)
    assert both(nbytes=0) == (ARG, ARG)
    # the WTA form takes the depths tmvs_softmax_wta has an instance for: 40 and 56 are multiples of 8 that
    # the plain form accepts and it does not
    for d in (40, 56, 72, 128, 0, -8):
        assert cw(p, p, 1, d, 8, 8, ctypes.byref(good), p, 1 << 40, 425.0, 935.0, q, q, q, q, None) == SHAPE, d

    # ---- tmvs_softmax_wta(logits, hyp, batch, ndepth, height, width, clamp_lo, clamp_hi, prob, depth, depth_raw,
    #                       conf, stream)
    sw = lib.tmvs_softmax_wta
    for nul in range(6):
        a = [p, p, q, q, q, q]
        a[nul] = None
        assert sw(a[0], a[1], 1, 8, 2, 2, 425.0, 935.0, a[2], a[3], a[4], a[5], None) == ARG
    for pos in range(3):  # batch, height, width
        for bad in (0, -1):
            e = [1, 2, 2]
            e[pos] = bad
            assert sw(p, p, e[0], 8, e[1], e[2], 425.0, 935.0, q, q, q, q, None) == ARG, (pos, bad)
    # the depths without an instance, 0 and negative ones included, are a shape
    for d in (12, 40, 0, -8, 1, 2, 56, 128):
        assert sw(p, p, 1, d, 2, 2, 425.0, 935.0, q, q, q, q, None) == SHAPE, d


def test_forward_refuses_cpu_tensors():
    from transmvsnet_amd import TransMVSNet, synthetic
    m = TransMVSNet(ndepths=[8, 8, 8]).eval()
    feats = synthetic.synthetic_features(3, 64, 80)
    proj = synthetic.synthetic_cameras(3, 64, 80)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_features(feats, proj, synthetic.synthetic_depth_values(1), (64, 80))


def test_deform_conv2d_pack_host(lib):
    """tmvs_deform_conv2d_pack (HOST): A fragments [tap][mtile][half][lane][e], k-step s = 4*half + e feeds
    channel 16*half + 4*(lane/16) + e (the kernel's B lanes hold channels 4j..4j+3 and 16+4j..16+4j+3)."""
    import numpy as np
    import torch
    from transmvsnet_amd import ops
    for co in (8, 16, 32):
        w = torch.randn(co, 32, 3, 3)
        pk = ops.deform_conv2d_pack(w).numpy()
        mt_n = (co + 15) // 16
        assert pk.size == 9 * 8 * mt_n * 64
        wn = w.numpy()
        for k in (0, 4, 8):
            for s in (0, 3, 7):
                for mt in range(mt_n):
                    for lane in (0, 5, 17, 63):
                        h, e = s // 4, s % 4
                        c_o, c_i = 16 * mt + lane % 16, 16 * h + 4 * (lane // 16) + e
                        want = wn[c_o, c_i, k // 3, k % 3] if c_o < co else 0.0
                        assert pk[((((k * mt_n + mt) * 2 + h) * 64) + lane) * 4 + e] == want


def test_conv2d_pack_host(lib):
    """tmvs_conv2d_pack (HOST): [k-block][mtile][lane][e]; lane group j of k-block b owns the (tap, chunk) pair
    idx = 4b + j, element e = channel 4*chunk + e; zero padding past cin / cout / the last pair."""
    import numpy as np
    import torch
    from transmvsnet_amd import ops
    for (co, ci, k) in ((8, 3, 3), (16, 8, 5), (32, 32, 1), (32, 16, 3)):
        w = torch.randn(co, ci, k, k)
        pk = ops.conv2d_pack(w).numpy()
        cip = max(ci, 4)
        g = cip // 4
        nidx = k * k * g
        nb, mt = (nidx + 3) // 4, (co + 15) // 16
        assert pk.size == nb * mt * 64 * 4
        wn = w.numpy()
        for b in range(nb):
            for m in range(mt):
                for lane in (0, 7, 21, 63):
                    for e in range(4):
                        idx, c_o = 4 * b + lane // 16, 16 * m + lane % 16
                        want = 0.0
                        if idx < nidx and c_o < co:
                            tap, c = idx // g, 4 * (idx % g) + e
                            if c < ci:
                                want = wn[c_o, c, tap // k, tap % k]
                        assert pk[((b * mt + m) * 64 + lane) * 4 + e] == want


def test_host_rot_order_matches_torch_matmul():
    """ops.host_rot_order names the rounding this host's torch.matmul gives rot·(x, y, 1) (the
    reference's homo_warping grid, models/module.py:303); emulate it and compare bit for bit."""
    import numpy as np
    import torch
    from transmvsnet_amd import ops
    h, w = 216, 288
    order = ops.host_rot_order(h * w)
    assert order in ("fma", "plain")
    assert ops.warp_flags("auto", h * w) == (_lib.WARP_ROT_PLAIN if order == "plain" else 0)
    assert ops.warp_flags("fma", h * w) == 0 and ops.warp_flags("plain", h * w) == _lib.WARP_ROT_PLAIN
    rot = np.float32([[0.99, -0.02, -3.1], [0.015, 1.01, 2.7], [1.2e-5, -3e-6, 1.0]])
    y, x = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    x, y = x.reshape(-1), y.reshape(-1)
    got = torch.matmul(torch.from_numpy(rot)[None], torch.from_numpy(np.stack([x, y, np.ones_like(x)]))[None])[0]
    r0, r1, r2 = rot[:, 0:1], rot[:, 1:2], rot[:, 2:3]
    if order == "fma":
        emu = (r1.astype(np.float64) * y + (r0 * x)).astype(np.float32) + r2
    else:
        emu = (r0 * x + r1 * y) + r2
    assert (emu == got.numpy()).mean() == 1.0


def test_training_host_logic():
    """Training-path host logic (no GPU): the FMT weight block _FMTTrain packs from the 16 layer
    parameters is exactly EncoderLayer.packed() (the tmvs_fmt_* layout, include/transmvs.h
    TMVS_ENC_*); fmt_params walks the 8 layers in _ENC_PARAMS order; every training entry point
    refuses CPU tensors instead of falling back."""
    import torch
    from transmvsnet_amd import TransMVSNet
    from transmvsnet_amd.train import (_ENC_PARAMS, _pack_enc, costregnet_train, fmt_params, fmt_train,
                                       pathway_train, warp_corr_views)
    m = TransMVSNet()
    layers = m.FMT_with_pathway.FMT.layers
    ps = fmt_params(m)
    assert len(ps) == 8 * len(_ENC_PARAMS) == 128
    for i, layer in enumerate(layers):
        named = dict(layer.named_parameters())
        assert all(ps[16 * i + j] is named[n] for j, n in enumerate(_ENC_PARAMS))
        assert torch.equal(_pack_enc(ps[16 * i:16 * i + 16]), layer.packed())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fmt_train(m, torch.zeros(3, 32, 8, 10))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        warp_corr_views(torch.zeros(8, 10, 32), torch.zeros(2, 8, 10, 32), torch.zeros(4, 8, 10), None)
    with pytest.raises(RuntimeError):
        costregnet_train(m.cost_regularization[0], torch.zeros(1, 8, 16, 16))
    with pytest.raises(RuntimeError):
        pathway_train(m, torch.zeros(3, 8, 10, 32), torch.zeros(3, 16, 16, 20), torch.zeros(3, 8, 32, 40))


def test_every_launching_op_is_device_guarded():
    """Every public op in ops.py that launches on the current stream (through _launch(, which the shared
    bodies' names *_launch( end in too, or _stream() itself) runs under the device guard of its first GPU
    tensor argument (costregnet_wta was missing)."""
    import inspect

    from transmvsnet_amd import ops
    missing = []
    for name, fn in vars(ops).items():
        if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != ops.__name__:
            continue
        src = inspect.getsource(inspect.unwrap(fn))
        if ("_launch(" in src or "_stream()" in src) and not getattr(fn, "device_guarded", False):
            missing.append(name)
    assert not missing, missing


def test_training_device_packs_equal_host_packs():
    """featurenet_train packs weights on the device (no host sync per step) with index gathers that
    must reproduce the host packers tmvs_conv2d_pack / tmvs_deform_conv2d_pack bit for bit."""
    import torch

    from transmvsnet_amd import ops
    from transmvsnet_amd.featurenet_train import device_pack
    g = torch.Generator().manual_seed(0)
    for co, ci, k in ((8, 3, 3), (8, 8, 3), (16, 8, 5), (16, 16, 3), (32, 16, 5), (32, 32, 3), (32, 32, 1)):
        w = torch.randn(co, ci, k, k, generator=g)
        assert torch.equal(ops.conv2d_pack(w), device_pack("conv2d", w)), (co, ci, k)
    for co in (8, 16, 27, 32):
        w = torch.randn(co, 32, 3, 3, generator=g)
        assert torch.equal(ops.deform_conv2d_pack(w), device_pack("dcn", w)), co
