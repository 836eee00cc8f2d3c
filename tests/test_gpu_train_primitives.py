"""The training-only token and glue kernels, each called on its own through its transmvsnet_amd.ops
wrapper, at the tail shapes the whole-layer tests never reach: token counts that are no multiple of
the 16-token MFMA tile, of a wave's 64 or a block's 256 tokens, odd K/V groups, single pixels, the
sizes at which a reduction's chunk doubles.

  csrc/fmt_train.hip        token_linear(_res), token_wgrad, layer_norm_fwd/bwd, linattn_fwd/bwd_q/bwd_kv
  csrc/pathway_train.hip    upsample2_add_nhwc, upsample2_backward_nhwc
  csrc/featurenet_train.hip colsum, nearest_up2_backward_nhwc, softmax_backward
  csrc/loss.hip             depth_metrics

Every reference is plain torch on the CPU, written out below (nothing from oracle/ or train.py),
and evaluated in fp32 and in fp64. Error = max|got - ref64| / max|ref64| (test_gpu_train.py's _rel).
The bar is err_gpu <= max(2 x err_fp32ref, 1e-5): err_fp32ref is the CPU fp32 reference's own error
against fp64 on the same inputs, 2 x is the project's margin, and 1e-5 is the floor -- the kernels
reduce across tokens in fp64, so they should sit well below it. Measured err_fp32ref stays below 5e-6
(so the floor is the bar) except for the linear-attention dkv of the two longest single groups, where
the CPU's fp32 sum over the group drifts: 7.4e-6 at 131072 tokens and 6.6e-6 at 128 * 513; there the
2 x term sets the bar, about 1.5e-5 and 1.3e-5 (the kernel measured 1.1e-7 and 5.5e-8 on an MI355X).
Outputs the caller supplies are contiguous slices of larger buffers whose other rows hold a
sentinel that must survive bit for bit; the reductions documented as fixed-order are run twice
and must repeat bit for bit.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from transmvsnet_amd import ops

from tests._primitives import (DEV, FLOOR, SENTINEL, _assert_guard, _bar, _bits, _gen, _guarded, _hold,  # noqa: F401
                               _judge, _rel)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ token_linear
LIN_PAIRS = [(32, 32), (32, 64), (64, 32)]
LIN_OPTIONS = ["nobias", "transpose", "relu", "accumulate", "residual", "transpose_relu", "transpose_residual"]


def _linear_ref(dt, x, w, b, transpose_w, relu_of, base):
    y = x.to(dt) @ w.to(dt) if transpose_w else F.linear(x.to(dt), w.to(dt))
    if b is not None:
        y = y + b.to(dt)
    if relu_of is not None:
        y = torch.where(relu_of > 0, y, torch.zeros_like(y))
    if base is not None:
        y = base.to(dt) + y
    return y


def _judge_rows(name, got, r32, r64):
    _judge(name, got, r32, r64)
    _judge(name + " [last 3 rows]", got[-3:], r32[-3:], r64[-3:])  # the partial tile


@pytest.mark.parametrize("T", [1, 15, 17, 77, 256, 257, 1961])
@pytest.mark.parametrize("fin,fout", LIN_PAIRS)
def test_token_linear_token_sweep(fin, fout, T):
    """y = x W^T + b against F.linear: T below one 16-token tile, one either side of it, a partial last
    tile (77, 1961), exactly one block (256: the t0 >= T break is never taken) and one token past it."""
    g = _gen(fin, fout, T)
    x, w, b = torch.randn(T, fin, generator=g), torch.randn(fout, fin, generator=g), torch.randn(fout, generator=g)
    got = ops.token_linear(x.to(DEV), w.to(DEV), b.to(DEV))
    r32, r64 = (F.linear(x.to(dt), w.to(dt), b.to(dt)) for dt in (torch.float32, torch.float64))
    _judge_rows(f"token_linear {fin}->{fout} T={T}", got, r32, r64)


@pytest.mark.parametrize("option", LIN_OPTIONS)
@pytest.mark.parametrize("T", [77, 1961])
@pytest.mark.parametrize("fin,fout", LIN_PAIRS)
def test_token_linear_options(fin, fout, T, option):
    """Every option of tmvs_token_linear / tmvs_token_linear_res on its own and in the two combinations the
    backward uses, for every (in, out) pair. transpose_w takes a [in', out'] weight (for 32 -> 32 a swapped
    index passes every shape check: only the non-symmetric random weight tells); relu_of holds about half
    non-positive entries with exact 0.0 and -0.0 among them (both mask); out= accumulates into a slice of
    a sentinel-filled buffer."""
    g = _gen(fin, fout, T, LIN_OPTIONS.index(option) + 1)
    tr = "transpose" in option
    x = torch.randn(T, fin, generator=g)
    w = torch.randn(*((fin, fout) if tr else (fout, fin)), generator=g)
    assert not torch.equal(w[:32, :32], w[:32, :32].t())
    b = None if option == "nobias" else torch.randn(fout, generator=g)
    relu_of = base = None
    if "relu" in option:
        relu_of = torch.randn(T, fout, generator=g)
        relu_of.view(-1)[::7] = 0.0
        relu_of.view(-1)[3::11] = -0.0
        relu_of[-1, :4] = torch.tensor([0.0, -0.0, 1.0, -1.0])
        assert 0.35 < float((relu_of <= 0).float().mean()) < 0.75
    if option == "accumulate" or "residual" in option:
        base = torch.randn(T, fout, generator=g)
    d = lambda t: None if t is None else t.to(DEV)
    if option == "accumulate":
        buf, out = _guarded((T, fout), 2, base)
        got = ops.token_linear(d(x), d(w), d(b), out=out)
        assert got.data_ptr() == out.data_ptr()
        _assert_guard(buf, 2, T, "token_linear(out=)")
    else:
        res = d(base) if "residual" in option else None
        got = ops.token_linear(d(x), d(w), d(b), transpose_w=tr, relu_of=d(relu_of), residual=res)
        if res is not None:
            assert torch.equal(res.cpu(), base)  # the residual is read, never written
    r32, r64 = (_linear_ref(dt, x, w, b, tr, relu_of, base) for dt in (torch.float32, torch.float64))
    _judge_rows(f"token_linear {fin}->{fout} T={T} {option}", got, r32, r64)
    if relu_of is not None and base is None:
        assert torch.equal(got.cpu() == 0, relu_of <= 0)  # exactly the masked entries are (exact) zeros


# ------------------------------------------------------------------------------------------- token_wgrad
WG_PAIRS = [(32, 32), (64, 32), (32, 64)]


def _wgrad_ref(dt, dy, x):
    return dy.to(dt).t() @ x.to(dt), dy.to(dt).sum(0)


def _wgrad_case(a, b, T):
    g = _gen(a, b, T, 3)
    dy, x = torch.randn(T, a, generator=g), torch.randn(T, b, generator=g)
    dyd, xd = dy.to(DEV), x.to(DEV)
    dw, db = ops.token_wgrad(dyd, xd)
    dw2, db2 = ops.token_wgrad(dyd, xd)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)  # fixed-order reduction
    (w32, b32), (w64, b64) = (_wgrad_ref(dt, dy, x) for dt in (torch.float32, torch.float64))
    _judge(f"token_wgrad ({a},{b}) T={T} dw", dw, w32, w64)
    _judge(f"token_wgrad ({a},{b}) T={T} db", db, b32, b64)
    return dy, x, dw, db, (w32, b32), (w64, b64)


@pytest.mark.parametrize("T", [1, 63, 77, 1961])
@pytest.mark.parametrize("a,b", WG_PAIRS)
def test_token_wgrad(a, b, T):
    """dW = dy^T x, db = column sums of dy: one token, one short of the 64-token LDS chunk, a zero-filled
    tail chunk (77), several blocks with a tail (1961). At T = 77 the bar must also tell the result from
    the same sums without the last token (a one-token slip is visible at that size)."""
    dy, x, dw, db, (w32, b32), (w64, b64) = _wgrad_case(a, b, T)
    if T == 77:
        w_drop, b_drop = _wgrad_ref(torch.float64, dy[:-1], x[:-1])
        assert _rel(dw, w_drop) > _bar(_rel(w32, w64)), "the bar cannot see a dropped token in dw"
        assert _rel(db, b_drop) > _bar(_rel(b32, b64)), "the bar cannot see a dropped token in db"


def test_token_wgrad_chunk_doubles():
    """T = 512 * 256 + 77: the first size at which tok_chunk doubles to 512 tokens per block."""
    _wgrad_case(64, 32, 512 * 256 + 77)


@pytest.mark.parametrize("a,b", WG_PAIRS)
def test_token_wgrad_accumulate(a, b):
    """dw / db given: the result is their former content plus the gradient; the buffers around them stay."""
    T = 77
    g = _gen(a, b, T, 5)
    dy, x = torch.randn(T, a, generator=g), torch.randn(T, b, generator=g)
    dw0, db0 = torch.randn(a, b, generator=g) * 5, torch.randn(a, generator=g) * 5
    wbuf, dw = _guarded((a, b), 2, dw0)
    bbuf, db = _guarded((a,), 8, db0)
    got_w, got_b = ops.token_wgrad(dy.to(DEV), x.to(DEV), dw=dw, db=db)
    assert got_w.data_ptr() == dw.data_ptr() and got_b.data_ptr() == db.data_ptr()
    _assert_guard(wbuf, 2, a, "token_wgrad(dw=)")
    _assert_guard(bbuf, 8, a, "token_wgrad(db=)")
    refs = []
    for dt in (torch.float32, torch.float64):
        w, bb = _wgrad_ref(dt, dy, x)
        refs.append((dw0.to(dt) + w, db0.to(dt) + bb))
    _judge(f"token_wgrad ({a},{b}) accumulate dw", dw, refs[0][0], refs[1][0])
    _judge(f"token_wgrad ({a},{b}) accumulate db", db, refs[0][1], refs[1][1])


# -------------------------------------------------------------------------------------------- LayerNorm
def _ln_inputs(T, seed):
    g = _gen(T, seed)
    x = torch.randn(T, 32, generator=g) * 2 + 0.5
    gam, bet = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g)
    dy = torch.randn(T, 32, generator=g)
    return x, gam, bet, dy


def _ln_ref(dt, x, gam, bet, dy):
    xr, gr, br = (t.to(dt).clone().requires_grad_() for t in (x, gam, bet))
    y = F.layer_norm(xr, (32,), gr, br, 1e-5)
    y.backward(dy.to(dt))
    return y.detach(), xr.grad, gr.grad, br.grad


def _ln_bwd_case(T):
    x, gam, bet, dy = _ln_inputs(T, 11)
    dyd, xd, gd = dy.to(DEV), x.to(DEV), gam.to(DEV)
    dx, dgb = ops.layer_norm_bwd(dyd, xd, gd)
    dx2, dgb2 = ops.layer_norm_bwd(dyd, xd, gd)
    assert torch.equal(dgb, dgb2) and torch.equal(dx, dx2)  # fixed-order reduction
    r32, r64 = (_ln_ref(dt, x, gam, bet, dy) for dt in (torch.float32, torch.float64))
    _judge(f"layer_norm_bwd T={T} dx", dx, r32[1], r64[1])
    _judge(f"layer_norm_bwd T={T} dx [last 3 rows]", dx[-3:], r32[1][-3:], r64[1][-3:])
    _judge(f"layer_norm_bwd T={T} dgamma", dgb[:32], r32[2], r64[2])
    _judge(f"layer_norm_bwd T={T} dbeta", dgb[32:], r32[3], r64[3])


@pytest.mark.parametrize("T", [1, 255, 257, 1961])
def test_layer_norm_fwd(T):
    """LayerNorm(32) against F.layer_norm: one token, one short of and one past a 256-token block."""
    x, gam, bet, dy = _ln_inputs(T, 7)
    got = ops.layer_norm_fwd(x.to(DEV), gam.to(DEV), bet.to(DEV))
    r32, r64 = (_ln_ref(dt, x, gam, bet, dy)[0] for dt in (torch.float32, torch.float64))
    _judge(f"layer_norm_fwd T={T}", got, r32, r64)
    _judge(f"layer_norm_fwd T={T} [last 3 rows]", got[-3:], r32[-3:], r64[-3:])


@pytest.mark.parametrize("T", [1, 255, 257, 1961])
def test_layer_norm_bwd(T):
    """dx, dgamma, dbeta against autograd of F.layer_norm; T = 1 and 255 leave threads without a token."""
    _ln_bwd_case(T)


def test_layer_norm_bwd_chunk_doubles():
    """T = 1024 * 256 + 77: the first size at which tok_chunk doubles to 512 tokens per block."""
    _ln_bwd_case(1024 * 256 + 77)


def test_layer_norm_bwd_accumulate():
    """dgb given: dgamma | dbeta are added to its content; the floats around it stay."""
    T = 257
    x, gam, bet, dy = _ln_inputs(T, 13)
    dgb0 = torch.randn(64, generator=_gen(T, 17)) * 5
    buf, dgb = _guarded((64,), 8, dgb0)
    dx, got = ops.layer_norm_bwd(dy.to(DEV), x.to(DEV), gam.to(DEV), dgb=dgb)
    assert got.data_ptr() == dgb.data_ptr()
    _assert_guard(buf, 8, 64, "layer_norm_bwd(dgb=)")
    r32, r64 = (_ln_ref(dt, x, gam, bet, dy) for dt in (torch.float32, torch.float64))
    _judge("layer_norm_bwd accumulate dx", dx, r32[1], r64[1])
    _judge("layer_norm_bwd accumulate dgb", dgb, dgb0 + torch.cat([r32[2], r32[3]]),
           dgb0.double() + torch.cat([r64[2], r64[3]]))


# ------------------------------------------------------------------------------------- linear attention
# what each size reaches: see the docstring of test_linattn_fwd_bwd_q
ATTN_GROUPS = [(1961, 3), (320, 3), (6, 2), (1, 4), (2 * 1961, 1), (128 * 513, 1), (131072, 1)]  # (tpg, groups)
# the query side: one K/V row per group, plus three groups against one shared row (the source side,
# test_linattn_bwd_kv, has no shared form: it takes a dKV row per group)
ATTN_CASES = [(tpg, groups, groups) for tpg, groups in ATTN_GROUPS] + [(320, 3, 1)]


def _kv_rows(K, V):
    """K, V [G, S, 8, 4] (K after elu + 1) -> kv rows [G, 160] in the layout at the top of fmt_train.hip:
    row[h*16 + m*4 + d] = sum_s K[s,h,d] V[s,h,m], row[128 + h*4 + d] = sum_s K[s,h,d]"""
    G = K.shape[0]
    kv = torch.einsum("gshd,gshm->ghmd", K, V)
    return torch.cat([kv.reshape(G, 128), K.sum(1).reshape(G, 32)], 1)


def _attn_ref(dt, q, rows, tpg, dmsg):
    """models/FMT.py LinearAttention with the K/V sums given: -> (msg, dq, dKV per group)"""
    T = q.shape[0]
    G = T // tpg
    qr = q.to(dt).clone().requires_grad_()
    rr = rows.to(dt).expand(G, 160).clone().requires_grad_()  # one leaf row per group, shared or not
    Q = (F.elu(qr) + 1).view(G, tpg, 8, 4)
    KV, Ks = rr[:, :128].view(G, 8, 4, 4), rr[:, 128:].view(G, 8, 4)
    num = torch.einsum("gthd,ghmd->gthm", Q, KV)
    den = torch.einsum("gthd,ghd->gth", Q, Ks) + 1e-6
    msg = (num / den[..., None]).reshape(T, 32)
    msg.backward(dmsg.to(dt))
    return msg.detach(), qr.grad, rr.grad


@pytest.mark.parametrize("tpg,groups,nrows", ATTN_CASES)
def test_linattn_fwd_bwd_q(tpg, groups, nrows):
    """msg, dq and the per-group dKV | dKsum against autograd of the reference's LinearAttention, the K/V
    rows built on the CPU from random k, v (V scaled by 1/S as the model does; group g's K scaled by 1 + g,
    so a token reading another group's row is off by orders of magnitude).
      1961 x 3   odd group: one token per block (8 live threads), the combine's tail, forward blocks of 32
                 tokens that straddle two groups
      320 x 3    64-token blocks; 6 x 2: fewer tokens than a block; 1 x 4: one token per group
      2*1961     one shared row (kv_stride == 0), 2-token blocks -- the cross-layer form
      128*513    513 > 512 blocks per group, but 256 does not divide the group: the doubling loop refuses
      131072     the loop doubles to 256-token blocks
      320 x 3, 1 row: three groups reduce separately against one shared row"""
    T, S = tpg * groups, 50
    g = _gen(tpg, groups, nrows)
    k, v = torch.randn(nrows, S, 8, 4, generator=g, dtype=torch.float64), torch.randn(nrows, S, 8, 4, generator=g,
                                                                                      dtype=torch.float64)
    scale = (1.0 + torch.arange(nrows, dtype=torch.float64)).view(nrows, 1, 1, 1)
    rows = _kv_rows((F.elu(k) + 1) * scale, v / S).float()
    q, dmsg = torch.randn(T, 32, generator=g), torch.randn(T, 32, generator=g)
    qd, dd, rd = q.to(DEV), dmsg.to(DEV), rows.to(DEV)
    msg = ops.linattn_fwd(qd, rd, tpg)
    dq, dkv = ops.linattn_bwd_q(qd, dd, rd, tpg)
    dq2, dkv2 = ops.linattn_bwd_q(qd, dd, rd, tpg)
    assert torch.equal(dkv, dkv2) and torch.equal(dq, dq2)  # fixed-order reduction
    r32, r64 = (_attn_ref(dt, q, rows, tpg, dmsg) for dt in (torch.float32, torch.float64))
    tag = f"linattn tpg={tpg} groups={groups} rows={nrows}"
    for name, got, i in (("msg", msg, 0), ("dq", dq, 1), ("dkv", dkv, 2)):
        _judge(f"{tag} {name}", got, r32[i], r64[i])
    _judge(f"{tag} msg [last 3 rows]", msg[-3:], r32[0][-3:], r64[0][-3:])
    _judge(f"{tag} dq [last 3 rows]", dq[-3:], r32[1][-3:], r64[1][-3:])
    if groups > 1:  # the last token of group g and the first of group g + 1
        edge = torch.tensor([t for gi in range(1, groups) for t in (gi * tpg - 1, gi * tpg)])
        _judge(f"{tag} msg [group edges]", msg.cpu()[edge], r32[0][edge], r64[0][edge])
        _judge(f"{tag} dq [group edges]", dq.cpu()[edge], r32[1][edge], r64[1][edge])
        for gi in range(groups):
            _judge(f"{tag} dkv [group {gi}]", dkv[gi], r32[2][gi], r64[2][gi])


def _attn_kv_ref(dt, k, v, dkv, spg):
    G = k.shape[0] // spg
    kr, vr = (t.to(dt).clone().requires_grad_() for t in (k, v))
    rows = _kv_rows((F.elu(kr) + 1).view(G, spg, 8, 4), vr.view(G, spg, 8, 4))
    rows.backward(dkv.to(dt))
    return kr.grad, vr.grad


@pytest.mark.parametrize("spg,groups", ATTN_GROUPS)
def test_linattn_bwd_kv(spg, groups):
    """dk (through the elu), dv of the source tokens against autograd of the K/V sums, given a dKV | dKsum
    row per group that differs strongly between groups (scaled by 1 + g)."""
    S = spg * groups
    g = _gen(spg, groups, 23)
    k, v = torch.randn(S, 32, generator=g), torch.randn(S, 32, generator=g)
    dkv = torch.randn(groups, 160, generator=g) * (1.0 + torch.arange(groups, dtype=torch.float32)).view(groups, 1)
    dk, dv = ops.linattn_bwd_kv(k.to(DEV), v.to(DEV), dkv.to(DEV), spg)
    r32, r64 = (_attn_kv_ref(dt, k, v, dkv, spg) for dt in (torch.float32, torch.float64))
    tag = f"linattn_bwd_kv spg={spg} groups={groups}"
    for name, got, i in (("dk", dk, 0), ("dv", dv, 1)):
        _judge(f"{tag} {name}", got, r32[i], r64[i])
        _judge(f"{tag} {name} [last 3 rows]", got[-3:], r32[i][-3:], r64[i][-3:])
        if groups > 1:
            edge = torch.tensor([t for gi in range(1, groups) for t in (gi * spg - 1, gi * spg)])
            _judge(f"{tag} {name} [group edges]", got.cpu()[edge], r32[i][edge], r64[i][edge])


# -------------------------------------------------------------------------------------------- upsample2
UP_SHAPES = [(1, 1, 1), (2, 1, 3), (1, 3, 1), (2, 5, 7), (1, 16, 20)]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _up_ref(dt, r_nhwc, lat_nchw, du_nhwc):
    r = r_nhwc.to(dt).permute(0, 3, 1, 2).contiguous().requires_grad_()
    up = F.interpolate(r, scale_factor=2, mode="bilinear", align_corners=False)
    up.backward(du_nhwc.to(dt).permute(0, 3, 1, 2))
    return _nhwc(up.detach() + lat_nchw.to(dt)), _nhwc(r.grad), _nhwc(up.detach())


@pytest.mark.parametrize("n,h,w", UP_SHAPES)
@pytest.mark.parametrize("C", [8, 16])
def test_upsample2_forward_backward(C, n, h, w):
    """bilinear x2 (align_corners=False) + lateral, and its adjoint, against F.interpolate and its autograd:
    a single pixel and single rows / columns (in_size == 1: i1 == i0), odd sizes, border rows and columns.
    The adjoint identity <up(r), du> = <r, up_backward(du)> must hold for the GPU results themselves: the
    two sums (fp64, from the GPU tensors) may differ by the bar relative to sum |up(r) du|, the size of
    the terms whose fp32 rounding (about 1e-7 each) is all that separates them."""
    g = _gen(C, n, h, w)
    r, lat = torch.randn(n, h, w, C, generator=g), torch.randn(n, C, 2 * h, 2 * w, generator=g)
    du = torch.randn(n, 2 * h, 2 * w, C, generator=g)
    rd, dud = r.to(DEV), du.to(DEV)
    u = ops.upsample2_add_nhwc(rd, lat.to(DEV))
    dr = ops.upsample2_backward_nhwc(dud)
    r32, r64 = (_up_ref(dt, r, lat, du) for dt in (torch.float32, torch.float64))
    tag = f"upsample2 C={C} {n}x{h}x{w}"
    _judge(f"{tag} forward", u, r32[0], r64[0])
    _judge(f"{tag} backward", dr, r32[1], r64[1])
    for name, got, i in (("forward", u, 0), ("backward", dr, 1)):  # border rows and columns on their own
        for edge, sl in (("top", (slice(None), 0)), ("bottom", (slice(None), -1)),
                         ("left", (slice(None), slice(None), 0)), ("right", (slice(None), slice(None), -1))):
            _judge(f"{tag} {name} [{edge}]", got[sl], r32[i][sl], r64[i][sl])
    up = ops.upsample2_add_nhwc(rd, torch.zeros_like(lat, device=DEV)).double().cpu()

    def gap(up_r, dr_):
        lhs, rhs = float((up_r.double() * du.double()).sum()), float((r.double() * dr_.double()).sum())
        return abs(lhs - rhs) / float((up_r.double() * du.double()).abs().sum())
    _hold(f"{tag} adjoint", gap(up, dr.cpu()), gap(r32[2], r32[1]))


@pytest.mark.parametrize("shape", [(1, 3, 4, 8), (1, 4, 3, 8), (2, 5, 7, 16)])
def test_upsample2_backward_refuses_odd_extent(shape):
    with pytest.raises(ValueError, match="2h, 2w"):
        ops.upsample2_backward_nhwc(torch.zeros(shape, device=DEV))


# ------------------------------------------------------------------------------ nearest_up2_backward_nhwc
@pytest.mark.parametrize("n,h,w,C", [(1, 1, 1, 8), (2, 3, 5, 16), (1, 7, 9, 32)])
def test_nearest_up2_backward_bitwise(n, h, w, C):
    """The kernel fixes the order (p00 + p01) + (p10 + p11); the same fp32 additions on the CPU must give
    the same bits, without out= and, accumulating, as out + s into a slice of a sentinel-filled buffer."""
    g = _gen(n, h, w, C)
    d = torch.randn(n, 2 * h, 2 * w, C, generator=g)
    s = (d[:, 0::2, 0::2] + d[:, 0::2, 1::2]) + (d[:, 1::2, 0::2] + d[:, 1::2, 1::2])
    got = ops.nearest_up2_backward_nhwc(d.to(DEV))
    assert got.shape == s.shape and torch.equal(_bits(got), _bits(s))
    out0 = torch.randn(n, h, w, C, generator=g)
    buf, out = _guarded((n, h, w, C), 1, out0)
    got = ops.nearest_up2_backward_nhwc(d.to(DEV), out=out)
    assert got.data_ptr() == out.data_ptr()
    _assert_guard(buf, 1, n, "nearest_up2_backward_nhwc(out=)")
    assert torch.equal(_bits(out), _bits(out0 + s))


@pytest.mark.parametrize("shape", [(1, 3, 4, 8), (1, 4, 3, 8), (2, 5, 7, 16)])
def test_nearest_up2_backward_refuses_odd_extent(shape):
    with pytest.raises(ValueError, match="2h, 2w"):
        ops.nearest_up2_backward_nhwc(torch.zeros(shape, device=DEV))


# --------------------------------------------------------------------------------------- softmax_backward
@pytest.mark.parametrize("B,D,H,W", [(1, 1, 3, 5), (2, 8, 5, 7), (2, 48, 9, 11), (1, 32, 17, 16)])
def test_softmax_backward(B, D, H, W):
    """d logits = prob (dprob - sum_d prob dprob) with prob = softmax(logits, 1) in fp64 (the kernel gets
    prob.float()). With one depth plane the exact answer is zero everywhere."""
    g = _gen(B, D, H, W)
    logits = torch.randn(B, D, H, W, generator=g, dtype=torch.float64) * 3
    dprob = torch.randn(B, D, H, W, generator=g)
    prob = torch.softmax(logits, 1)
    got = ops.softmax_backward(prob.float().to(DEV), dprob.to(DEV))
    assert got.shape == prob.shape
    if D == 1:
        assert float(got.abs().max()) <= 1e-6 * float(dprob.abs().max())
        return
    r64 = prob * (dprob.double() - (prob * dprob.double()).sum(1, keepdim=True))
    p32 = torch.softmax(logits.float(), 1)
    r32 = p32 * (dprob - (p32 * dprob).sum(1, keepdim=True))
    _judge(f"softmax_backward {B}x{D}x{H}x{W}", got, r32, r64)
    _judge(f"softmax_backward {B}x{D}x{H}x{W} [last pixel]", got[-1, :, -1, -1], r32[-1, :, -1, -1], r64[-1, :, -1, -1])


# ------------------------------------------------------------------------------------------------- colsum
def _colsum_case(n, C):
    x = torch.randn(n, C, generator=_gen(n, C)) + 0.3  # non-zero mean: a dropped row shifts the sum
    xd = x.to(DEV)
    got = ops.colsum(xd)
    assert torch.equal(got, ops.colsum(xd))  # fixed-order reduction
    _judge(f"colsum n={n} C={C}", got, x.sum(0), x.double().sum(0))


@pytest.mark.parametrize("n", [1, 7, 1025])
@pytest.mark.parametrize("C", [1, 8, 27, 32])
def test_colsum(C, n):
    """Column sums of [n, C] for channel counts that are no power of two, fewer rows than the 8 row slots
    of a block (1, 7) and one row past a 1024-row block."""
    _colsum_case(n, C)


def test_colsum_chunk_doubles():
    """n = 1024 * 1024 + 3: the first size at which ppb_for doubles to 2048 rows per block."""
    _colsum_case(1024 * 1024 + 3, 8)


# ------------------------------------------------------------------------------------------ depth_metrics
INTERVAL = 2.5


def _metrics_inputs(n):
    g = _gen(n, 29)
    scale = INTERVAL * 192.0 / 128.0
    e = torch.rand(n, generator=g, dtype=torch.float64) * 5.0
    for edge in (1.0, 3.0):  # keep the scaled error away from the two thresholds
        e = torch.where((e - edge).abs() < 0.02, e + 0.05, e)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    gt = (torch.rand(n, generator=g, dtype=torch.float64) * 500 + 400).float()
    depth = (gt.double() + sign * e * scale).float()
    mask = (torch.rand(n, generator=g) < 0.6).float()
    mask[0] = 1.0
    return depth, gt, mask, scale


@pytest.mark.parametrize("n", [1, 257, 1024 * 256 + 5])
def test_depth_metrics(n):
    """focal_loss_bld's metrics: |gt - depth| / (interval * 192 / 128) over mask > 0.5 -> its mean and the
    fractions below 1 and below 3. No scaled error lies within 1e-3 of a threshold, so the fractions are
    exact counts and must equal the fp64 ones rounded to float; n = 1024 * 256 + 5 wraps the grid stride."""
    depth, gt, mask, scale = _metrics_inputs(n)
    got = ops.depth_metrics(depth.to(DEV), gt.to(DEV), mask.to(DEV), INTERVAL).cpu()
    sel = mask > 0.5
    x64 = (gt.double() - depth.double()).abs()[sel] / scale
    assert float((x64 - 1.0).abs().min()) > 1e-3 and float((x64 - 3.0).abs().min()) > 1e-3
    assert 0.5 < float(sel.float().mean()) < 0.7 or n == 1
    cnt = int(sel.sum())
    for i, thr in ((1, 1.0), (2, 3.0)):
        assert float(got[i]) == float(np.float32(int((x64 < thr).sum()) / cnt)), (i, float(got[i]))
    x32 = (gt - depth).abs()[sel] / (torch.tensor(INTERVAL) * 192. / 128.)
    _judge(f"depth_metrics n={n} epe", got[0], x32.mean(), x64.mean())


def test_depth_metrics_empty_mask():
    """The reference's mean over an empty selection is NaN, for all three outputs."""
    depth, gt, mask, _ = _metrics_inputs(257)
    got = ops.depth_metrics(depth.to(DEV), gt.to(DEV), torch.zeros_like(mask).to(DEV), INTERVAL)
    assert bool(torch.isnan(got).all()), got
