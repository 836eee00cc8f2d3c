"""The inference Feature Matching Transformer kernels (csrc/fmt.hip, orchestrated by csrc/pipeline.hip) and the
two pathway kernels (csrc/pathway.hip), kernel by kernel, at the tile and token tails the whole-network tests
never reach: token counts that are no multiple of the 16-token tile or of the 64-pixel embed block, every
tiling of the apply's two-tile loop (1 .. 5 tiles per wave: both early exits, the clamped prefetch of row
L - 1, waves that own no tile), the K/V reduction at 2, 4 and 8 tiles per wave with a ragged last block and
with more than 32 blocks (a second trip of the combine's strided loop), one K/V shared by every view
(stride 0), a positional-encoding table wider and taller than the map, view strides larger than a view,
coarse maps 1 pixel high or wide (the bilinear axis degenerates to i1 == i0), every height tail of the
16 x 32 stage-3 tile, more than one row of tiles, and grids that xcd_remap permutes.

  fmt_embed_kernel                       tmvs_fmt_embed
  fmt_kv_partial_kernel, fmt_kv_combine_kernel   tmvs_fmt_kv_grouped (2, 4, 8 tiles per wave; 1 .. 35 blocks)
  fmt_apply_kernel                       tmvs_fmt_apply_tiled (0 = occupancy-sized, 1 .. 5 tiles per wave)
  tmvs_fmt_forward, tmvs_fmt_forward_split   all of the above, 8 layers, one stream and two
  pathway16_mfma_kernel<32>              tmvs_fmt_pathway 32 -> 16 (stage 2)
  pathway_rows_kernel<16, 8, 2>          tmvs_fmt_pathway 16 -> 8 (stage 3)

Every reference is plain torch on the CPU, evaluated in fp32 and in fp64: the einsum of
oracle.linear_attention for the K/V summary, EncoderLayer.forward from the point where the summary is given
for the apply, oracle.fmt_ref / fmt_src on the golden state dict for the whole FMT, F.conv2d / F.interpolate
for the pathway. Error = max|got - ref64| / max|ref64|; the bar is err_gpu <= max(2 x err_fp32ref, 1e-5)
(tests/_primitives.py). The embedding is one fp32 addition and must be bit-exact; the apply's results must
also be bitwise the same for every tiling, and a view's K/V bitwise the same in a one-view and a two-view
launch. Outputs are contiguous slices of larger buffers whose other rows hold a sentinel that must survive
bit for bit; inputs are slices of buffers whose other rows (and, for strided views, the gaps between views)
are NaN, so a read outside the views poisons the output; the apply works in place, so its token buffer's
guard rows are NaN, must survive bit for bit, and the result must be finite. Weights are the golden state
dict's (non-trivial LayerNorm gains and biases) and, for every kernel, a set drawn fresh (every weight, bias,
gain and shift random, a quarter of the gains negative), so a swapped pair of features cannot hide behind a
symmetric weight.

Measured on an MI355X, worst (err_gpu, err_fp32ref) over all cases of a kernel: the embedding bit-exact, K/V
(2.3e-7, 1.3e-6), the apply (1.9e-7, 2.4e-7) with every tiling bitwise equal, the whole FMT on one stream and
on two (4.1e-7, 9.3e-7), the stage-2 pathway (5.2e-7, 4.7e-7), the stage-3 pathway (3.3e-7, 3.6e-7): the floor
is the bar everywhere. 67 tests, about 3 s.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import transmvs_ref as oracle
from tests._primitives import DEV, _assert_guard, _bits, _gen, _guarded, _judge
from tests._util import golden_state_dict
from transmvsnet_amd import _lib, ops

pytestmark = pytest.mark.gpu
DTS = (torch.float32, torch.float64)
NAN = float("nan")
KD = 32  # d_model
WEIGHTS = ["golden", "fresh"]


def _nan_guarded(t):
    """(buffer, view): `view` holds the CPU tensor `t` between one NaN row (one view's size) on either side"""
    buf = torch.full((t.shape[0] + 2, *t.shape[1:]), NAN, device=DEV)
    view = buf[1:1 + t.shape[0]]
    view.copy_(t)
    assert view.is_contiguous() and bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())
    return buf, view


def _nan_strided(t, pad):
    """(buffer, first view, view stride): the views of the CPU tensor `t` laid out with `pad` NaN floats after
    each, between one NaN row on either side"""
    n, per = t.shape[0], t[0].numel()
    buf = torch.full((n + 2, per + pad), NAN, device=DEV)
    buf[1:1 + n, :per].copy_(t.reshape(n, per))
    return buf, buf[1], per + pad


def _nan_rows_intact(buf):
    want = _bits(torch.full(tuple(buf.shape[1:]), NAN))
    return torch.equal(_bits(buf[0]), want) and torch.equal(_bits(buf[-1]), want)


def _cur_stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def sd():
    return golden_state_dict()


@pytest.fixture(scope="module")
def sd64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


# ------------------------------------------------------------------------------------- encoder-layer weights
_LINEARS = (("q", "attention.query_projection.", 32, 32), ("k", "attention.key_projection.", 32, 32),
            ("v", "attention.value_projection.", 32, 32), ("o", "attention.out_projection.", 32, 32),
            ("l1", "linear1.", 64, 32), ("l2", "linear2.", 32, 64))
_NORMS = (("n1", "norm1."), ("n2", "norm2."))


def _enc_weights(sd, kind, layer=0):
    """One EncoderLayer's 16 tensors (fp32, CPU) as {"q.w": [out][in], "q.b", ..., "n2.w", "n2.b"}: the golden
    state dict's layer `layer`, or every one drawn fresh: W = randn / sqrt(in), b = 0.5 randn, LayerNorm gain in
    [0.5, 1.5) with every fourth negated, LayerNorm shift = 0.5 randn"""
    w = {}
    if kind == "golden":
        p = f"FMT_with_pathway.FMT.layers.{layer}."
        for name, key, _, _ in _LINEARS:
            w[name + ".w"], w[name + ".b"] = sd[p + key + "weight"].float(), sd[p + key + "bias"].float()
        for name, key in _NORMS:
            w[name + ".w"], w[name + ".b"] = sd[p + key + "weight"].float(), sd[p + key + "bias"].float()
        assert not torch.equal(w["n1.w"], torch.ones(KD)) and bool((w["n2.b"] != 0).any())
        return w
    gen = _gen(97, layer)
    for name, _, n_out, n_in in _LINEARS:
        w[name + ".w"] = torch.randn(n_out, n_in, generator=gen) / math.sqrt(n_in)
        w[name + ".b"] = 0.5 * torch.randn(n_out, generator=gen)
    for name, _ in _NORMS:
        g = torch.rand(KD, generator=gen) + 0.5
        g[1::4] = -g[1::4]
        w[name + ".w"], w[name + ".b"] = g, 0.5 * torch.randn(KD, generator=gen)
    return w


def _pack(w):
    """The TMVS_ENC_* block of include/transmvs.h: the K, V projections and linear2 transposed"""
    parts = [w["q.w"], w["q.b"], w["k.w"].t(), w["k.b"], w["v.w"].t(), w["v.b"], w["o.w"], w["o.b"], w["l1.w"],
             w["l1.b"], w["l2.w"].t(), w["l2.b"], w["n1.w"], w["n1.b"], w["n2.w"], w["n2.b"]]
    flat = torch.cat([p.contiguous().reshape(-1) for p in parts])
    assert flat.numel() == _lib.ENC_NPARAMS
    return flat


def _lin(x, w, name, dt):
    return F.linear(x, w[name + ".w"].to(dt), w[name + ".b"].to(dt))


# ---------------------------------------------------------------------------------------------- 1. the embedding
EMBED_GEOS = [(1, 5, 7), (3, 9, 13), (2, 8, 8)]  # 35, 117 and 64 pixels: a partial block, 1 block + 53, one full


@pytest.mark.parametrize("table", ["exact", "larger"])
@pytest.mark.parametrize("geo", EMBED_GEOS, ids=lambda g: "x".join(map(str, g)))
def test_embed_bit_exact(geo, table):
    """tmvs_fmt_embed against feat + pe rearranged 'n c h w -> n (h w) c', bit for bit: token counts of 35, 64
    and 117, the positional-encoding table as the exact h x w slice and (h + 3) x (w + 5) (pe_w != width), the
    views dense (ops.fmt_embed) and 64 floats apart (NaN between them)."""
    nv, h, w = geo
    gen = _gen(nv, h, w)
    feat = torch.randn(nv, KD, h, w, generator=gen)
    ph, pw = (h, w) if table == "exact" else (h + 3, w + 5)
    pe = oracle._pe(KD)[0, :, :ph, :pw].contiguous()
    want = (feat + pe[:, :h, :w]).permute(0, 2, 3, 1).reshape(nv, h * w, KD)
    lib = _lib.load()
    for layout in ("dense", "strided"):
        tag = f"embed {nv}x{h}x{w} pe {ph}x{pw} {layout}"
        obuf, out = _guarded((nv, h * w, KD), 1)
        if layout == "dense":
            fbuf, fd = _nan_guarded(feat)
            ops.fmt_embed(fd, pe.to(DEV), out)
        else:
            fbuf, fd, stride = _nan_strided(feat, 64)
            assert stride == KD * h * w + 64
            ped = pe.to(DEV)
            _lib.check(lib.tmvs_fmt_embed(fd.data_ptr(), stride, ped.data_ptr(), ph, pw, nv, KD, h, w, out.data_ptr(),
                                          _cur_stream()), "tmvs_fmt_embed")
        _assert_guard(obuf, 1, nv, tag)
        assert torch.equal(_bits(out), _bits(want)), tag + ": tokens are not feat + pe bit for bit"


# -------------------------------------------------------------------------------------------- 2. the K/V summary
def _kv_ref(dt, src, w):
    """[nv][160]: KV[h][m][d] = sum_s K[s,h,d] V[s,h,m] (the einsum of oracle.linear_attention), then Ksum[h][d]"""
    n, s, _ = src.shape
    k = _lin(src.to(dt), w, "k", dt).view(n, s, 8, 4)
    v = _lin(src.to(dt), w, "v", dt).view(n, s, 8, 4)
    kf = F.elu(k) + 1
    kv = torch.einsum("nshd,nshm->nhmd", kf, v)
    return torch.cat([kv.reshape(n, 128), kf.sum(dim=1).reshape(n, 32)], dim=1)


# (source tokens S, group_nv, blocks per view): tiles per wave 2, 2, 2, 2 | 2, 4, 8 | 2. At S = 1961 (123 tiles,
# the last of 9 tokens) the last block has a wave with a partial tile at every tiling, waves that own no tile at
# 2 and 4 tiles per wave; 35 blocks: the combine's groups 0 .. 2 sum two slabs
KV_CASES = [(1, 2, 1), (9, 2, 1), (16, 2, 1), (17, 2, 1), (1961, 1, 16), (1961, 70, 8), (1961, 128, 4), (4355, 1, 35)]


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("s,group_nv,nblk", KV_CASES, ids=[f"S{c[0]}-g{c[1]}" for c in KV_CASES])
def test_kv_tilings(sd, s, group_nv, nblk, weights):
    """tmvs_fmt_kv_grouped on two views against the fp64 / fp32 einsum; the workspace size proves the block
    count, hence the tiles per wave, the case is meant to reach; each view's K/V is bitwise that of a one-view
    launch with the same group_nv."""
    nv = 2
    w = _enc_weights(sd, weights, layer=1)
    src = torch.randn(nv, s, KD, generator=_gen(s, group_nv, len(weights)))
    r32, r64 = (_kv_ref(dt, src, w) for dt in DTS)
    lib = _lib.load()
    assert lib.tmvs_fmt_kv_grouped_workspace(nv, group_nv, s) == nv * nblk * _lib.KV_NFLOATS * 4
    tag = f"kv S={s} group_nv={group_nv} ({nblk} blocks) {weights}"
    enc = _pack(w).to(DEV)
    sbuf, sdv = _nan_guarded(src)
    obuf, out = _guarded((nv, _lib.KV_NFLOATS), 1)
    got = ops.fmt_kv(sdv, enc, out=out, group_nv=group_nv)
    assert got.data_ptr() == out.data_ptr()
    _assert_guard(obuf, 1, nv, tag)
    assert torch.equal(_bits(sdv), _bits(src)) and _nan_rows_intact(sbuf), tag + ": the source was written"
    _judge(tag, got, r32, r64)
    for v in range(nv):  # each view, and its Ksum, on their own scale
        _judge(f"{tag} [view {v}]", got[v], r32[v], r64[v])
        _judge(f"{tag} [view {v} Ksum]", got[v, 128:], r32[v, 128:], r64[v, 128:])
        alone = ops.fmt_kv(sdv[v:v + 1], enc, group_nv=group_nv)
        assert torch.equal(_bits(alone[0]), _bits(got[v])), f"{tag}: view {v} alone differs from the two-view launch"


# ------------------------------------------------------------------------------------------------- 3. the apply
def _apply_ref(dt, x, kv, w):
    """EncoderLayer.forward (oracle.encoder_layer) from the point where the fp32 (KV, Ksum) summary `kv`
    [nv or 1][160] is given"""
    n, l, _ = x.shape
    kv = kv.to(dt).expand(n, -1)
    big, ksum = kv[:, :128].reshape(n, 8, 4, 4), kv[:, 128:].reshape(n, 8, 4)
    qf = F.elu(_lin(x.to(dt), w, "q", dt).view(n, l, 8, 4)) + 1
    z = 1 / (torch.einsum("nlhd,nhd->nlh", qf, ksum) + oracle.ATTN_EPS)
    msg = torch.einsum("nlhd,nhmd,nlh->nlhm", qf, big, z).reshape(n, l, KD)
    y = F.layer_norm(x.to(dt) + _lin(msg, w, "o", dt), (KD,), w["n1.w"].to(dt), w["n1.b"].to(dt), oracle.LN_EPS)
    f = _lin(F.relu(_lin(y, w, "l1", dt)), w, "l2", dt)
    return F.layer_norm(y + f, (KD,), w["n2.w"].to(dt), w["n2.b"].to(dt), oracle.LN_EPS)


# (query tokens L, views, one shared K/V, tiles per wave to launch). L = 1961 is 123 tiles, the last of 9 tokens:
# at 2 tiles per wave the last block's second wave runs one partial tile and leaves the pair early, its third and
# fourth own nothing; 3 and 5 leave through `it + NT >= tpw`; 1 never enters the second half; 0 is the
# occupancy-sized default. The short ones fit one block, whose waves mostly own no tile.
APPLY_CASES = [(1961, 2, False, (0, 1, 2, 3, 4, 5)), (1, 2, False, (1, 2, 3)), (9, 2, False, (1, 2, 3)),
               (16, 2, False, (1, 2, 3)), (17, 2, False, (1, 2, 3)), (33, 2, False, (1, 2, 3)),
               (1961, 3, True, (0, 2, 3)), (33, 3, True, (1, 2, 3))]


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("l,nv,shared,tilings", APPLY_CASES,
                         ids=[f"L{c[0]}-nv{c[1]}{'-shared' if c[2] else ''}" for c in APPLY_CASES])
def test_apply_tilings(sd, l, nv, shared, tilings, weights):
    """tmvs_fmt_apply_tiled, in place, at every tiling of the case: each result under the bar, finite, the NaN
    rows around the tokens intact, and all of them bitwise equal to each other (the arithmetic is per token)."""
    w = _enc_weights(sd, weights, layer=3 if shared else 2)
    gen = _gen(l, nv, int(shared), len(weights))
    x = torch.randn(nv, l, KD, generator=gen)
    src = torch.randn(1 if shared else nv, 77, KD, generator=gen)
    kv = _kv_ref(torch.float64, src, w).float()  # the fp32 summary the kernel and both references receive
    r32, r64 = (_apply_ref(dt, x, kv, w) for dt in DTS)
    enc = _pack(w).to(DEV)
    kbuf, kd = _nan_guarded(kv)
    first = None
    for tpw in tilings:
        tag = f"apply L={l} nv={nv}{' shared kv' if shared else ''} tiles/wave={tpw} {weights}"
        tbuf, td = _nan_guarded(x)
        got = ops.fmt_apply(td, kd, enc, shared_kv=shared, tiles_per_wave=tpw)
        assert got.data_ptr() == td.data_ptr()
        assert _nan_rows_intact(tbuf), tag + ": rows around the tokens were written"
        assert bool(torch.isfinite(got).all()), tag + ": non-finite tokens"
        _judge(tag, got, r32, r64)
        _judge(tag + " [last view]", got[-1], r32[-1], r64[-1])
        _judge(tag + " [last token]", got[:, -1], r32[:, -1], r64[:, -1])
        if first is None:
            first = _bits(got)
        else:
            assert torch.equal(_bits(got), first), f"{tag}: differs from tiles/wave={tilings[0]}"
    assert torch.equal(_bits(kd), _bits(kv)) and _nan_rows_intact(kbuf), "the K/V summary was written"


# ----------------------------------------------------------------------------------------------- 4. the whole FMT
FMT_GEOS = [(1, 5, 7), (2, 9, 13), (3, 37, 53)]


@pytest.mark.parametrize("geo", FMT_GEOS, ids=lambda g: "x".join(map(str, g)))
def test_fmt_forward_vs_oracle(sd, sd64, geo):
    """tmvs_fmt_forward, and tmvs_fmt_forward_split for two views or more, against oracle.fmt_ref / fmt_src in
    fp64 and fp32 on the golden state dict, both sides reading the same fp32 positional-encoding table."""
    nv, h, w = geo
    s1 = torch.randn(nv, KD, h, w, generator=_gen(nv, h, w, 8))
    refs = []
    with torch.no_grad():
        for dt, d in ((torch.float32, sd), (torch.float64, sd64)):
            outs = oracle.fmt_ref(d, s1[:1].to(dt))
            views = [outs[-1]] + [oracle.fmt_src(d, outs, s1[v:v + 1].to(dt)) for v in range(1, nv)]
            refs.append(torch.cat(views).permute(0, 2, 3, 1).reshape(nv, h * w, KD))
    r32, r64 = refs
    assert r32.dtype == torch.float32 and r64.dtype == torch.float64
    pe = oracle._pe(KD)[0, :, :h, :w].contiguous().to(DEV)
    enc = [_pack(_enc_weights(sd, "golden", layer=i)).to(DEV) for i in range(8)]
    sbuf, sdv = _nan_guarded(s1)
    streams = [None] + ([torch.cuda.Stream(torch.device(DEV))] if nv >= 2 else [])
    for side in streams:
        tag = f"fmt {nv}x{h}x{w} {'two streams' if side is not None else 'one stream'}"
        obuf, out = _guarded((nv, h * w, KD), 1)
        got = ops.fmt_forward(sdv, pe, enc, tokens=out, side_stream=side)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        _assert_guard(obuf, 1, nv, tag)
        _judge(tag, got, r32, r64)
        for v in range(nv):
            _judge(f"{tag} [view {v}]", got[v], r32[v], r64[v])
    assert torch.equal(_bits(sdv), _bits(s1)) and _nan_rows_intact(sbuf), "the stage-1 features were written"


# ------------------------------------------------------------------------------------------------- 5. the pathway
# stage -> (cc, cf, reduce key, smooth key, output tile (TH, TW))
STAGES = {2: (32, 16, "dim_reduction_1", "smooth_1", (16, 16)), 3: (16, 8, "dim_reduction_2", "smooth_2", (32, 16))}
# (stage, (nv, coarse h, w), lateral views 48 floats apart). Stage 3: 2h % 32 = 2, 6, 16, 18, 30, 0, then two
# rows of tiles. The last case of each stage has 12 / 10 tiles, which xcd_remap deals out in another order.
PATHWAY_CASES = [(2, (1, 1, 1), False), (2, (1, 1, 9), False), (2, (2, 5, 1), True), (2, (2, 9, 13), False),
                 (2, (3, 8, 8), False), (2, (1, 9, 41), False),
                 (3, (1, 1, 1), False), (3, (2, 3, 5), False), (3, (2, 8, 9), True), (3, (1, 9, 13), False),
                 (3, (2, 15, 4), False), (3, (3, 16, 8), False), (3, (1, 17, 36), False)]


def _pathway_ref(dt, coarse, lat, w_red, w_sm):
    h, w = coarse.shape[2:]
    up = F.interpolate(F.conv2d(coarse.to(dt), w_red.to(dt)), size=(2 * h, 2 * w), mode="bilinear")
    return F.conv2d(up + lat.to(dt), w_sm.to(dt), padding=1).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("stage,geo,strided", PATHWAY_CASES,
                         ids=[f"stage{c[0]}-{'x'.join(map(str, c[1]))}{'-strided' if c[2] else ''}" for c in PATHWAY_CASES])
def test_pathway_tails(sd, stage, geo, strided, weights):
    """tmvs_fmt_pathway against smooth(bilinear(reduce(coarse)) + lateral) in fp64 and fp32."""
    cc, cf, red_key, sm_key, (th, tw) = STAGES[stage]
    nv, h, w = geo
    gen = _gen(stage, nv, h, w, len(weights))
    coarse = torch.randn(nv, cc, h, w, generator=gen)
    lat = torch.randn(nv, cf, 2 * h, 2 * w, generator=gen)
    if weights == "golden":
        w_red = sd[f"FMT_with_pathway.{red_key}.weight"].float()
        w_sm = sd[f"FMT_with_pathway.{sm_key}.weight"].float()
    else:
        w_red = torch.randn(cf, cc, 1, 1, generator=gen) / math.sqrt(cc)
        w_sm = torch.randn(cf, cf, 3, 3, generator=gen) / math.sqrt(9 * cf)
    assert tuple(w_red.shape) == (cf, cc, 1, 1) and tuple(w_sm.shape) == (cf, cf, 3, 3)
    r32, r64 = (_pathway_ref(dt, coarse, lat, w_red, w_sm) for dt in DTS)
    tiles = nv * -(-2 * h // th) * -(-2 * w // tw)
    tag = f"pathway stage {stage} {cc}->{cf} {nv}x{h}x{w} ({tiles} tiles){' strided' if strided else ''} {weights}"
    red = w_red.reshape(cf, cc).t().contiguous().to(DEV)       # [cc][cf]
    sm = w_sm.permute(1, 2, 3, 0).contiguous().to(DEV)         # [cf_in][3][3][cf_out]
    cbuf, cd = _nan_guarded(coarse.permute(0, 2, 3, 1).contiguous())
    obuf, out = _guarded((nv, 2 * h, 2 * w, cf), 1)
    if strided:
        lbuf, ld, stride = _nan_strided(lat, 48)
        _lib.check(_lib.load().tmvs_fmt_pathway(cd.data_ptr(), ld.data_ptr(), stride, red.data_ptr(), sm.data_ptr(), nv,
                                                cc, cf, h, w, out.data_ptr(), _cur_stream()), "tmvs_fmt_pathway")
        got = out
    else:
        lbuf, ld = _nan_guarded(lat)
        got = ops.fmt_pathway(cd, ld, red, sm, out=out)
        assert got.data_ptr() == out.data_ptr()
    _assert_guard(obuf, 1, nv, tag)
    assert _nan_rows_intact(cbuf) and torch.equal(_bits(cd), _bits(coarse.permute(0, 2, 3, 1))), tag + ": coarse written"
    _judge(tag, got, r32, r64)
    if nv > 1:
        _judge(tag + " [last view]", got[-1], r32[-1], r64[-1])
