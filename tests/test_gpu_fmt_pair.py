"""The source views' self + cross layer pair as one launch (fmt_pair_kernel, csrc/fmt.hip), reached through
tmvs_fmt_forward and tmvs_fmt_forward_split (csrc/pipeline.hip): the whole FMT must be bit for bit the
composition of the per-layer entry points, which this change leaves as they were:

  ops.fmt_embed, then for j = 0 .. 3:
    ops.fmt_kv(all views, layer 2j, group_nv=nv)      ops.fmt_apply(all views, their own K/V, layer 2j)
    ops.fmt_kv(reference view, layer 2j+1)            ops.fmt_apply(source views, shared_kv=True, layer 2j+1)

with eight distinct encoder blocks drawn as the "fresh" weights of tests/test_gpu_fmt_layers.py (every
weight, bias, gain and shift random, a quarter of the gains negative), so a swapped layer, or a cross layer
fed a self layer's K/V, cannot pass. Both forms are compared: one stream (tmvs_fmt_forward) and the reference
view's chain on a side stream (tmvs_fmt_forward_split). The output sits between sentinel rows that must survive.

Token counts: 1, 15, 16, 17 (a lone partial tile, one tile - 1, one tile, one tile + 1: one 8-wave block of
the pair launch, most of whose waves own no tile), 259 (17 tiles, the last of 3 tokens: three 8-wave blocks, the
last with one tile and seven waves that own none), 528 (just over one 512-token K/V block), each with 2, 3
and 5 views; and, with 5 views, two lengths at which the pair launch
walks 2 and 3 tiles per wave -- both halves of its by-two loop, and the odd count that leaves it in the
middle. The pair kernel holds 2 blocks of 8 waves per CU (4 waves/SIMD: profiles/fmt_pair/resources.md), so a
GPU of C compute units has 16 C wave slots, and a launch over the 4 source views of T = ceil(L / 16) tiles
each walks ceil(4 T / 16 C) tiles per wave: k of them for (k - 1) 4 C < T <= 4 C k. _walk_len(k) takes
T >= (k - 1) 4 C + 40 on rows of 131 tokens; on an MI355X (C = 256) that is T >= 1064, L = 130 x 131 =
17,030 (1065 tiles) for k = 2, and T >= 2088, L = 255 x 131 = 33,405 (2088 tiles) for k = 3.
"""
import pytest
import torch

from oracle import transmvs_ref as oracle
from tests._primitives import DEV, _assert_guard, _bits, _gen, _guarded
from tests.test_gpu_fmt_layers import KD, _enc_weights, _pack
from transmvsnet_amd import ops

pytestmark = pytest.mark.gpu

PAIR_WAVES_PER_CU = 16  # fmt_pair_kernel: 2 resident blocks x 8 waves
ROW = 131


def _walk_len(k):
    """(h, w): the smallest h x 131 tokens at which 4 source views make the pair launch walk k tiles per wave"""
    slots = PAIR_WAVES_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (k - 1) * slots // 4 + 40
    h = -(-(16 * (tiles - 1) + 1) // ROW)
    t = -(-h * ROW // 16)
    assert (k - 1) * slots < 4 * t <= k * slots and h <= 600, (k, slots, h, t)
    return h, ROW


SMALL = [(1, 1), (3, 5), (4, 4), (1, 17), (7, 37), (16, 33)]  # 1, 15, 16, 17, 259, 528 tokens
CASES = [(nv, hw) for nv in (2, 3, 5) for hw in SMALL] + [(5, 2), (5, 3)]  # an int: _walk_len of it


def _case_id(c):
    nv, hw = c
    return f"nv{nv}-" + (f"{hw}tiles-per-wave" if isinstance(hw, int) else f"L{hw[0] * hw[1]}")


@pytest.fixture(scope="module")
def enc():
    blocks = [_pack(_enc_weights(None, "fresh", layer=i)) for i in range(8)]
    for a in range(8):
        for b in range(a):
            assert not torch.equal(blocks[a], blocks[b])
    return [b.to(DEV) for b in blocks]


def _composition(s1, pe, enc):
    """the FMT from the per-layer ops, in the order of pipeline.hip"""
    nv, _, h, w = s1.shape
    tokens = ops.fmt_embed(s1, pe, torch.empty(nv, h * w, KD, device=DEV))
    for j in range(4):
        i = 2 * j
        ops.fmt_apply(tokens, ops.fmt_kv(tokens, enc[i], group_nv=nv), enc[i])
        ops.fmt_apply(tokens[1:], ops.fmt_kv(tokens[:1], enc[i + 1]), enc[i + 1], shared_kv=True)
    torch.cuda.synchronize()
    return tokens


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_fmt_forward_is_the_layer_composition(enc, case):
    """ops.fmt_forward, on one stream and with a side stream, torch.equal to the per-layer composition."""
    nv, hw = case
    h, w = _walk_len(hw) if isinstance(hw, int) else hw
    s1 = torch.randn(nv, KD, h, w, generator=_gen(nv, h, w, 11)).to(DEV)
    pe = oracle._pe(KD)[0, :, :h, :w].contiguous().to(DEV)
    want = _composition(s1, pe, enc)
    assert bool(torch.isfinite(want).all())
    for side in (torch.cuda.Stream(torch.device(DEV)), None):
        tag = f"fmt {nv}x{h}x{w} {'two streams' if side is not None else 'one stream'}"
        obuf, out = _guarded((nv, h * w, KD), 1)
        got = ops.fmt_forward(s1, pe, enc, tokens=out, side_stream=side)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        _assert_guard(obuf, 1, nv, tag)
        assert torch.equal(got, want), f"{tag}: {int((_bits(got) != _bits(want)).sum())} token values differ from the composition"
