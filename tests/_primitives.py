"""Helpers shared by the direct kernel tests (test_gpu_train_primitives.py, test_gpu_train_conv_bn.py):
the error measure, the one bar, seeded generators and sentinel-guarded output buffers."""
import torch

DEV = "cuda"
FLOOR = 1e-5
SENTINEL = -12345.678


def _rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) % (2 ** 31))


def _bar(e_ref, floor=FLOOR):
    """the one bar of this file, from the fp32 reference's own error"""
    return max(2.0 * e_ref, floor)


def _hold(name, e_gpu, e_ref, floor=FLOOR):
    """print (err_gpu, err_fp32ref) and hold err_gpu to the bar"""
    print(f"{name}: (err_gpu, err_fp32ref) = ({e_gpu:.2e}, {e_ref:.2e})")
    assert e_gpu <= _bar(e_ref, floor), (name, e_gpu, e_ref)


def _judge(name, got, r32, r64, floor=FLOOR):
    assert tuple(got.shape) == tuple(r64.shape), (name, tuple(got.shape), tuple(r64.shape))
    _hold(name, _rel(got, r64), _rel(r32, r64), floor)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _guarded(rows, lead, fill=None):
    """(buffer, view): `view` is rows [lead, lead + n) of a sentinel-filled buffer with `lead` spare rows
    on either side; `fill` (CPU, the view's shape) initialises the view."""
    n = rows[0]
    buf = torch.full((n + 2 * lead, *rows[1:]), SENTINEL, device=DEV)
    view = buf[lead:lead + n]
    assert view.is_contiguous()
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _assert_guard(buf, lead, n, name):
    want = torch.full((lead, *buf.shape[1:]), SENTINEL)
    assert torch.equal(_bits(buf[:lead]), _bits(want)), f"{name}: rows before the output were written"
    assert torch.equal(_bits(buf[lead + n:]), _bits(want)), f"{name}: rows after the output were written"
