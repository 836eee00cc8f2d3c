"""Torch-tensor wrappers over the C-ABI (device memory + current HIP stream in, status checked).

Each op mirrors one reference callable (file:line in include/transmvs.h). Tensors must be
fp32, contiguous and on the GPU; nothing here computes on the CPU except the 4x4 camera
algebra that produces kernel arguments (proj_rows), which is done exactly as the
reference does it so the warp coordinates match bit for bit.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from . import _lib

_lib_h = _lib.load


_TIMER = None


def set_timer(timer):
    """Install an object with begin(name) -> token / end(token) around every C-ABI launch
    (bench.py uses HIP events on the launching stream); None disables."""
    global _TIMER
    _TIMER = timer


def _call(name, *args, span=None):
    """One C-ABI call, status checked: tensors go as their data_ptr(), None as NULL and the rest as ctypes
    converts it by the entry's argtypes (_lib.SIGNATURES). The timer span (`span`, else the entry's name)
    brackets the library call alone."""
    fn = getattr(_lib_h(), name)
    args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    tok = _TIMER.begin(span or name) if _TIMER is not None else None
    try:
        _lib.check(fn(*args), name)
    finally:
        if tok is not None:
            _TIMER.end(tok)


def _launch(name, *args, span=None):
    """_call with the current stream as the entry's last argument."""
    _call(name, *args, _stream(), span=span)


def _workspace(query, *dims, device):
    """(scratch tensor, its size in bytes) for one launch, from the entry's size query `query`(*dims)."""
    ws = torch.empty(getattr(_lib_h(), query)(*dims) // 4 + 64, device=device)
    return ws, ws.numel() * 4


def _stream():
    """The current HIP stream of the current device. Every public op below runs under a device guard
    set from its first GPU tensor argument (_on_tensor_device), so this is that tensor's device."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on_tensor_device(fn):
    """Run `fn` with the current device = the device of its first GPU tensor argument, so its kernels
    launch on that device and on that device's current stream (a model on cuda:1 works without
    torch.cuda.set_device(1))."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        for a in (*args, *kwargs.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if a.device.index == torch.cuda.current_device():
                    return fn(*args, **kwargs)
                with torch.cuda.device(a.device):
                    return fn(*args, **kwargs)
        return fn(*args, **kwargs)
    wrapped.device_guarded = True
    return wrapped


def _dev(t, name):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous float32")


# ----------------------------------------------------------------- host-side parameter math
def bn_fold(gamma, beta, mean, var, eps=1e-5):
    """(alpha, shift) CPU float32 arrays, reference batch_norm eval semantics (tmvs_bn_fold)."""
    g = np.ascontiguousarray(gamma.detach().cpu().numpy(), np.float32)
    b = np.ascontiguousarray(beta.detach().cpu().numpy(), np.float32)
    m = np.ascontiguousarray(mean.detach().cpu().numpy(), np.float32)
    v = np.ascontiguousarray(var.detach().cpu().numpy(), np.float32)
    a = np.empty_like(g)
    s = np.empty_like(g)
    _call("tmvs_bn_fold", g.ctypes.data, b.ctypes.data, m.ctypes.data, v.ctypes.data, g.size, eps, a.ctypes.data,
          s.ctypes.data)
    return a, s


def compose_proj(proj):
    """[B,2,4,4] -> [B,4,4] with rows 0..2 = K·E[:3,:4] (models/TransMVSNet.py:75-78), CPU fp32."""
    new = proj[:, 0].clone()
    new[:, :3, :4] = torch.matmul(proj[:, 1, :3, :3], proj[:, 0, :3, :4])
    return new


def proj_rows(proj_matrix_stage):
    """[B,N,2,4,4] -> float32 [B, N-1, 12] = rows of P_src·P_ref^-1 (models/module.py:295-297).

    Same torch-CPU fp32 ops as the reference, so the homography is bit-identical.
    """
    pm = proj_matrix_stage.detach().to("cpu", torch.float32)
    ref = compose_proj(pm[:, 0])
    inv = torch.inverse(ref)
    rows = []
    for v in range(1, pm.shape[1]):
        p = torch.matmul(compose_proj(pm[:, v]), inv)
        rows.append(p[:, :3, :4].reshape(pm.shape[0], 12))
    return torch.stack(rows, 1).contiguous().numpy()


_ROT_ORDER = {}


def host_rot_order(n_pixels):
    """'fma' or 'plain': how THIS host's torch.matmul rounds homo_warping's rot·(x, y, 1)
    (models/module.py:303, a [3,3] x [3,H*W] bmm). The reference's sample coordinates depend on it:
    MKL contracts the 3-term dot into fmaf(r1, y, r0·x) + r2 on AVX-512 Xeons and computes
    (r0·x + r1·y) + r2 on AMD EPYC (scripts/diag/warp_bits.py). Probed once per size with the
    reference's own call shape; the warp kernels then reproduce the host's coordinates bit for bit."""
    order = _ROT_ORDER.get(n_pixels)
    if order is None:
        g = np.random.default_rng(12345)
        w = 1 << max(1, int(np.ceil(np.log2(max(2.0, np.sqrt(n_pixels))))))
        xs = (np.arange(n_pixels) % w).astype(np.float32)
        ys = (np.arange(n_pixels) // w).astype(np.float32)
        rot = g.uniform(-1.0, 1.0, (3, 3)).astype(np.float32)
        rot[:, 2] *= 300.0
        xyz = torch.from_numpy(np.stack([xs, ys, np.ones_like(xs)]))[None]
        got = torch.matmul(torch.from_numpy(rot)[None], xyz)[0].numpy()
        r0, r1, r2 = rot[:, 0:1], rot[:, 1:2], rot[:, 2:3]
        fma = (r1.astype(np.float64) * ys + (r0 * xs)).astype(np.float32) + r2
        plain = (r0 * xs + r1 * ys) + r2
        order = "plain" if (plain == got).sum() > (fma == got).sum() else "fma"
        _ROT_ORDER[n_pixels] = order
    return order


def warp_flags(rot_order, n_pixels):
    """TMVS_WARP_ROT_PLAIN or 0 for rot_order 'fma' / 'plain' / 'auto' (= host_rot_order)."""
    if rot_order == "auto":
        rot_order = host_rot_order(n_pixels)
    if rot_order not in ("fma", "plain"):
        raise ValueError(f"rot_order must be 'auto', 'fma' or 'plain', got {rot_order!r}")
    return _lib.WARP_ROT_PLAIN if rot_order == "plain" else 0


# ----------------------------------------------------------------- ops
@_on_tensor_device
def stage_hypotheses(depth_values, prev_depth, ndepth, ratio, full_hw, stage_scale):
    """Stage glue (models/TransMVSNet.py:174-204): -> [B, D, H/s, W/s]."""
    _dev(depth_values, "depth_values")
    _dev(prev_depth, "prev_depth")
    b = depth_values.shape[0]
    h, w = full_hw
    out = torch.empty(b, ndepth, h // stage_scale, w // stage_scale, device=depth_values.device)
    ph, pw = (prev_depth.shape[1], prev_depth.shape[2]) if prev_depth is not None else (0, 0)
    _launch("tmvs_stage_hypotheses", depth_values, depth_values.shape[1], prev_depth, ph, pw, b, ndepth, ratio, h, w,
            stage_scale, out)
    return out


@_on_tensor_device
def warp_corr(ref_nhwc, src_nhwc, proj12, hyp, view_w_in=None, vw_shift=0, vw_offset=0, vw_total=None,
              pw_params=None, partial=False, view_w_out=None, sim_out=None, wsum_out=None, rot_order="auto"):
    """Fused cost volume (models/TransMVSNet.py:58-93). ref [B,H,W,C], src [B,V,H,W,C], proj12 HOST [B,V,12].

    Returns sim [B,D,H,W] (and w_sum [B,H,W] when partial) ; stage 1 writes view_w_out [B,vw_total,H,W].
    rot_order: the reference's rounding of rot·(x, y, 1) ('auto' = this host's torch, host_rot_order).
    """
    for t, n in ((ref_nhwc, "ref"), (src_nhwc, "src"), (hyp, "hyp"), (view_w_in, "view_w_in"), (view_w_out, "view_w_out")):
        _dev(t, n)
    b, v, h, w, c = src_nhwc.shape
    d = hyp.shape[1]
    vw_total = v if vw_total is None else vw_total
    proj = np.ascontiguousarray(proj12, np.float32).reshape(b, v, 12)
    sim = torch.empty(b, d, h, w, device=hyp.device) if sim_out is None else sim_out
    wsum = (torch.empty(b, h, w, device=hyp.device) if wsum_out is None else wsum_out) if partial else None
    if sim.shape != (b, d, h, w) or not sim.is_contiguous():
        raise ValueError(f"sim_out must be a contiguous [{b},{d},{h},{w}] tensor")
    if wsum is not None and (wsum.numel() != b * h * w or not wsum.is_contiguous()):
        raise ValueError(f"wsum_out must be a contiguous [{b},{h},{w}] tensor")
    if view_w_in is None:
        if view_w_out is None:
            view_w_out = torch.empty(b, vw_total, h, w, device=hyp.device)
        pw = np.ascontiguousarray(pw_params, np.float32)
        assert pw.size == _lib.PW_NPARAMS
        pw_ptr = pw.ctypes.data
    else:
        pw_ptr = None
    _launch("tmvs_warp_corr", ref_nhwc, src_nhwc, proj.ctypes.data, hyp, view_w_in, vw_shift, vw_offset, vw_total,
            pw_ptr, b, v, c, d, h, w, (_lib.WARP_PARTIAL if partial else 0) | warp_flags(rot_order, h * w), sim, wsum,
            view_w_out if view_w_in is None else None)
    return sim, wsum, (view_w_out if view_w_in is None else None)


@_on_tensor_device
def aggregate_finalize(sim_sum, w_sum):
    _dev(sim_sum, "sim_sum")
    _dev(w_sum, "w_sum")
    b, d, h, w = sim_sum.shape
    _launch("tmvs_aggregate_finalize", sim_sum, w_sum, b, d, h, w)
    return sim_sum


@_on_tensor_device
def homo_warping(src_fea, src_proj, ref_proj, depth_values, rot_order="auto"):
    """Seam-compatible homo_warping (models/module.py:284-322): [B,C,H,W] -> [B,C,D,H,W]."""
    _dev(src_fea, "src_fea")
    _dev(depth_values, "depth_values")
    b, c, h, w = src_fea.shape
    d = depth_values.shape[1]
    p = torch.matmul(src_proj.detach().cpu().float(), torch.inverse(ref_proj.detach().cpu().float()))
    rows = np.ascontiguousarray(p[:, :3, :4].reshape(b, 12).numpy(), np.float32)
    out = torch.empty(b, c, d, h, w, device=src_fea.device)
    _launch("tmvs_homo_warping", src_fea, rows.ctypes.data, depth_values.contiguous(), b, c, d, h, w,
            warp_flags(rot_order, h * w), out)
    return out


@_on_tensor_device
def softmax_wta(logits, hyp, clamp=(425.0, 935.0)):
    """prob, depth (clamped), depth_raw, conf (models/TransMVSNet.py:97-103,217-221)."""
    _dev(logits, "logits")
    _dev(hyp, "hyp")
    b, d, h, w = logits.shape
    prob = torch.empty_like(logits)
    depth = torch.empty(b, h, w, device=logits.device)
    raw = torch.empty_like(depth)
    conf = torch.empty_like(depth)
    _launch("tmvs_softmax_wta", logits, hyp, b, d, h, w, clamp[0], clamp[1], prob, depth, raw, conf)
    return prob, depth, raw, conf


@_on_tensor_device
def costregnet(x, weights: "_lib.CostRegWeights", keepalive=None):
    """CostRegNet forward (models/module.py:447-456): [B,D,H,W] -> logits [B,D,H,W]."""
    _dev(x, "x")
    b, d, h, w = x.shape
    out = torch.empty_like(x)
    _launch("tmvs_costregnet", x, b, d, h, w, ctypes.byref(weights),
            *_workspace("tmvs_costregnet_workspace", b, d, h, w, weights.base_ch, device=x.device), out)
    return out


@_on_tensor_device
def costregnet_wta(x, weights: "_lib.CostRegWeights", hyp, clamp=(425.0, 935.0)):
    """CostRegNet -> softmax/WTA (models/module.py:447-456, TransMVSNet.py:97-103,214-221) in one
    call: prob, depth (clamped), depth_raw, conf, equal bit for bit to costregnet -> softmax_wta."""
    _dev(x, "x")
    _dev(hyp, "hyp")
    b, d, h, w = x.shape
    if tuple(hyp.shape) != (b, d, h, w):
        raise ValueError(f"costregnet_wta: hyp shape {tuple(hyp.shape)} != volume shape {(b, d, h, w)}")
    prob = torch.empty_like(x)
    depth = torch.empty(b, h, w, device=x.device)
    raw = torch.empty_like(depth)
    conf = torch.empty_like(depth)
    # costregnet's span: bench.py groups by it
    _launch("tmvs_costregnet_wta", x, hyp, b, d, h, w, ctypes.byref(weights),
            *_workspace("tmvs_costregnet_workspace", b, d, h, w, weights.base_ch, device=x.device), clamp[0], clamp[1],
            prob, depth, raw, conf, span="tmvs_costregnet")
    return prob, depth, raw, conf


def _layer_args(op, x, wpk, alpha, shift, cout):
    """What the single-layer entry points cannot see and would read past: every tensor contiguous fp32 on
    x's device, 27 * cout * cin packed weights, cout floats of alpha / shift (None: the raw epilogue)."""
    if x.dim() != 5:
        raise ValueError(f"{op}: x must be NDHWC [B, D, H, W, cin]")
    for name, t in (("x", x), ("wpk", wpk), ("alpha", alpha), ("shift", shift)):
        _layer_tensor(op, name, t, x.device)
    cin = x.shape[4]
    if wpk.numel() != 27 * cout * cin:
        raise ValueError(f"{op}: wpk must hold 27 * cout * cin = {27 * cout * cin} floats, not {wpk.numel()}")
    for name, t in (("alpha", alpha), ("shift", shift)):
        if t is not None and t.numel() < cout:
            raise ValueError(f"{op}: {name} must hold cout = {cout} floats, not {t.numel()}")


def _layer_tensor(op, name, t, device):
    if t is None:
        return
    if not t.is_cuda or t.device != device:
        raise ValueError(f"{op}: {name} must be a GPU tensor on x's device (the HIP path has no CPU fallback)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{op}: {name} must be contiguous float32")


def _layer_like(op, name, t, shape, device):
    """`t` (skip or out, may be None) is a contiguous fp32 device tensor of `shape`"""
    _layer_tensor(op, name, t, device)
    if t is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{op}: {name} must be a contiguous {list(shape)} tensor, not {list(t.shape)}")


def _layer_no_alias(op, skip, out):
    if skip is not None and out is not None and skip.data_ptr() == out.data_ptr():
        raise ValueError(f"{op}: out must not alias skip (the kernels read skip while they write out)")


def _conv_out_dhw(d, h, w, stride):
    return (d, h, w) if stride == 1 else ((d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1)


@_on_tensor_device
def conv3d_bn_relu(x, wpk, alpha, shift, cout, stride, out=None):
    """tmvs_conv3d_bn_relu: x NDHWC, wpk [27][cout][cin] -> relu(conv * alpha + shift), written to `out` when given."""
    _layer_args("conv3d_bn_relu", x, wpk, alpha, shift, cout)
    b, d, h, w, cin = x.shape
    shape = (b, *_conv_out_dhw(d, h, w, stride), cout)
    _layer_like("conv3d_bn_relu", "out", out, shape, x.device)
    y = torch.empty(shape, device=x.device) if out is None else out
    _launch("tmvs_conv3d_bn_relu", x, b, cin, d, h, w, wpk, alpha, shift, cout, stride, y)
    return y


@_on_tensor_device
def deconv3d_bn_relu_add(x, wpk, alpha, shift, cout, skip, out=None, route=None, max_workgroups=0):
    """tmvs_deconv3d_bn_relu_add: skip + relu(conv_transpose * alpha + shift) at twice x's extents, written to
    `out` (not skip itself) when given. route "generic" / "persistent" pins the kernel
    (tmvs_deconv3d_bn_relu_add_generic / _persistent, the latter with its grid bound max_workgroups)."""
    _layer_args("deconv3d_bn_relu_add", x, wpk, alpha, shift, cout)
    b, d, h, w, cin = x.shape
    shape = (b, 2 * d, 2 * h, 2 * w, cout)
    if skip is None:
        raise ValueError("deconv3d_bn_relu_add: skip is required")
    _layer_like("deconv3d_bn_relu_add", "skip", skip, shape, x.device)
    _layer_like("deconv3d_bn_relu_add", "out", out, shape, x.device)
    _layer_no_alias("deconv3d_bn_relu_add", skip, out)
    y = torch.empty(shape, device=x.device) if out is None else out
    if route not in (None, "generic", "persistent"):
        raise ValueError(f"deconv3d_bn_relu_add: unknown route {route!r}")
    bound = (int(max_workgroups),) if route == "persistent" else ()
    _launch("tmvs_deconv3d_bn_relu_add" + ("_" + route if route else ""), x, b, cin, d, h, w, wpk, alpha, shift, cout,
            skip, y, *bound)
    return y


@_on_tensor_device
def fmt_embed(feat_nchw, pe, out_tokens):
    """x + PE, 'n c h w -> n (h w) c' (FMT.py:152): feat [nv,C,H,W] -> tokens [nv,H*W,C] (written in place)."""
    nv, c, h, w = feat_nchw.shape
    _launch("tmvs_fmt_embed", feat_nchw, c * h * w, pe, pe.shape[1], pe.shape[2], nv, c, h, w, out_tokens)
    return out_tokens


@_on_tensor_device
def fmt_kv(source_tokens, enc_w, out=None, group_nv=None):
    """(KV, Ksum) of one encoder layer over source tokens [nv,S,32] -> [nv,160].

    group_nv: the partial sums are grouped as in a launch over group_nv views (tmvs_fmt_kv_grouped), so a
    view's K/V is bitwise the same in any subset of those views; None = nv."""
    nv, s, _ = source_tokens.shape
    group_nv = nv if group_nv is None else int(group_nv)
    nbytes = _lib_h().tmvs_fmt_kv_grouped_workspace(nv, group_nv, s)
    ws = torch.empty(max(1, nbytes // 4), device=source_tokens.device)  # exactly the bytes asked for
    kv = out if out is not None else torch.empty(nv, _lib.KV_NFLOATS, device=source_tokens.device)
    # the ungrouped entry's span: bench.py groups by it
    _launch("tmvs_fmt_kv_grouped", source_tokens, nv, group_nv, s, enc_w, ws, ws.numel() * 4, kv, span="tmvs_fmt_kv")
    return kv


@_on_tensor_device
def fmt_apply(x_tokens, kv, enc_w, shared_kv=False, tiles_per_wave=0):
    """Rest of EncoderLayer.forward in place on x [nv,L,32] (FMT.py:96-111).

    tiles_per_wave > 0 fixes the 16-token tiles each wave walks (tmvs_fmt_apply_tiled; the result is bitwise
    the same for every tiling); 0 sizes it from the kernel's occupancy."""
    nv, l, _ = x_tokens.shape
    # the untiled entry's span: bench.py groups by it
    _launch("tmvs_fmt_apply_tiled", x_tokens, nv, l, kv, 0 if shared_kv else _lib.KV_NFLOATS, enc_w,
            int(tiles_per_wave), span="tmvs_fmt_apply")
    return x_tokens


@_on_tensor_device
def fmt_pathway(coarse_nhwc, lateral_nchw, w_reduce, w_smooth, out=None):
    """smooth(up2(reduce(coarse)) + lateral) (FMT.py:221-228): coarse [nv,h,w,cc], lateral [nv,cf,2h,2w].

    out: optional contiguous [nv,2h,2w,cf] destination (e.g. a view slice of a larger batch)."""
    for name, t in (("coarse", coarse_nhwc), ("lateral", lateral_nchw), ("w_reduce", w_reduce), ("w_smooth", w_smooth),
                    ("out", out)):
        _dev(t, name)
    nv, h, w, cc = coarse_nhwc.shape
    cf = lateral_nchw.shape[1]
    if out is None:
        out = torch.empty(nv, 2 * h, 2 * w, cf, device=coarse_nhwc.device)
    elif tuple(out.shape) != (nv, 2 * h, 2 * w, cf) or not out.is_contiguous():
        raise ValueError(f"fmt_pathway: out must be a contiguous [{nv},{2 * h},{2 * w},{cf}] tensor")
    _launch("tmvs_fmt_pathway", coarse_nhwc, lateral_nchw, cf * 4 * h * w, w_reduce, w_smooth, nv, cc, cf, h, w, out)
    return out


# ----------------------------------------------------------------- native orchestration
@_on_tensor_device
def fmt_forward(stage1_nchw, pe, enc_list, tokens=None, side_stream=None):
    """Whole FMT (models/FMT.py:147-177): stage1 [nv,32,H,W] -> tokens [nv,H*W,32].

    side_stream (a torch.cuda.Stream): the reference view's chain runs on it, concurrently with the source
    views (tmvs_fmt_forward_split; bitwise the same tokens). It forks from and joins back into the current
    stream inside the call.
    """
    _dev(stage1_nchw, "stage1")
    nv, c, h, w = stage1_nchw.shape
    tokens = torch.empty(nv, h * w, c, device=stage1_nchw.device) if tokens is None else tokens
    name = "tmvs_fmt_forward_split" if side_stream is not None and nv > 1 else "tmvs_fmt_forward"
    ws, nbytes = _workspace(name + "_workspace", nv, h * w, device=stage1_nchw.device)
    ptrs = (ctypes.c_void_p * 8)(*[e.data_ptr() for e in enc_list])
    args = (stage1_nchw, c * h * w, pe, pe.shape[1], pe.shape[2], nv, h, w, ptrs, ws, nbytes, tokens)
    if name == "tmvs_fmt_forward":
        _launch(name, *args)
    else:  # the side stream follows the current one; the span is the unsplit entry's: bench.py groups by it
        _call(name, *args, _stream(), side_stream.cuda_stream, span="tmvs_fmt_forward")
        if not torch.cuda.is_current_stream_capturing():  # allocator: ws / tokens are also used on the side stream
            ws.record_stream(side_stream)
            tokens.record_stream(side_stream)
    return tokens


@_on_tensor_device
def depth_stage(depth_values, prev_depth, feat_nhwc, ndepth, ratio, full_hw, stage_scale, proj12, pw_params,
                view_w, vw_shift, cr_weights, clamp=(425.0, 935.0), rot_order="auto"):
    """One cascade stage for one sample (models/TransMVSNet.py:174-221). feat [N,h,w,C] NHWC.

    Returns dict(depth, photo_confidence, prob_volume, depth_values) with a batch dim of 1, and depth_raw.
    """
    _dev(depth_values, "depth_values")
    _dev(prev_depth, "prev_depth")
    _dev(feat_nhwc, "feat")
    _dev(view_w, "view_w")
    n, h, w, c = feat_nhwc.shape
    dev = feat_nhwc.device
    hyp = torch.empty(1, ndepth, h, w, device=dev)
    prob = torch.empty_like(hyp)
    depth = torch.empty(1, h, w, device=dev)
    raw = torch.empty_like(depth)
    conf = torch.empty_like(depth)
    proj = np.ascontiguousarray(proj12, np.float32).reshape(n - 1, 12)
    pw = None if pw_params is None else np.ascontiguousarray(pw_params, np.float32)
    ph, pwd = (prev_depth.shape[-2], prev_depth.shape[-1]) if prev_depth is not None else (0, 0)
    _launch("tmvs_depth_stage", depth_values, depth_values.shape[-1], prev_depth, ph, pwd, feat_nhwc, n, c, ndepth,
            ratio, full_hw[0], full_hw[1], stage_scale, proj.ctypes.data, None if pw is None else pw.ctypes.data,
            view_w, vw_shift, warp_flags(rot_order, h * w), ctypes.byref(cr_weights),
            *_workspace("tmvs_depth_stage_workspace", ndepth, h, w, cr_weights.base_ch, device=dev), clamp[0], clamp[1],
            hyp, prob, depth, raw, conf)
    return {"depth": depth, "photo_confidence": conf, "prob_volume": prob, "depth_values": hyp}, raw


def deform_conv2d_pack(weight):
    """HOST packing of a DCN weight [Co][32][3][3] (Co 8/16/32, or 27 for conv_offset_mask) into the
    kernel's A-fragment order (CPU float32)."""
    w = np.ascontiguousarray(weight.detach().float().cpu().numpy(), np.float32)
    co, ci = w.shape[:2]
    out = np.empty(_lib_h().tmvs_deform_conv2d_packed_floats(co), np.float32)
    _lib.check(_lib_h().tmvs_deform_conv2d_pack(w.ctypes.data, co, ci, out.ctypes.data), "tmvs_deform_conv2d_pack")
    return torch.from_numpy(out)


@_on_tensor_device
def deform_conv2d(x_nhwc, offset_mask, w_packed, bias, cout, bn=None, relu=False, want_nhwc=False):
    """DCN.forward's deform_conv2d (models/dcn.py:71-80) + optional folded BN / ReLU of the head.

    x_nhwc [B,H,W,32], offset_mask [B,27,H,W] (conv_offset_mask output), w_packed from
    deform_conv2d_pack (on the device). Returns out [B,cout,H,W] (and [B,H,W,cout] if want_nhwc).
    """
    for t, n in ((x_nhwc, "x_nhwc"), (offset_mask, "offset_mask"), (w_packed, "w_packed"), (bias, "bias")):
        _dev(t, n)
    b, h, w, cin = x_nhwc.shape
    if offset_mask.shape != (b, 27, h, w) or not offset_mask.is_contiguous() or not x_nhwc.is_contiguous():
        raise ValueError("deform_conv2d: expects contiguous x_nhwc [B,H,W,C] and offset_mask [B,27,H,W]")
    out = torch.empty(b, cout, h, w, device=x_nhwc.device)
    out_nhwc = torch.empty(b, h, w, cout, device=x_nhwc.device) if want_nhwc else None
    alpha, shift = bn if bn is not None else (None, None)
    _launch("tmvs_deform_conv2d", x_nhwc, offset_mask, w_packed, bias, alpha, shift, int(relu), b, cin, cout, h, w, out,
            out_nhwc)
    return (out, out_nhwc) if want_nhwc else out


@_on_tensor_device
def dcn_fused(x_nhwc, wom_packed, bom, w_packed, bias, cout, bn=None, relu=False, want_nchw=True, want_nhwc=False):
    """The whole DCN.forward (models/dcn.py:66-80): conv_offset_mask computed in-kernel, then the
    modulated deformable conv + optional folded BN / ReLU. x_nhwc [B,H,W,32] -> out [B,cout,H,W]
    and/or [B,H,W,cout] (returned as (out_nchw, out_nhwc), None where not requested)."""
    for t, n in ((x_nhwc, "x_nhwc"), (wom_packed, "wom_packed"), (bom, "bom"), (w_packed, "w_packed"), (bias, "bias")):
        _dev(t, n)
    if not (want_nchw or want_nhwc):
        raise ValueError("dcn_fused: request at least one output layout")
    b, h, w, cin = x_nhwc.shape
    if not x_nhwc.is_contiguous():
        raise ValueError("dcn_fused: expects a contiguous x_nhwc [B,H,W,C]")
    out = torch.empty(b, cout, h, w, device=x_nhwc.device) if want_nchw else None
    out_nhwc = torch.empty(b, h, w, cout, device=x_nhwc.device) if want_nhwc else None
    alpha, shift = bn if bn is not None else (None, None)
    _launch("tmvs_dcn_fused", x_nhwc, wom_packed, bom, w_packed, bias, alpha, shift, int(relu), b, cin, cout, h, w, out,
            out_nhwc)
    return out, out_nhwc


@_on_tensor_device
def conv3x3_nhwc(x_nhwc, w_packed, bn=None, relu=False, bias=None, want_nchw=False, want_nhwc=True):
    """Conv2d(32, 32, 3, 1, 1) [+ bias] + folded BN + ReLU on x_nhwc [B,H,W,32] (models/module.py:24-61).
    Returns (out_nchw, out_nhwc), None where not requested."""
    for t, n in ((x_nhwc, "x_nhwc"), (w_packed, "w_packed")):
        _dev(t, n)
    if not x_nhwc.is_contiguous():
        raise ValueError("conv3x3_nhwc: expects a contiguous x_nhwc [B,H,W,32]")
    b, h, w, cin = x_nhwc.shape
    out = torch.empty(b, 32, h, w, device=x_nhwc.device) if want_nchw else None
    out_nhwc = torch.empty(b, h, w, 32, device=x_nhwc.device) if want_nhwc else None
    alpha, shift = bn if bn is not None else (None, None)
    _launch("tmvs_conv3x3_nhwc", x_nhwc, w_packed, bias, alpha, shift, int(relu), b, cin, 32, h, w, out, out_nhwc)
    return out, out_nhwc


@_on_tensor_device
def conv3x3_nhwc_acc(x_nhwc, w_packed, out_nhwc):
    """out_nhwc [B,H,W,32] += Conv2d(32, 32, 3, 1, 1, bias=False)(x_nhwc) in the conv's epilogue
    (tmvs_conv3x3_nhwc_acc; each element out + conv, as out.add_(conv))."""
    for t, n in ((x_nhwc, "x_nhwc"), (w_packed, "w_packed"), (out_nhwc, "out_nhwc")):
        _dev(t, n)
    if not x_nhwc.is_contiguous() or not out_nhwc.is_contiguous() or out_nhwc.shape != x_nhwc.shape:
        raise ValueError("conv3x3_nhwc_acc: expects contiguous x_nhwc and out_nhwc [B,H,W,32] of one shape")
    b, h, w, cin = x_nhwc.shape
    _launch("tmvs_conv3x3_nhwc_acc", x_nhwc, w_packed, b, cin, 32, h, w, out_nhwc)
    return out_nhwc


@_on_tensor_device
def fpn_merge(prev_nhwc, lat_nhwc, w_inner, b_inner):
    """interpolate(prev, 2, nearest) + Conv2d_1x1(lat) (models/module.py:409-417), all NHWC:
    prev [B,h,w,32], lat [B,2h,2w,cl] (cl 8/16), w_inner [32,cl] -> [B,2h,2w,32]."""
    for t, n in ((prev_nhwc, "prev_nhwc"), (lat_nhwc, "lat_nhwc"), (w_inner, "w_inner"), (b_inner, "b_inner")):
        _dev(t, n)
    b, h, w, c = prev_nhwc.shape
    cl = lat_nhwc.shape[-1]
    if c != 32 or tuple(lat_nhwc.shape) != (b, 2 * h, 2 * w, cl) or not prev_nhwc.is_contiguous() \
            or not lat_nhwc.is_contiguous():
        raise ValueError("fpn_merge: expects contiguous prev [B,h,w,32] and lat [B,2h,2w,cl]")
    out = torch.empty(b, 2 * h, 2 * w, 32, device=prev_nhwc.device)
    _launch("tmvs_fpn_merge", prev_nhwc, lat_nhwc, cl, w_inner, b_inner, b, h, w, out)
    return out


def conv2d_pack(weight):
    """HOST packing of a Conv2d weight [Co][Ci][k][k] into tmvs_conv2d_bn_relu's k-block order."""
    w = np.ascontiguousarray(weight.detach().float().cpu().numpy(), np.float32)
    co, ci, k, _ = w.shape
    out = np.empty(_lib_h().tmvs_conv2d_packed_floats(co, ci, k), np.float32)
    _lib.check(_lib_h().tmvs_conv2d_pack(w.ctypes.data, co, ci, k, out.ctypes.data), "tmvs_conv2d_pack")
    return torch.from_numpy(out)


@_on_tensor_device
def conv2d_bn_relu(x, w_packed, cout, k, stride, bn=None, relu=True, nchw_input=False):
    """Conv2d(k, stride, padding k//2, no bias) + folded BN + ReLU (models/module.py:24-61) -> NHWC.
    x: NHWC [B,H,W,Ci], or the NCHW image [B,3,H,W] with nchw_input=True."""
    _dev(x, "x")
    _dev(w_packed, "w_packed")
    if not x.is_contiguous():
        raise ValueError("conv2d_bn_relu: expects a contiguous input")
    if nchw_input:
        b, cin, h, w = x.shape
    else:
        b, h, w, cin = x.shape
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    out = torch.empty(b, ho, wo, cout, device=x.device)
    alpha, shift = bn if bn is not None else (None, None)
    _launch("tmvs_conv2d_bn_relu", x, b, cin, h, w, w_packed, cout, k, stride, alpha, shift, int(relu), out)
    return out


@_on_tensor_device
def entropy_loss(prob, depth_values, depth_gt, mask, grad_scale=0.0, want_grad=False, wta=None, conf=None, grad=None):
    """One stage's entropy_loss (models/module.py:495-531) + smooth-L1 depth loss (:549), and with
    want_grad the gradient of grad_scale * loss w.r.t. the stage's softmax logits.
    Returns (loss [], depth_loss [], wta_depth [B,H,W], photo_conf [B,H,W], grad_logits or None).
    wta / conf / grad: caller-provided contiguous outputs of those shapes (grad only with want_grad)."""
    for t, n in ((prob, "prob"), (depth_values, "depth_values"), (depth_gt, "depth_gt"), (mask, "mask"),
                 (wta, "wta"), (conf, "conf"), (grad, "grad")):
        _dev(t, n)
    b, d, h, w = prob.shape
    if depth_values.dim() == 4:
        if tuple(depth_values.shape) != (b, d, h, w):
            raise ValueError("depth_values must be [B,D,H,W] or [B,D]")
        per_pixel = 1
    elif tuple(depth_values.shape) == (b, d):
        per_pixel = 0
    else:
        raise ValueError("depth_values must be [B,D,H,W] or [B,D]")
    if tuple(depth_gt.shape) != (b, h, w) or tuple(mask.shape) != (b, h, w):
        raise ValueError("depth_gt and mask must be [B,H,W]")
    out = torch.empty(2, device=prob.device)
    if grad is not None and not want_grad:
        raise ValueError("entropy_loss: grad given without want_grad")
    wta = torch.empty(b, h, w, device=prob.device) if wta is None else wta
    conf = torch.empty(b, h, w, device=prob.device) if conf is None else conf
    if want_grad and grad is None:
        grad = torch.empty_like(prob)
    for t, n, shape in ((wta, "wta", (b, h, w)), (conf, "conf", (b, h, w)), (grad, "grad", (b, d, h, w))):
        if t is not None and (tuple(t.shape) != shape or t.device != prob.device):
            raise ValueError(f"entropy_loss: {n} must be a contiguous {list(shape)} tensor on prob's device")
    _launch("tmvs_entropy_loss", prob, depth_values, per_pixel, depth_gt, mask, b, d, h, w, grad_scale,
            *_workspace("tmvs_entropy_loss_workspace", b, h, w, device=prob.device), out, wta, conf, grad)
    return out[0], out[1], wta, conf, grad


@_on_tensor_device
def depth_metrics(depth, depth_gt, mask, depth_interval):
    """focal_loss_bld's epe / less1 / less3 (models/module.py:581-587) -> tensor [3]."""
    for t, n in ((depth, "depth"), (depth_gt, "depth_gt"), (mask, "mask")):
        _dev(t, n)
    if depth.shape != depth_gt.shape or depth.shape != mask.shape:
        raise ValueError("depth, depth_gt and mask must have one shape")
    n = depth.numel()
    out = torch.empty(3, device=depth.device)
    _launch("tmvs_depth_metrics", depth, depth_gt, mask, n, float(depth_interval),
            *_workspace("tmvs_depth_metrics_workspace", n, device=depth.device), out)
    return out


EVAL_METRIC_NAMES = ("abs_depth_error", "thres2mm_error", "thres4mm_error", "thres8mm_error", "thres14mm_error",
                     "thres20mm_error", "thres2mm_abserror", "thres4mm_abserror", "thres8mm_abserror",
                     "thres14mm_abserror", "thres20mm_abserror", "thres>20mm_abserror")  # train.py:216-228


@_on_tensor_device
def depth_eval_metrics(depth_est, depth_gt, mask, out=None):
    """The twelve DTU validation scalars of train.py:216-228 (EVAL_METRIC_NAMES) -> device tensor [12]; no
    host sync. `out`: a caller-provided contiguous float32 [12] (a row of a per-interval log buffer)."""
    for t, n in ((depth_est, "depth_est"), (depth_gt, "depth_gt"), (mask, "mask"), (out, "out")):
        _dev(t, n)
    if depth_est.shape != depth_gt.shape or depth_est.shape != mask.shape:
        raise ValueError("depth_est, depth_gt and mask must have one shape")
    n = depth_est.numel()
    nbytes = _lib_h().tmvs_depth_eval_metrics_workspace(n)
    ws = torch.empty(nbytes // 8 + 8, dtype=torch.float64, device=depth_est.device)  # the kernel's doubles
    if out is None:
        out = torch.empty(12, device=depth_est.device)
    elif tuple(out.shape) != (12,) or out.device != depth_est.device:
        raise ValueError("depth_eval_metrics: out must be a contiguous [12] tensor on depth_est's device")
    _launch("tmvs_depth_eval_metrics", depth_est, depth_gt, mask, n, ws, ws.numel() * 8, out)
    return out


@_on_tensor_device
def gt_pyramid(depth_raw, rows, cols, mode="bld", depth_min=0.0, depth_end=0.0, mask_png=None, target_hw=(512, 640)):
    """tmvs_gt_pyramid: the raw depth map [h, w] (and, mode "dtu", the raw depth_visual PNG [h, w] uint8) ->
    ({stage: depth}, {stage: mask}), float32 [H, W] maps at the three stage sizes. rows / cols: the int32
    device tables of data.gt_pyramid_tables for this size and mode."""
    if mode not in ("bld", "dtu"):
        raise ValueError(f"gt_pyramid: mode must be 'bld' or 'dtu', got {mode!r}")
    _dev(depth_raw, "depth_raw")
    if depth_raw.dim() != 2:
        raise ValueError("gt_pyramid: depth_raw must be [h, w]")
    h, w = depth_raw.shape
    for t, n in ((rows, "rows"), (cols, "cols")):
        if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.device != depth_raw.device:
            raise RuntimeError(f"gt_pyramid: {n} must be a contiguous int32 tensor on depth_raw's device")
    if mode == "dtu":
        if mask_png is None or not mask_png.is_cuda or mask_png.dtype != torch.uint8 or not mask_png.is_contiguous() \
                or tuple(mask_png.shape) != (h, w) or mask_png.device != depth_raw.device:
            raise RuntimeError("gt_pyramid: mode 'dtu' needs mask_png, a contiguous uint8 [h, w] tensor on "
                               "depth_raw's device")
        h3, w3 = int(target_hw[0]), int(target_hw[1])
        if h3 <= 0 or w3 <= 0 or h3 > h // 2 or w3 > w // 2:
            raise ValueError(f"gt_pyramid: the crop {h3} x {w3} does not fit the halved image {h // 2} x {w // 2}")
    else:
        h3, w3 = h, w
    if h3 < 4 or w3 < 4:
        raise ValueError("gt_pyramid: the stage-3 size must be at least 4 x 4")
    if rows.numel() != h3 + h3 // 2 + h3 // 4 or cols.numel() != w3 + w3 // 2 + w3 // 4:
        raise ValueError("gt_pyramid: rows / cols do not hold one entry per output row / column of the 3 stages")
    depth = {f"stage{3 - s}": torch.empty(h3 >> s, w3 >> s, device=depth_raw.device) for s in range(3)}
    mask = {k: torch.empty_like(v) for k, v in depth.items()}
    _launch("tmvs_gt_pyramid", _lib.GT_DTU if mode == "dtu" else _lib.GT_BLD, depth_raw,
            mask_png if mode == "dtu" else None, h, w, h3, w3, depth_min, depth_end, rows, cols, depth["stage3"],
            depth["stage2"], depth["stage1"], mask["stage3"], mask["stage2"], mask["stage1"])
    return depth, mask


# ----------------------------------------------------------------- CostRegNet training (train.py)
@_on_tensor_device
def conv3d_generic(x, w_packed, cout, out_dhw, stride, transposed=False, out=None):
    """tmvs_conv3d_generic: x NDHWC [B,D,H,W,Cin], w_packed [27][cout][Cin] -> y [B,*out_dhw,cout]
    (accumulated into `out` when given)."""
    _dev(x, "x")
    _dev(w_packed, "w_packed")
    b, d, h, w, cin = x.shape
    if w_packed.numel() != 27 * cout * cin:
        raise ValueError("conv3d_generic: w_packed must hold [27, cout, cin] floats")
    flags = (_lib.CONV_TRANSPOSED if transposed else 0) | (_lib.CONV_ACCUMULATE if out is not None else 0)
    y = torch.empty(b, *out_dhw, cout, device=x.device) if out is None else out
    if tuple(y.shape) != (b, *out_dhw, cout) or not y.is_contiguous():
        raise ValueError("conv3d_generic: out must be a contiguous [B, D, H, W, cout] tensor")
    _launch("tmvs_conv3d_generic", x, b, cin, d, h, w, w_packed, cout, out_dhw[0], out_dhw[1], out_dhw[2], stride,
            flags, y)
    return y


# (cin, cout, stride) of the inference layers' MFMA kernels (tmvs_conv3d_mfma); transposed: (cin, cout)
MFMA_CONV = {(16, 16, 1), (32, 32, 1), (64, 64, 1), (8, 16, 2), (16, 32, 2), (32, 64, 2), (1, 8, 1), (8, 1, 1)}
MFMA_DECONV = {(64, 32), (32, 16), (16, 8)}


def prob_pack(w27):
    """[27][1][8] (tap = kd*9 + kh*3 + kw) -> prob_kernel's [3][72] packing (model.CostRegNet.packed):
    per kh, the {kd=1, kd=2} pairs in (kw, c) order, then kd=0 in (kw, c) order."""
    pw = w27.reshape(3, 3, 3, 8).permute(3, 0, 1, 2)  # [c][kd][kh][kw]
    pairs = pw[:, 1:3].permute(2, 3, 0, 1).reshape(3, -1)
    single = pw[:, 0].permute(1, 2, 0).reshape(3, -1)
    return torch.cat([pairs, single], 1).contiguous()


@_on_tensor_device
def conv3d_mfma(x, w_packed, cout, stride, transposed=False, skip=None, out=None):
    """tmvs_conv3d_mfma: x NDHWC [B,D,H,W,Cin], w_packed [27][cout][Cin] -> y [B,D',H',W',cout], the raw
    convolution (no BN / ReLU) on the inference MFMA kernels; transposed = ConvTranspose3d k3 s2 p1 op1
    (+ skip, a separate [B,2D,2H,2W,cout] tensor). Written to `out` when given."""
    _layer_args("conv3d_mfma", x, w_packed, None, None, cout)
    b, d, h, w, cin = x.shape
    shape = (b, 2 * d, 2 * h, 2 * w, cout) if transposed else (b, *_conv_out_dhw(d, h, w, stride), cout)
    _layer_like("conv3d_mfma", "skip", skip, shape, x.device)
    _layer_like("conv3d_mfma", "out", out, shape, x.device)
    _layer_no_alias("conv3d_mfma", skip, out)
    if (cin, cout) == (8, 1):
        if tuple(w_packed.shape) != (3, 72):
            raise ValueError("conv3d_mfma: the 8 -> 1 conv takes the prob packing [3, 72] (prob_pack)")
    elif tuple(w_packed.shape) != (27, cout, cin):
        raise ValueError("conv3d_mfma: w_packed must be [27, cout, cin]")
    y = torch.empty(shape, device=x.device) if out is None else out
    _launch("tmvs_conv3d_mfma", x, b, cin, d, h, w, w_packed, cout, stride, int(transposed), skip, y)
    return y


@_on_tensor_device
def conv3d_wgrad(direct, gathered, stride):
    """tmvs_conv3d_wgrad: direct [B,pd,ph,pw,A], gathered [B,gd,gh,gw,BC] -> dw [27][A][BC]."""
    _dev(direct, "direct")
    _dev(gathered, "gathered")
    b, pd, ph, pw, a = direct.shape
    gb, gd, gh, gw, bc = gathered.shape
    if gb != b:
        raise ValueError("conv3d_wgrad: direct and gathered must have the same batch size")
    dw = torch.empty(27, a, bc, device=direct.device)
    _launch("tmvs_conv3d_wgrad", direct, a, b, pd, ph, pw, gathered, bc, gd, gh, gw, stride,
            *_workspace("tmvs_conv3d_wgrad_workspace", b, pd, ph, pw, a, bc, device=direct.device), dw)
    return dw


def _bn_shapes(what, z, per_channel, like_z):
    """the statistics / affine vectors hold groups * C (or C) floats and the element-wise tensors z's count:
    the entry points take one size for all of them"""
    c = z.shape[-1]
    for name, t, n in per_channel:
        if t.numel() != n * c:
            raise ValueError(f"{what}: {name} must hold {n * c} floats")
    for name, t in like_z:
        if t is not None and t.numel() != z.numel():
            raise ValueError(f"{what}: {name} must have z's size")


def _bn_groups(z, g):
    """(leading size arguments, entry suffix, voxels per group, C) of the plain (g None) or per-group entries"""
    c = z.shape[-1]
    return ((), "", z.numel() // c, c) if g is None else ((g,), "_grouped", z.numel() // (g * c), c)


def _bn_stats_launch(z, g):
    _dev(z, "z")
    lead, sfx, nvox, c = _bn_groups(z, g)
    mean = torch.empty(*lead, c, device=z.device)
    var = torch.empty(*lead, c, device=z.device)
    _launch("tmvs_bn_stats" + sfx, z, *lead, nvox, c,
            *_workspace("tmvs_bn_train_workspace" + sfx, *lead, nvox, c, device=z.device), mean, var)
    return mean, var


def _bn_relu_train_launch(z, g, mean, var, gamma, beta, eps, skip=None, out=None):
    for t, n in ((z, "z"), (mean, "mean"), (var, "var"), (gamma, "gamma"), (beta, "beta"), (skip, "skip"),
                 (out, "out")):
        _dev(t, n)
    lead, sfx, nvox, c = _bn_groups(z, g)
    _bn_shapes("bn_relu_train" + sfx, z, (("mean", mean, g or 1), ("var", var, g or 1), ("gamma", gamma, 1),
                                          ("beta", beta, 1)), (("skip", skip), ("out", out)))
    out = torch.empty_like(z) if out is None else out
    _launch("tmvs_bn_relu_train" + sfx, z, *lead, nvox, c, mean, var, gamma, beta, eps, skip, out)
    return out


def _bn_relu_backward_launch(dy, z, g, mean, var, gamma, beta, eps, dz=None):
    for t, n in ((dy, "dy"), (z, "z"), (mean, "mean"), (var, "var"), (gamma, "gamma"), (beta, "beta"), (dz, "dz")):
        _dev(t, n)
    lead, sfx, nvox, c = _bn_groups(z, g)
    _bn_shapes("bn_relu_backward" + sfx, z, (("mean", mean, g or 1), ("var", var, g or 1), ("gamma", gamma, 1),
                                             ("beta", beta, 1)), (("dy", dy), ("dz", dz)))
    dz = torch.empty_like(z) if dz is None else dz
    dg = torch.empty(c, device=z.device)
    db = torch.empty(c, device=z.device)
    _launch("tmvs_bn_relu_backward" + sfx, dy, z, *lead, nvox, c, mean, var, gamma, beta, eps,
            *_workspace("tmvs_bn_train_workspace" + sfx, *lead, nvox, c, device=z.device), dz, dg, db)
    return dz, dg, db


@_on_tensor_device
def bn_stats(z):
    """tmvs_bn_stats: z [..., C] -> (batch mean [C], biased variance [C])."""
    return _bn_stats_launch(z, None)


@_on_tensor_device
def bn_relu_train(z, mean, var, gamma, beta, eps, skip=None, out=None):
    """tmvs_bn_relu_train: relu(BN_batch(z)) [+ skip], z [..., C] (written into `out` when given)."""
    return _bn_relu_train_launch(z, None, mean, var, gamma, beta, eps, skip, out)


@_on_tensor_device
def bn_relu_backward(dy, z, mean, var, gamma, beta, eps, dz=None):
    """tmvs_bn_relu_backward -> (dz, dgamma, dbeta) (dz written into `dz` when given)."""
    return _bn_relu_backward_launch(dy, z, None, mean, var, gamma, beta, eps, dz)


@_on_tensor_device
def bn_stats_grouped(z):
    """tmvs_bn_stats_grouped: z [G, ..., C] -> (mean [G, C], biased variance [G, C]), statistics per group."""
    return _bn_stats_launch(z, z.shape[0])


@_on_tensor_device
def bn_relu_train_grouped(z, mean, var, gamma, beta, eps):
    """tmvs_bn_relu_train_grouped: relu(BN_batch(z)) per group, z [G, ..., C], mean / var [G, C]."""
    return _bn_relu_train_launch(z, z.shape[0], mean, var, gamma, beta, eps)


@_on_tensor_device
def bn_relu_backward_grouped(dy, z, mean, var, gamma, beta, eps):
    """tmvs_bn_relu_backward_grouped -> (dz, dgamma, dbeta), dgamma / dbeta summed over the groups in order."""
    return _bn_relu_backward_launch(dy, z, z.shape[0], mean, var, gamma, beta, eps)


@_on_tensor_device
def warp_corr_backward(ref_nhwc, src_nhwc, proj12, hyp, dsim, rot_order="auto", planes=False, dref_out=None,
                       dsrc_out=None):
    """tmvs_warp_corr_backward: one sample, ref [H,W,C], src [V,H,W,C] NHWC, proj12 HOST [V,12],
    hyp [D,H,W], dsim [V,D,H,W] -> (dref [H,W,C], dsrc [V,H,W,C], flag tensor [1] int32: bit 0 a
    non-finite dsim / ref, bit 1 non-planar hyp under planes=True). planes=True (TMVS_WARP_BWD_PLANES:
    hyp[d] is one depth per plane, stage 1) gathers dsrc per source texel instead of scattering it.
    dref_out / dsrc_out: caller-provided contiguous outputs of those shapes."""
    for t, n in ((ref_nhwc, "ref"), (src_nhwc, "src"), (hyp, "hyp"), (dsim, "dsim"), (dref_out, "dref_out"),
                 (dsrc_out, "dsrc_out")):
        _dev(t, n)
    v, h, w, c = src_nhwc.shape
    d = hyp.shape[0]
    if tuple(dsim.shape) != (v, d, h, w) or tuple(ref_nhwc.shape) != (h, w, c):
        raise ValueError("warp_corr_backward: shapes must be ref [H,W,C], src [V,H,W,C], hyp [D,H,W], dsim [V,D,H,W]")
    proj = np.ascontiguousarray(proj12, np.float32).reshape(v, 12)
    dref = torch.empty_like(ref_nhwc) if dref_out is None else dref_out
    dsrc = torch.empty_like(src_nhwc) if dsrc_out is None else dsrc_out
    if tuple(dref.shape) != (h, w, c) or not dref.is_contiguous():
        raise ValueError(f"dref_out must be a contiguous [{h},{w},{c}] tensor")
    if tuple(dsrc.shape) != (v, h, w, c) or not dsrc.is_contiguous():
        raise ValueError(f"dsrc_out must be a contiguous [{v},{h},{w},{c}] tensor")
    ws, nbytes = _workspace("tmvs_warp_corr_backward_workspace", v, c, h, w, d, device=hyp.device)
    _launch("tmvs_warp_corr_backward", ref_nhwc, src_nhwc, proj.ctypes.data, hyp, dsim, v, c, d, h, w,
            warp_flags(rot_order, h * w) | (_lib.WARP_BWD_PLANES if planes else 0), ws, nbytes, dref, dsrc)
    flag = ws.view(torch.int32)[2 * v * h * w * c: 2 * v * h * w * c + 1]
    return dref, dsrc, flag


def _pw_shaped(op, t, name, shape, like, dtype=torch.float32):
    """`t` is a contiguous `dtype` tensor of `shape` on `like`'s device: the PixelwiseNet / aggregation entry
    points take one V, D, H, W for all their tensors and would read or write any other size past its end"""
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or t.device != like.device
            or tuple(t.shape) != tuple(shape)):
        kind = "int32" if dtype == torch.int32 else "float32"
        got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{op}: {name} must be a contiguous {kind} {list(shape)} tensor on sims' device, not {got}")


def _pw_sims(op, sims, batched=False):
    _dev(sims, "sims")
    if sims.dim() != 4 + batched:
        raise ValueError(f"{op}: sims must be [{'B, ' if batched else ''}V, D, H, W], not {list(sims.shape)}")
    return sims.shape


def _vw_map_shape(op, v, h, w, vw_shift):
    """[V, H >> s, W >> s]: the map the aggregate kernels read at (y >> s, x >> s), which covers the image only
    when H and W are multiples of 2^s"""
    s = int(vw_shift)
    if not 0 <= s <= 4:
        raise ValueError(f"{op}: vw_shift must be in [0, 4], not {vw_shift}")
    if h % (1 << s) or w % (1 << s):
        raise ValueError(f"{op}: H = {h} and W = {w} must be multiples of 2^vw_shift = {1 << s}")
    return (v, h >> s, w >> s)


def _pixelwise_train_forward_launch(sims, pwp, batched):
    """sims [V,D,H,W], or [B,V,D,H,W] through the _batched entry"""
    op = "pixelwise_train_forward" + ("_batched" if batched else "")
    *b, v, d, h, w = _pw_sims(op, sims, batched)
    _pw_shaped(op, pwp, "pwp", (_lib.PW_NPARAMS,), sims)
    stats = torch.empty(v, 48, device=sims.device)
    vw = torch.empty(*b, v, h, w, device=sims.device)
    dstar = torch.empty(*b, v, h, w, device=sims.device, dtype=torch.int32)
    _launch("tmvs_" + op, sims, *b, v, d, h, w, pwp, *_workspace("tmvs_pixelwise_train_workspace", device=sims.device),
            stats, vw, dstar)
    return stats, vw, dstar


def _pixelwise_train_backward_launch(sims, pwp, stats, view_w, dstar, dview_w, dsims, batched):
    op = "pixelwise_train_backward" + ("_batched" if batched else "")
    *b, v, d, h, w = _pw_sims(op, sims, batched)
    for t, n, shape in ((pwp, "pwp", (_lib.PW_NPARAMS,)), (stats, "stats", (v, 48)), (view_w, "view_w", (*b, v, h, w)),
                        (dview_w, "dview_w", (*b, v, h, w)), (dsims, "dsims", (*b, v, d, h, w))):
        _pw_shaped(op, t, n, shape, sims)
    _pw_shaped(op, dstar, "dstar", (*b, v, h, w), sims, torch.int32)
    dpwp = torch.zeros(_lib.PW_NPARAMS, device=sims.device)
    _launch("tmvs_" + op, sims, *b, v, d, h, w, pwp, stats, view_w, dstar, dview_w,
            *_workspace("tmvs_pixelwise_train_workspace", device=sims.device), dsims, dpwp)
    return dpwp


@_on_tensor_device
def pixelwise_train_forward(sims, pwp):
    """tmvs_pixelwise_train_forward: sims [V,D,H,W], pwp [201] -> (stats [V,48], view_w [V,H,W], dstar int32)."""
    return _pixelwise_train_forward_launch(sims, pwp, False)


@_on_tensor_device
def aggregate_train(sims, view_w, vw_shift, sim=None):
    """tmvs_aggregate_train: sims [V,D,H,W], view_w [V,H>>s,W>>s] -> (sim [D,H,W], wsum [H,W]).
    sim: a caller-provided contiguous [D,H,W] output."""
    op = "aggregate_train"
    v, d, h, w = _pw_sims(op, sims)
    _pw_shaped(op, view_w, "view_w", _vw_map_shape(op, v, h, w, vw_shift), sims)
    if sim is None:
        sim = torch.empty(d, h, w, device=sims.device)
    _pw_shaped(op, sim, "sim", (d, h, w), sims)
    wsum = torch.empty(h, w, device=sims.device)
    _launch("tmvs_aggregate_train", sims, view_w, v, d, h, w, vw_shift, sim, wsum)
    return sim, wsum


@_on_tensor_device
def aggregate_train_backward(dsim, sims, sim, wsum, view_w, vw_shift, want_dview_w, dsims=None, dview_w=None):
    """tmvs_aggregate_train_backward -> (dsims [V,D,H,W], dview_w [V,H,W] or None).
    dsims / dview_w: caller-provided contiguous outputs of those shapes (dview_w only with want_dview_w)."""
    op = "aggregate_train_backward"
    v, d, h, w = _pw_sims(op, sims)
    _pw_shaped(op, view_w, "view_w", _vw_map_shape(op, v, h, w, vw_shift), sims)
    for t, n, shape in ((dsim, "dsim", (d, h, w)), (sim, "sim", (d, h, w)), (wsum, "wsum", (h, w))):
        _pw_shaped(op, t, n, shape, sims)
    if dview_w is not None and not want_dview_w:
        raise ValueError(f"{op}: dview_w given without want_dview_w")
    if dsims is None:
        dsims = torch.empty_like(sims)
    if want_dview_w and dview_w is None:
        dview_w = torch.empty(v, h, w, device=sims.device)
    _pw_shaped(op, dsims, "dsims", (v, d, h, w), sims)
    if want_dview_w:
        _pw_shaped(op, dview_w, "dview_w", (v, h, w), sims)
    _launch("tmvs_aggregate_train_backward", dsim, sims, sim, wsum, view_w, v, d, h, w, vw_shift, dsims, dview_w)
    return dsims, dview_w


@_on_tensor_device
def pixelwise_train_backward(sims, pwp, stats, view_w, dstar, dview_w, dsims):
    """tmvs_pixelwise_train_backward: adds the PixelwiseNet path into dsims (in place) -> dpwp [201]."""
    return _pixelwise_train_backward_launch(sims, pwp, stats, view_w, dstar, dview_w, dsims, False)


@_on_tensor_device
def pixelwise_train_forward_batched(sims, pwp):
    """tmvs_pixelwise_train_forward_batched: sims [B,V,D,H,W], pwp [201] -> (stats [V,48] joint over each view's
    B*D*H*W elements, view_w [B,V,H,W], dstar int32 [B,V,H,W])."""
    return _pixelwise_train_forward_launch(sims, pwp, True)


@_on_tensor_device
def pixelwise_train_backward_batched(sims, pwp, stats, view_w, dstar, dview_w, dsims):
    """tmvs_pixelwise_train_backward_batched: sims / dsims [B,V,D,H,W], stats [V,48], view_w / dstar / dview_w
    [B,V,H,W]; adds the PixelwiseNet path into dsims (in place) -> dpwp [201]."""
    return _pixelwise_train_backward_launch(sims, pwp, stats, view_w, dstar, dview_w, dsims, True)


@_on_tensor_device
def upsample2_add_nhwc(r, lateral_nchw):
    """tmvs_upsample2_add_nhwc: r [N,h,w,C] -> bilinear x2 + lateral [N,C,2h,2w] -> [N,2h,2w,C]."""
    _dev(r, "r")
    _dev(lateral_nchw, "lateral")
    n, h, w, c = r.shape
    if tuple(lateral_nchw.shape) != (n, c, 2 * h, 2 * w):
        raise ValueError("upsample2_add_nhwc: lateral must be [N, C, 2h, 2w]")
    u = torch.empty(n, 2 * h, 2 * w, c, device=r.device)
    _launch("tmvs_upsample2_add_nhwc", r, lateral_nchw, n, h, w, c, u)
    return u


@_on_tensor_device
def upsample2_backward_nhwc(du):
    """tmvs_upsample2_backward_nhwc: du [N,2h,2w,C] -> dr [N,h,w,C]."""
    _dev(du, "du")
    n, hh, ww, c = du.shape
    if hh % 2 or ww % 2:
        raise ValueError("upsample2_backward_nhwc: du must be [N, 2h, 2w, C]")
    dr = torch.empty(n, hh // 2, ww // 2, c, device=du.device)
    _launch("tmvs_upsample2_backward_nhwc", du, n, hh // 2, ww // 2, c, dr)
    return dr


def _tokens(x, name, c=None):
    _dev(x, name)
    if x.dim() != 2 or (c is not None and x.shape[1] != c):
        raise ValueError(f"{name}: expected a [T, {c or 'C'}] token matrix, got {tuple(x.shape)}")
    return x.shape[0]


@_on_tensor_device
def token_linear(x, w, b=None, transpose_w=False, relu_of=None, out=None, residual=None):
    """tmvs_token_linear: x [T,in] -> x w^T + b (w [out,in]) or, transpose_w, x w (w [in',out'] -> out = in').

    relu_of [T,out] masks the result where relu_of <= 0; out (given) is accumulated into; residual (given,
    tmvs_token_linear_res) -> a new residual + result (the same additions as out=residual.clone())."""
    t = _tokens(x, "x")
    for a, n in ((w, "w"), (b, "b"), (relu_of, "relu_of"), (out, "out"), (residual, "residual")):
        _dev(a, n)
    if residual is not None:
        if out is not None:
            raise ValueError("token_linear: give out or residual, not both")
        o_f = w.shape[0] if not transpose_w else w.shape[1]
        if x.shape[1] != (w.shape[1] if not transpose_w else w.shape[0]) or tuple(residual.shape) != (t, o_f) or \
                (relu_of is not None and tuple(relu_of.shape) != (t, o_f)):
            raise ValueError("token_linear: shape mismatch")
        y = torch.empty(t, o_f, device=x.device)
        _launch("tmvs_token_linear_res", x, t, x.shape[1], o_f, w, b, int(transpose_w), relu_of, residual, y)
        return y
    o_f = w.shape[0] if not transpose_w else w.shape[1]
    if x.shape[1] != (w.shape[1] if not transpose_w else w.shape[0]):
        raise ValueError("token_linear: x / w feature mismatch")
    acc = out is not None
    for a, n in ((relu_of, "relu_of"), (out, "out")):
        if a is not None and tuple(a.shape) != (t, o_f):
            raise ValueError(f"token_linear: {n} must be [{t}, {o_f}]")
    y = out if acc else torch.empty(t, o_f, device=x.device)
    _launch("tmvs_token_linear", x, t, x.shape[1], o_f, w, b, int(transpose_w), relu_of, int(acc), y)
    return y


@_on_tensor_device
def token_wgrad(dy, x, dw=None, db=None):
    """tmvs_token_wgrad: dy [T,a], x [T,b] -> (dw [a,b] = dy^T x, db [a] = column sums of dy); accumulates into
    dw/db when both are given."""
    t = _tokens(dy, "dy")
    if _tokens(x, "x") != t:
        raise ValueError("token_wgrad: token counts differ")
    a, b = dy.shape[1], x.shape[1]
    acc = dw is not None
    if acc != (db is not None):
        raise ValueError("token_wgrad: give both dw and db or neither")
    if not acc:
        dw, db = torch.empty(a, b, device=dy.device), torch.empty(a, device=dy.device)
    for z, n, shp in ((dw, "dw", (a, b)), (db, "db", (a,))):
        _dev(z, n)
        if tuple(z.shape) != shp:
            raise ValueError(f"token_wgrad: {n} must be {shp}")
    _launch("tmvs_token_wgrad", dy, a, x, b, t, *_workspace("tmvs_token_wgrad_workspace", t, a, b, device=dy.device),
            dw, db, int(acc))
    return dw, db


@_on_tensor_device
def layer_norm_fwd(x, g, b):
    """tmvs_layer_norm_fwd: LayerNorm(32) of x [T,32]."""
    t = _tokens(x, "x", 32)
    _dev(g, "g")
    _dev(b, "b")
    y = torch.empty_like(x)
    _launch("tmvs_layer_norm_fwd", x, t, g, b, y)
    return y


@_on_tensor_device
def layer_norm_bwd(dy, x, g, dgb=None):
    """tmvs_layer_norm_bwd: -> (dx [T,32], dgb [64] = dgamma | dbeta); accumulates into dgb when given."""
    t = _tokens(dy, "dy", 32)
    if _tokens(x, "x", 32) != t:
        raise ValueError("layer_norm_bwd: token counts differ")
    _dev(g, "g")
    _dev(dgb, "dgb")
    acc = dgb is not None
    dgb = dgb if acc else torch.empty(64, device=dy.device)
    dx = torch.empty_like(dy)
    _launch("tmvs_layer_norm_bwd", dy, x, t, g, *_workspace("tmvs_layer_norm_bwd_workspace", t, device=dy.device), dx,
            dgb, int(acc))
    return dx, dgb


@_on_tensor_device
def linattn_fwd(q, kv, tokens_per_group):
    """tmvs_linattn_fwd: q [T,32] (pre-elu), kv [G,160] (G == 1: shared) -> msg [T,32]."""
    t = _tokens(q, "q", 32)
    _dev(kv, "kv")
    msg = torch.empty_like(q)
    stride = 0 if kv.shape[0] == 1 else _lib.KV_NFLOATS
    _launch("tmvs_linattn_fwd", q, t, tokens_per_group, kv, stride, msg)
    return msg


@_on_tensor_device
def linattn_bwd_q(q, dmsg, kv, tokens_per_group):
    """tmvs_linattn_bwd_q: -> (dq [T,32], dkv [T / tokens_per_group, 160])."""
    t = _tokens(q, "q", 32)
    if _tokens(dmsg, "dmsg", 32) != t:
        raise ValueError("linattn_bwd_q: token counts differ")
    if t % tokens_per_group:
        raise ValueError("linattn_bwd_q: tokens must be a multiple of tokens_per_group")
    _dev(kv, "kv")
    groups = t // tokens_per_group
    stride = 0 if kv.shape[0] == 1 else _lib.KV_NFLOATS
    if stride and kv.shape[0] != groups:
        raise ValueError("linattn_bwd_q: kv must have one row per group (or one shared row)")
    dq = torch.empty_like(q)
    dkv = torch.empty(groups, _lib.KV_NFLOATS, device=q.device)
    _launch("tmvs_linattn_bwd_q", q, dmsg, t, tokens_per_group, kv, stride,
            *_workspace("tmvs_linattn_bwd_workspace", t, tokens_per_group, device=q.device), dq, dkv)
    return dq, dkv


@_on_tensor_device
def linattn_bwd_kv(k, v, dkv, tokens_per_group):
    """tmvs_linattn_bwd_kv: k (pre-elu), v [S,32], dkv [S / tokens_per_group, 160] -> (dk, dv)."""
    s = _tokens(k, "k", 32)
    if _tokens(v, "v", 32) != s or dkv.shape[0] * tokens_per_group != s:
        raise ValueError("linattn_bwd_kv: shape mismatch")
    _dev(dkv, "dkv")
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    _launch("tmvs_linattn_bwd_kv", k, v, s, tokens_per_group, dkv, dk, dv)
    return dk, dv


@_on_tensor_device
def adam_step(param_flat, grad_flat, exp_avg, exp_avg_sq, lr, betas, eps, weight_decay, step):
    """tmvs_adam_step: one Adam update (torch's order) of a flat fp32 parameter buffer, in place."""
    for t, n in ((param_flat, "param"), (grad_flat, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _dev(t, n)
        if t.numel() != param_flat.numel():
            raise ValueError(f"adam_step: {n} must have {param_flat.numel()} elements")
    _launch("tmvs_adam_step", param_flat, grad_flat, exp_avg, exp_avg_sq, param_flat.numel(), float(lr),
            float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step))


@_on_tensor_device
def adam_step_dev(param_flat, grad_flat, exp_avg, exp_avg_sq, lr, betas, eps, weight_decay, step_counter, scalars,
                  lr_dev=None):
    """tmvs_adam_step_dev: adam_step with the step number advanced on the device (graph-replayable).
    lr_dev: an optional device float64 [1] read by the launch when it runs (a replayed graph then
    follows the value the caller writes there); None = lr by value."""
    for t, n in ((param_flat, "param"), (grad_flat, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"),
                 (scalars, "scalars")):
        _dev(t, n)
    if step_counter.dtype != torch.int32 or not step_counter.is_cuda:
        raise RuntimeError("step_counter must be a device int32 tensor")
    if lr_dev is not None and (lr_dev.dtype != torch.float64 or not lr_dev.is_cuda or lr_dev.numel() != 1):
        raise RuntimeError("lr_dev must be a device float64 tensor of one element")
    # adam_step's span: bench.py groups by it
    _launch("tmvs_adam_step_dev", param_flat, grad_flat, exp_avg, exp_avg_sq, param_flat.numel(), float(lr), lr_dev,
            float(betas[0]), float(betas[1]), float(eps), float(weight_decay), step_counter, scalars,
            span="tmvs_adam_step")


# ----------------------------------------------------------------- FeatureNet training (featurenet_train.py)
@_on_tensor_device
def conv2d_generic(x, w_taps, cout, out_hw, k, stride, pad, bias=None, transposed=False, out=None):
    """tmvs_conv2d_generic: x NHWC [B,H,W,Cin], w_taps [k*k][cout][Cin] -> y [B,*out_hw,cout] (+ bias);
    accumulated into `out` when given."""
    _dev(x, "x")
    _dev(w_taps, "w_taps")
    _dev(bias, "bias")
    b, h, w, cin = x.shape
    if w_taps.numel() != k * k * cout * cin or (bias is not None and bias.numel() != cout):
        raise ValueError("conv2d_generic: w_taps must hold [k*k, cout, cin] floats and bias [cout]")
    flags = (_lib.CONV_TRANSPOSED if transposed else 0) | (_lib.CONV_ACCUMULATE if out is not None else 0)
    y = torch.empty(b, *out_hw, cout, device=x.device) if out is None else out
    if tuple(y.shape) != (b, *out_hw, cout) or not y.is_contiguous():
        raise ValueError("conv2d_generic: out must be a contiguous [B, H, W, cout] tensor")
    _launch("tmvs_conv2d_generic", x, b, cin, h, w, w_taps, bias, cout, out_hw[0], out_hw[1], k, stride, pad, flags, y)
    return y


@_on_tensor_device
def conv2d_wgrad(direct, gathered, k, stride, pad):
    """tmvs_conv2d_wgrad: direct [B,ph,pw,A] (dz), gathered [B,gh,gw,BC] (x) -> dw [k*k][A][BC]."""
    _dev(direct, "direct")
    _dev(gathered, "gathered")
    b, ph, pw, a = direct.shape
    gb, gh, gw, bc = gathered.shape
    if gb != b:
        raise ValueError("conv2d_wgrad: direct and gathered must have the same batch size")
    dw = torch.empty(k * k, a, bc, device=direct.device)
    _launch("tmvs_conv2d_wgrad", direct, a, b, ph, pw, gathered, bc, gh, gw, k, stride, pad,
            *_workspace("tmvs_conv2d_wgrad_workspace", b, ph, pw, a, bc, k, device=direct.device), dw)
    return dw


@_on_tensor_device
def colsum(x):
    """tmvs_colsum: x [..., C] -> [C] (sum over every other axis; C <= 32)."""
    _dev(x, "x")
    c = x.shape[-1]
    n = x.numel() // c
    out = torch.empty(c, device=x.device)
    _launch("tmvs_colsum", x, n, c, *_workspace("tmvs_colsum_workspace", n, c, device=x.device), out)
    return out


@_on_tensor_device
def dcn_forward_train(x_nhwc, wom_packed, bom, w_packed, bias, cout, want_nchw=False):
    """tmvs_dcn_forward_train: DCN.forward without BN/ReLU -> (out_nhwc [B,H,W,cout], offset_mask
    [B,27,H,W], out_nchw or None)."""
    for t, n in ((x_nhwc, "x_nhwc"), (wom_packed, "wom_packed"), (bom, "bom"), (w_packed, "w_packed"), (bias, "bias")):
        _dev(t, n)
    b, h, w, cin = x_nhwc.shape
    out_nhwc = torch.empty(b, h, w, cout, device=x_nhwc.device)
    out = torch.empty(b, cout, h, w, device=x_nhwc.device) if want_nchw else None
    om = torch.empty(b, 27, h, w, device=x_nhwc.device)
    _launch("tmvs_dcn_forward_train", x_nhwc, wom_packed, bom, w_packed, bias, b, cin, cout, h, w, out, out_nhwc, om)
    return out_nhwc, om, out


@_on_tensor_device
def dcn_backward(x_nhwc, offset_mask, w_taps, dy_nhwc, dx_nhwc):
    """tmvs_dcn_backward: -> (dom [B,H,W,32] (channels 27..31 zero), dw_taps [9][cout][32]); dx_nhwc is
    accumulated into."""
    for t, n in ((x_nhwc, "x_nhwc"), (offset_mask, "offset_mask"), (w_taps, "w_taps"), (dy_nhwc, "dy_nhwc"),
                 (dx_nhwc, "dx_nhwc")):
        _dev(t, n)
    b, h, w, cin = x_nhwc.shape
    cout = dy_nhwc.shape[-1]
    if tuple(offset_mask.shape) != (b, 27, h, w) or tuple(dy_nhwc.shape) != (b, h, w, cout) or \
            tuple(w_taps.shape) != (9, cout, cin) or tuple(dx_nhwc.shape) != tuple(x_nhwc.shape):
        raise ValueError("dcn_backward: shape mismatch")
    dom = torch.empty(b, h, w, 32, device=x_nhwc.device)
    dw = torch.empty(9, cout, cin, device=x_nhwc.device)
    _launch("tmvs_dcn_backward", x_nhwc, offset_mask, w_taps, dy_nhwc, b, cin, cout, h, w,
            *_workspace("tmvs_dcn_backward_workspace", b, cout, h, w, device=x_nhwc.device), dx_nhwc, dom, dw)
    return dom, dw


_DCN_FAR = {}


@_on_tensor_device
def dcn_backward_set(x_nhwc, offset_mask, w_taps, dy_nhwc):
    """tmvs_dcn_backward_set: -> (dx [B,H,W,32] written, not accumulated; dom; dw_taps). The corners beyond the
    LDS windows go through a zeroed far buffer kept per (device, shape) and cleared again by the call, so no
    activation-sized zero fill runs per call. One buffer per shape: an eager call on another stream waits for
    the previous call's stream (event), and the buffer is created outside any HIP-graph capture (raises if a
    shape is first seen while capturing)."""
    for t, n in ((x_nhwc, "x_nhwc"), (offset_mask, "offset_mask"), (w_taps, "w_taps"), (dy_nhwc, "dy_nhwc")):
        _dev(t, n)
    b, h, w, cin = x_nhwc.shape
    cout = dy_nhwc.shape[-1]
    if tuple(offset_mask.shape) != (b, 27, h, w) or tuple(dy_nhwc.shape) != (b, h, w, cout) or \
            tuple(w_taps.shape) != (9, cout, cin):
        raise ValueError("dcn_backward_set: shape mismatch")
    key = (str(x_nhwc.device), tuple(x_nhwc.shape))
    capturing = torch.cuda.is_current_stream_capturing()
    ent = _DCN_FAR.get(key)
    if ent is None:
        if capturing:  # a zero fill recorded in the graph would run per replay, and an eager call before the
            # first replay would read an unfilled buffer: the buffer must exist before the capture
            raise RuntimeError("dcn_backward_set: first call for this shape inside a HIP-graph capture; run one eager "
                               "step first (the far buffer is allocated and zeroed outside any capture)")
        ent = _DCN_FAR[key] = [torch.zeros_like(x_nhwc), None, None]  # buffer, last stream, its done event
    far = ent[0]
    cur = torch.cuda.current_stream(x_nhwc.device)
    if not capturing and ent[1] is not None and ent[1] != cur:  # a call on another stream: order after its use
        cur.wait_event(ent[2])
    dx = torch.empty_like(x_nhwc)
    dom = torch.empty(b, h, w, 32, device=x_nhwc.device)
    dw = torch.empty(9, cout, cin, device=x_nhwc.device)
    _launch("tmvs_dcn_backward_set", x_nhwc, offset_mask, w_taps, dy_nhwc, b, cin, cout, h, w,
            *_workspace("tmvs_dcn_backward_workspace", b, cout, h, w, device=x_nhwc.device), dx, dom, dw, far)
    if not capturing:
        ev = ent[2] or torch.cuda.Event()
        ev.record(cur)
        ent[1], ent[2] = cur, ev
    return dx, dom, dw


@_on_tensor_device
def nearest_up2_backward_nhwc(d, out=None):
    """tmvs_nearest_up2_backward_nhwc: d [n,2h,2w,C] -> [n,h,w,C] (accumulated into `out` when given)."""
    _dev(d, "d")
    n, h2, w2, c = d.shape
    if h2 % 2 or w2 % 2:
        raise ValueError("nearest_up2_backward_nhwc: d must be [n, 2h, 2w, C]")
    y = torch.empty(n, h2 // 2, w2 // 2, c, device=d.device) if out is None else out
    _launch("tmvs_nearest_up2_backward_nhwc", d, n, h2 // 2, w2 // 2, c, int(out is not None), y)
    return y


@_on_tensor_device
def softmax_backward(prob, dprob):
    """tmvs_softmax_backward: prob, dprob [B,D,H,W] -> d logits."""
    _dev(prob, "prob")
    _dev(dprob, "dprob")
    b, d, h, w = prob.shape
    out = torch.empty_like(prob)
    _launch("tmvs_softmax_backward", prob, dprob, b, d, h, w, out)
    return out


# ----------------------------------------------------------------- DTU evaluation (csrc/dtu_eval.hip)
def _dtu_t(t, name, dtype, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous {dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, not {tuple(t.shape)}")
    return t


def _dtu_xyz(t, name):
    _dtu_t(t, name, torch.float32)
    if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] == 0:
        raise ValueError(f"{name} must be [N, 3] with N >= 1")
    return t.shape[0]


def _dtu_host(values, n, name):
    a = np.ascontiguousarray(np.asarray(values, np.float64).reshape(-1))
    if a.size != n:
        raise ValueError(f"{name} must hold {n} numbers")
    return a


@_on_tensor_device
def dtu_cell_keys(xyz, grid):
    """tmvs_dtu_cell_keys: xyz [N,3] -> int64 [N] cell keys under grid = (origin x, y, z, cell edge)."""
    n = _dtu_xyz(xyz, "xyz")
    g = _dtu_host(grid, 4, "grid")
    keys = torch.empty(n, dtype=torch.int64, device=xyz.device)
    _launch("tmvs_dtu_cell_keys", xyz, n, g.ctypes.data, keys)
    return keys


@_on_tensor_device
def dtu_gather_points(xyz, order, payload=None):
    """tmvs_dtu_gather_points: float32 [N,4] records (xyz[order], int32 payload bits) in sorted order."""
    n = _dtu_xyz(xyz, "xyz")
    _dtu_t(order, "order", torch.int64, (n,))
    if payload is not None:
        _dtu_t(payload, "payload", torch.int32, (n,))
    pts = torch.empty(n, 4, dtype=torch.float32, device=xyz.device)
    _launch("tmvs_dtu_gather_points", xyz, order, payload, n, pts)
    return pts


@_on_tensor_device
def dtu_grid_table(sorted_keys, head_rank, n_cells):
    """tmvs_dtu_grid_table: the unique keys and run starts of ascending keys, as one int64 buffer."""
    _dtu_t(sorted_keys, "sorted_keys", torch.int64)
    n = sorted_keys.numel()
    _dtu_t(head_rank, "head_rank", torch.int64, (n,))
    nbytes = _lib_h().tmvs_dtu_grid_table_bytes(int(n_cells))
    if nbytes == 0:
        raise ValueError("dtu_grid_table: n_cells must be positive")
    table = torch.empty(nbytes // 8, dtype=torch.int64, device=sorted_keys.device)
    _launch("tmvs_dtu_grid_table", sorted_keys, head_rank, n, int(n_cells), table, nbytes)
    return table


@_on_tensor_device
def dtu_thin_round(points4, table, n_cells, grid, radius, state_in, state_out, undecided):
    """tmvs_dtu_thin_round: one round of the thinning; adds the points left undecided to `undecided`."""
    _dtu_t(points4, "points4", torch.float32)
    n = points4.shape[0]
    _dtu_t(table, "table", torch.int64)
    _dtu_t(state_in, "state_in", torch.uint8, (n,))
    _dtu_t(state_out, "state_out", torch.uint8, (n,))
    _dtu_t(undecided, "undecided", torch.int32, (1,))
    g = _dtu_host(grid, 4, "grid")
    if points4.dim() != 2 or points4.shape[1] != 4 or table.numel() * 8 < _lib_h().tmvs_dtu_grid_table_bytes(int(n_cells)):
        raise ValueError("dtu_thin_round: points4 must be [N, 4] and table must hold n_cells cells")
    _launch("tmvs_dtu_thin_round", points4, n, table, int(n_cells), g.ctypes.data, float(radius), state_in, state_out,
            undecided)


@_on_tensor_device
def dtu_nearest_pass(from4, to4, table, n_cells, grid, bb, max_dist, block, max_ring, skip_below, d2):
    """tmvs_dtu_nearest_pass: refine d2 [N_from] float64 in place against the to-points' grid."""
    _dtu_t(from4, "from4", torch.float32)
    _dtu_t(to4, "to4", torch.float32)
    _dtu_t(table, "table", torch.int64)
    if from4.dim() != 2 or from4.shape[1] != 4 or to4.dim() != 2 or to4.shape[1] != 4:
        raise ValueError("dtu_nearest_pass: from4 and to4 must be [N, 4]")
    _dtu_t(d2, "d2", torch.float64, (from4.shape[0],))
    if table.numel() * 8 < _lib_h().tmvs_dtu_grid_table_bytes(int(n_cells)):
        raise ValueError("dtu_nearest_pass: table must hold n_cells cells")
    g = _dtu_host(grid, 4, "grid")
    b = _dtu_host(bb, 6, "bb")
    _launch("tmvs_dtu_nearest_pass", from4, from4.shape[0], to4, to4.shape[0], table, int(n_cells), g.ctypes.data,
            b.ctypes.data, float(max_dist), float(block), int(max_ring), float(skip_below), d2)
    return d2


@_on_tensor_device
def dtu_in_mask(xyz, mask, bb_low, res):
    """tmvs_dtu_in_mask: xyz [N,3], mask uint8 [X,Y,Z] -> uint8 [N] (PointCompareMain.m:37-45)."""
    n = _dtu_xyz(xyz, "xyz")
    _dtu_t(mask, "mask", torch.uint8)
    if mask.dim() != 3 or mask.numel() == 0:
        raise ValueError("mask must be [X, Y, Z]")
    b = _dtu_host(bb_low, 3, "bb_low")
    out = torch.empty(n, dtype=torch.uint8, device=xyz.device)
    _launch("tmvs_dtu_in_mask", xyz, n, mask, *mask.shape, b.ctypes.data, float(res), out)
    return out


@_on_tensor_device
def dtu_above_plane(xyz, plane):
    """tmvs_dtu_above_plane: xyz [N,3], plane (4 numbers) -> uint8 [N] (PointCompareMain.m:57)."""
    n = _dtu_xyz(xyz, "xyz")
    p = _dtu_host(plane, 4, "plane")
    out = torch.empty(n, dtype=torch.uint8, device=xyz.device)
    _launch("tmvs_dtu_above_plane", xyz, n, p.ctypes.data, out)
    return out

