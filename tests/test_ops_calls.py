"""What every Python wrapper hands to the C-ABI, pinned on the CPU.

A recording stand-in replaces the library (the seams scripts/diag/dryrun.py uses: ops._lib_h, ops._dev,
ops._stream, _lib.check) and a recording timer is installed with ops.set_timer. Each wrapper of ops.py and
the call sites of reconstruct.py, fusion.py and dynamic_fusion.py is invoked once per branch with small CPU
tensors of distinct shapes, and for every library call the entry name, the timer spans open around it and
the arguments as ctypes converts them are compared with tests/golden/ops_calls.json. Integers and floats
are recorded as the library receives them; a pointer as NULL, stream / side_stream, in:<parameter> (a
tensor passed in), ret:<index> (a tensor returned), scratch:<numel> (another tensor of the wrapper's) or
host (a numpy or ctypes buffer).

    python tests/test_ops_calls.py --write     regenerates the golden file
"""
import contextlib
import ctypes
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from transmvsnet_amd import _lib, dynamic_fusion, fusion, ops, reconstruct  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "ops_calls.json")
STREAM, SIDE_STREAM = 0x57AE0, 0x51DE0  # what ops._stream() and the side stream's cuda_stream return here
WORKSPACE_BYTES = 4096  # every size query (restype size_t) answers this

# entries of _lib.SIGNATURES that the table below cannot reach, each with its reason
NOT_REACHED = {
    "tmvs_abi_version",       # called by _lib.load() alone, which the stand-in replaces
    "tmvs_status_string",     # called by _lib.check() on a failure alone
    "tmvs_fmt_kv",            # no Python caller: fmt_kv goes through tmvs_fmt_kv_grouped (kept for C callers)
    "tmvs_fmt_kv_workspace",  # no Python caller, as tmvs_fmt_kv
    "tmvs_fmt_apply",         # no Python caller: fmt_apply goes through tmvs_fmt_apply_tiled (kept for C callers)
}
# public names of ops.py that never reach the library
NO_LIBRARY_CALL = {"set_timer", "compose_proj", "proj_rows", "host_rot_order", "warp_flags", "prob_pack"}


# ------------------------------------------------------------------ the recording stand-in
def _tensors(value, path):
    """(path, tensor) of every tensor in value, through lists, tuples and dicts, in order"""
    if isinstance(value, torch.Tensor):
        yield path, value
    elif isinstance(value, (list, tuple)):
        for i, v in enumerate(value):
            yield from _tensors(v, f"{path}[{i}]")
    elif isinstance(value, dict):
        for k, v in value.items():
            yield from _tensors(v, f"{path}[{k}]")


class Recorder:
    """The library (attribute = entry point), the timer (begin / end) and the list of calls seen."""

    def __init__(self):
        self.calls, self.open = [], []

    # timer
    def begin(self, name):
        self.open.append(name)
        return len(self.open)

    def end(self, token):
        assert token == len(self.open), "timer spans must close in order"
        self.open.pop()

    # library
    def __getattr__(self, name):
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)
        restype, argtypes = _lib.SIGNATURES[name]

        def entry(*args):
            assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for {len(argtypes)} parameters"
            self.calls.append({"entry": name, "spans": list(self.open),
                               "args": [self._convert(name, i, a, t) for i, (a, t) in enumerate(zip(args, argtypes))],
                               "scratch": self._wrapper_tensors()})
            return WORKSPACE_BYTES if restype is _lib.S else 0
        return entry

    @staticmethod
    def _convert(name, i, a, ctype):
        """the value the library would receive; ctypes' own from_param rejects what the real call would"""
        try:
            ctype.from_param(a)
        except (TypeError, ctypes.ArgumentError) as e:
            raise TypeError(f"{name}: argument {i} ({a!r}) does not convert to {ctype.__name__}") from e
        if ctype is _lib.P:
            if a is None:
                return ("ptr", 0)
            if isinstance(a, ctypes.c_void_p):
                return ("ptr", a.value or 0)
            if isinstance(a, int):
                return ("ptr", a)
            return "host"  # ctypes.byref(...) or a ctypes array
        value = a.value if isinstance(a, ctypes._SimpleCData) else a
        if ctype is _lib.F:
            return ctypes.c_float(value).value
        if ctype is _lib.D:
            return float(value)
        assert isinstance(value, int), f"{name}: argument {i} ({a!r}) is no integer"
        return int(value)

    @staticmethod
    def _wrapper_tensors():
        """data_ptr -> numel of the tensors alive in the package's frames above the library call"""
        found = {}
        frame = sys._getframe(2)
        while frame is not None:
            if frame.f_globals.get("__name__", "").startswith("transmvsnet_amd"):
                for _, t in _tensors(list(frame.f_locals.values()), ""):
                    found.setdefault(t.data_ptr(), t.numel())
            frame = frame.f_back
        return found


def _resolve(calls, bound, result):
    """name the raw pointers of `calls` once the wrapper has returned"""
    names = {}
    for i, (_, t) in reversed(list(enumerate(_tensors(result, "")))):
        names[t.data_ptr()] = f"ret:{i}"
    for param, value in reversed(list(bound.items())):
        for path, t in reversed(list(_tensors(value, param))):
            names[t.data_ptr()] = f"in:{path}"
    names.update({0: "NULL", STREAM: "stream", SIDE_STREAM: "side_stream"})
    out = []
    for c in calls:
        scratch = c.pop("scratch")
        c["args"] = [a if not isinstance(a, tuple) else
                     names.get(a[1]) or (f"scratch:{scratch[a[1]]}" if a[1] in scratch else "host") for a in c["args"]]
        out.append(c)
    return out


class _FakeStream:
    cuda_stream = STREAM

    def wait_event(self, event):
        pass

    def __eq__(self, other):
        return isinstance(other, _FakeStream)

    __hash__ = None


class _SideStream:
    cuda_stream = SIDE_STREAM


class _FakeEvent:
    def record(self, stream=None):
        pass


def _relaxed_dev(t, name):
    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
        raise RuntimeError(f"{name} must be contiguous float32")


def _check(status, what):
    assert status == 0, what


def _install(mp, rec):
    """The stand-in library behind every seam, CPU tensors accepted as device tensors, and the torch.cuda
    calls of the wrappers (fmt_forward's side stream, dcn_backward_set, the device guards) answered without
    a GPU. `mp` (pytest's MonkeyPatch) restores everything."""
    mp.setattr(ops, "_lib_h", lambda: rec)
    mp.setattr(ops, "_dev", _relaxed_dev)
    mp.setattr(ops, "_stream", lambda: STREAM)
    mp.setattr(ops, "_DCN_FAR", {})
    mp.setattr(_lib, "check", _check)
    for module in (reconstruct, fusion, dynamic_fusion):
        mp.setattr(module, "load", lambda: rec, raising=False)
        mp.setattr(module, "check", _check, raising=False)
    mp.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    mp.setattr(torch.Tensor, "record_stream", lambda self, stream: None, raising=False)
    mp.setattr(torch.cuda, "current_device", lambda: None)  # == torch.device("cpu").index: no device switch
    mp.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    mp.setattr(torch.cuda, "current_stream", lambda device=None: _FakeStream())
    mp.setattr(torch.cuda, "Event", _FakeEvent)


# ------------------------------------------------------------------ one invocation per wrapper and branch
def _t(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def _eye(*lead):
    return torch.eye(4).expand(*lead, 4, 4).contiguous()


def _weights():
    w = _lib.CostRegWeights()
    w.base_ch = 8
    return w


def _table():
    """(id, function, keyword arguments)"""
    f32 = np.float32
    i32, i64, u8, f64 = torch.int32, torch.int64, torch.uint8, torch.float64
    bn4 = lambda c=8, g=None: dict(mean=_t(*((c,) if g is None else (g, c))), var=_t(*((c,) if g is None else (g, c))),  # noqa: E731
                                   gamma=_t(c), beta=_t(c), eps=1e-5)
    dcn_x = lambda: dict(x_nhwc=_t(1, 5, 7, 32), wom_packed=_t(101), bom=_t(27), w_packed=_t(103), bias=_t(8), cout=8)  # noqa: E731
    pw_back = lambda *b: dict(sims=_t(*b, 2, 4, 6, 10), pwp=_t(201), stats=_t(2, 48), view_w=_t(*b, 2, 6, 10),  # noqa: E731
                              dstar=_t(*b, 2, 6, 10, dtype=i32), dview_w=_t(*b, 2, 6, 10), dsims=_t(*b, 2, 4, 6, 10))
    entropy = lambda dv: dict(prob=_t(2, 4, 5, 7), depth_values=dv, depth_gt=_t(2, 5, 7), mask=_t(2, 5, 7))  # noqa: E731
    outputs = lambda: {"depth": _t(1, 8, 12), "photo_confidence": _t(1, 8, 12),  # noqa: E731
                       "stage2": {"photo_confidence": _t(1, 4, 6)}, "stage1": {"photo_confidence": _t(1, 2, 3)}}
    cams = np.stack([np.eye(3, dtype=f32)] * 3), np.stack([np.eye(4, dtype=f32)] * 3)
    return [
        ("bn_fold", ops.bn_fold, dict(gamma=_t(8), beta=_t(8), mean=_t(8), var=_t(8), eps=1e-3)),
        ("stage_hypotheses/first", ops.stage_hypotheses,
         dict(depth_values=_t(2, 5), prev_depth=None, ndepth=4, ratio=2.0, full_hw=(8, 12), stage_scale=4)),
        ("stage_hypotheses/prev", ops.stage_hypotheses,
         dict(depth_values=_t(2, 5), prev_depth=_t(2, 4, 6), ndepth=3, ratio=0.7, full_hw=(8, 12), stage_scale=2)),
        ("warp_corr/stage1", ops.warp_corr,
         dict(ref_nhwc=_t(1, 6, 10, 8), src_nhwc=_t(1, 2, 6, 10, 8), proj12=np.zeros((1, 2, 12), f32), hyp=_t(1, 4, 6, 10),
              pw_params=np.zeros(201, f32), rot_order="plain")),
        ("warp_corr/weights_partial", ops.warp_corr,
         dict(ref_nhwc=_t(1, 6, 10, 8), src_nhwc=_t(1, 2, 6, 10, 8), proj12=np.zeros((1, 2, 12), f32), hyp=_t(1, 4, 6, 10),
              view_w_in=_t(1, 3, 3, 5), vw_shift=1, vw_offset=1, vw_total=3, partial=True, rot_order="fma")),
        ("warp_corr/outputs_given", ops.warp_corr,
         dict(ref_nhwc=_t(1, 6, 10, 8), src_nhwc=_t(1, 2, 6, 10, 8), proj12=np.zeros((1, 2, 12), f32), hyp=_t(1, 4, 6, 10),
              pw_params=np.zeros(201, f32), partial=True, view_w_out=_t(1, 2, 6, 10), sim_out=_t(1, 4, 6, 10),
              wsum_out=_t(1, 6, 10), rot_order="fma")),
        ("aggregate_finalize", ops.aggregate_finalize, dict(sim_sum=_t(2, 4, 5, 7), w_sum=_t(2, 5, 7))),
        ("homo_warping", ops.homo_warping,
         dict(src_fea=_t(1, 8, 5, 7), src_proj=_eye(1), ref_proj=_eye(1), depth_values=_t(1, 4), rot_order="plain")),
        ("softmax_wta", ops.softmax_wta, dict(logits=_t(2, 4, 5, 7), hyp=_t(2, 4, 5, 7), clamp=(1.5, 9.25))),
        ("costregnet", ops.costregnet, dict(x=_t(2, 4, 6, 8), weights=_weights())),
        ("costregnet_wta", ops.costregnet_wta, dict(x=_t(2, 4, 6, 8), weights=_weights(), hyp=_t(2, 4, 6, 8), clamp=(1.5, 9.25))),
        ("conv3d_bn_relu/stride1_out", ops.conv3d_bn_relu,
         dict(x=_t(1, 2, 4, 6, 8), wpk=_t(27 * 16 * 8), alpha=_t(16), shift=_t(17), cout=16, stride=1, out=_t(1, 2, 4, 6, 16))),
        ("conv3d_bn_relu/stride2_raw", ops.conv3d_bn_relu,
         dict(x=_t(1, 2, 4, 6, 8), wpk=_t(27 * 16 * 8), alpha=None, shift=None, cout=16, stride=2)),
        *[(f"deconv3d_bn_relu_add/{route}", ops.deconv3d_bn_relu_add,
           dict(x=_t(1, 2, 3, 4, 16), wpk=_t(27 * 8 * 16), alpha=_t(8), shift=_t(9), cout=8, skip=_t(1, 4, 6, 8, 8), route=route,
                max_workgroups=5)) for route in (None, "generic", "persistent")],
        ("deconv3d_bn_relu_add/out", ops.deconv3d_bn_relu_add,
         dict(x=_t(1, 2, 3, 4, 16), wpk=_t(27 * 8 * 16), alpha=_t(8), shift=_t(9), cout=8, skip=_t(1, 4, 6, 8, 8),
              out=_t(1, 4, 6, 8, 8))),
        ("fmt_embed", ops.fmt_embed, dict(feat_nchw=_t(2, 32, 4, 6), pe=_t(32, 8, 10), out_tokens=_t(2, 24, 32))),
        ("fmt_kv", ops.fmt_kv, dict(source_tokens=_t(2, 24, 32), enc_w=_t(64))),
        ("fmt_kv/grouped_out", ops.fmt_kv, dict(source_tokens=_t(2, 24, 32), enc_w=_t(64), out=_t(2, 160), group_nv=5)),
        ("fmt_apply", ops.fmt_apply, dict(x_tokens=_t(2, 24, 32), kv=_t(2, 160), enc_w=_t(64))),
        ("fmt_apply/shared_tiled", ops.fmt_apply,
         dict(x_tokens=_t(2, 24, 32), kv=_t(1, 160), enc_w=_t(64), shared_kv=True, tiles_per_wave=3)),
        ("fmt_pathway", ops.fmt_pathway,
         dict(coarse_nhwc=_t(2, 3, 4, 32), lateral_nchw=_t(2, 16, 6, 8), w_reduce=_t(65), w_smooth=_t(66))),
        ("fmt_pathway/out", ops.fmt_pathway,
         dict(coarse_nhwc=_t(2, 3, 4, 32), lateral_nchw=_t(2, 16, 6, 8), w_reduce=_t(65), w_smooth=_t(66), out=_t(2, 6, 8, 16))),
        ("fmt_forward", ops.fmt_forward,
         dict(stage1_nchw=_t(3, 32, 4, 6), pe=_t(32, 8, 10), enc_list=[_t(16) for _ in range(8)])),
        ("fmt_forward/side_stream", ops.fmt_forward,
         dict(stage1_nchw=_t(3, 32, 4, 6), pe=_t(32, 8, 10), enc_list=[_t(16) for _ in range(8)], tokens=_t(3, 24, 32),
              side_stream=_SideStream())),
        ("depth_stage/stage1", ops.depth_stage,
         dict(depth_values=_t(1, 5), prev_depth=None, feat_nhwc=_t(3, 6, 10, 8), ndepth=4, ratio=2.0, full_hw=(24, 40),
              stage_scale=4, proj12=np.zeros((2, 12), f32), pw_params=np.zeros(201, f32), view_w=_t(2, 6, 10), vw_shift=0,
              cr_weights=_weights(), clamp=(1.5, 9.25), rot_order="plain")),
        ("depth_stage/later", ops.depth_stage,
         dict(depth_values=_t(1, 5), prev_depth=_t(1, 3, 5), feat_nhwc=_t(3, 6, 10, 8), ndepth=4, ratio=0.7, full_hw=(12, 20),
              stage_scale=2, proj12=np.zeros((2, 12), f32), pw_params=None, view_w=_t(2, 3, 5), vw_shift=1,
              cr_weights=_weights(), rot_order="fma")),
        ("deform_conv2d_pack", ops.deform_conv2d_pack, dict(weight=_t(8, 32, 3, 3))),
        ("deform_conv2d", ops.deform_conv2d,
         dict(x_nhwc=_t(1, 5, 7, 32), offset_mask=_t(1, 27, 5, 7), w_packed=_t(103), bias=_t(8), cout=8)),
        ("deform_conv2d/bn_relu_nhwc", ops.deform_conv2d,
         dict(x_nhwc=_t(1, 5, 7, 32), offset_mask=_t(1, 27, 5, 7), w_packed=_t(103), bias=_t(8), cout=8, bn=(_t(8), _t(9)),
              relu=True, want_nhwc=True)),
        ("dcn_fused/nchw", ops.dcn_fused, dict(dcn_x())),
        ("dcn_fused/bn_relu_nhwc", ops.dcn_fused, dict(dcn_x(), bn=(_t(8), _t(9)), relu=True, want_nchw=False, want_nhwc=True)),
        ("conv3x3_nhwc", ops.conv3x3_nhwc, dict(x_nhwc=_t(1, 5, 7, 32), w_packed=_t(67))),
        ("conv3x3_nhwc/bn_relu_bias_nchw", ops.conv3x3_nhwc,
         dict(x_nhwc=_t(1, 5, 7, 32), w_packed=_t(67), bn=(_t(32), _t(33)), relu=True, bias=_t(34), want_nchw=True,
              want_nhwc=False)),
        ("conv3x3_nhwc_acc", ops.conv3x3_nhwc_acc, dict(x_nhwc=_t(1, 5, 7, 32), w_packed=_t(67), out_nhwc=_t(1, 5, 7, 32))),
        ("fpn_merge", ops.fpn_merge, dict(prev_nhwc=_t(1, 3, 4, 32), lat_nhwc=_t(1, 6, 8, 16), w_inner=_t(32, 16), b_inner=_t(32))),
        ("conv2d_pack", ops.conv2d_pack, dict(weight=_t(8, 3, 5, 5))),
        ("conv2d_bn_relu", ops.conv2d_bn_relu, dict(x=_t(1, 5, 7, 3), w_packed=_t(68), cout=8, k=3, stride=1)),
        ("conv2d_bn_relu/nchw_bn", ops.conv2d_bn_relu,
         dict(x=_t(1, 3, 6, 8), w_packed=_t(68), cout=8, k=5, stride=2, bn=(_t(8), _t(9)), relu=False, nchw_input=True)),
        ("entropy_loss/per_pixel", ops.entropy_loss, entropy(_t(2, 4, 5, 7))),
        ("entropy_loss/per_sample_grad", ops.entropy_loss, dict(entropy(_t(2, 4)), grad_scale=0.5, want_grad=True)),
        ("entropy_loss/outputs_given", ops.entropy_loss,
         dict(entropy(_t(2, 4)), grad_scale=0.25, want_grad=True, wta=_t(2, 5, 7), conf=_t(2, 5, 7), grad=_t(2, 4, 5, 7))),
        ("depth_metrics", ops.depth_metrics, dict(depth=_t(2, 5, 7), depth_gt=_t(2, 5, 7), mask=_t(2, 5, 7), depth_interval=2.5)),
        ("depth_eval_metrics", ops.depth_eval_metrics, dict(depth_est=_t(2, 5, 7), depth_gt=_t(2, 5, 7), mask=_t(2, 5, 7))),
        ("depth_eval_metrics/out", ops.depth_eval_metrics,
         dict(depth_est=_t(2, 5, 7), depth_gt=_t(2, 5, 7), mask=_t(2, 5, 7), out=_t(12))),
        ("gt_pyramid/bld", ops.gt_pyramid, dict(depth_raw=_t(8, 12), rows=_t(14, dtype=i32), cols=_t(21, dtype=i32))),
        ("gt_pyramid/dtu", ops.gt_pyramid,
         dict(depth_raw=_t(16, 28), rows=_t(14, dtype=i32), cols=_t(21, dtype=i32), mode="dtu", depth_min=1.5, depth_end=9.25,
              mask_png=_t(16, 28, dtype=u8), target_hw=(8, 12))),
        ("conv3d_generic", ops.conv3d_generic, dict(x=_t(1, 2, 4, 6, 8), w_packed=_t(27 * 16 * 8), cout=16, out_dhw=(2, 4, 6), stride=1)),
        ("conv3d_generic/transposed_acc", ops.conv3d_generic,
         dict(x=_t(1, 2, 3, 4, 16), w_packed=_t(27 * 8 * 16), cout=8, out_dhw=(4, 6, 8), stride=2, transposed=True,
              out=_t(1, 4, 6, 8, 8))),
        ("conv3d_mfma", ops.conv3d_mfma, dict(x=_t(1, 2, 4, 6, 8), w_packed=_t(27, 16, 8), cout=16, stride=2)),
        ("conv3d_mfma/transposed_skip_out", ops.conv3d_mfma,
         dict(x=_t(1, 2, 3, 4, 16), w_packed=_t(27, 8, 16), cout=8, stride=2, transposed=True, skip=_t(1, 4, 6, 8, 8),
              out=_t(1, 4, 6, 8, 8))),
        ("conv3d_mfma/prob", ops.conv3d_mfma, dict(x=_t(1, 2, 4, 6, 8), w_packed=_t(3, 72), cout=1, stride=1)),
        ("conv3d_wgrad", ops.conv3d_wgrad, dict(direct=_t(1, 2, 4, 6, 16), gathered=_t(1, 3, 5, 7, 8), stride=1)),
        ("bn_stats", ops.bn_stats, dict(z=_t(2, 3, 4, 8))),
        ("bn_relu_train", ops.bn_relu_train, dict(z=_t(2, 3, 4, 8), **bn4())),
        ("bn_relu_train/skip_out", ops.bn_relu_train, dict(z=_t(2, 3, 4, 8), **bn4(), skip=_t(2, 3, 4, 8), out=_t(2, 3, 4, 8))),
        ("bn_relu_backward", ops.bn_relu_backward, dict(dy=_t(2, 3, 4, 8), z=_t(2, 3, 4, 8), **bn4())),
        ("bn_relu_backward/dz", ops.bn_relu_backward, dict(dy=_t(2, 3, 4, 8), z=_t(2, 3, 4, 8), **bn4(), dz=_t(2, 3, 4, 8))),
        ("bn_stats_grouped", ops.bn_stats_grouped, dict(z=_t(2, 3, 4, 8))),
        ("bn_relu_train_grouped", ops.bn_relu_train_grouped, dict(z=_t(2, 3, 4, 8), **bn4(g=2))),
        ("bn_relu_backward_grouped", ops.bn_relu_backward_grouped, dict(dy=_t(2, 3, 4, 8), z=_t(2, 3, 4, 8), **bn4(g=2))),
        ("warp_corr_backward", ops.warp_corr_backward,
         dict(ref_nhwc=_t(3, 4, 8), src_nhwc=_t(2, 3, 4, 8), proj12=np.zeros((2, 12), f32), hyp=_t(5, 3, 4), dsim=_t(2, 5, 3, 4),
              rot_order="plain")),
        ("warp_corr_backward/planes_outputs_given", ops.warp_corr_backward,
         dict(ref_nhwc=_t(3, 4, 8), src_nhwc=_t(2, 3, 4, 8), proj12=np.zeros((2, 12), f32), hyp=_t(5, 3, 4), dsim=_t(2, 5, 3, 4),
              rot_order="fma", planes=True, dref_out=_t(3, 4, 8), dsrc_out=_t(2, 3, 4, 8))),
        ("pixelwise_train_forward", ops.pixelwise_train_forward, dict(sims=_t(2, 4, 6, 10), pwp=_t(201))),
        ("aggregate_train", ops.aggregate_train, dict(sims=_t(2, 4, 6, 10), view_w=_t(2, 3, 5), vw_shift=1)),
        ("aggregate_train/sim", ops.aggregate_train, dict(sims=_t(2, 4, 6, 10), view_w=_t(2, 6, 10), vw_shift=0, sim=_t(4, 6, 10))),
        ("aggregate_train_backward", ops.aggregate_train_backward,
         dict(dsim=_t(4, 6, 10), sims=_t(2, 4, 6, 10), sim=_t(4, 6, 10), wsum=_t(6, 10), view_w=_t(2, 3, 5), vw_shift=1,
              want_dview_w=True)),
        ("aggregate_train_backward/no_dview_w_dsims", ops.aggregate_train_backward,
         dict(dsim=_t(4, 6, 10), sims=_t(2, 4, 6, 10), sim=_t(4, 6, 10), wsum=_t(6, 10), view_w=_t(2, 6, 10), vw_shift=0,
              want_dview_w=False, dsims=_t(2, 4, 6, 10))),
        ("pixelwise_train_backward", ops.pixelwise_train_backward, pw_back()),
        ("pixelwise_train_forward_batched", ops.pixelwise_train_forward_batched, dict(sims=_t(3, 2, 4, 6, 10), pwp=_t(201))),
        ("pixelwise_train_backward_batched", ops.pixelwise_train_backward_batched, pw_back(3)),
        ("upsample2_add_nhwc", ops.upsample2_add_nhwc, dict(r=_t(2, 3, 4, 8), lateral_nchw=_t(2, 8, 6, 8))),
        ("upsample2_backward_nhwc", ops.upsample2_backward_nhwc, dict(du=_t(2, 6, 8, 16))),
        ("token_linear", ops.token_linear, dict(x=_t(5, 6), w=_t(7, 6))),
        ("token_linear/bias_transposed_relu_acc", ops.token_linear,
         dict(x=_t(5, 6), w=_t(6, 7), b=_t(7), transpose_w=True, relu_of=_t(5, 7), out=_t(5, 7))),
        ("token_linear/residual", ops.token_linear, dict(x=_t(5, 6), w=_t(7, 6), residual=_t(5, 7))),
        ("token_linear/residual_bias_transposed_relu", ops.token_linear,
         dict(x=_t(5, 6), w=_t(6, 7), b=_t(7), transpose_w=True, relu_of=_t(5, 7), residual=_t(5, 7))),
        ("token_wgrad", ops.token_wgrad, dict(dy=_t(5, 7), x=_t(5, 6))),
        ("token_wgrad/acc", ops.token_wgrad, dict(dy=_t(5, 7), x=_t(5, 6), dw=_t(7, 6), db=_t(7))),
        ("layer_norm_fwd", ops.layer_norm_fwd, dict(x=_t(5, 32), g=_t(32), b=_t(33))),
        ("layer_norm_bwd", ops.layer_norm_bwd, dict(dy=_t(5, 32), x=_t(5, 32), g=_t(32))),
        ("layer_norm_bwd/acc", ops.layer_norm_bwd, dict(dy=_t(5, 32), x=_t(5, 32), g=_t(32), dgb=_t(64))),
        ("linattn_fwd", ops.linattn_fwd, dict(q=_t(6, 32), kv=_t(2, 160), tokens_per_group=3)),
        ("linattn_fwd/shared", ops.linattn_fwd, dict(q=_t(6, 32), kv=_t(1, 160), tokens_per_group=6)),
        ("linattn_bwd_q", ops.linattn_bwd_q, dict(q=_t(6, 32), dmsg=_t(6, 32), kv=_t(2, 160), tokens_per_group=3)),
        ("linattn_bwd_kv", ops.linattn_bwd_kv, dict(k=_t(6, 32), v=_t(6, 32), dkv=_t(2, 160), tokens_per_group=3)),
        ("adam_step", ops.adam_step,
         dict(param_flat=_t(10), grad_flat=_t(10), exp_avg=_t(10), exp_avg_sq=_t(10), lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
              weight_decay=0.01, step=7)),
        ("adam_step_dev", ops.adam_step_dev,
         dict(param_flat=_t(10), grad_flat=_t(10), exp_avg=_t(10), exp_avg_sq=_t(10), lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
              weight_decay=0.01, step_counter=_t(1, dtype=i32), scalars=_t(4))),
        ("adam_step_dev/lr_dev", ops.adam_step_dev,
         dict(param_flat=_t(10), grad_flat=_t(10), exp_avg=_t(10), exp_avg_sq=_t(10), lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
              weight_decay=0.01, step_counter=_t(1, dtype=i32), scalars=_t(4), lr_dev=_t(1, dtype=f64))),
        ("conv2d_generic", ops.conv2d_generic,
         dict(x=_t(1, 5, 7, 3), w_taps=_t(9 * 4 * 3), cout=4, out_hw=(5, 7), k=3, stride=1, pad=1, bias=_t(4))),
        ("conv2d_generic/transposed_acc", ops.conv2d_generic,
         dict(x=_t(1, 5, 7, 3), w_taps=_t(25 * 4 * 3), cout=4, out_hw=(10, 14), k=5, stride=2, pad=2, transposed=True,
              out=_t(1, 10, 14, 4))),
        ("conv2d_wgrad", ops.conv2d_wgrad, dict(direct=_t(1, 5, 7, 4), gathered=_t(1, 9, 13, 3), k=5, stride=2, pad=1)),
        ("colsum", ops.colsum, dict(x=_t(3, 5, 8))),
        ("dcn_forward_train", ops.dcn_forward_train, dcn_x()),
        ("dcn_forward_train/nchw", ops.dcn_forward_train, dict(dcn_x(), want_nchw=True)),
        ("dcn_backward", ops.dcn_backward,
         dict(x_nhwc=_t(1, 5, 7, 32), offset_mask=_t(1, 27, 5, 7), w_taps=_t(9, 8, 32), dy_nhwc=_t(1, 5, 7, 8),
              dx_nhwc=_t(1, 5, 7, 32))),
        ("dcn_backward_set", ops.dcn_backward_set,
         dict(x_nhwc=_t(1, 5, 7, 32), offset_mask=_t(1, 27, 5, 7), w_taps=_t(9, 8, 32), dy_nhwc=_t(1, 5, 7, 8))),
        ("nearest_up2_backward_nhwc", ops.nearest_up2_backward_nhwc, dict(d=_t(2, 4, 6, 8))),
        ("nearest_up2_backward_nhwc/acc", ops.nearest_up2_backward_nhwc, dict(d=_t(2, 4, 6, 8), out=_t(2, 2, 3, 8))),
        ("softmax_backward", ops.softmax_backward, dict(prob=_t(2, 4, 5, 7), dprob=_t(2, 4, 5, 7))),
        ("dtu_cell_keys", ops.dtu_cell_keys, dict(xyz=_t(5, 3), grid=(0.0, 0.0, 0.0, 1.0))),
        ("dtu_gather_points", ops.dtu_gather_points, dict(xyz=_t(5, 3), order=_t(5, dtype=i64))),
        ("dtu_gather_points/payload", ops.dtu_gather_points,
         dict(xyz=_t(5, 3), order=_t(5, dtype=i64), payload=_t(5, dtype=i32))),
        ("dtu_grid_table", ops.dtu_grid_table, dict(sorted_keys=_t(5, dtype=i64), head_rank=_t(5, dtype=i64), n_cells=3)),
        ("dtu_thin_round", ops.dtu_thin_round,
         dict(points4=_t(5, 4), table=_t(512, dtype=i64), n_cells=3, grid=(0.0, 0.0, 0.0, 1.0), radius=0.2,
              state_in=_t(5, dtype=u8), state_out=_t(5, dtype=u8), undecided=_t(1, dtype=i32))),
        ("dtu_nearest_pass", ops.dtu_nearest_pass,
         dict(from4=_t(5, 4), to4=_t(6, 4), table=_t(512, dtype=i64), n_cells=3, grid=(0.0, 0.0, 0.0, 1.0), bb=(0.0,) * 6,
              max_dist=20.0, block=60.0, max_ring=2, skip_below=-1.0, d2=_t(5, dtype=f64))),
        ("dtu_in_mask", ops.dtu_in_mask, dict(xyz=_t(5, 3), mask=_t(2, 3, 4, dtype=u8), bb_low=(0.0, 0.0, 0.0), res=0.5)),
        ("dtu_above_plane", ops.dtu_above_plane, dict(xyz=_t(5, 3), plane=(0.0, 0.0, 1.0, 0.0))),
        ("reconstruct.postprocess_view", reconstruct.postprocess_view,
         dict(outputs=outputs(), conf_threshold=0.25, depth_min=1.5, depth_max=9.25)),
        ("reconstruct.postprocess_view/image", reconstruct.postprocess_view, dict(outputs=outputs(), image=_t(3, 8, 12))),
        ("reconstruct.resize_image/u8", reconstruct.resize_image, dict(src=_t(5, 7, 3, dtype=u8), new_w=9, new_h=11)),
        ("reconstruct.resize_image/f32", reconstruct.resize_image, dict(src=_t(2, 5, 7), new_w=9, new_h=11)),
        ("fusion.fuse", fusion.fuse,
         dict(rgbd=_t(2, 5, 7, 4), cams_packed=np.zeros((2, fusion.CAM_FLOATS), f32), consistent_threshold=2,
              depth_threshold=0.5)),
        ("dynamic_fusion.filter_view", dynamic_fusion.filter_view,
         dict(depths=_t(3, 5, 7), confidence=_t(5, 7), Ks=cams[0], Es=cams[1], ref=1, srcs=[2, 0], photo_threshold=0.25,
              thres_view=2, subpixel_bits=0)),
    ]


def record():
    """{invocation id: {"calls": [...], "returns": [...]}} under the stand-in library."""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        rec = Recorder()
        _install(mp, rec)
        ops.set_timer(rec)
        try:
            for name, fn, kwargs in _table():
                rec.calls = []
                result = fn(**kwargs)
                assert not rec.open, f"{name}: a timer span was left open"
                bound = inspect.signature(fn).bind(**kwargs).arguments
                out[name] = {"function": f"{fn.__module__.rsplit('.', 1)[-1]}.{fn.__name__}",
                             "calls": _resolve(rec.calls, bound, result),
                             "returns": [[str(t.dtype).replace("torch.", ""), list(t.shape)] for _, t in _tensors(result, "")]}
        finally:
            ops.set_timer(None)
    return out


@pytest.fixture(scope="module")
def recorded():
    return record()


def test_wrappers_send_what_the_golden_file_records(recorded):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = json.loads(json.dumps(recorded))
    assert list(got) == list(golden), "the invocation table and the golden file list different invocations"
    for name in golden:
        assert got[name] == golden[name], name


def test_every_entry_and_every_wrapper_is_recorded(recorded):
    got = recorded
    entries = {c["entry"] for inv in got.values() for c in inv["calls"]}
    assert entries == set(_lib.SIGNATURES) - NOT_REACHED
    invoked = {inv["function"] for inv in got.values()}
    public = {f"ops.{n}" for n, fn in vars(ops).items()
              if not n.startswith("_") and inspect.isfunction(fn) and fn.__module__ == ops.__name__}
    assert public - invoked == {f"ops.{n}" for n in NO_LIBRARY_CALL}
    for n in NO_LIBRARY_CALL:  # and those really hold no call
        src = inspect.getsource(inspect.unwrap(getattr(ops, n)))
        assert "_lib_h" not in src and "_call(" not in src and "_launch(" not in src, n


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    written = record()
    with open(GOLDEN, "w") as f:
        json.dump(written, f, indent=1, sort_keys=False)
        f.write("\n")
    print(f"{GOLDEN}: {len(written)} invocations, {sum(len(v['calls']) for v in written.values())} library calls")
