"""Torch-tensor wrappers over include/transmvs_view_select.h (csrc/view_select.hip): which views of a COLMAP
sparse model see which points, the depth of every observation, and MVSNet's view-selection score of every pair
of views. colmap_scene.py drives them. As in ops.py: device tensors and the current HIP stream in, status
checked, no CPU fallback.

Observations are int32 (view, point) pairs [M, 2] or two int32 [M] tensors; everything else is float64.
"""
from __future__ import annotations

import torch

from . import _lib, ops

MAX_BITS_BYTES = _lib.VS_MAX_BITS_BYTES  # the workspace cap: a [V][ceil(P / 64)] uint64 bit matrix above it is refused
MAX_POINTS = 2 ** 31 - 64


def _t(t, name, dtype, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous {dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, not {tuple(t.shape)}")
    return t


def words(n_points):
    """W: the 64-bit words of one view's row of the bit matrix."""
    return (int(n_points) + 63) // 64


def check_sizes(n_views, n_points):
    """What the C entries refuse with TMVS_ERR_SHAPE, with the reason spelled out."""
    n_views, n_points = int(n_views), int(n_points)
    if n_views < 2:
        raise ValueError(f"view selection needs at least 2 views, got {n_views}")
    if n_points < 1 or n_points >= MAX_POINTS:
        raise ValueError(f"view selection takes 1 <= points < 2^31 - 64, got {n_points}")
    nbytes = n_views * words(n_points) * 8
    if nbytes > MAX_BITS_BYTES:
        raise ValueError(f"the visibility bit matrix of {n_views} views x {n_points} points is {nbytes} bytes, above "
                         f"the workspace cap of {MAX_BITS_BYTES} (view_select.MAX_BITS_BYTES); split the model")


def _obs(obs_view, obs_point):
    _t(obs_view, "obs_view", torch.int32)
    if obs_view.dim() != 1 or obs_view.numel() == 0:
        raise ValueError("obs_view must be [M] with M >= 1")
    _t(obs_point, "obs_point", torch.int32, obs_view.shape)
    return obs_view.numel()


def _raise_on(errors, what):
    bad = int(errors.item())
    if bad:
        raise ValueError(f"{what}: {bad} observations name a view or a point outside the model")


@ops._on_tensor_device
def set_bits(obs_view, obs_point, n_views, n_points, bits=None):
    """tmvs_vs_set_bits: the [V, W] visibility bit matrix (int64 storage of the uint64 words) of the
    observations. `bits`, when given, must be zeroed. An index out of range raises ValueError and writes
    nothing for that observation."""
    m = _obs(obs_view, obs_point)
    check_sizes(n_views, n_points)
    shape = (int(n_views), words(n_points))
    if bits is None:
        bits = torch.zeros(shape, dtype=torch.int64, device=obs_view.device)
    _t(bits, "bits", torch.int64, shape)
    errors = torch.zeros(1, dtype=torch.int32, device=obs_view.device)
    ops._launch("tmvs_vs_set_bits", obs_view, obs_point, m, int(n_views), int(n_points), bits, errors)
    _raise_on(errors, "set_bits")
    return bits


@ops._on_tensor_device
def obs_depth(obs_view, obs_point, r3, tz, xyz):
    """tmvs_vs_obs_depth: z [M] float64, the camera-frame depth ((r0 x + r1 y) + r2 z) + tz of every
    observation; r3 [V, 3] the rotations' third rows, tz [V], xyz [P, 3]."""
    m = _obs(obs_view, obs_point)
    _t(r3, "r3", torch.float64)
    _t(xyz, "xyz", torch.float64)
    if r3.dim() != 2 or r3.shape[1] != 3 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("r3 must be [V, 3] and xyz [P, 3]")
    v, p = r3.shape[0], xyz.shape[0]
    _t(tz, "tz", torch.float64, (v,))
    check_sizes(v, p)
    z = torch.empty(m, dtype=torch.float64, device=obs_view.device)
    errors = torch.zeros(1, dtype=torch.int32, device=obs_view.device)
    ops._launch("tmvs_vs_obs_depth", obs_view, obs_point, m, v, p, r3, tz, xyz, z, errors)
    _raise_on(errors, "obs_depth")
    return z


@ops._on_tensor_device
def pair_scores(bits, n_points, centres, xyz, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """tmvs_vs_pair_scores: (scores [V, V] float64, counts [V, V] int32), symmetric with a zero diagonal, over
    the points both views of a pair see. bits [V, W] int64 as set_bits returns it; centres [V, 3]; xyz [P, 3]."""
    _t(bits, "bits", torch.int64)
    if bits.dim() != 2:
        raise ValueError("bits must be [V, W]")
    v = bits.shape[0]
    check_sizes(v, n_points)
    _t(bits, "bits", torch.int64, (v, words(n_points)))
    _t(centres, "centres", torch.float64, (v, 3))
    _t(xyz, "xyz", torch.float64, (int(n_points), 3))
    scores = torch.empty(v, v, dtype=torch.float64, device=bits.device)
    counts = torch.empty(v, v, dtype=torch.int32, device=bits.device)
    ops._launch("tmvs_vs_pair_scores", bits, v, int(n_points), centres, xyz, float(theta0), float(sigma1),
                float(sigma2), scores, counts)
    return scores, counts
