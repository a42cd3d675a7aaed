"""What the native heads share on the host: a camera rig's validated geometry (``Rig``) and the check of a
per-view tensor argument (``check_views``).  Plain Python over torch CPU tensors; nothing here touches the GPU."""
from __future__ import annotations

import torch

from .geometry import kornia_src_norm_from_dst_norm

MAX_VIEWS = 16  # kWarpMaxViews (csrc/warp_common.h), kIhMaxViews (csrc/img_head.hip)


def norm_matrices(mats, src_hw, grid_hw) -> torch.Tensor:
    """[N,3,3] fp32: the matrix kornia hands to transform_points for each view, from the fp32-cast projection
    matrix as ``persp_trans_detector.py:67-69`` feeds kornia (``normalize_homography`` + ``_torch_inverse_cast``)."""
    return torch.stack([kornia_src_norm_from_dst_norm(M.float().reshape(1, 3, 3), src_hw, grid_hw)[0] for M in mats])


class Rig:
    """One camera rig: ``proj_mats`` the reference's per-camera 3x3 matrices (source pixels -> grid pixels),
    ``upsample_shape`` (H, W) of the warp's source, ``reducedgrid_shape`` (Ho, Wo).  Holds ``up_hw``, ``grid_hw``,
    ``num_views``, ``mats``, the normalised matrices ``m_norm_cpu`` and a keyed cache of what a head derives from
    the geometry alone (adjoint plans, frustum boxes)."""

    def __init__(self, proj_mats, upsample_shape, reducedgrid_shape):
        if isinstance(proj_mats, torch.Tensor) or not hasattr(proj_mats, "__len__"):
            raise TypeError(f"proj_mats must be a sequence of 3x3 matrices, got {type(proj_mats).__name__}")
        if not 0 < len(proj_mats) <= MAX_VIEWS:
            raise ValueError(f"1 .. {MAX_VIEWS} views, got {len(proj_mats)}")
        try:
            self.up_hw = tuple(int(s) for s in upsample_shape)
            self.grid_hw = tuple(int(s) for s in reducedgrid_shape)
        except (TypeError, ValueError):
            raise TypeError("upsample_shape and reducedgrid_shape must be (rows, columns)") from None
        if len(self.up_hw) != 2 or len(self.grid_hw) != 2 or min(self.up_hw + self.grid_hw) <= 0:
            raise ValueError(f"sizes must be two positive integers, got {upsample_shape!r} and {reducedgrid_shape!r}")
        self.mats = [torch.as_tensor(M) for M in proj_mats]
        for i, M in enumerate(self.mats):
            if tuple(M.shape) != (3, 3):
                raise ValueError(f"proj_mats[{i}] must be 3x3, got {tuple(M.shape)}")
        self.m_norm_cpu = norm_matrices(self.mats, self.up_hw, self.grid_hw)
        self.num_views = len(self.mats)
        self._cache = {}

    def cached(self, key, make):
        """``make()`` once per ``key``."""
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]


def check_views(name, views, head, n_views, params, shape_error, params_on_device=True):
    """The checks every head makes of its per-view argument ``views`` (called ``name`` in the messages): a
    sequence of 1 .. 16 float32 tensors (``n_views`` of them unless None) of one shape for which ``shape_error(t)`` is
    None (else what the view "must be"), on one ROCm GPU (``head`` names the caller in that message), none empty.
    ``params``: (name, tensor) pairs that go through the same dtype and, with ``params_on_device``, device checks."""
    if isinstance(views, torch.Tensor) or not hasattr(views, "__len__"):
        raise TypeError(f"{name} must be a sequence of tensors, got {type(views).__name__}")
    if not 0 < len(views) <= MAX_VIEWS:
        raise ValueError(f"1 .. {MAX_VIEWS} views per call, got {len(views)}")
    if n_views is not None and len(views) != n_views:
        raise ValueError(f"{len(views)} views for a head built for {n_views}")
    named = [(f"{name}[{i}]", t) for i, t in enumerate(views)]
    for k, t in named + list(params):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{k} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{k} must be float32, got {t.dtype}")
    v0 = views[0]
    for k, t in named:
        if shape_error(t) is not None:
            raise ValueError(f"{k} must be {shape_error(t)}")
        if t.shape != v0.shape:
            raise ValueError(f"{k} {tuple(t.shape)} differs from {name}[0] {tuple(v0.shape)}")
    for k, t in named + (list(params) if params_on_device else []):
        if not t.is_cuda:
            raise ValueError(f"{k} is on {t.device}: {head} runs on a ROCm GPU only (no CPU fallback)")
        if t.device != v0.device:
            raise ValueError(f"{k} is on {t.device}, {name}[0] on {v0.device}")
    if min(v0.shape) == 0:
        raise ValueError(f"empty {name}[0] {tuple(v0.shape)}")
