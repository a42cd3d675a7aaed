"""The perspective transform itself as a standalone, differentiable op: upsample + warp of every view, concat and
the two coord channels (``persp_trans_detector.py:65-77``) for a ground-plane head of your own.

``ProjectFuse`` and the variant heads fuse this step with their own convs and write internal layouts.
``ProjectViews`` stops after the concat and returns a plain tensor, so a different head (another width, an
attention block, a torch head under autocast) keeps the fast path.  In exact arithmetic, with ``coord_map`` the
reference's ``create_coord_map``,

    world = torch.cat([kornia.warp_perspective(F.interpolate(f, upsample_shape, mode='bilinear'),
                                               M_v.repeat(B, 1, 1).float(), reducedgrid_shape)
                       for f, M_v in zip(feats, proj_mats)] + [coord_map.repeat(B, 1, 1, 1)], dim=1)

The upsampled maps are never written.  Two paths, chosen by the inputs; neither has a CPU or torch fallback:

* contiguous fp32 views -> a contiguous fp32 ``[B,Ctot,Ho,Wo]``: the existing NCHW warps into channel slices
  (``mvbev_warp_views_upsampled_ex`` / ``mvbev_warp_views_f32``), ``mvbev_fill_coord_map_f32``, and the plan gather
  ``mvbev_warp_views_adjoint`` backward;
* ``channels_last`` views, fp32 / bf16 / fp16 (what the detector's backbone emits) -> a ``channels_last`` result of
  the views' dtype, or fp32 with ``out_dtype=torch.float32``: ``mvdet_amd/csrc/project_views.hip``, one launch
  forward (every view and the coord channels) and one launch backward.  All math is fp32: a 16-bit value is
  converted exactly at the load and every output value is rounded once at the store.

The backward is a gather over the CSR adjoint plans (``ops.WarpAdjointPlan``): no float atomics, bitwise
repeatable, nothing saved but the plans (the warp is linear in the maps), which are built once per (rig, device,
source size) when a backward is first needed.  A view that requires grad gets a gradient in its own dtype and
memory format, accumulated in fp32 and rounded once; a view that does not costs no work.  Neither direction
synchronises the host.

Contract edges: a sample whose coordinates are non-finite is NaN (as ``mvbev_warp_perspective_f32``) and passes no
gradient; a sample outside the source is 0 and passes no gradient; NaN / inf in the *features* is outside the
contract, as for the variant heads (the fused upsample merges zero-weight taps).
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _native, ops
from .ops import _stream
from .rig import MAX_VIEWS, Rig  # noqa: F401  (MAX_VIEWS: this module's public limit)

_KINDS = {torch.float32: _native.KIND_F32, torch.float16: _native.KIND_F16, torch.bfloat16: _native.KIND_BF16}
_CL = torch.channels_last


def _cl_strides(B, C, H, W):
    """Element strides of a dense channels-last [B,C,H,W] (torch reports any stride for a dimension of size 1)."""
    return (H * W * C, 1, W * C, C)


def _check(pv, feats):
    """The checks of the per-view argument in the style of ``rig.check_views``; returns True for the
    channels-last path."""
    if isinstance(feats, torch.Tensor) or not hasattr(feats, "__len__"):
        raise TypeError(f"feats must be a sequence of tensors, got {type(feats).__name__}")
    if len(feats) != pv.num_views:
        raise ValueError(f"{len(feats)} views for a rig of {pv.num_views}")
    for i, t in enumerate(feats):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"feats[{i}] must be a tensor, got {type(t).__name__}")
    f0 = feats[0]
    for i, t in enumerate(feats):
        if t.dim() != 4:
            raise ValueError(f"feats[{i}] must be 4-D [B,C,h,w], got {t.dim()}-D")
        if t.shape != f0.shape:
            raise ValueError(f"feats[{i}] {tuple(t.shape)} differs from feats[0] {tuple(f0.shape)}")
        if t.dtype != f0.dtype:
            raise TypeError(f"feats[{i}] is {t.dtype}, feats[0] {f0.dtype}: the views share one dtype")
    if f0.dtype not in _KINDS:
        raise TypeError(f"feats must be float32, float16 or bfloat16, got {f0.dtype}")
    h, w = f0.shape[2:]
    if h > pv.up_hw[0] or w > pv.up_hw[1]:
        raise ValueError(f"views {tuple(f0.shape)} are larger than the upsampled size {pv.up_hw}")
    for i, t in enumerate(feats):
        if not t.is_cuda:
            raise ValueError(f"feats[{i}] is on {t.device}: ProjectViews runs on a ROCm GPU only (no CPU fallback)")
        if t.device != f0.device:
            raise ValueError(f"feats[{i}] is on {t.device}, feats[0] on {f0.device}")
    if min(f0.shape) == 0:
        raise ValueError(f"empty feats[0] {tuple(f0.shape)}")
    nchw = f0.dtype == torch.float32 and all(t.is_contiguous() for t in feats)
    if nchw:
        if pv.out_dtype not in (None, torch.float32):
            raise TypeError("contiguous fp32 views give an fp32 result")
        return False
    if not all(t.is_contiguous(memory_format=_CL) for t in feats):
        raise ValueError("the views must share one memory format: all contiguous (fp32) or all channels_last "
                         "(fp32, bf16, fp16)")
    return True


class _ProjectViewsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pv, cl, *feats):
        lib = _native.load()
        n = len(feats)
        B, C, h, w = feats[0].shape
        H, W = pv.up_hw
        Ho, Wo = pv.grid_hw
        dev, dtype = feats[0].device, feats[0].dtype
        ctot = n * C + (2 if pv.coord_channels else 0)
        srcs = [f.detach() for f in feats]
        if cl:
            odt = pv.out_dtype or dtype
            out = torch.empty((B, ctot, Ho, Wo), dtype=odt, device=dev, memory_format=_CL)
            arr = ops._view_table(srcs, pv.m_norm_cpu)
            for v in arr:
                v.src_strides = _native._i64x4(*_cl_strides(B, C, h, w))
            _native.check(lib.mvbev_project_views_cl_forward(
                arr, n, _KINDS[dtype], B, C, h, w, H, W, Ho, Wo, out.data_ptr(), _KINDS[odt], ctot,
                int(pv.coord_channels), _stream(out)), "mvbev_project_views_cl_forward")
        else:
            out = torch.empty((B, ctot, Ho, Wo), dtype=torch.float32, device=dev)
            dsts = [out[:, v * C:(v + 1) * C] for v in range(n)]
            if (h, w) == (H, W):
                ops.warp_views_into(srcs, pv.m_norm_cpu, dsts)
            else:
                ops.warp_views_upsampled_into(srcs, (H, W), pv.m_norm_cpu, dsts)
            if pv.coord_channels:
                ops.fill_coord_map(out[:, n * C:])
        ctx.pv, ctx.cl, ctx.dims, ctx.dtype = pv, cl, (B, C, h, w), dtype
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        pv, cl, (B, C, h, w), dtype = ctx.pv, ctx.cl, ctx.dims, ctx.dtype
        want = ctx.needs_input_grad[2:]
        n = len(want)
        Ho, Wo = pv.grid_hw
        idx = [i for i, wz in enumerate(want) if wz]  # a view that needs no gradient is not gathered
        grads = [None] * n
        if not idx:
            return (None, None) + tuple(grads)
        dev = grad_out.device
        plans = pv.plans(dev, (h, w))
        if cl:
            if grad_out.dtype not in (torch.float32, dtype):
                grad_out = grad_out.to(dtype)
            if not grad_out.is_contiguous(memory_format=_CL):
                grad_out = grad_out.contiguous(memory_format=_CL)
            ctot = grad_out.shape[1]
            arr = (_native.ProjectViewsGrad * n)()
            for i in idx:
                grads[i] = torch.empty((B, C, h, w), dtype=dtype, device=dev, memory_format=_CL)
                arr[i] = _native.ProjectViewsGrad(plans[i].row_ptr.data_ptr(), plans[i].col.data_ptr(),
                                                  plans[i].val.data_ptr(), grads[i].data_ptr(),
                                                  (ctypes.c_int64 * 4)(*_cl_strides(B, C, h, w)))
            _native.check(_native.load().mvbev_project_views_cl_backward(
                grad_out.data_ptr(), _KINDS[grad_out.dtype], ctot, arr, n, _KINDS[dtype], B, C, h, w, Ho, Wo,
                _stream(grad_out)), "mvbev_project_views_cl_backward")
        else:
            if grad_out.dtype != torch.float32 or not grad_out.is_contiguous():
                grad_out = grad_out.to(torch.float32).contiguous()
            for i in idx:
                grads[i] = torch.empty((B, C, h, w), dtype=torch.float32, device=dev)
            ops.warp_views_adjoint([grad_out[:, i * C:(i + 1) * C] for i in idx], [plans[i] for i in idx],
                                   [grads[i] for i in idx])
        return (None, None) + tuple(grads)


class ProjectViews(torch.nn.Module):
    """``world = cat([warp(upsample(feat_v)) for v] + [coord_map])`` for one camera rig; no parameters.

    ``proj_mats``, ``upsample_shape``, ``reducedgrid_shape``: the reference's ``self.proj_mats`` (per-camera 3x3,
    upsampled-image pixels -> grid pixels), ``self.upsample_shape`` (H, W) and ``self.reducedgrid_shape`` (Ho, Wo),
    as ``ProjectFuse`` and the variant heads take them.  ``coord_channels=False`` leaves the two coord channels
    out.  ``out_dtype``: None (the views' dtype) or ``torch.float32`` (16-bit channels-last views, fp32 result).

    ``forward(feats)``: N tensors ``[B,C,h,w]`` of one shape, dtype, memory format and device, ``(h, w)`` at most
    ``upsample_shape`` (equal: only the warp runs) -> ``[B, N*C (+2), Ho, Wo]``, views in list order, the coord
    channels (the values of ``mvbev_fill_coord_map_f32``) last.  Contiguous fp32 views give a contiguous fp32
    result; ``channels_last`` fp32 / bf16 / fp16 views a ``channels_last`` one.  See the module docstring for the
    backward and the contract edges (non-finite coordinates -> NaN and no gradient, outside the source -> 0 and no
    gradient, non-finite features outside the contract)."""

    def __init__(self, proj_mats, upsample_shape, reducedgrid_shape, coord_channels: bool = True, out_dtype=None):
        super().__init__()
        self.rig = Rig(proj_mats, upsample_shape, reducedgrid_shape)
        if min(self.rig.grid_hw) < 2:
            # create_coord_map and kornia's normalised meshgrid divide by (side - 1)
            raise ValueError(f"a grid side of 1 has no coord map and no normalised grid: {self.rig.grid_hw}")
        if out_dtype not in (None, torch.float32):
            raise TypeError(f"out_dtype must be None (the views' dtype) or torch.float32, got {out_dtype}")
        self.coord_channels = bool(coord_channels)
        self.out_dtype = out_dtype
        self.up_hw, self.grid_hw = self.rig.up_hw, self.rig.grid_hw
        self.num_views, self.m_norm_cpu = self.rig.num_views, self.rig.m_norm_cpu

    def plans(self, device, src_hw):
        """The views' ``ops.WarpAdjointPlan``s for sources of ``src_hw``, built once per (device, size)."""
        dev, hw = torch.device(device), tuple(int(s) for s in src_hw)
        bb = None if hw == self.up_hw else hw
        return self.rig.cached(("plans", dev, hw), lambda: [
            ops.WarpAdjointPlan(m, self.up_hw, self.grid_hw, dev, backbone_hw=bb) for m in self.m_norm_cpu])

    def forward(self, feats):
        cl = _check(self, feats)
        return _ProjectViewsFn.apply(self, cl, *feats)
