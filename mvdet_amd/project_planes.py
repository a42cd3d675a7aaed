"""The weighted multi-plane projection as a standalone, differentiable op: every view is projected through D
ground-parallel planes and a per-pixel weight (a softmax over planes, say, predicted from the image features)
chooses among them,

    world_v = sum_d warp_{v,d}(upsample(w_v[:, d:d+1] * feat_v)),   world = cat([world_v for v] + [coord_map])

with ``warp_{v,d}`` the ``kornia.warp_perspective`` of plane d's homography and ``upsample`` the bilinear
``F.interpolate`` to ``upsample_shape`` — ``ProjectViews`` with a sum over planes inside.  The sum commutes with the
gather, so one kernel (``mvdet_amd/csrc/project_planes.hip``) reads ``feat_v`` and the D weight planes in place and
writes the N C channels once: neither the D products nor the D warped maps exist, forward or backward.

* ``channels_last`` maps, fp32 / bf16 / fp16; fp32 contiguous weights ``[B,D,h,w]``.  The result is
  ``channels_last`` in the maps' dtype, or fp32 with ``out_dtype=torch.float32``.  All math is fp32: a 16-bit map
  value is converted exactly at the load and every output value is rounded once at the store.
* Per tap the term is ``(a_t * w[b,d,q_t]) * f[b,c,q_t]`` with ``a_t`` the tap coefficient of ``ProjectViews``;
  planes are added in order.  With D = 1 and weights of exactly 1.0 the result is ``ProjectViews``' bit for bit.
* One launch forward (every view, plane and the coord channels), one launch backward; neither synchronises the host.

The op is bilinear, so the backward saves the maps and the weights.  With ``G_d = adjoint of warp_{v,d}(upsample(.))``
applied to the view's slice of the upstream gradient (a gather over the N D CSR plans, ``ops.WarpAdjointPlan``, built
once per (rig, device, source size)),

    grad_feats[v] = sum_d w_v[:, d] * G_d         (the maps' dtype and memory format, fp32 sums rounded once)
    grad_weights[v][:, d] = sum_c feat_v * G_d    (fp32; reduced in a fixed order)

No float atomics, bitwise repeatable; an input that needs no gradient costs no work and gets ``None``.

Contract edges, as for ``ProjectViews``: a plane whose sample coordinates are non-finite makes that output pixel NaN
and passes no gradient; a sample outside the source contributes 0; non-finite features or weights are outside the
contract.  Contiguous (NCHW) maps are not taken.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _native, ops
from .ops import _stream
from .project_views import _KINDS, _cl_strides
from .rig import MAX_VIEWS, Rig, norm_matrices

MAX_PLANES = 8  # kMaxPlanes (csrc/project_planes.hip)
_CL = torch.channels_last


class _PlanePlans:
    """One view's D adjoint plans side by side: ``row_ptr`` [D][P + 1] indexes the concatenated ``col`` / ``val``
    (each plan keeps its allocated length, so the offsets are known on the host: no sync)."""

    def __init__(self, plans):
        offs, at = [], 0
        for p in plans:
            offs.append(at)
            at += p.col.numel()
        self.row_ptr = torch.cat([p.row_ptr + o for p, o in zip(plans, offs)])
        self.col = torch.cat([p.col for p in plans])
        self.val = torch.cat([p.val for p in plans])


def _check(pp, feats, weights):
    """The checks of both per-view arguments, in the style of ``project_views._check``."""
    for name, ts in (("feats", feats), ("weights", weights)):
        if isinstance(ts, torch.Tensor) or not hasattr(ts, "__len__"):
            raise TypeError(f"{name} must be a sequence of tensors, got {type(ts).__name__}")
        if len(ts) != pp.num_views:
            raise ValueError(f"{len(ts)} {name} for a rig of {pp.num_views} views")
        for i, t in enumerate(ts):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name}[{i}] must be a tensor, got {type(t).__name__}")
            if t.dim() != 4:
                raise ValueError(f"{name}[{i}] must be 4-D, got {t.dim()}-D")
    f0 = feats[0]
    for i, t in enumerate(feats):
        if t.shape != f0.shape:
            raise ValueError(f"feats[{i}] {tuple(t.shape)} differs from feats[0] {tuple(f0.shape)}")
        if t.dtype != f0.dtype:
            raise TypeError(f"feats[{i}] is {t.dtype}, feats[0] {f0.dtype}: the views share one dtype")
    if f0.dtype not in _KINDS:
        raise TypeError(f"feats must be float32, float16 or bfloat16, got {f0.dtype}")
    B, C, h, w = f0.shape
    if h > pp.up_hw[0] or w > pp.up_hw[1]:
        raise ValueError(f"views {tuple(f0.shape)} are larger than the upsampled size {pp.up_hw}")
    for i, t in enumerate(weights):
        if t.shape[1] != pp.num_planes:
            raise ValueError(f"weights[{i}] has {t.shape[1]} planes, the rig {pp.num_planes}")
        if (t.shape[0], t.shape[2], t.shape[3]) != (B, h, w):
            raise ValueError(f"weights[{i}] {tuple(t.shape)} does not match feats[{i}] {tuple(f0.shape)}: "
                             f"[B,D,h,w] = [{B},{pp.num_planes},{h},{w}]")
        if t.dtype != torch.float32:
            raise TypeError(f"weights[{i}] must be float32, got {t.dtype}")
    for name, ts in (("feats", feats), ("weights", weights)):
        for i, t in enumerate(ts):
            if not t.is_cuda:
                raise ValueError(f"{name}[{i}] is on {t.device}: ProjectPlanes runs on a ROCm GPU only "
                                 f"(no CPU fallback)")
            if t.device != f0.device:
                raise ValueError(f"{name}[{i}] is on {t.device}, feats[0] on {f0.device}")
    if min(f0.shape) == 0:
        raise ValueError(f"empty feats[0] {tuple(f0.shape)}")
    if not all(t.is_contiguous(memory_format=_CL) for t in feats):
        raise ValueError("the maps must be channels_last (fp32, bf16 or fp16): contiguous NCHW maps are not taken, "
                         "use feat.contiguous(memory_format=torch.channels_last)")
    for i, t in enumerate(weights):
        if not t.is_contiguous():
            raise ValueError(f"weights[{i}] must be contiguous [B,D,h,w]")


class _ProjectPlanesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pp, *tensors):
        n, D = pp.num_views, pp.num_planes
        feats = [t.detach() for t in tensors[:n]]
        weights = [t.detach() for t in tensors[n:]]
        B, C, h, w = feats[0].shape
        H, W = pp.up_hw
        Ho, Wo = pp.grid_hw
        dev, dtype = feats[0].device, feats[0].dtype
        ctot = n * C + (2 if pp.coord_channels else 0)
        odt = pp.out_dtype or dtype
        out = torch.empty((B, ctot, Ho, Wo), dtype=odt, device=dev, memory_format=_CL)
        arr = (_native.ProjectPlanesView * n)()
        for i in range(n):
            arr[i] = _native.ProjectPlanesView(feats[i].data_ptr(), (ctypes.c_int64 * 4)(*_cl_strides(B, C, h, w)),
                                               weights[i].data_ptr())
        with torch.cuda.device(dev):
            _native.check(_native.load().mvbev_project_planes_cl_forward(
                arr, n, D, pp.mats_on(dev).data_ptr(), _KINDS[dtype], B, C, h, w, H, W, Ho, Wo, out.data_ptr(),
                _KINDS[odt], ctot, int(pp.coord_channels), _stream(out)), "mvbev_project_planes_cl_forward")
        ctx.pp, ctx.dims, ctx.dtype = pp, (B, C, h, w), dtype
        ctx.save_for_backward(*tensors)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        pp, (B, C, h, w), dtype = ctx.pp, ctx.dims, ctx.dtype
        n, D = pp.num_views, pp.num_planes
        want = ctx.needs_input_grad[1:]
        grads = [None] * (2 * n)
        if not any(want):
            return (None,) + tuple(grads)
        saved = ctx.saved_tensors
        Ho, Wo = pp.grid_hw
        dev = grad_out.device
        plans = pp.plans(dev, (h, w))
        if grad_out.dtype not in (torch.float32, dtype):
            grad_out = grad_out.to(dtype)
        if not grad_out.is_contiguous(memory_format=_CL):
            grad_out = grad_out.contiguous(memory_format=_CL)
        ctot = grad_out.shape[1]
        strides = _cl_strides(B, C, h, w)
        arr = (_native.ProjectPlanesGrad * n)()
        for i in range(n):
            gf = gw = None
            if want[i]:
                gf = grads[i] = torch.empty((B, C, h, w), dtype=dtype, device=dev, memory_format=_CL)
            if want[n + i]:
                gw = grads[n + i] = torch.empty((B, D, h, w), dtype=torch.float32, device=dev)
            if gf is None and gw is None:
                continue  # the zeroed entry: the view is skipped
            arr[i] = _native.ProjectPlanesGrad(
                plans[i].row_ptr.data_ptr(), plans[i].col.data_ptr(), plans[i].val.data_ptr(),
                saved[i].data_ptr(), (ctypes.c_int64 * 4)(*strides), saved[n + i].data_ptr(),
                None if gf is None else gf.data_ptr(), (ctypes.c_int64 * 4)(*strides),
                None if gw is None else gw.data_ptr())
        with torch.cuda.device(dev):
            _native.check(_native.load().mvbev_project_planes_cl_backward(
                grad_out.data_ptr(), _KINDS[grad_out.dtype], ctot, arr, n, D, _KINDS[dtype], B, C, h, w, Ho, Wo,
                _stream(grad_out)), "mvbev_project_planes_cl_backward")
        return (None,) + tuple(grads)


class ProjectPlanes(torch.nn.Module):
    """``world = cat([sum_d warp_{v,d}(upsample(w_v[:, d] * feat_v)) for v] + [coord_map])``; no parameters.

    ``proj_mats``: N sequences of D 3x3 matrices (upsampled-image pixels -> grid pixels of plane d;
    ``geometry.plane_projection_matrices``), 1 <= N <= 16 views, 1 <= D <= 8 planes, the same D for every view.
    ``upsample_shape`` (H, W), ``reducedgrid_shape`` (Ho, Wo), ``coord_channels`` and ``out_dtype`` as
    ``ProjectViews``.

    ``forward(feats, weights)``: N ``channels_last`` maps ``[B,C,h,w]`` (fp32 / bf16 / fp16, one shape and dtype,
    ``(h, w)`` at most ``upsample_shape``; equal: the plain warp) and N contiguous fp32 weights ``[B,D,h,w]`` ->
    ``[B, N*C (+2), Ho, Wo]`` ``channels_last``, views in list order, the coord channels (the values of
    ``mvbev_fill_coord_map_f32``) last.  See the module docstring for the arithmetic, the backward and the contract
    edges."""

    def __init__(self, proj_mats, upsample_shape, reducedgrid_shape, coord_channels: bool = True, out_dtype=None):
        super().__init__()
        if isinstance(proj_mats, torch.Tensor) or not hasattr(proj_mats, "__len__"):
            raise TypeError(f"proj_mats must be N sequences of D 3x3 matrices, got {type(proj_mats).__name__}")
        if not 0 < len(proj_mats) <= MAX_VIEWS:
            raise ValueError(f"1 .. {MAX_VIEWS} views, got {len(proj_mats)}")
        views = []
        for i, planes in enumerate(proj_mats):
            if isinstance(planes, torch.Tensor) and planes.dim() == 3:
                planes = list(planes)
            if isinstance(planes, torch.Tensor) or not hasattr(planes, "__len__"):
                raise TypeError(f"proj_mats[{i}] must be a sequence of 3x3 matrices (one per plane)")
            if not 0 < len(planes) <= MAX_PLANES:
                raise ValueError(f"1 .. {MAX_PLANES} planes per view, got {len(planes)} for view {i}")
            views.append([torch.as_tensor(M) for M in planes])
        D = len(views[0])
        for i, planes in enumerate(views):
            if len(planes) != D:
                raise ValueError(f"every view has the same number of planes: view {i} has {len(planes)}, view 0 {D}")
            for d, M in enumerate(planes):
                if tuple(M.shape) != (3, 3):
                    raise ValueError(f"proj_mats[{i}][{d}] must be 3x3, got {tuple(M.shape)}")
        self.rig = Rig([planes[0] for planes in views], upsample_shape, reducedgrid_shape)  # sizes, cache
        if min(self.rig.grid_hw) < 2:
            raise ValueError(f"a grid side of 1 has no coord map and no normalised grid: {self.rig.grid_hw}")
        if out_dtype not in (None, torch.float32):
            raise TypeError(f"out_dtype must be None (the maps' dtype) or torch.float32, got {out_dtype}")
        self.coord_channels = bool(coord_channels)
        self.out_dtype = out_dtype
        self.up_hw, self.grid_hw = self.rig.up_hw, self.rig.grid_hw
        self.num_views, self.num_planes = len(views), D
        # [N, D, 3, 3] fp32: each plane's normalised matrix, as every other warp here gets its own
        self.m_norm_cpu = torch.stack([norm_matrices(planes, self.up_hw, self.grid_hw) for planes in views])

    def mats_on(self, device):
        """``m_norm_cpu`` as a device tensor [N, D, 9], copied once per device."""
        dev = torch.device(device)
        return self.rig.cached(("mats", dev), lambda: self.m_norm_cpu.reshape(
            self.num_views, self.num_planes, 9).to(torch.float32).contiguous().to(dev))

    def plans(self, device, src_hw):
        """Per view, the D planes' ``ops.WarpAdjointPlan``s side by side, built once per (device, size)."""
        dev, hw = torch.device(device), tuple(int(s) for s in src_hw)
        bb = None if hw == self.up_hw else hw
        return self.rig.cached(("plans", dev, hw), lambda: [
            _PlanePlans([ops.WarpAdjointPlan(m, self.up_hw, self.grid_hw, dev, backbone_hw=bb) for m in planes])
            for planes in self.m_norm_cpu])

    def forward(self, feats, weights):
        _check(self, feats, weights)
        return _ProjectPlanesFn.apply(self, *feats, *weights)
