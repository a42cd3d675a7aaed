"""The ground-plane head of the reference's ``NoJointConvVariant`` after its first 1x1 conv, fused:
upsample + warp of every view, the sum over views, bias, coord term, ReLU and the second 1x1 conv in one
HIP launch, with a native backward.

``no_joint_conv_variant.py:64-81`` upsamples each view's 512-channel map, warps it, concatenates the views
with the coord map and runs ``Conv2d(512 N + 2, 512, 1) -> ReLU -> Conv2d(512, 1, 1, bias=False)``.  A 1x1
conv is a per-pixel linear map over channels; the bilinear upsample and the zero-padded bilinear warp are
per-channel linear maps over pixels; so they commute, and with ``W_v`` the block of the first conv's weight
that multiplies view v, ``W_c`` its two coord columns and ``b`` its bias

    z_v       = W_v feat_v                                       (at backbone resolution: a GEMM, the caller's)
    hidden[p] = relu(b + W_c coord(p) + sum_v warp_v(upsample(z_v))[p])
    map[p]    = w2 . hidden[p]

``ProjectSumHead`` evaluates the last two lines on ``mvdet_amd/csrc/warp_sum_head.hip``
(``mvbev_warp_sum_head_forward_f32`` / ``_backward_f32`` / ``_grad_params_f32``).  Neither the upsampled maps
nor the concatenated slab exist; inference writes the map only, training keeps ``hidden`` ([B,Cm,Ho,Wo],
88 MB at config 2) and nothing else of that size.  The gradient to ``z_v`` is the existing adjoint of the
fused upsample + warp (``ops.warp_views_adjoint`` with the upsampled ``WarpAdjointPlan``), a deterministic
gather; the parameter gradients are fixed-order sums.  Everything is fp32 and bitwise repeatable.

Non-finite *geometry* is inside the contract (a pixel whose sample coordinates are not finite for some view
is NaN, as the reference's warp makes it).  Non-finite *features or view weights* are outside it, as for
``mvbev_warp_views_upsampled``: the commuted order cannot reproduce where the reference's 0 * NaN lands.  A
non-finite bias, coord weight or ``w2`` with finite features is inside it: every product is formed, and an
infinite map value is stored as NaN, as ``no_joint_conv_variant.py:81``'s same-size interpolate makes it.
"""
from __future__ import annotations

import torch

from . import _native, ops
from .ops import _stream
from .rig import MAX_VIEWS, Rig, check_views  # noqa: F401  (MAX_VIEWS: this module's public limit)

MAX_CM = 512    # kShMaxCm (csrc/warp_sum_head.hip)


def _check(n_views, zs, bias, w_coord, w2):
    check_views("zs", zs, "the warp-sum head", n_views, [("bias", bias), ("w_coord", w_coord), ("w2", w2)],
                lambda z: None if z.dim() == 4 else f"4-D [B,Cm,h,w], got {z.dim()}-D")
    cm = zs[0].shape[1]
    if cm > MAX_CM:
        raise ValueError(f"{cm} channels: the kernel takes Cm <= {MAX_CM}")
    if bias.numel() != cm or bias.dim() != 1:
        raise ValueError(f"bias must be [{cm}], got {tuple(bias.shape)}")
    if w2.numel() != cm or tuple(w2.shape) not in ((cm,), (1, cm), (1, cm, 1, 1)):
        raise ValueError(f"w2 must be [{cm}], [1,{cm}] or [1,{cm},1,1], got {tuple(w2.shape)}")
    if tuple(w_coord.shape) not in ((cm, 2), (cm, 2, 1, 1)):
        raise ValueError(f"w_coord must be [{cm},2] or [{cm},2,1,1], got {tuple(w_coord.shape)}")


def _lines(z: torch.Tensor) -> torch.Tensor:
    """``z`` with channel stride 1 (channels-last lines); a copy only when it is not already."""
    if z.shape[1] == 1 or z.stride(1) == 1:
        return z
    return z.contiguous(memory_format=torch.channels_last)


class WarpSumHead(torch.autograd.Function):
    """One forward launch; backward: one launch for the pre-activation gradient and the parameter partial sums,
    the fixed-order reduction, and the upsampled warp adjoint for the views that need a gradient.  Saves
    ``hidden`` and ``w2``."""

    @staticmethod
    def forward(ctx, head, return_hidden, bias, w_coord, w2, *zs):
        lib = _native.load()
        n = len(zs)
        B, cm, h, w = zs[0].shape
        dev = zs[0].device
        H, W = head.up_hw
        Ho, Wo = head.grid_hw
        lines = [_lines(z.detach()) for z in zs]
        need = any(ctx.needs_input_grad[2:])
        keep = need or return_hidden
        out = torch.empty((B, 1, Ho, Wo), dtype=torch.float32, device=dev)
        hidden = torch.empty((B, cm, Ho, Wo), dtype=torch.float32, device=dev) if keep else None
        arr = ops._view_table(lines, head.m_norm_cpu, unit_dim=1)  # (a single channel: any stride torch reports)
        pb, pc, pw = bias.detach().contiguous(), w_coord.detach().reshape(cm, 2).contiguous(), \
            w2.detach().reshape(cm).contiguous()
        boxes = head.boxes(dev, (h, w))
        _native.check(lib.mvbev_warp_sum_head_forward_f32(
            arr, n, B, cm, h, w, H, W, Ho, Wo, pb.data_ptr(), pc.data_ptr(), pw.data_ptr(), out.data_ptr(),
            hidden.data_ptr() if keep else None, boxes.data_ptr(), _stream(out)), "mvbev_warp_sum_head_forward_f32")
        ctx.head, ctx.dims, ctx.shapes = head, (B, cm, h, w), (bias.shape, w_coord.shape, w2.shape)
        if need:
            ctx.save_for_backward(hidden, pw)
        if return_hidden:
            ctx.mark_non_differentiable(hidden)
            return out, hidden
        return out

    @staticmethod
    def backward(ctx, dmap, *_):
        lib = _native.load()
        hidden, pw = ctx.saved_tensors
        head = ctx.head
        B, cm, h, w = ctx.dims
        Ho, Wo = head.grid_hw
        dev = hidden.device
        want_b, want_c, want_w = ctx.needs_input_grad[2:5]
        want_z = ctx.needs_input_grad[5:]
        dmap = dmap.detach()
        if dmap.dtype != torch.float32 or dmap.device != dev or not dmap.is_contiguous():
            dmap = dmap.to(device=dev, dtype=torch.float32).contiguous()
        stream = _stream(hidden)
        params = want_b or want_c or want_w
        blocks = _native.backward_blocks("mvbev_warp_sum_head_backward_blocks", B, cm, Ho, Wo)
        partials = torch.empty(4 * cm * blocks, dtype=torch.float32, device=dev) if params else None
        # (not in place over hidden: a caller may hold it, and the graph may be kept for a second backward)
        dhidden = torch.empty_like(hidden) if any(want_z) else None
        _native.check(lib.mvbev_warp_sum_head_backward_f32(
            dmap.data_ptr(), hidden.data_ptr(), pw.data_ptr(), B, cm, Ho, Wo,
            dhidden.data_ptr() if dhidden is not None else None, partials.data_ptr() if params else None, stream),
            "mvbev_warp_sum_head_backward_f32")
        gb = gc = gw = None
        if params:
            gb = torch.empty(cm, dtype=torch.float32, device=dev) if want_b else None
            gc = torch.empty((cm, 2), dtype=torch.float32, device=dev) if want_c else None
            gw = torch.empty(cm, dtype=torch.float32, device=dev) if want_w else None
            _native.check(lib.mvbev_warp_sum_head_grad_params_f32(
                partials.data_ptr(), blocks, cm, gw.data_ptr() if want_w else None, gb.data_ptr() if want_b else None,
                gc.data_ptr() if want_c else None, stream), "mvbev_warp_sum_head_grad_params_f32")
            sb, sc, sw = ctx.shapes
            gb = gb.view(sb) if want_b else None
            gc = gc.view(sc) if want_c else None
            gw = gw.view(sw) if want_w else None
        gz = [None] * len(want_z)
        idx = [i for i, wz in enumerate(want_z) if wz]  # a view that needs no gradient is not gathered
        if idx:
            plans = head.plans(dev, (h, w))
            for i in idx:
                gz[i] = torch.empty((B, cm, h, w), dtype=torch.float32, device=dev)
            ops.warp_views_adjoint([dhidden] * len(idx), [plans[i] for i in idx], [gz[i] for i in idx])
        return (None, None, gb, gc, gw) + tuple(gz)


class ProjectSumHead(Rig):
    """``map = w2 . relu(bias + w_coord . coord + sum_v warp_v(upsample(z_v)))`` for one camera rig.

    ``proj_mats``: the reference's per-camera 3x3 ``proj_mats`` (upsampled-image pixels -> grid pixels);
    ``upsample_shape``: (H, W) the reference upsamples the backbone maps to; ``reducedgrid_shape``: (Ho, Wo).
    Holds the normalised matrices (computed as ``ProjectFuse`` computes them), and per device and backbone
    size the geometry-only frustum boxes and, lazily, the adjoint plans."""

    def boxes(self, device, backbone_hw):
        dev, hw = torch.device(device), tuple(backbone_hw)
        return self.cached(("boxes", dev, hw), lambda: ops.warp_wino_boxes(self.m_norm_cpu, self.up_hw, self.grid_hw,
                                                                           dev, backbone_hw=hw))

    def plans(self, device, backbone_hw):
        dev, hw = torch.device(device), tuple(backbone_hw)
        return self.cached(("plans", dev, hw), lambda: [ops.WarpAdjointPlan(m, self.up_hw, self.grid_hw, dev,
                                                                            backbone_hw=hw) for m in self.m_norm_cpu])

    def __call__(self, zs, bias, w_coord, w2, return_hidden: bool = False):
        """``zs``: one fp32 ``[B,Cm,h,w]`` tensor per view on one GPU (Cm <= 512, h <= H, w <= W; a ``z`` whose
        channel stride is not 1 is copied to channels-last); ``bias`` [Cm]; ``w_coord`` [Cm,2] (the x and y
        coord columns); ``w2`` [Cm] (or the conv's [1,Cm,1,1]).  Returns the ``[B,1,Ho,Wo]`` map, with
        ``return_hidden`` also the post-ReLU ``[B,Cm,Ho,Wo]`` activations (no gradient flows through them).
        Finite ``zs`` and parameters only (see the module docstring)."""
        _check(self.num_views, zs, bias, w_coord, w2)
        _, _, h, w = zs[0].shape
        if h > self.up_hw[0] or w > self.up_hw[1]:
            raise ValueError(f"views {tuple(zs[0].shape)} are larger than the upsampled size {self.up_hw}")
        return WarpSumHead.apply(self, bool(return_hidden), bias, w_coord, w2, *zs)
