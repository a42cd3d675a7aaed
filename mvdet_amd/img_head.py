"""The per-view image head after its first 1x1 conv, fused: bilinear upsample -> ReLU -> bias-free
1x1 conv, for every view in one launch, with a native backward.

``persp_trans_detector.py:65-66`` evaluates ``img_classifier(F.interpolate(feat, upsample_shape))``
per view; ``mvdet_amd.detector`` runs the head's first conv at backbone resolution (it commutes with
the bilinear upsample), and what is left is

    out[v] = F.conv2d(F.relu(F.interpolate(g[v], size, mode="bilinear")), weight)

on the HIP kernels of ``mvdet_amd/csrc/img_head.hip`` (``mvbev_img_head_forward_f32``,
``mvbev_img_head_backward_f32``, ``mvbev_img_head_grad_weight_f32``).  The upsampled tensor
([B,Cm,Hu,Wu], 33 MB per view at config 2) is never written: the forward keeps it in registers and the
backward recomputes it from ``g``, so autograd holds ``g`` and ``weight`` only.  The gradients are
bitwise repeatable (no float atomics).  Everything is fp32; ``g`` may be NCHW or channels_last (any
strides), no copy is made.
"""
from __future__ import annotations

import torch

from . import _native
from .ops import _stream
from .rig import MAX_VIEWS, check_views

MAX_CM = 256    # kIhMaxCm
MAX_CO = 4      # kIhMaxCo


def supported(n_views: int, g_shape, co: int, size) -> bool:
    """Whether the kernels take this shape: 1..16 views, Cm <= 256, Co <= 4, no downsampling."""
    _, cm, h, w = g_shape
    return (0 < n_views <= MAX_VIEWS and 0 < cm <= MAX_CM and 0 < co <= MAX_CO and size[0] >= h > 0
            and size[1] >= w > 0)


def _check(gs, weight, size):
    check_views("gs", gs, "the image head", None, [("weight", weight)],
                lambda g: None if g.dim() == 4 else f"4-D [B,Cm,h,w], got {g.dim()}-D", params_on_device=False)
    g0 = gs[0]
    if not (weight.dim() == 2 or (weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1))):
        raise ValueError(f"weight must be [Co,Cm] or [Co,Cm,1,1], got {tuple(weight.shape)}")
    if weight.shape[1] != g0.shape[1]:
        raise ValueError(f"weight {tuple(weight.shape)} does not match the views' {g0.shape[1]} channels")
    if weight.device != g0.device:
        raise ValueError(f"weight is on {weight.device}, the views on {g0.device}")
    try:
        hu, wu = (int(s) for s in size)
    except (TypeError, ValueError):
        raise TypeError(f"size must be (Hu, Wu), got {size!r}") from None
    if hu <= 0 or wu <= 0:
        raise ValueError(f"size must be positive, got {(hu, wu)}")
    if not supported(len(gs), g0.shape, weight.shape[0], (hu, wu)):
        raise ValueError(f"views {tuple(g0.shape)} -> {(hu, wu)} with weight {tuple(weight.shape)} is outside the "
                         f"kernels' range (Cm <= {MAX_CM}, Co <= {MAX_CO}, Hu >= h, Wu >= w)")
    return hu, wu


def _dims(g, co, hu, wu):
    B, cm, h, w = g.shape
    return B, cm, h, w, co, hu, wu


class UpsampleReluConv1x1(torch.autograd.Function):
    """All views in one forward launch; one backward launch plus the grad_W reduction.  Saves the
    views and the weight, nothing of the upsampled size."""

    @staticmethod
    def forward(ctx, weight, size, *gs):
        lib = _native.load()
        hu, wu = size
        n, co = len(gs), weight.shape[0]
        B = gs[0].shape[0]
        w2 = weight.detach()  # contiguous [Co,Cm]: upsample_relu_conv1x1 made it so
        outs = [torch.empty((B, co, hu, wu), dtype=torch.float32, device=w2.device) for _ in range(n)]
        items = (_native.ImgHeadItem * n)()
        for i, (g, o) in enumerate(zip(gs, outs)):
            items[i].g, items[i].g_strides = g.data_ptr(), _native.strides4(g)
            items[i].out, items[i].out_strides = o.data_ptr(), _native.strides4(o)
        _native.check(lib.mvbev_img_head_forward_f32(items, n, *_dims(gs[0], co, hu, wu), w2.data_ptr(), _stream(w2)),
                      "mvbev_img_head_forward_f32")
        ctx.save_for_backward(weight, *gs)
        ctx.size = (hu, wu)
        ctx.set_materialize_grads(False)  # a view the loss does not use arrives as None and is skipped
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grad_outs):
        lib = _native.load()
        weight, *gs = ctx.saved_tensors
        hu, wu = ctx.size
        n, co, cm = len(gs), weight.shape[0], weight.shape[1]
        want_w, want_g = ctx.needs_input_grad[0], ctx.needs_input_grad[2:]
        w2 = weight.detach()
        dev = w2.device
        grads = [None] * n
        items = (_native.ImgHeadItem * n)()
        keep = []
        for i, (g, go) in enumerate(zip(gs, grad_outs)):
            items[i].g, items[i].g_strides = g.data_ptr(), _native.strides4(g)
            if go is None:
                continue
            go = go.detach()
            if go.dtype != torch.float32 or go.device != dev:
                go = go.to(device=dev, dtype=torch.float32)
            keep.append(go)
            items[i].grad_out, items[i].grad_out_strides = go.data_ptr(), _native.strides4(go)
            if want_g[i]:
                grads[i] = torch.empty_like(g)  # dense g keeps its layout (channels_last included)
                items[i].grad_g, items[i].grad_g_strides = grads[i].data_ptr(), _native.strides4(grads[i])
        dims = _dims(gs[0], co, hu, wu)
        grad_w = None
        if not keep:
            return (None, None) + tuple(grads)
        partials, blocks = None, 0
        if want_w:
            blocks = _native.backward_blocks("mvbev_img_head_backward_blocks", items, n, *dims)
            partials = torch.empty(co * cm * blocks, dtype=torch.float32, device=dev)
        stream = _stream(w2)
        _native.check(lib.mvbev_img_head_backward_f32(items, n, *dims, w2.data_ptr(),
                                                      partials.data_ptr() if want_w else None,
                                                      partials.numel() if want_w else 0, stream),
                      "mvbev_img_head_backward_f32")
        if want_w:
            grad_w = torch.empty((co, cm), dtype=torch.float32, device=dev)
            _native.check(lib.mvbev_img_head_grad_weight_f32(partials.data_ptr(), blocks, cm, co, grad_w.data_ptr(),
                                                             stream), "mvbev_img_head_grad_weight_f32")
            grad_w = grad_w.view(weight.shape)
        return (grad_w, None) + tuple(grads)


def upsample_relu_conv1x1(gs, weight, size):
    """``[F.conv2d(F.relu(F.interpolate(g, size, mode="bilinear")), weight) for g in gs]`` in one launch.

    ``gs``: 1..16 fp32 ``[B,Cm,h,w]`` tensors of one shape on one GPU (any strides: NCHW, channels_last
    or slices); ``weight``: ``[Co,Cm,1,1]`` or ``[Co,Cm]`` (Cm <= 256, Co <= 4); ``size``: ``(Hu, Wu)``
    with ``Hu >= h`` and ``Wu >= w``.  Returns a list of ``[B,Co,Hu,Wu]`` fp32 tensors (NCHW) with a
    ``grad_fn``; gradients go to every view and to ``weight``.  NaN / Inf in ``g`` or ``weight`` reach the
    output as in the torch sequence (a zero-weight tap on an Inf gives NaN; ReLU keeps NaN)."""
    hu, wu = _check(gs, weight, size)
    w2 = weight.reshape(weight.shape[0], weight.shape[1]).contiguous()  # views of weight unless it is strided
    return list(UpsampleReluConv1x1.apply(w2, (hu, wu), *gs))
