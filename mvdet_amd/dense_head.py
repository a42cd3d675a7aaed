"""The ground-plane head of the reference's ``ImageProjVariant`` (the paper's "early fusion" ablation), native.

``image_proj_variant.py:53-56,91-92`` runs ``Conv2d(512, 512, 3, padding=1) -> ReLU -> Conv2d(512, 512, 3,
dilation 2) -> ReLU -> Conv2d(512, 1, 3, dilation 4)`` on the DENSE world feature ``[B,512,h',w']`` the ground-plane
ResNet produces at 1/8 of the grid (no warp, no coord channels, no frustum), then a real ~8x bilinear
``F.interpolate`` to the grid.  Nothing here needs a new conv kernel: conv1 is the 3xbf16 MFMA conv reading the fp32
feature and writing y1 in the split-bf16 layout conv2 reads (bias and ReLU in its epilogue), and everything after y1
is the ``ProjectFuse`` engine's own code, as in ``mvdet_amd.thin_fuse``: conv2 -> conv3 partials in inference,
conv2 / conv3 and their native backward in training (``autograd.backward_to_dy1``).  The engine is a
``ProjectFuse(..., channels=1)`` at the world-feature resolution whose slab is never warped; it is built lazily from
the first input's shape and cached per shape.  The closing interpolate is ``ops.upsample_map`` (equal sizes: the
elided identity), its adjoint the backward's first step.

Training keeps the world feature (its NCHW form), y1 (split-bf16) and y2.  The backward's conv1 gradients are the
existing kernels': ``ops.conv3x3_bias_coord_grad`` (bias), ``ops.conv3x3_wgrad`` (weight, from the fp32 feature) and
``ops.conv3x3_dgrad`` (to the world feature).  No float atomics anywhere.

Non-finite world features are outside the contract (the 3xbf16 split turns inf into NaN), as non-finite planes are
for ``mvdet_amd.thin_fuse``.
"""
from __future__ import annotations

import torch

from . import ops
from . import autograd as native_autograd
from .pipeline import ProjectFuse, Workspace, band_rows
from .thin_fuse import _mods


def _check(x, w1, b1, w2, b2, w3, grid_hw=None):
    named = [("x", x), ("w1", w1), ("w2", w2), ("w3", w3)] + [(k, t) for k, t in (("b1", b1), ("b2", b2))
                                                              if t is not None]
    for k, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{k} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{k} must be float32, got {t.dtype}")
    if x.dim() != 4 or min(x.shape) == 0:
        raise ValueError(f"x must be a non-empty [B,C,h,w] world feature, got {tuple(x.shape)}")
    C = x.shape[1]
    mid = w1.shape[0] if w1.dim() == 4 else -1
    if w1.dim() != 4 or tuple(w1.shape[1:]) != (C, 3, 3) or mid % ops.BN or C % ops.KC:
        raise ValueError(f"w1 must be [Cout, {C}, 3, 3] with Cout % {ops.BN} == 0 and Cin % {ops.KC} == 0, got "
                         f"{tuple(w1.shape)}")
    if tuple(w2.shape) != (mid, mid, 3, 3):
        raise ValueError(f"w2 must be [{mid}, {mid}, 3, 3], got {tuple(w2.shape)}")
    if tuple(w3.shape) != (1, mid, 3, 3):
        raise ValueError(f"w3 must be [1, {mid}, 3, 3], got {tuple(w3.shape)}")
    for name, t in (("b1", b1), ("b2", b2)):
        if t is not None and tuple(t.shape) != (mid,):
            raise ValueError(f"{name} must be [{mid}], got {tuple(t.shape)}")
    if grid_hw is not None and (grid_hw[0] < x.shape[2] or grid_hw[1] < x.shape[3]):
        raise ValueError(f"the world feature {tuple(x.shape[2:])} is larger than the grid {tuple(grid_hw)}")
    for k, t in named:
        if not t.is_cuda:
            raise ValueError(f"{k} is on {t.device}: the dense head runs on a ROCm GPU only (no CPU fallback)")
        if t.device != x.device:
            raise ValueError(f"{k} is on {t.device}, x on {x.device}")


def _nchw(x: torch.Tensor) -> torch.Tensor:
    """The world feature as the conv reads it (a channels-last backbone's map is copied: 1.4 MB at config 2)."""
    return x.detach().contiguous()


class DenseFuseFunction(torch.autograd.Function):
    """``map = upsample(conv3(relu(conv2(relu(conv1(x))))))``; inputs after the head: x, w1, b1, w2, b2, w3.
    Forward: the dense conv1 into y1, then the engine's conv2 and conv3 (y2 kept), then ``ops.upsample_map``.
    Backward: the upsample's adjoint, ``autograd.backward_to_dy1``, then conv1's bias, weight and data gradients.
    The saved activations are released after the first backward."""

    @staticmethod
    def forward(ctx, head, x, w1, b1, w2, b2, w3):
        B, C, H, W = x.shape
        eng = head.engine((H, W), w1.shape[0])
        dev = x.device
        y1r, y2r = band_rows(0, H, H)
        if eng.y1_split:
            y1 = torch.empty(ops.split_shape(B, eng.mid, H, W), dtype=torch.bfloat16, device=dev)
        else:
            y1 = torch.empty((B, eng.mid, H, W), dtype=torch.float32, device=dev)
        y2 = torch.empty((B, eng.mid, H, W), dtype=torch.float32, device=dev)
        # (the engine's slab is never warped here: an empty one stands in)
        slab = torch.empty((eng.S, B, 0), dtype=torch.bfloat16, device=dev)
        ws = Workspace(slab, y1, y2, eng.m_norm_cpu, (0, H), y1r, y2r, store_y2=True, slab_rows=(0, H))
        c1, c2, c3 = _mods(w1.detach(), None if b1 is None else b1.detach(), w2.detach(),
                           None if b2 is None else b2.detach(), w3.detach())
        xc = _nchw(x)
        head.conv1(eng, xc, c1, ws.y1)
        eng.conv2(ws, c2)
        low = eng.conv3(ws, c3)
        ctx.head, ctx.eng, ctx.ws, ctx.xc = head, eng, ws, xc
        ctx.low_hw = (H, W)
        ctx.x_cl = x.dim() == 4 and not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)
        ctx.save_for_backward(w1, b1, w2, b2, w3)
        return ops.upsample_map(low, head.out_hw((H, W)))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dmap):
        ws = ctx.ws
        if ws is None:
            raise RuntimeError("DenseFuseFunction: trying to backward through this graph a second time; its saved "
                               "activations (x, y1, y2) are released after the first backward (the native "
                               "kernels keep no retain_graph copy). Run the forward again.")
        eng = ctx.eng
        w1, b1, w2, b2, w3 = ctx.saved_tensors
        need_x, need_w1 = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        need_b1 = ctx.needs_input_grad[3] and b1 is not None
        xc = ctx.xc
        B, C, H, W = xc.shape
        dev = xc.device
        mid = eng.mid
        st = native_autograd._bwd_state(eng)
        dlow = ops.upsample_map_backward(dmap.contiguous().float(), ctx.low_hw)
        dy1, dy1s, dw2, db2, dw3 = native_autograd.backward_to_dy1(eng, st, ws, w2, b2, w3, dlow, split_dy1=need_x)
        dw1 = db1 = dx = None
        if need_b1:
            db1 = torch.empty(mid, dtype=torch.float32, device=dev)
            ops.conv3x3_bias_coord_grad(dy1, 1, db=db1)
        d1 = ops.conv_desc(B, C, H, W, group=C, group_stride=0, batch_stride=C * H * W)
        if need_w1:
            dw1 = ops.conv3x3_wgrad(xc, d1, dy1, 1, C, workspace=native_autograd._wgrad_ws(st, d1, mid, dev))
        if need_x:
            pack = ctx.head.dgrad_pack(C)
            dx = ops.conv3x3_dgrad(dy1 if dy1s is None else dy1s, pack, w1, 1)
            if dx.shape[1] != C:
                dx = dx[:, :C]
            dx = dx.contiguous(memory_format=torch.channels_last if ctx.x_cl else torch.contiguous_format)
        ctx.ws = ctx.xc = None
        return (None, dx, dw1, db1, dw2, db2, dw3)


class DenseFuseHead:
    """``map_classifier`` + the closing ``F.interpolate`` of ``ImageProjVariant`` over the dense world feature.

    ``reducedgrid_shape``: (Ho, Wo) of the returned map (None: the world feature's own size, i.e. no upsample).
    Holds, per world-feature shape, the ``ProjectFuse`` engine whose conv2 / conv3 methods and workspaces run after
    conv1 (built on the first input of that shape), and conv1's weight packs."""

    def __init__(self, reducedgrid_shape=None, precision: str = "bf16x3"):
        self.grid_hw = None if reducedgrid_shape is None else tuple(int(s) for s in reducedgrid_shape)
        if self.grid_hw is not None and (len(self.grid_hw) != 2 or min(self.grid_hw) <= 0):
            raise ValueError(f"reducedgrid_shape must be two positive integers, got {reducedgrid_shape!r}")
        self.precision = precision
        self._engines = {}
        self._pack1 = ops.PackedConv3x3(None, precision)
        self._dgrad = {}

    def out_hw(self, low_hw):
        return tuple(low_hw) if self.grid_hw is None else self.grid_hw

    def engine(self, low_hw, mid_channels: int = 512) -> ProjectFuse:
        """The engine at the world-feature resolution ``low_hw`` (one identity "view" of one channel: its slab is
        allocated with the workspace and never warped)."""
        key = (int(low_hw[0]), int(low_hw[1]), int(mid_channels))
        eng = self._engines.get(key)
        if eng is None:
            eye = [torch.eye(3, dtype=torch.float64)]
            eng = self._engines[key] = ProjectFuse(eye, key[:2], key[:2], 1, mid_channels=key[2],
                                                   precision=self.precision)
        return eng

    def dgrad_pack(self, cin: int) -> "ops.PackedDgrad3x3":
        if cin not in self._dgrad:
            self._dgrad[cin] = ops.PackedDgrad3x3(cin)
        return self._dgrad[cin]

    def conv1(self, eng: ProjectFuse, xc: torch.Tensor, c1, y1: torch.Tensor) -> torch.Tensor:
        """y1 = relu(conv3x3(x) + b1) from the contiguous fp32 ``xc`` [B,C,h,w] into ``y1`` (the engine's layout:
        split-bf16 under bf16x3), bias and ReLU in the conv's epilogue."""
        B, C, H, W = xc.shape
        d1 = ops.conv_desc(B, C, H, W, group=C, group_stride=0, batch_stride=C * H * W)
        return ops.conv3x3_desc(xc, d1, self._pack1.get(c1.weight), eng.mid, bias=c1.bias, dilation=1, relu=True,
                                out=y1, workspace=eng._sk_ws(d1, xc.device))

    def __call__(self, x, w1, b1, w2, b2, w3) -> torch.Tensor:
        """``x``: the fp32 world feature ``[B,C,h,w]`` on a GPU (NCHW or channels-last); ``w1`` [Cout,C,3,3],
        ``b1`` [Cout] or None, ``w2`` [Cout,Cout,3,3], ``b2`` [Cout] or None, ``w3`` [1,Cout,3,3] — the reference's
        ``map_classifier`` parameters.  Returns the ``[B,1,Ho,Wo]`` map.  When autograd is recording and an input
        needs a gradient, the native backward is attached."""
        _check(x, w1, b1, w2, b2, w3, self.grid_hw)
        tensors = [t for t in (x, w1, b1, w2, b2, w3) if t is not None]
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            return DenseFuseFunction.apply(self, x, w1, b1, w2, b2, w3)
        return self.infer(x, w1, b1, w2, b2, w3)

    def infer(self, x, w1, b1, w2, b2, w3) -> torch.Tensor:
        """The inference path: conv1 writes y1 into the engine's cached workspace, then the engine's conv2 -> conv3
        (fused through conv3's partials where the engine fuses them), then the upsample."""
        B, _, H, W = x.shape
        eng = self.engine((H, W), w1.shape[0])
        ws = eng.workspace(B, x.device)
        c1, c2, c3 = _mods(w1.detach(), None if b1 is None else b1.detach(), w2.detach(),
                           None if b2 is None else b2.detach(), w3.detach())
        self.conv1(eng, _nchw(x), c1, ws.y1)
        if eng.conv3_fused_applies(ws):
            eng.conv2_partials(ws, c2, c3)
            low = eng.conv3_from_partials(ws, c3)
        else:
            eng.conv2(ws, c2)
            low = eng.conv3(ws, c3)
        return ops.upsample_map(low, self.out_hw((H, W)))
