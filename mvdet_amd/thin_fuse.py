"""The ground-plane head of the reference's ``ResProjVariant`` (the paper's "late fusion" ablation), native.

``res_proj_variant.py:70-82`` warps ONE plane per view (the foot channel of the image result), concatenates the N
warped planes with the coord map and runs ``Conv2d(N + 2, 512, 3, padding=1) -> ReLU -> Conv2d(512, 512, 3,
dilation 2) -> ReLU -> Conv2d(512, 1, 3, dilation 4)``.  The first conv has N + 2 input channels (K = 81 at
config 2): its cost is the write of y1, so ``mvdet_amd/csrc/thin_conv1.hip`` does warp + coord channels + conv1 +
bias + ReLU in one fp32 launch that writes y1 once, in the layout conv2 reads.  Everything after y1 is the
``ProjectFuse`` engine's own code: conv2 -> conv3 partials in inference (direct or row-Winograd by the engine's
own rules), conv2 / conv3 and their native backward in training (``autograd.backward_to_dy1``).  The engine here
is a ``ProjectFuse(..., channels=1)`` whose slab is never warped.

Training keeps y1 (split-bf16), y2 and the N warped planes ``xw`` (1.2 MB at config 2).  The backward's new
kernels give the gradient of the warped planes and the view channels of conv1's weight gradient (fixed-order
sums, no float atomics); the bias and coord-channel gradients come from ``ops.conv3x3_bias_coord_grad`` and the
gradient to the planes from ``ops.warp_views_adjoint`` with the plain plans (C = 1).

Non-finite *geometry* is inside the contract (a NaN sample reaches exactly its 3 x 3 neighbourhood in y1, as the
reference's direct conv makes it).  So are non-finite conv1 *parameters*: a view is skipped over a tile only when
its geometry is dead there AND its w1 columns are finite (``ProjectThinFuse.w1_mask``: a device word per weight
version, read by every block), so y1 keeps the reference's ``0 * NaN = NaN`` pixels.  Non-finite *planes* are
outside it, as for ``mvdet_amd.sum_head``, and conv2 / conv3 behind y1 are the engine's fast kernels.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import _native, ops
from . import autograd as native_autograd
from .ops import _stream
from .pipeline import ProjectFuse, Workspace, band_rows
from .rig import MAX_VIEWS, Rig, check_views  # noqa: F401  (MAX_VIEWS: this module's public limit)


def _check(n_views, src_hw, planes, w1, b1, w2, b2, w3):
    params = [("w1", w1), ("w2", w2), ("w3", w3)] + [(k, t) for k, t in (("b1", b1), ("b2", b2)) if t is not None]
    check_views("planes", planes, "the thin fused conv1", n_views, params,
                lambda p: None if p.dim() == 4 and p.shape[1] == 1 else f"[B,1,H,W], got {tuple(p.shape)}")
    p0 = planes[0]
    if tuple(p0.shape[2:]) != tuple(src_hw):
        raise ValueError(f"planes are {tuple(p0.shape[2:])}, the head was built for {tuple(src_hw)}")
    mid = w1.shape[0] if w1.dim() == 4 else -1
    if w1.dim() != 4 or tuple(w1.shape[1:]) != (n_views + 2, 3, 3) or mid % 8:
        raise ValueError(f"w1 must be [Cout, {n_views + 2}, 3, 3] with Cout % 8 == 0, got {tuple(w1.shape)}")
    if tuple(w2.shape) != (mid, mid, 3, 3):
        raise ValueError(f"w2 must be [{mid}, {mid}, 3, 3], got {tuple(w2.shape)}")
    if tuple(w3.shape) != (1, mid, 3, 3):
        raise ValueError(f"w3 must be [1, {mid}, 3, 3], got {tuple(w3.shape)}")
    for name, t in (("b1", b1), ("b2", b2)):
        if t is not None and tuple(t.shape) != (mid,):
            raise ValueError(f"{name} must be [{mid}], got {tuple(t.shape)}")


def _rows(p: torch.Tensor) -> torch.Tensor:
    """``p`` [B,1,H,W] with column stride 1 (any batch / channel stride); a copy only when it is not already."""
    return p if p.stride(3) == 1 or p.shape[3] == 1 else p.contiguous()


def thin_conv1_weight_mask(w1: torch.Tensor, n_views: int, out=None) -> torch.Tensor:
    """``mvbev_thin_conv1_weight_mask``: a device int32 word, bit v set when ``w1[:, v]`` holds a NaN / inf."""
    if not w1.is_contiguous() or w1.dtype != torch.float32 or tuple(w1.shape[1:]) != (n_views + 2, 3, 3):
        raise ValueError(f"w1 must be a contiguous fp32 [Cout, {n_views + 2}, 3, 3] tensor")
    if out is None:
        out = torch.empty(1, dtype=torch.int32, device=w1.device)
    _native.check(_native.load().mvbev_thin_conv1_weight_mask(w1.data_ptr(), n_views, w1.shape[0], out.data_ptr(),
                                                              _stream(w1)), "mvbev_thin_conv1_weight_mask")
    return out


def thin_conv1_forward(planes, m_norms, grid_hw, w1, b1, y1: torch.Tensor, xw=None, w_mask=None) -> torch.Tensor:
    """``mvbev_thin_conv1_forward_f32_ex``: ``planes`` N fp32 ``[B,1,H,W]`` tensors with column stride 1, ``m_norms``
    their kornia matrices (host), ``w1`` ``[Cout,N+2,3,3]``, ``b1`` ``[Cout]`` or None, ``y1`` a contiguous fp32
    ``[B,Cout,Ho,Wo]`` or split-bf16 (``ops.split_shape``) tensor, ``xw`` None or fp32 ``[B,N,Ho,Wo]``, ``w_mask``
    None (finite weights taken for granted) or ``thin_conv1_weight_mask``'s word for this ``w1``."""
    n = len(planes)
    B, _, H, W = planes[0].shape
    Ho, Wo = int(grid_hw[0]), int(grid_hw[1])
    cout = w1.shape[0]
    layout = ops._out_layout(y1, B, cout, Ho, Wo)
    arr = ops._view_table(planes, m_norms, unit_dim=3)  # (a single column: any stride torch reports)
    if not w1.is_contiguous() or (b1 is not None and not b1.is_contiguous()):
        raise ValueError("w1 and b1 must be contiguous")
    if xw is not None and (tuple(xw.shape) != (B, n, Ho, Wo) or xw.dtype != torch.float32 or not xw.is_contiguous()):
        raise ValueError(f"xw must be a contiguous fp32 {(B, n, Ho, Wo)} tensor")
    if w_mask is not None and (w_mask.dtype != torch.int32 or w_mask.numel() < 1 or w_mask.device != y1.device):
        raise ValueError("w_mask must be an int32 word on y1's device")
    _native.check(_native.load().mvbev_thin_conv1_forward_f32_ex(
        arr, n, B, H, W, Ho, Wo, w1.data_ptr(), None if b1 is None else b1.data_ptr(), cout, y1.data_ptr(), layout,
        None if xw is None else xw.data_ptr(), None if w_mask is None else w_mask.data_ptr(), _stream(y1)),
        "mvbev_thin_conv1_forward_f32_ex")
    return y1


def thin_conv1_backward(dpre: torch.Tensor, w1: torch.Tensor, xw, n_views: int, need_dx: bool = True, dw=None):
    """``mvbev_thin_conv1_backward_f32`` (+ ``_grad_weight_f32``): ``dpre`` the masked gradient of the
    pre-activation, contiguous fp32 ``[B,Cout,Ho,Wo]``.  Returns ``dxw`` ``[B,N,Ho,Wo]`` (None without ``need_dx``);
    with ``dw`` (a contiguous ``[Cout,N+2,3,3]`` tensor) its N view channels are overwritten with the weight
    gradient (``xw``: the forward's warped planes)."""
    lib = _native.load()
    B, cout, Ho, Wo = dpre.shape
    if dpre.dtype != torch.float32 or not dpre.is_contiguous() or not w1.is_contiguous():
        raise ValueError("dpre and w1 must be contiguous fp32 tensors")
    dev = dpre.device
    dxw = torch.empty((B, n_views, Ho, Wo), dtype=torch.float32, device=dev) if need_dx else None
    partials, blocks = None, 0
    if dw is not None:
        if tuple(dw.shape) != (cout, n_views + 2, 3, 3) or dw.dtype != torch.float32 or not dw.is_contiguous():
            raise ValueError(f"dw must be a contiguous fp32 {(cout, n_views + 2, 3, 3)} tensor")
        blocks = _native.backward_blocks("mvbev_thin_conv1_backward_blocks", B, Ho, Wo)
        partials = torch.empty(blocks * cout * n_views * 9, dtype=torch.float32, device=dev)
    if dxw is None and partials is None:
        return None
    stream = _stream(dpre)
    _native.check(lib.mvbev_thin_conv1_backward_f32(
        dpre.data_ptr(), w1.data_ptr(), None if xw is None else xw.data_ptr(), n_views, B, cout, Ho, Wo,
        None if dxw is None else dxw.data_ptr(), None if partials is None else partials.data_ptr(),
        0 if partials is None else partials.numel(), stream), "mvbev_thin_conv1_backward_f32")
    if partials is not None:
        _native.check(lib.mvbev_thin_conv1_grad_weight_f32(partials.data_ptr(), blocks, n_views, cout, dw.data_ptr(),
                                                           stream), "mvbev_thin_conv1_grad_weight_f32")
    return dxw


def _mods(w1, b1, w2, b2, w3):
    return (SimpleNamespace(weight=w1, bias=b1), SimpleNamespace(weight=w2, bias=b2),
            SimpleNamespace(weight=w3, bias=None))


class ThinFuseFunction(torch.autograd.Function):
    """``map = conv3(relu(conv2(relu(conv1(cat(warp(planes[v]) for v) + coord)))))``; inputs after the head: w1, b1,
    w2, b2, w3, then the N planes.  Forward: the thin kernel, then the engine's conv2 and conv3 (y2 kept).
    Backward: ``autograd.backward_to_dy1``, then the thin kernel's backward and the warp adjoint.  The saved
    activations are released after the first backward."""

    @staticmethod
    def forward(ctx, head, w1, b1, w2, b2, w3, *planes):
        eng = head.engine
        B = planes[0].shape[0]
        dev = planes[0].device
        H, W = eng.grid_hw
        n = head.num_views
        y1r, y2r = band_rows(0, H, H)
        if eng.y1_split:
            y1 = torch.empty(ops.split_shape(B, eng.mid, H, W), dtype=torch.bfloat16, device=dev)
        else:
            y1 = torch.empty((B, eng.mid, H, W), dtype=torch.float32, device=dev)
        y2 = torch.empty((B, eng.mid, H, W), dtype=torch.float32, device=dev)
        # (the engine's slab is never warped here: an empty one stands in)
        slab = torch.empty((eng.S, B, 0), dtype=torch.bfloat16, device=dev)
        ws = Workspace(slab, y1, y2, eng.m_norm_cpu, (0, H), y1r, y2r, store_y2=True, slab_rows=(0, H))
        xw = torch.empty((B, n, H, W), dtype=torch.float32, device=dev)
        c1, c2, c3 = _mods(w1.detach(), None if b1 is None else b1.detach(), w2.detach(),
                           None if b2 is None else b2.detach(), w3.detach())
        w1c = c1.weight.contiguous()
        thin_conv1_forward([_rows(p.detach()) for p in planes], eng.m_norm_cpu, (H, W), w1c,
                           None if c1.bias is None else c1.bias.contiguous(), y1, xw, w_mask=head.w1_mask(c1.weight, w1c))
        eng.conv2(ws, c2)
        out = eng.conv3(ws, c3)
        ctx.head, ctx.ws, ctx.xw = head, ws, xw
        ctx.plane_shape = tuple(planes[0].shape)
        ctx.save_for_backward(w1, b1, w2, b2, w3)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dmap):
        ws = ctx.ws
        if ws is None:
            raise RuntimeError("ThinFuseFunction: trying to backward through this graph a second time; its saved "
                               "activations (xw, y1, y2) are released after the first backward (the native "
                               "kernels keep no retain_graph copy). Run the forward again.")
        head = ctx.head
        eng = head.engine
        w1, b1, w2, b2, w3 = ctx.saved_tensors
        n = head.num_views
        need_w1, need_b1 = ctx.needs_input_grad[1], ctx.needs_input_grad[2] and b1 is not None
        need_planes = ctx.needs_input_grad[6:]
        dev = ws.y1.device
        mid = eng.mid
        st = native_autograd._bwd_state(eng)
        dy1, _, dw2, db2, dw3 = native_autograd.backward_to_dy1(eng, st, ws, w2, b2, w3, dmap, split_dy1=False)
        dw1 = db1 = None
        if need_w1 or need_b1:
            dw1 = torch.zeros_like(w1, memory_format=torch.contiguous_format) if need_w1 else None
            db1 = torch.empty(mid, dtype=torch.float32, device=dev) if need_b1 else None
            ops.conv3x3_bias_coord_grad(dy1, 1, db=db1, dw=dw1, coord_ch=n)
        dxw = thin_conv1_backward(dy1, w1.detach().contiguous(), ctx.xw, n, need_dx=any(need_planes), dw=dw1)
        grads = [None] * n
        idx = [i for i, want in enumerate(need_planes) if want]  # a view that needs no gradient is not gathered
        if idx:
            plans = head.plans(dev)
            for i in idx:
                grads[i] = torch.empty(ctx.plane_shape, dtype=torch.float32, device=dev)
            ops.warp_views_adjoint([dxw[:, i:i + 1] for i in idx], [plans[i] for i in idx], [grads[i] for i in idx])
        ctx.ws = ctx.xw = None
        return (None, dw1, db1, dw2, db2, dw3, *grads)


class ProjectThinFuse(Rig):
    """``map_classifier`` of ``ResProjVariant`` over the warped foot planes, for one camera rig.

    ``proj_mats``: the reference's per-camera 3x3 ``proj_mats`` (image-result pixels -> grid pixels);
    ``upsample_shape``: (H, W) of the planes; ``reducedgrid_shape``: (Ho, Wo).  Holds the normalised matrices
    (computed as ``ProjectFuse`` / ``ProjectSumHead`` compute them: the internal engine's), the engine whose
    conv2 / conv3 methods and workspaces run after the thin kernel, and per device the adjoint plans."""

    def __init__(self, proj_mats, upsample_shape, reducedgrid_shape, mid_channels: int = 512):
        super().__init__(proj_mats, upsample_shape, reducedgrid_shape)
        # conv2 / conv3, their workspaces and the direct-vs-Winograd rules are the engine's; its slab (one padded
        # 8-channel slot per view) is allocated with the workspace and never warped
        self.engine = ProjectFuse(self.mats, self.up_hw, self.grid_hw, 1, mid_channels=mid_channels)
        self.m_norm_cpu = self.engine.m_norm_cpu  # (the engine's tensor: the same values, one object)

    def plans(self, device):
        dev = torch.device(device)
        return self.cached(("plans", dev), lambda: [ops.WarpAdjointPlan(m, self.up_hw, self.grid_hw, dev)
                                                    for m in self.m_norm_cpu])

    def w1_mask(self, w1: torch.Tensor, w1c: torch.Tensor) -> torch.Tensor:
        """The views whose conv1 columns hold a NaN / inf (``thin_conv1_weight_mask`` of ``w1c``, the contiguous
        form of ``w1``), once per weight version (keyed on ``w1``'s ``(data_ptr, _version, strides)``, per device;
        one small launch into a word of the head's, no host sync): the thin kernel evaluates those views over
        every tile."""
        st = self.cached(("w1_mask", w1.device), lambda: SimpleNamespace(
            word=torch.zeros(1, dtype=torch.int32, device=w1.device), key=None))
        key = (w1.data_ptr(), w1._version, tuple(w1.stride()))
        if key != st.key:
            thin_conv1_weight_mask(w1c, self.num_views, st.word)
            st.key = key
        return st.word

    def __call__(self, planes, w1, b1, w2, b2, w3) -> torch.Tensor:
        """``planes``: one fp32 ``[B,1,H,W]`` tensor per view on one GPU (any batch / channel stride: a channel
        slice of the image result is read in place; a plane whose column stride is not 1 is copied);
        ``w1`` [Cout,N+2,3,3], ``b1`` [Cout] or None, ``w2`` [Cout,Cout,3,3], ``b2`` [Cout] or None, ``w3``
        [1,Cout,3,3] — the reference's ``map_classifier`` parameters.  Returns the ``[B,1,Ho,Wo]`` map.  When
        autograd is recording and an input needs a gradient, the native backward is attached."""
        _check(self.num_views, self.up_hw, planes, w1, b1, w2, b2, w3)
        if w1.shape[0] != self.engine.mid:
            raise ValueError(f"w1 has {w1.shape[0]} output channels, the head was built for {self.engine.mid}")
        tensors = list(planes) + [t for t in (w1, b1, w2, b2, w3) if t is not None]
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            return ThinFuseFunction.apply(self, w1, b1, w2, b2, w3, *planes)
        return self.infer(planes, w1, b1, w2, b2, w3)

    def infer(self, planes, w1, b1, w2, b2, w3) -> torch.Tensor:
        """The inference path: the thin kernel writes y1 into the engine's cached workspace, then the engine's
        conv2 -> conv3 (fused through conv3's partials where the engine fuses them)."""
        eng = self.engine
        B, dev = planes[0].shape[0], planes[0].device
        ws = eng.workspace(B, dev)
        c1, c2, c3 = _mods(w1.detach(), None if b1 is None else b1.detach(), w2.detach(),
                           None if b2 is None else b2.detach(), w3.detach())
        w1c = c1.weight.contiguous()
        thin_conv1_forward([_rows(p.detach()) for p in planes], self.m_norm_cpu, self.grid_hw, w1c,
                           None if c1.bias is None else c1.bias.contiguous(), ws.y1, w_mask=self.w1_mask(c1.weight, w1c))
        if eng.conv3_fused_applies(ws):
            eng.conv2_partials(ws, c2, c3)
            return eng.conv3_from_partials(ws, c3)
        eng.conv2(ws, c2)
        return eng.conv3(ws, c3)
