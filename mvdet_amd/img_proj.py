"""The front of the reference's ``ImageProjVariant`` (the paper's "early fusion" ablation), native.

``image_proj_variant.py:64-88`` resizes every camera image with a bilinear ``F.interpolate`` (``:67``, 720 x 1280 ->
270 x 480 in the Wildtrack set-up: a DOWNsample), warps the resized 3-channel image onto the ground plane (``:69``)
and concatenates the N warped maps with the coord map (``:88``) into the ``[B, 3 N + 2, Ho, Wo]`` input of a
ResNet-18.  ``mvdet_amd/csrc/img_proj.hip`` does all of it in one launch: every corner of the resized image that a
warp sample reads is evaluated from the full-resolution image (at most 16 taps per sample and channel), the coord
channels are written by the same threads, and the N resized images (6.2 MB each at config 2) are never written.
The output is addressed by element strides, so it is born in the memory format the backbone runs in
(channels-last by default) with bitwise the same values as NCHW.

There is no backward: nothing in front of this op has parameters.  An input that requires a gradient while
autograd is recording raises ``NotImplementedError`` (the gradient is not silently dropped).

Non-finite image values are outside the contract, as non-finite planes are for ``mvdet_amd.thin_fuse`` (a corner
outside the resized image is replaced by 0, not multiplied).  Non-finite *geometry* is inside it: a sample with
non-finite coordinates is NaN in its three channels, as kornia's.
"""
from __future__ import annotations

import torch

from . import _native, ops
from .ops import _stream
from .rig import MAX_VIEWS, Rig, check_views  # noqa: F401  (MAX_VIEWS: this module's public limit)


def _check(n_views, imgs, resized_hw, grid_hw):
    for name, hw in (("resized_hw", resized_hw), ("grid_hw", grid_hw)):
        if len(hw) != 2 or min(int(s) for s in hw) <= 0:
            raise ValueError(f"{name} must be two positive integers, got {hw!r}")
    check_views("imgs", imgs, "the fused image projection", n_views, [],
                lambda p: None if p.dim() == 4 and p.shape[1] == 3 else f"[B,3,H,W], got {tuple(p.shape)}")


def _rows(p: torch.Tensor) -> torch.Tensor:
    """``p`` [B,3,H,W] with column stride 1 (any batch / channel / row stride); a copy only when it is not already."""
    return p if p.stride(3) == 1 or p.shape[3] == 1 else p.contiguous()


def img_proj_forward(imgs, m_norms, resized_hw, grid_hw, channels_last: bool = True, per_pixel: bool = True,
                     out=None) -> torch.Tensor:
    """``mvbev_img_proj_forward_f32``: ``imgs`` N fp32 ``[B,3,H,W]`` tensors on one GPU (slices ``x[:, v]`` of one
    ``[B,N,3,H,W]`` tensor are read in place: any batch, channel or row stride, column stride 1), ``m_norms`` their
    kornia matrices (host) for a source of ``resized_hw``.  Returns a fresh ``[B, 3 N + 2, Ho, Wo]`` fp32 tensor in
    torch's ``channels_last`` memory format, or NCHW without ``channels_last``; the two hold bitwise-equal values.
    ``per_pixel`` (default): one thread per grid pixel walks the views (``MVBEV_IMG_PROJ_PER_PIXEL``); off: one
    thread per (pixel, view) — the same values, and at config 2 the same time within the spread (0.057 ms,
    ``profiles/img_proj_bench.json``).  ``out``: a
    ``[B, 3 N + 2, Ho, Wo]`` fp32 tensor of any non-negative strides to write instead.  Non-finite image values are
    outside the contract."""
    _check(None, imgs, resized_hw, grid_hw)
    n = len(imgs)
    if len(m_norms) != n:
        raise ValueError(f"{len(m_norms)} matrices for {n} views")
    if torch.is_grad_enabled() and any(p.requires_grad for p in imgs):
        raise NotImplementedError("the fused image projection has no backward (nothing in front of it has "
                                  "parameters): detach the images, or run it under torch.no_grad()")
    B, _, H, W = imgs[0].shape
    Hr, Wr = int(resized_hw[0]), int(resized_hw[1])
    Ho, Wo = int(grid_hw[0]), int(grid_hw[1])
    shape = (B, 3 * n + 2, Ho, Wo)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=imgs[0].device,
                          memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != imgs[0].device:
        raise ValueError(f"out must be an fp32 {shape} tensor on {imgs[0].device}")
    arr = ops._view_table([_rows(p.detach()) for p in imgs], m_norms)
    _native.check(_native.load().mvbev_img_proj_forward_f32(
        arr, n, B, H, W, Hr, Wr, Ho, Wo, out.data_ptr(), _native.strides4(out),
        _native.IMG_PROJ_PER_PIXEL if per_pixel else 0, _stream(out)), "mvbev_img_proj_forward_f32")
    return out


class ImageProjection(Rig):
    """The front of ``ImageProjVariant`` for one camera rig: ``proj_mats`` the reference's per-camera 3x3
    ``proj_mats`` (resized-image pixels -> grid pixels), ``upsample_shape`` (Hr, Wr) of the resized images,
    ``reducedgrid_shape`` (Ho, Wo).  Holds the normalised matrices, computed as every other head computes them."""

    def __call__(self, imgs, channels_last: bool = True, per_pixel: bool = True) -> torch.Tensor:
        """``imgs``: one fp32 ``[B,3,H,W]`` tensor per view, or one ``[B,N,3,H,W]`` tensor (its slices are read in
        place).  Returns ``[B, 3 N + 2, Ho, Wo]``."""
        if isinstance(imgs, torch.Tensor):
            if imgs.dim() != 5:
                raise ValueError(f"imgs must be [B,N,3,H,W] or a sequence of [B,3,H,W], got {tuple(imgs.shape)}")
            imgs = list(imgs.unbind(1))
        _check(self.num_views, imgs, self.up_hw, self.grid_hw)
        return img_proj_forward(imgs, self.m_norm_cpu, self.up_hw, self.grid_hw, channels_last=channels_last,
                                per_pixel=per_pixel)
