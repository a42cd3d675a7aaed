"""The camera-frame front: decoded uint8 frames to the normalized fp32 views the detectors take, in one launch.

The reference builds ``T.Compose([T.Resize([720, 1280]), T.ToTensor(), normalize])`` (``main.py:38-40``) and
``frameDataset.__getitem__`` applies it to every camera's decoded ``PIL.Image``, one after another
(``frameDataset.py:127-133``): Pillow's antialiased bilinear resize on one host core, a float conversion, a normalize,
a stack, and the fp32 result over PCIe.  Here the decoded bytes go up as they are (``pack_frames``: one pinned uint8
buffer, a quarter of the fp32 bytes at the resized size) and ``mvdet_amd/csrc/frames.hip`` does the rest for every view
and batch item in one launch.

The arithmetic is integer and exact, so the result is bit for bit the CPU transform's:

* Pillow resizes 8-bit images in two separable passes, horizontal first, with coefficients in 22-bit fixed point, and
  rounds and clips to uint8 after each pass.  ``resample_table`` restates its ``precompute_coeffs`` and
  ``normalize_coeffs_8bpc`` for the bilinear filter in float64.
* ``ToTensor`` and ``Normalize`` map each of a channel's 256 byte values to one fp32 value: ``value_table`` runs the
  transform's own torch-CPU ops on a ramp.

``resize_normalize`` is the op, ``FrameTransform`` the counterpart of the reference's ``train_trans`` (a callable that
holds the tables of its sizes), ``pack_frames`` the host side of one upload per frame.  Only the bilinear filter on
three-channel 8-bit frames is covered; all views of a call share one input size.  There is no backward and no CPU
fallback.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native
from .ops import _stream
from .rig import MAX_VIEWS

__all__ = ["FrameTransform", "resize_normalize", "resample_table", "value_table", "supported", "pack_frames"]

PRECISION_BITS = 32 - 8 - 2  # Pillow's fixed-point precision for 8-bit images
MAX_TAPS = 64                # taps per axis the kernel's tables may hold
LDS_LIMIT = 65536            # bytes of LDS one workgroup of the kernel may stage
TILES = ((16, 64), (8, 64), (8, 32))  # (rows, columns) of output per workgroup, in the order they are tried

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)  # main.py:37

_tables: dict = {}
_luts: dict = {}


def ksize(in_size: int, out_size: int) -> int:
    """Pillow's coefficient row length for the bilinear filter: ``ceil(support) * 2 + 1`` with ``support`` =
    ``max(in / out, 1)``."""
    return int(math.ceil(max(float(in_size) / out_size, 1.0))) * 2 + 1


def resample_table(in_size: int, out_size: int):
    """``(bounds [out, 2] int32, coef [out, ksize] int32)`` of one axis, as Pillow's ``precompute_coeffs`` and
    ``normalize_coeffs_8bpc`` build them for ``Image.BILINEAR`` on an 8-bit image: ``bounds[x]`` = (first input
    index, tap count), ``coef[x, :count]`` the taps' weights times ``2 ** 22``, rounded half away from zero; the
    rest of a row is 0.  float64 throughout, in Pillow's order of operations."""
    n_in, n_out = int(in_size), int(out_size)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"sizes must be positive, got {in_size} -> {out_size}")
    scale = float(n_in) / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in)
    count = xmax - xmin
    x = np.arange(ks, dtype=np.int64)[None, :]
    arg = np.abs(((x + xmin[:, None]) - center[:, None] + 0.5) * ss)
    w = np.where((arg < 1.0) & (x < count[:, None]), 1.0 - arg, 0.0)
    ww = np.zeros(n_out, dtype=np.float64)
    for k in range(ks):  # Pillow's left-to-right sum, term by term (np.sum would pair the terms)
        ww += w[:, k]
    ww = ww[:, None]
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    coef = np.trunc(0.5 + w * float(1 << PRECISION_BITS)).astype(np.int32)
    bounds = np.stack([xmin, count], axis=1).astype(np.int32)
    return bounds, coef


def value_table(mean=IMAGENET_MEAN, std=IMAGENET_STD) -> torch.Tensor:
    """``[3, 256]`` fp32 on the host: what ``T.ToTensor()`` then ``T.Normalize(mean, std)`` make of byte ``v`` in
    channel ``c``, by the transform's own torch ops in its own order (``to(float32).div(255)``, ``sub_(mean)``,
    ``div_(std)`` with ``mean`` and ``std`` as float32)."""
    mean_t = torch.as_tensor(mean, dtype=torch.float32).reshape(-1)
    std_t = torch.as_tensor(std, dtype=torch.float32).reshape(-1)
    if mean_t.numel() != 3 or std_t.numel() != 3:
        raise ValueError("mean and std must hold three values (one per channel)")
    if bool((std_t == 0).any()):
        raise ValueError("std holds a zero (T.Normalize refuses it too)")
    x = torch.arange(256, dtype=torch.uint8).repeat(3, 1).to(torch.float32).div(255)
    return x.sub_(mean_t[:, None]).div_(std_t[:, None])


def _box_cap(n_in: int, n_out: int, ks: int, tile: int) -> int:
    """Input positions the staged box of ``tile`` outputs can span (``fr_cap`` of frames.hip, the same doubles)."""
    span = float(tile - 1) * (float(n_in) / float(n_out)) + float(ks - 1) + 1.0
    return min(n_in, int(span) + 2)


def lds_bytes(in_hw, out_hw, tile) -> int:
    """LDS one workgroup stages for a ``tile`` = (rows, columns) of output (``fr_layout`` of frames.hip)."""
    (H, W), (h, w), (th, tw) = in_hw, out_hw, tile
    ksx, ksy = ksize(W, w), ksize(H, h)
    cap_w, cap_h = _box_cap(W, w, ksx, tw), _box_cap(H, h, ksy, th)
    pitch = (cap_w * 3 + 3 + 3) // 4 * 4
    return 3 * 256 * 4 + tw * (ksx + 2) * 4 + th * (ksy + 2) * 4 + cap_h * pitch + cap_h * tw * 3


def pick_tile(in_hw, out_hw):
    """The output tile the kernel takes for this resize: the first of ``TILES`` whose staged box fits, or None."""
    (H, W), (h, w) = in_hw, out_hw
    if max(ksize(W, w), ksize(H, h)) > MAX_TAPS:
        return None
    for tile in TILES:
        if lds_bytes(in_hw, out_hw, tile) <= LDS_LIMIT:
            return tile
    return None


def supported(in_hw, out_hw, n_views: int = 1) -> bool:
    """Whether one launch holds this resize: 1 .. 16 views, positive sizes, and an input box per output tile that
    fits the kernel's LDS at its smallest tile (downscales up to 7x on both axes; any upscale)."""
    (H, W), (h, w) = (int(s) for s in in_hw), (int(s) for s in out_hw)
    if min(H, W, h, w) <= 0 or not 0 < int(n_views) <= MAX_VIEWS:
        return False
    return pick_tile((H, W), (h, w)) is not None


def _device_tables(n_in, n_out, device):
    key = (int(n_in), int(n_out), str(device))
    hit = _tables.get(key)
    if hit is None:
        bounds, coef = resample_table(n_in, n_out)
        hit = _tables[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(coef).to(device), coef.shape[1])
    return hit


def _device_lut(mean, std, device):
    key = (tuple(float(m) for m in mean), tuple(float(s) for s in std), str(device))
    hit = _luts.get(key)
    if hit is None:
        hit = _luts[key] = value_table(mean, std).to(device)
    return hit


def _views_of(frames):
    """The per-view ``[B, H, W, 3]`` uint8 tensors of ``frames``, checked."""
    if isinstance(frames, torch.Tensor):
        if frames.dim() != 5:
            raise ValueError(f"frames must be [B,N,H,W,3] or a sequence of [B,H,W,3], got {tuple(frames.shape)}")
        views = list(frames.unbind(1))
    elif hasattr(frames, "__len__"):
        views = list(frames)
    else:
        raise TypeError(f"frames must be a tensor or a sequence of tensors, got {type(frames).__name__}")
    if not 0 < len(views) <= MAX_VIEWS:
        raise ValueError(f"1 .. {MAX_VIEWS} views per call, got {len(views)}")
    for i, t in enumerate(views):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"frames[{i}] must be a tensor, got {type(t).__name__}")
        if t.dim() != 4 or t.shape[3] != 3:
            raise ValueError(f"frames[{i}] must be [B,H,W,3] (decoded RGB, channels innermost), got {tuple(t.shape)}")
        if t.dtype != torch.uint8:
            raise TypeError(f"frames[{i}] must be uint8 (decoded bytes; float images are already transformed), "
                            f"got {t.dtype}")
        if t.requires_grad:
            raise ValueError("the frame transform has no backward")
        if t.shape != views[0].shape:
            raise ValueError(f"frames[{i}] {tuple(t.shape)} differs from frames[0] {tuple(views[0].shape)}")
        if t.device != views[0].device:
            raise ValueError(f"frames[{i}] is on {t.device}, frames[0] on {views[0].device}")
    if min(views[0].shape) == 0:
        raise ValueError(f"empty frames[0] {tuple(views[0].shape)}")
    return views


def _in_place(p: torch.Tensor) -> torch.Tensor:
    """``p`` [B,H,W,3] with channel stride 1 and pixel stride 3 (any batch and row stride >= 0: a slice of a wider
    buffer); a copy only when it is not already."""
    B, H, W, _ = p.shape
    ok = p.stride(3) == 1 and (W == 1 or p.stride(2) == 3) and p.stride(0) >= 0 and p.stride(1) >= 0
    return p if ok else p.contiguous()


def resize_normalize(frames, size, mean=IMAGENET_MEAN, std=IMAGENET_STD, channels_last: bool = True,
                     out=None) -> torch.Tensor:
    """``T.Normalize(mean, std)(T.ToTensor()(T.Resize(size)(frame)))`` of every frame, bit for bit, in one launch
    (``mvbev_frames_resize_normalize_u8``).

    ``frames``: a uint8 ``[B,N,H,W,3]`` tensor on a ROCm GPU, or a sequence of N ``[B,H,W,3]`` tensors (decoded RGB;
    slices of a wider buffer are read in place: any batch and row stride).  ``size``: ``(h, w)``.  Returns an fp32
    ``[B,N,3,h,w]`` tensor whose every ``out[:, v]`` is contiguous in torch's ``channels_last`` memory format (what
    the detectors' backbone runs in), or NCHW-contiguous without ``channels_last``; the two hold bitwise-equal
    values.  ``out``: an fp32 ``[B,N,3,h,w]`` tensor of any non-negative strides to write instead.  A resize that
    ``supported`` refuses raises ``ValueError``."""
    views = _views_of(frames)
    if len(size) != 2 or min(int(s) for s in size) <= 0:
        raise ValueError(f"size must be two positive integers (h, w), got {size!r}")
    h, w = int(size[0]), int(size[1])
    n = len(views)
    B, H, W, _ = views[0].shape
    dev = views[0].device
    shape = (B, n, 3, h, w)
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape
                            or out.dtype != torch.float32 or out.device != dev):
        raise ValueError(f"out must be an fp32 {shape} tensor on {dev}")
    if not supported((H, W), (h, w), n):
        raise ValueError(f"the resize {H} x {W} -> {h} x {w} is outside the kernel's range: the input box of its "
                         f"smallest output tile {TILES[-1]} needs {lds_bytes((H, W), (h, w), TILES[-1])} bytes of "
                         f"LDS, above {LDS_LIMIT}")
    if dev.type != "cuda":
        raise ValueError(f"frames are on {dev}: the frame transform runs on a ROCm GPU only (no CPU fallback)")
    if out is None:
        if channels_last:
            out = torch.empty((n, B, h, w, 3), dtype=torch.float32, device=dev).permute(1, 0, 4, 2, 3)
        else:
            out = torch.empty((n, B, 3, h, w), dtype=torch.float32, device=dev).transpose(0, 1)
    elif min(out.stride()) < 0:
        raise ValueError("out must have non-negative strides")
    bx, cx, ksx = _device_tables(W, w, dev)
    by, cy, ksy = _device_tables(H, h, dev)
    lut = _device_lut(mean, std, dev)
    keep = [_in_place(p) for p in views]
    arr = (_native.FrameView * n)()
    for i, p in enumerate(keep):
        arr[i].src, arr[i].batch_stride, arr[i].row_stride = p.data_ptr(), p.stride(0), p.stride(1)
    _native.check(_native.load().mvbev_frames_resize_normalize_u8(
        arr, n, B, H, W, h, w, bx.data_ptr(), cx.data_ptr(), ksx, by.data_ptr(), cy.data_ptr(), ksy, lut.data_ptr(),
        out.data_ptr(), (_native._i64 * 5)(*out.stride()), _stream(out)), "mvbev_frames_resize_normalize_u8")
    return out


class FrameTransform:
    """The GPU counterpart of ``main.py``'s ``train_trans``: ``FrameTransform(size, mean, std)(frames)`` is
    ``resize_normalize(frames, size, mean, std)``.  The value table is checked at construction; the coefficient
    tables of every input size it meets are built and uploaded once per device."""

    def __init__(self, size=(720, 1280), mean=IMAGENET_MEAN, std=IMAGENET_STD, channels_last: bool = True):
        if len(size) != 2 or min(int(s) for s in size) <= 0:
            raise ValueError(f"size must be two positive integers (h, w), got {size!r}")
        self.size = (int(size[0]), int(size[1]))
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        self.channels_last = bool(channels_last)
        self.lut = value_table(self.mean, self.std)  # (host copy: raises on a bad mean / std)

    def __call__(self, frames, out=None) -> torch.Tensor:
        return resize_normalize(frames, self.size, self.mean, self.std, channels_last=self.channels_last, out=out)

    def takes(self, x) -> bool:
        """Whether ``x`` is decoded frames (a uint8 ``[B,N,H,W,3]`` tensor) and not an already transformed fp32
        ``[B,N,3,h,w]`` input: what a detector built with ``frame_transform=`` asks before its forward."""
        return isinstance(x, torch.Tensor) and x.dtype == torch.uint8 and x.dim() == 5 and x.shape[-1] == 3

    def __repr__(self):
        return f"FrameTransform(size={self.size}, mean={self.mean}, std={self.std})"


def pack_frames(images) -> torch.Tensor:
    """N decoded images of one size (anything ``np.asarray`` turns into ``H x W x 3`` uint8: a ``PIL.Image`` in mode
    RGB, an array) in one pinned uint8 ``[1,N,H,W,3]`` tensor, for one ``.to(device, non_blocking=True)`` per frame.
    The role ``targets.pack_step`` plays for the ground truth.  Without a GPU runtime the buffer is not pinned."""
    arrays = [np.asarray(im) for im in images]
    if not 0 < len(arrays) <= MAX_VIEWS:
        raise ValueError(f"1 .. {MAX_VIEWS} views per frame, got {len(arrays)}")
    for i, a in enumerate(arrays):
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise ValueError(f"images[{i}] must be H x W x 3 uint8 (decoded RGB), got {a.shape} {a.dtype}")
        if a.shape != arrays[0].shape:
            raise ValueError(f"images[{i}] {a.shape} differs from images[0] {arrays[0].shape}")
    H, W, _ = arrays[0].shape
    buf = torch.empty((1, len(arrays), H, W, 3), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    dst = buf.numpy()
    for i, a in enumerate(arrays):
        dst[0, i] = a
    return buf
