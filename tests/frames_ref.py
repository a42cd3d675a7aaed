"""A numpy restatement of the reference's frame transform ``T.Compose([T.Resize(size), T.ToTensor(), normalize])``
(``main.py:38-40``) for the frame tests: Pillow's 8-bit bilinear ``Image.resize`` as its C code does it, one output
position at a time in plain Python floats (C doubles), then ``ToTensor`` / ``Normalize`` by the transform's own
torch-CPU ops.  Written apart from ``mvdet_amd.frames`` on purpose (scalar loops, no shared code).

Pillow (``src/libImaging/Resample.c``): ``precompute_coeffs`` builds per output position the first input index, the
tap count and the normalised weights of the filter (bilinear: ``1 - |x|`` on a support of ``max(in / out, 1)``);
``normalize_coeffs_8bpc`` turns them into 22-bit fixed point; ``ImagingResampleHorizontal_8bpc`` then
``ImagingResampleVertical_8bpc`` accumulate ``ss = 1 << 21; ss += px * k`` in int32 and store ``clip8(ss)`` =
``clamp(ss >> 22, 0, 255)`` as uint8 after EACH pass; a pass whose sizes are equal is skipped.
"""
import math
from pathlib import Path

import numpy as np
import torch

PRECISION_BITS = 32 - 8 - 2
GOLDEN = Path(__file__).resolve().parent / "golden" / "frames_pil.npz"

# (input H x W, output h x w) pairs the restatement was checked on against live Pillow
SHAPE_PAIRS = [((1080, 1920), (720, 1280)), ((1080, 1920), (270, 480)), ((2160, 3840), (720, 1280)),
               ((37, 53), (16, 24)), ((23, 41), (23, 17)), ((16, 24), (37, 53)), ((9, 11), (9, 11)),
               ((31, 17), (7, 40))]


def coeffs(in_size, out_size):
    """``(bounds [out, 2], kk [out, ksize])`` int32 of one axis: ``precompute_coeffs`` + ``normalize_coeffs_8bpc``."""
    scale = float(in_size) / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)  # (int() truncates, as the C cast)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ww, k = 0.0, [0.0] * ksize
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            k[x] = 1.0 - a if a < 1.0 else 0.0
            ww += k[x]
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
        bounds[xx] = (xmin, xmax)
        kk[xx] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in k]
    return bounds, kk


def _pass(img, bounds, kk, axis):
    """One pass along ``axis`` (0: vertical, 1: horizontal) of an ``[H, W, C]`` uint8 image."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(bounds),) + src.shape[1:], dtype=np.uint8)
    for o, (first, count) in enumerate(bounds):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for t in range(count):
            acc += src[first + t] * int(kk[o, t])
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, size):
    """``Image.fromarray(img).resize((w, h), Image.BILINEAR)`` of an ``[H, W, 3]`` uint8 array, ``size`` = (h, w)."""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    (H, W), (h, w) = img.shape[:2], size
    if W != w:
        img = _pass(img, *coeffs(W, w), axis=1)
    if H != h:
        img = _pass(img, *coeffs(H, h), axis=0)
    return img


def to_tensor_normalize(img, mean, std):
    """``T.Normalize(mean, std)(T.ToTensor()(img))`` of an ``[H, W, 3]`` uint8 array: fp32 ``[3, H, W]``, by
    torchvision's own ops in its order."""
    t = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).contiguous()
    t = t.to(dtype=torch.float32).div(255)
    mean = torch.as_tensor(mean, dtype=torch.float32)
    std = torch.as_tensor(std, dtype=torch.float32)
    return t.sub_(mean.view(-1, 1, 1)).div_(std.view(-1, 1, 1))


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def transform(frames, size, mean=MEAN, std=STD):
    """The whole transform of a uint8 ``[B, N, H, W, 3]`` array: fp32 ``[B, N, 3, h, w]`` tensor."""
    frames = np.asarray(frames)
    B, N = frames.shape[:2]
    return torch.stack([torch.stack([to_tensor_normalize(resize(frames[b, v], size), mean, std) for v in range(N)])
                        for b in range(B)])


def random_frames(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def alternating(H, W, rows=True):
    """0 / 255 alternating by row (or by column), ``[H, W, 3]`` uint8."""
    img = np.zeros((H, W, 3), dtype=np.uint8)
    if rows:
        img[1::2] = 255
    else:
        img[:, 1::2] = 255
    return img


def golden():
    return np.load(GOLDEN)
