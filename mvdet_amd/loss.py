"""The training criterion and the per-batch metrics on the GPU.

Drop-ins for ``multiview_detector/loss/gaussian_mse.py:7-20`` and for the loss / precision-recall
lines of ``multiview_detector/trainer.py:43-56``, on the HIP kernels of ``libmvbev.so``
(``mvbev_adaptive_max_pool_f32``, ``mvbev_gaussian_mse_f32`` / ``mvbev_gaussian_mse_points_f32``,
``mvbev_loss_finalize_f32``, ``mvbev_gaussian_mse_backward_f32``; ``mvdet_amd/csrc/loss.hip``):

* ``GaussianMSE`` — the reference's ``nn.Module``: ``forward(x, target, kernel)`` and
  ``_traget_transform(x, target, kernel)`` (the reference's spelling; ``trainer.py:131`` calls it).
* ``detection_loss(map_res, imgs_res, map_gt, imgs_gt, map_kernel, img_kernel, alpha, cls_thres)
  -> (loss, stats)`` — ``trainer.py:43-56`` in one pooling launch, one conv+MSE launch over the
  map and every view and one finalize launch; the backward is one launch.
* ``gaussian_kernels(grid_reduce, img_reduce) -> (map_kernel, img_kernel)`` — the closed form of
  ``frameDataset.py:17-18,40-57`` for datasets that carry no kernels (``mvdet_amd.synthetic``).

A target is a dense fp32 tensor or a ``mvdet_amd.targets.PointTargets`` (its non-zero cells), item
by item: a point item is pooled by the conv kernel's own staging (no dense tensor, no pooled scratch,
no pooling launch) and gives bitwise the result of its ``dense()``.

Everything is fp32.  The gradient goes to ``x`` only, as in the reference (its conv runs under
``no_grad`` and the targets / kernels require none).  Non-finite values in ``target`` are not
defined behaviour: ground-truth maps are counts.  A NaN or Inf in ``x`` or in the kernel behaves as
in the reference (a NaN tap reaches the transformed target as ``0 * NaN``).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
from torch import nn

from . import _native
from .ops import _require_cuda, _stream
from .targets import PointTargets

MAX_ITEMS = 16  # kLossMaxItems (csrc/loss.hip)
MAX_C = 8       # kLossMaxC: the slice mask is 64 bits
TILE_H, TILE_W = 16, 64  # kLossTH / kLossTW: the conv kernel's output tile


def pool_windows(in_size: int, out_size: int):
    """``F.adaptive_max_pool2d``'s windows along one axis: (starts, ends) with window ``i`` =
    ``[floor(i * in / out), ceil((i + 1) * in / out))`` — uneven and overlapping when ``in`` is no
    multiple of ``out``, one repeated element when ``in < out``."""
    i = np.arange(int(out_size), dtype=np.int64)
    starts = (i * int(in_size)) // int(out_size)
    ends = ((i + 1) * int(in_size) + int(out_size) - 1) // int(out_size)
    return starts, ends


def gaussian_kernels(grid_reduce: int = 4, img_reduce: int = 4):
    """``(map_kernel [1,1,41,41], img_kernel [2,2,21,21])`` of ``frameDataset.py:17-18,40-57``:
    ``exp(-(x^2 + y^2) / (2 sigma))`` with ``sigma = 20 / grid_reduce`` (map) or ``10 / img_reduce``
    (views) used as the variance, as the reference does (it hands sigma to scipy as the covariance
    and divides by the maximum); ``img_kernel`` is block-diagonal (head -> head, foot -> foot)."""
    def one(half, sigma):
        r = np.arange(-half, half + 1, dtype=np.float64)
        x, y = np.meshgrid(r, r)
        return torch.from_numpy(np.exp(-(x * x + y * y) / (2.0 * sigma))).float()
    m, g = one(20, 20.0 / grid_reduce), one(10, 10.0 / img_reduce)
    map_kernel = torch.zeros(1, 1, 41, 41)
    map_kernel[0, 0] = m
    img_kernel = torch.zeros(2, 2, 21, 21)
    img_kernel[0, 0] = g
    img_kernel[1, 1] = g
    return map_kernel, img_kernel


def plan_slices(kernel: torch.Tensor):
    """The host-side plan of a ``[C,C,k,k]`` kernel: ``(slices, finite)``.  ``finite``: every value
    is finite; ``slices``: the ``(co, ci)`` pairs the conv multiplies — those holding a non-zero
    when ``finite``, every pair otherwise (no skip may hide a ``0 * NaN``)."""
    w = kernel.detach().float().cpu().numpy()
    C = w.shape[0]
    finite = bool(np.isfinite(w).all())
    slices = [(co, ci) for co in range(C) for ci in range(C) if not finite or bool((w[co, ci] != 0).any())]
    return slices, finite


def _check_kernel(kernel):
    if not isinstance(kernel, torch.Tensor):
        raise TypeError(f"kernel must be a tensor, got {type(kernel).__name__}")
    if kernel.dim() != 4 or kernel.shape[0] != kernel.shape[1] or kernel.shape[2] != kernel.shape[3] or \
            kernel.shape[2] % 2 == 0:
        raise ValueError(f"kernel must be [C,C,k,k] with odd k, got {tuple(kernel.shape)}")
    if not kernel.dtype.is_floating_point:
        raise TypeError(f"kernel must be a floating-point tensor, got {kernel.dtype}")
    if kernel.shape[0] > MAX_C:
        raise ValueError(f"kernel has {kernel.shape[0]} channels, the native criterion takes at most {MAX_C}")


class KernelPlan:
    """A kernel on the device plus its host-side plan (``plan_slices``).  The plan holds the
    caller's tensor too: while the plan is cached, that tensor's storage cannot be freed and its
    address handed to another kernel, so the cache key cannot name two different kernels."""

    def __init__(self, kernel: torch.Tensor, device):
        self.source = kernel
        self.slices, self.finite = plan_slices(kernel)
        self.C, self.k = int(kernel.shape[0]), int(kernel.shape[-1])
        self.mask = 0
        for co, ci in self.slices:
            self.mask |= 1 << (co * self.C + ci)
        self.dev = kernel.detach().float().to(device).contiguous()

    def struct(self) -> _native.LossKernel:
        return _native.LossKernel(self.dev.data_ptr(), self.C, self.k, self.mask, int(self.finite))


class _PlanCache:
    """Kernel plans keyed by ``(data_ptr, _version, device)`` — the weight packs' convention: an
    in-place change of the kernel bumps ``_version`` and makes a new plan; an unchanged kernel is
    neither re-read nor re-uploaded.  Every cached plan keeps its kernel tensor alive
    (``KernelPlan.source``), so a key stays bound to the tensor it was made from; at most
    ``capacity`` kernels (a few kB each) are held.  ``uploads`` counts the plans made."""

    def __init__(self, capacity: int = 32):
        self.capacity, self.plans, self.uploads = capacity, {}, 0

    def get(self, kernel: torch.Tensor, device) -> KernelPlan:
        key = (kernel.data_ptr(), kernel._version, tuple(kernel.shape), kernel.dtype, str(device))
        plan = self.plans.get(key)
        if plan is None:
            if len(self.plans) >= self.capacity:
                self.plans.clear()
            plan = self.plans[key] = KernelPlan(kernel, device)
            self.uploads += 1
        return plan


kernel_cache = _PlanCache()


def _check_pair(x, target, kernel):
    """``target``: a dense tensor or a ``PointTargets``, whose logical shape and device follow the
    dense target's rules."""
    for name, t in (("x", x), ("target", target)):
        if name == "target" and isinstance(t, PointTargets):
            continue  # 4-D and fp32 by construction
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor{' or a PointTargets' if name == 'target' else ''}, "
                            f"got {type(t).__name__}")
        if t.dim() != 4:
            raise ValueError(f"{name} must be 4-D [B,C,H,W], got {t.dim()}-D")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
    _check_kernel(kernel)
    if x.shape[:2] != target.shape[:2]:
        raise ValueError(f"x {tuple(x.shape)} and target {tuple(target.shape)} differ in batch or channels")
    if kernel.shape[0] != x.shape[1]:
        raise ValueError(f"kernel {tuple(kernel.shape)} does not match x's {x.shape[1]} channels")
    if target.device != x.device:
        raise ValueError(f"target is on {target.device}, x on {x.device}")
    if min(x.shape) == 0 or min(target.shape) == 0:
        raise ValueError(f"empty x {tuple(x.shape)} or target {tuple(target.shape)}")


class _Launch:
    """The item array of one step and the buffers its launches write."""

    def __init__(self, xs, targets, kernels, weights, stats_item=-1, cls_thres=0.0, want_t=False, want_diff=True,
                 with_x=True):
        if not 0 < len(xs) <= MAX_ITEMS:
            raise ValueError(f"1 .. {MAX_ITEMS} (prediction, target) pairs per call, got {len(xs)}")
        for x, t, k in zip(xs, targets, kernels):
            _check_pair(x, t, k)
        B = xs[0].shape[0]
        for x in xs:
            if x.shape[0] != B or x.device != xs[0].device:
                raise ValueError("every prediction of one call shares the batch size and the device")
        if stats_item >= 0 and targets[stats_item].shape != xs[stats_item].shape:
            raise ValueError(f"map_gt {tuple(targets[stats_item].shape)} must have map_res's shape "
                             f"{tuple(xs[stats_item].shape)} (trainer.py:51-54 compares them cell by cell)")
        _require_cuda(*xs)
        self.lib = _native.load()
        dev = xs[0].device
        self.n, self.B, self.dev, self.stats_item, self.cls_thres = len(xs), B, dev, stats_item, float(cls_thres)
        plans, ids = [], []
        for k in kernels:
            p = kernel_cache.get(k, dev)
            if not any(p is q for q in plans):
                plans.append(p)
            ids.append(next(i for i, q in enumerate(plans) if q is p))
        self.plans = plans
        self.kernels = (_native.LossKernel * len(plans))(*[p.struct() for p in plans])
        self.items = (_native.LossItem * self.n)()
        self.keep = [xs, targets]  # the tensors behind the raw pointers
        # one allocation per kind of buffer, an [B,C,h,w] slice per item
        shapes = [tuple(x.shape) for x in xs]
        sizes = [int(np.prod(s)) for s in shapes]
        same = [tuple(t.shape[2:]) == s[2:] for t, s in zip(targets, shapes)]
        # a point item is pooled by the conv kernel's own staging: no scratch, no pooling launch
        point = [isinstance(t, PointTargets) for t in targets]
        self.points = (_native.LossPoints * self.n)() if any(point) else None

        def slices(want):
            flat = torch.empty(sum(n for n, w in zip(sizes, want) if w), dtype=torch.float32, device=dev)
            out, off = [], 0
            for n, s, w in zip(sizes, shapes, want):
                out.append(flat[off:off + n].view(s) if w else None)
                off += n if w else 0
            return out
        pooled = slices([not s and not p for s, p in zip(same, point)])
        self.t_out = slices([want_t] * self.n)
        self.diff = slices([want_diff and with_x] * self.n)
        self.keep.append(pooled)
        for i, (x, t, w) in enumerate(zip(xs, targets, weights)):
            _, C, h, wd = shapes[i]
            ptr = [b[i].data_ptr() if b[i] is not None else None for b in (pooled, self.t_out, self.diff)]
            if point[i]:
                self.points[i] = _native.LossPoints(*t.pointers(), t.shape[2], t.shape[3])
            self.items[i] = _native.LossItem(
                x.data_ptr() if with_x else None, _native.strides4(x), None if point[i] else t.data_ptr(),
                _native._i64x4() if point[i] else _native.strides4(t), C, h, wd,
                t.shape[2], t.shape[3], ptr[0], ptr[1], ptr[2], ids[i], float(w))
        # the dense items that need pooling, for the pooling launch (none: no launch)
        to_pool = [i for i in range(self.n) if pooled[i] is not None]
        self.pool_items = (_native.LossItem * len(to_pool))(*[self.items[i] for i in to_pool]) if to_pool else None
        self.n_pooled = len(to_pool)  # pooled scratch buffers allocated
        self.launches = []            # what forward() enqueued, in order: "pool", "mse", "finalize"
        self.stream = _stream(xs[0])

    def forward(self, finalize=True):
        lib, n, B = self.lib, self.n, self.B
        if self.pool_items is not None:
            _native.check(lib.mvbev_adaptive_max_pool_f32(self.pool_items, len(self.pool_items), B, self.stream),
                          "mvbev_adaptive_max_pool_f32")
            self.launches.append("pool")
        blocks = int(lib.mvbev_gaussian_mse_blocks(self.items, n, B))
        if blocks <= 0:
            raise _native.NativeError("mvbev_gaussian_mse_blocks: the items do not fit one launch")
        partials = torch.empty(4 * blocks, dtype=torch.float64, device=self.dev)
        tail = (n, B, self.kernels, len(self.plans), self.cls_thres, self.stats_item, partials.data_ptr(),
                partials.numel(), self.stream)
        if self.points is None:
            _native.check(lib.mvbev_gaussian_mse_f32(self.items, *tail), "mvbev_gaussian_mse_f32")
        else:
            _native.check(lib.mvbev_gaussian_mse_points_f32(self.items, self.points, *tail),
                          "mvbev_gaussian_mse_points_f32")
        self.launches.append("mse")
        # everything that reads the predictions, the targets and the pooled scratch is enqueued (the
        # allocator keeps their memory until this stream is past it): the backward needs only diff
        self.keep = None
        if not finalize:
            return None, None
        loss = torch.empty((), dtype=torch.float32, device=self.dev)
        stats = torch.empty(3, dtype=torch.float64, device=self.dev) if self.stats_item >= 0 else None
        _native.check(lib.mvbev_loss_finalize_f32(self.items, n, B, partials.data_ptr(), partials.numel(),
                                                  self.stats_item, loss.data_ptr(),
                                                  stats.data_ptr() if stats is not None else None, self.stream),
                      "mvbev_loss_finalize_f32")
        self.launches.append("finalize")
        return loss, stats

    def backward(self, grad_out: torch.Tensor, wanted):
        g = grad_out.detach().to(device=self.dev, dtype=torch.float32).contiguous()
        flat = torch.empty(sum(d.numel() for d, w in zip(self.diff, wanted) if w), dtype=torch.float32, device=self.dev)
        grads, off = [], 0
        for d, w in zip(self.diff, wanted):
            grads.append(flat[off:off + d.numel()].view(d.shape) if w else None)
            off += d.numel() if w else 0
        ptrs = (ctypes.c_void_p * self.n)(*[t.data_ptr() if t is not None else None for t in grads])
        _native.check(self.lib.mvbev_gaussian_mse_backward_f32(self.items, self.n, self.B, g.data_ptr(), ptrs,
                                                               _native.stream_ptr(self.dev)),
                      "mvbev_gaussian_mse_backward_f32")
        return grads


class _LossFn(torch.autograd.Function):
    """loss (and the stats, not differentiable) of a list of pairs; gradients go to the xs only."""

    @staticmethod
    def forward(ctx, targets, kernels, weights, stats_item, cls_thres, *xs):
        want = any(ctx.needs_input_grad[5:])
        launch = _Launch(list(xs), targets, kernels, weights, stats_item, cls_thres, want_diff=want)
        loss, stats = launch.forward()
        ctx.launch = launch
        if stats is None:
            return loss
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, grad_loss, *_):
        grads = ctx.launch.backward(grad_loss, ctx.needs_input_grad[5:])
        return (None, None, None, None, None) + tuple(grads)


class GaussianMSE(nn.Module):
    """Drop-in for ``multiview_detector.loss.gaussian_mse.GaussianMSE``:
    ``mse_loss(x, conv2d(adaptive_max_pool2d(target, x.shape[2:]), kernel, padding=(k - 1) / 2))``.

    ``x`` [B,C,h,w] and ``target`` [B,C,Ht,Wt] are fp32 tensors on one GPU (``target`` may be a
    ``PointTargets`` of that logical shape instead); ``kernel`` [C,C,k,k]
    (odd k) may live on the host, as ``dataset.map_kernel`` does: it is uploaded once and its plan
    cached until it changes in place.  The gradient goes to ``x`` only.  Non-finite values in
    ``target`` are not defined behaviour (ground-truth maps are counts)."""

    def __init__(self):
        super().__init__()

    def forward(self, x, target, kernel):
        return _LossFn.apply([target], [kernel], [1.0], -1, 0.0, x)

    def _traget_transform(self, x, target, kernel):
        launch = _Launch([x], [target], [kernel], [1.0], want_t=True, want_diff=False, with_x=False)
        launch.forward(finalize=False)
        return launch.t_out[0]


def detection_loss(map_res, imgs_res, map_gt, imgs_gt, map_kernel, img_kernel, alpha=1.0, cls_thres=0.4):
    """``trainer.py:43-56`` fused: ``(loss, stats)`` with

        loss = criterion(map_res, map_gt, map_kernel)
               + sum_v criterion(imgs_res[v], imgs_gt[v], img_kernel) / len(imgs_gt) * alpha

    a 0-d fp32 tensor with a ``grad_fn`` (gradients to ``map_res`` and every ``imgs_res[v]``), and
    ``stats`` a 3-element fp64 device tensor ``(tp, fp, fn)`` of ``map_res > cls_thres`` against
    ``map_gt`` (which has ``map_res``'s shape).  Nothing here syncs with the host; read the metrics
    when they are wanted:

        tp, fp, fn = stats.tolist()
        precision = tp / (tp + fp + 1e-4)
        recall = tp / (tp + fn + 1e-4)

    Targets must be on the predictions' device (move them with ``.to(device, non_blocking=True)``);
    the kernels may stay on the host.  ``map_gt`` and every ``imgs_gt[v]`` may each be a dense tensor or
    a ``PointTargets`` (``mvdet_amd.targets.pack_step`` uploads a whole step's in one copy)."""
    imgs_res, imgs_gt = list(imgs_res), list(imgs_gt)
    if len(imgs_res) != len(imgs_gt):
        raise ValueError(f"{len(imgs_res)} view predictions but {len(imgs_gt)} view targets")
    n = len(imgs_gt)
    xs = [map_res] + imgs_res
    targets = [map_gt] + imgs_gt
    kernels = [map_kernel] + [img_kernel] * n
    weights = [1.0] + [float(alpha) / max(n, 1)] * n
    return _LossFn.apply(targets, kernels, weights, 0, float(cls_thres), *xs)
