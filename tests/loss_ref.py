"""CPU restatement of the reference criterion for the loss tests (stock torch on the CPU):
``multiview_detector/loss/gaussian_mse.py:12-20`` — ``adaptive_max_pool2d``, ``conv2d``,
``mse_loss`` — and the loss / count lines of ``trainer.py:43-56``, plus the reader of
``tests/golden/loss_cases.npz`` (written by ``tools/gen_golden_loss.py`` from the reference)."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = Path(__file__).resolve().parent / "golden" / "loss_cases.npz"


def target_transform(x, target, kernel):
    target = F.adaptive_max_pool2d(target, x.shape[2:])
    with torch.no_grad():
        target = F.conv2d(target, kernel.float(), padding=int((kernel.shape[-1] - 1) / 2))
    return target


def gaussian_mse(x, target, kernel):
    return F.mse_loss(x, target_transform(x, target, kernel))


def single(x, target, kernel, upstream=1.0):
    """(transformed target, diff, loss, x-gradient of upstream * loss) of one criterion call."""
    x = x.detach().clone().requires_grad_()
    loss = gaussian_mse(x, target, kernel)
    (upstream * loss).backward()
    t = target_transform(x.detach(), target, kernel)
    return t, x.detach() - t, loss.detach(), x.grad


def step(map_res, imgs_res, map_gt, imgs_gt, map_kernel, img_kernel, alpha=1.0, cls_thres=0.4):
    """trainer.py:43-56: (loss, [gradients of map_res and every view], (tp, fp, fn))."""
    map_res = map_res.detach().clone().requires_grad_()
    imgs_res = [v.detach().clone().requires_grad_() for v in imgs_res]
    loss = 0
    for img_res, img_gt in zip(imgs_res, imgs_gt):
        loss += gaussian_mse(img_res, img_gt, img_kernel)
    loss = gaussian_mse(map_res, map_gt, map_kernel) + loss / len(imgs_gt) * alpha
    loss.backward()
    pred = (map_res > cls_thres).int()
    tp = (pred.eq(map_gt) * pred.eq(1)).sum().item()
    fp = pred.sum().item() - tp
    fn = map_gt.sum().item() - tp
    return loss.detach(), [map_res.grad] + [v.grad for v in imgs_res], (tp, fp, fn)


def dense(shape, pts, vals):
    """A zero [B,C,H,W] target with vals at the (b, c, y, x) rows of pts."""
    t = torch.zeros(tuple(int(s) for s in shape))
    if len(pts):
        idx = torch.as_tensor(np.asarray(pts), dtype=torch.long)
        t[tuple(idx.t())] = torch.as_tensor(np.asarray(vals), dtype=torch.float32)
    return t


def points(shape, cells, value=1.0):
    """dense() from a list of (b, c, y, x) cells all holding value."""
    return dense(shape, np.array(cells, np.int64).reshape(-1, 4), np.full(len(cells), value, np.float32))


_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def golden_single(name):
    """dict(x, target, kernel, t, loss, grad) of one single-call golden case."""
    g = golden()
    p = f"s_{name}_"
    return {"x": torch.from_numpy(g[p + "x"]), "target": dense(g[p + "tshape"], g[p + "pts"], g[p + "vals"]),
            "kernel": torch.from_numpy(g[str(g[p + "kernel"])]), "t": torch.from_numpy(g[p + "t"]),
            "loss": float(g[p + "loss"]), "grad": torch.from_numpy(g[p + "grad"])}


def golden_step(name):
    """dict(xs, targets, map_kernel, img_kernel, alpha, thres, loss, grads, counts) of one whole-step case."""
    g = golden()
    n = int(g[f"{name}_views"]) + 1
    return {"xs": [torch.from_numpy(g[f"{name}_x{i}"]) for i in range(n)],
            "targets": [dense(g[f"{name}_tshape{i}"], g[f"{name}_pts{i}"], g[f"{name}_vals{i}"]) for i in range(n)],
            "map_kernel": torch.from_numpy(g["map_kernel_4"]), "img_kernel": torch.from_numpy(g["img_kernel_4"]),
            "alpha": float(g[f"{name}_alpha"]), "thres": float(g[f"{name}_thres"]), "loss": float(g[f"{name}_loss"]),
            "grads": [torch.from_numpy(g[f"{name}_grad{i}"]) for i in range(n)],
            "counts": tuple(float(v) for v in g[f"{name}_counts"])}


def normwise(got, ref):
    """max|got - ref| / max|ref| in fp64 (0 / 0 = 0)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    return err / scale if scale > 0 else err
