"""Forward + backward of the training criterion: ``mvdet_amd.detection_loss`` against the reference's
own op sequence (``trainer.py:43-48`` with ``gaussian_mse.py:12-20``: per item ``adaptive_max_pool2d``,
a host-to-device copy of the kernel, ``conv2d``, ``mse_loss``, then one autograd backward) in stock
torch on the same GPU.

Shapes: cfg2 training (map [1,1,120,360], k = 41; 7 views [1,2,270,480] from [1,2,1080,1920]
targets, k = 21) and cfg3 (map [1,1,480,1440], same views).  Inputs: 40 random ground-truth points
per map ("sparse", what training sees) and a dense random target ("dense", the worst case: no tile
is skipped).  Timing as ``bench.py``'s ``run_train_step``: warm-up steps, a synchronize, then the
wall time of K steps up to a final synchronize (host launch cost included), beside the GPU time
between two events around the same K steps.  ``torch_43_56`` adds the reference's three ``.item()``
counts (``trainer.py:51-54``), which ``detection_loss`` returns as a device tensor without a sync.

Usage:  python tools/loss_bench.py [--steps 50] [--warmup 10] [--cases cfg2_sparse,...]   (prints one JSON line)
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from mvdet_amd import detection_loss, gaussian_kernels  # noqa: E402

SHAPES = {"cfg2": (120, 360), "cfg3": (480, 1440)}
VIEWS, VIEW_SHAPE, VIEW_GT = 7, (270, 480), (1080, 1920)


def make_inputs(map_shape, dense, dev, seed=0):
    gen = torch.Generator().manual_seed(seed)

    def gt(shape):
        if dense:
            return torch.rand(shape, generator=gen)
        t = torch.zeros(shape)
        flat = torch.randperm(t.numel(), generator=gen)[:40]
        t.view(-1)[flat] = 1.0
        return t
    map_res = torch.rand((1, 1) + map_shape, generator=gen).to(dev).requires_grad_()
    imgs_res = [torch.rand((1, 2) + VIEW_SHAPE, generator=gen).to(dev).requires_grad_() for _ in range(VIEWS)]
    return map_res, imgs_res, gt((1, 1) + map_shape).to(dev), [gt((1, 2) + VIEW_GT).to(dev) for _ in range(VIEWS)]


def torch_criterion(x, target, kernel):
    target = F.adaptive_max_pool2d(target, x.shape[2:])
    with torch.no_grad():
        target = F.conv2d(target, kernel.float().to(target.device), padding=int((kernel.shape[-1] - 1) / 2))
    return F.mse_loss(x, target)


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"ms_per_step": round(dt * 1e3 / steps, 4), "gpu_ms_per_step": round(e0.elapsed_time(e1) / steps, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default="", help="comma-separated subset, e.g. cfg2_sparse,cfg3_dense (default: all)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    map_kernel, img_kernel = gaussian_kernels(4, 4)
    out = {"bench": "loss_bench", "device": torch.cuda.get_device_name(0), "steps": args.steps,
           "warmup": args.warmup, "alpha": 1.0, "cls_thres": 0.4, "results": {}}
    for cfg, map_shape in SHAPES.items():
        for kind in ("sparse", "dense"):
            if args.cases and f"{cfg}_{kind}" not in args.cases.split(","):
                continue
            map_res, imgs_res, map_gt, imgs_gt = make_inputs(map_shape, kind == "dense", dev)
            xs = [map_res] + imgs_res

            def zero():
                for x in xs:
                    x.grad = None

            def native():
                zero()
                loss, _ = detection_loss(map_res, imgs_res, map_gt, imgs_gt, map_kernel, img_kernel, 1.0, 0.4)
                loss.backward()
                return loss

            def stock(counts=False):
                zero()
                loss = 0
                for img_res, img_gt in zip(imgs_res, imgs_gt):
                    loss += torch_criterion(img_res, img_gt, img_kernel)
                loss = torch_criterion(map_res, map_gt, map_kernel) + loss / len(imgs_gt) * 1.0
                loss.backward()
                if counts:
                    pred = (map_res > 0.4).int()
                    tp = (pred.eq(map_gt) * pred.eq(1)).sum().item()
                    return loss, (tp, pred.sum().item() - tp, map_gt.sum().item() - tp)
                return loss

            ln = native().item()
            g_native = [x.grad.clone() for x in xs]
            ls = stock().item()
            g_err = max(((a - x.grad).abs().max() / x.grad.abs().max()).item() for a, x in zip(g_native, xs))
            res = {"loss_native": ln, "loss_torch": ls, "grad_normwise_vs_torch": g_err,
                   "native": timed(native, args.steps, args.warmup),
                   "torch_43_48": timed(stock, args.steps, args.warmup),
                   "torch_43_56": timed(lambda: stock(True), args.steps, args.warmup)}
            res["speedup_vs_torch_43_48"] = round(res["torch_43_48"]["ms_per_step"] / res["native"]["ms_per_step"], 2)
            out["results"][f"{cfg}_{kind}"] = res
            print(f"# {cfg}_{kind}: {res}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
