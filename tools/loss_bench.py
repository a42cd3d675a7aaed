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

``--points``: the sparse ground truth of cfg2 and cfg3 once as dense tensors and once as
``PointTargets`` through ``pack_step`` (``mvdet_amd.targets``), per side: the bytes a step uploads
(computed from the tensors), the step with the targets resident and with the per-step upload from
pinned host memory, and the GPU time of the pooling and of the conv + MSE launch (events around
``--reps`` back-to-back launches of the entry point alone).  ``--root DIR`` takes the package from
another checkout (one without ``mvdet_amd.targets`` measures the dense side only), and
``--alternate DIR --rounds R`` runs that checkout and this one in turn, R times each, one fresh process
per run, and reports every round, the medians and the spread of each side's repeated runs.

Usage:  python tools/loss_bench.py [--steps 50] [--warmup 10] [--cases cfg2_sparse,...]   (prints one JSON line)
        python tools/loss_bench.py --points [--root DIR] [--reps 500]
        python tools/loss_bench.py --alternate PARENT_CHECKOUT [--rounds 3] [--out profiles/loss_points_bench.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]

SHAPES = {"cfg2": (120, 360), "cfg3": (480, 1440)}
VIEWS, VIEW_SHAPE, VIEW_GT = 7, (270, 480), (1080, 1920)


def sparse_gt(shape, gen):
    t = torch.zeros(shape)
    flat = torch.randperm(t.numel(), generator=gen)[:40]
    t.view(-1)[flat] = 1.0
    return t


def make_inputs(map_shape, dense, dev, seed=0, host_gt=False):
    gen = torch.Generator().manual_seed(seed)

    def gt(shape):
        t = torch.rand(shape, generator=gen) if dense else sparse_gt(shape, gen)
        return t if host_gt else t.to(dev)
    map_res = torch.rand((1, 1) + map_shape, generator=gen).to(dev).requires_grad_()
    imgs_res = [torch.rand((1, 2) + VIEW_SHAPE, generator=gen).to(dev).requires_grad_() for _ in range(VIEWS)]
    return map_res, imgs_res, gt((1, 1) + map_shape), [gt((1, 2) + VIEW_GT) for _ in range(VIEWS)]


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


def launch_times(loss_mod, xs, targets, kernels, weights, reps):
    """GPU time per launch (us) of the pooling and of the conv + MSE entry point on these items: events
    around ``reps`` back-to-back launches of the one entry.  ``pool_launches``: pooling launches a
    step issues (0 when every item has points or needs no pooling)."""
    from mvdet_amd import _native
    launch = loss_mod._Launch(xs, targets, kernels, weights, 0, 0.4)
    lib, n, B, stream = launch.lib, launch.n, launch.B, launch.stream
    # a checkout from before the point targets hands every item to the pooling entry
    pool_items = getattr(launch, "pool_items", launch.items)
    points = getattr(launch, "points", None)
    blocks = int(lib.mvbev_gaussian_mse_blocks(launch.items, n, B))
    partials = torch.empty(4 * blocks, dtype=torch.float64, device=launch.dev)
    tail = (n, B, launch.kernels, len(launch.plans), launch.cls_thres, launch.stats_item, partials.data_ptr(),
            partials.numel(), stream)

    def pool():
        _native.check(lib.mvbev_adaptive_max_pool_f32(pool_items, len(pool_items), B, stream), "pool")

    def mse():
        if points is None:
            _native.check(lib.mvbev_gaussian_mse_f32(launch.items, *tail), "mse")
        else:
            _native.check(lib.mvbev_gaussian_mse_points_f32(launch.items, points, *tail), "mse")

    def per_launch(fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) * 1e3 / reps, 3)
    out = {"pool_launches": 0 if pool_items is None else 1, "pool_us": 0.0 if pool_items is None else per_launch(pool),
           "mse_us": per_launch(mse)}
    del launch
    return out


def run_points(args):
    """The ``--points`` mode: one JSON line for the package under ``--root``."""
    sys.path.insert(0, str(Path(args.root).resolve()))
    import mvdet_amd
    from mvdet_amd import detection_loss, gaussian_kernels, loss as loss_mod
    has_points = hasattr(mvdet_amd, "PointTargets")
    dev = torch.device("cuda:0")
    map_kernel, img_kernel = gaussian_kernels(4, 4)
    out = {"bench": "loss_points_bench", "root": str(args.root), "device": torch.cuda.get_device_name(0),
           "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "point_targets": has_points, "results": {}}
    for cfg, map_shape in SHAPES.items():
        map_res, imgs_res, map_host, imgs_host = make_inputs(map_shape, False, dev, host_gt=True)
        map_host, imgs_host = map_host.pin_memory(), [t.pin_memory() for t in imgs_host]
        xs = [map_res] + imgs_res
        kernels = [map_kernel] + [img_kernel] * VIEWS
        weights = [1.0] + [1.0 / VIEWS] * VIEWS

        def step(map_gt, imgs_gt):
            for x in xs:
                x.grad = None
            ls, _ = detection_loss(map_res, imgs_res, map_gt, imgs_gt, map_kernel, img_kernel, 1.0, 0.4)
            ls.backward()
            return ls

        def upload_dense():  # trainer.py:45-46 / INTEGRATION.md: one copy per tensor
            return map_host.to(dev, non_blocking=True), [t.to(dev, non_blocking=True) for t in imgs_host]
        sides = {"dense": (upload_dense, sum(t.numel() * t.element_size() for t in [map_host] + imgs_host))}
        if has_points:
            from mvdet_amd import PointTargets, pack_step
            map_pt = PointTargets.from_dense(map_host).pin_memory()
            imgs_pt = [PointTargets.from_dense(t).pin_memory() for t in imgs_host]

            def upload_points():  # the pack is part of the timed step (a collate_fn's work), then one copy
                pm, pvs = pack_step(map_pt, imgs_pt)
                return pm.to(dev, non_blocking=True), [t.to(dev, non_blocking=True) for t in pvs]
            pm, _ = pack_step(map_pt, imgs_pt)
            assert pm.buffer.is_pinned()
            sides["points"] = (upload_points, pm.buffer.numel() * pm.buffer.element_size())
        res = {}
        for side, (upload, nbytes) in sides.items():
            map_gt, imgs_gt = upload()
            torch.cuda.synchronize()
            r = {"upload_bytes_per_step": int(nbytes), "loss": step(map_gt, imgs_gt).item(),
                 "grad_sum": float(sum(x.grad.double().sum().item() for x in xs)),
                 "step_resident": timed(lambda: step(map_gt, imgs_gt), args.steps, args.warmup),
                 "step_with_upload": timed(lambda: step(*upload()), args.steps, args.warmup)}
            r.update(launch_times(loss_mod, [x.detach() for x in xs], [map_gt] + imgs_gt, kernels, weights, args.reps))
            res[side] = r
            print(f"# {cfg} {side}: {r}", file=sys.stderr, flush=True)
        if has_points:  # the two sides compute the same thing, bitwise
            assert res["points"]["loss"] == res["dense"]["loss"] and res["points"]["grad_sum"] == res["dense"]["grad_sum"]
        out["results"][cfg] = res
    print(json.dumps(out))


def run_alternate(args):
    """``--alternate``: the other checkout and this one in turn, a fresh process per run."""
    runs = {"parent": [], "this": []}
    for _ in range(args.rounds):
        for name, root in (("parent", args.alternate), ("this", str(ROOT))):
            cmd = [sys.executable, str(Path(__file__).resolve()), "--points", "--root", root, "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--reps", str(args.reps)]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
            if done.returncode != 0:
                raise SystemExit(f"{name} run failed with status {done.returncode}: nothing more is started")
            runs[name].append(json.loads(done.stdout.strip().splitlines()[-1]))
    first = runs["this"][0]
    out = {"bench": "loss_points_bench", "device": first["device"], "steps": args.steps, "warmup": args.warmup,
           "reps": args.reps, "rounds": args.rounds, "order": "parent, this, parent, this, ...",
           "units": {"step": "ms per step (wall, ending in a synchronize)", "launch": "us GPU time per launch"},
           "results": {}}

    def series(name, cfg, side, *path):
        vals = []
        for run in runs[name]:
            v = run["results"][cfg][side]
            for p in path:
                v = v[p]
            vals.append(v)
        return {"runs": vals, "median": statistics.median(vals), "spread": round(max(vals) - min(vals), 4)}
    for cfg in SHAPES:
        c = {}
        for name, side in (("parent", "dense"), ("this", "dense"), ("this", "points")):
            c[f"{name}_{side}"] = {
                "upload_bytes_per_step": runs[name][0]["results"][cfg][side]["upload_bytes_per_step"],
                "pool_launches": runs[name][0]["results"][cfg][side]["pool_launches"],
                "step_resident_ms": series(name, cfg, side, "step_resident", "ms_per_step"),
                "step_with_upload_ms": series(name, cfg, side, "step_with_upload", "ms_per_step"),
                "pool_us": series(name, cfg, side, "pool_us"),
                "mse_us": series(name, cfg, side, "mse_us")}
        par, pts = c["parent_dense"], c["this_points"]
        c["mse_points_minus_parent_us"] = round(pts["mse_us"]["median"] - par["mse_us"]["median"], 3)
        c["mse_parent_spread_us"] = par["mse_us"]["spread"]
        c["mse_points_within_parent_spread"] = bool(c["mse_points_minus_parent_us"] <= par["mse_us"]["spread"])
        c["same_loss_all_runs"] = len({run["results"][cfg][side]["loss"] for name, side in
                                      (("parent", "dense"), ("this", "dense"), ("this", "points"))
                                      for run in runs[name]}) == 1
        out["results"][cfg] = c
    text = json.dumps(out, indent=1)
    if args.out:
        Path(args.out).write_text(text + "\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default="", help="comma-separated subset, e.g. cfg2_sparse,cfg3_dense (default: all)")
    ap.add_argument("--points", action="store_true", help="dense against point-list ground truth (see the docstring)")
    ap.add_argument("--root", default=str(ROOT), help="the checkout whose mvdet_amd is measured")
    ap.add_argument("--reps", type=int, default=500, help="back-to-back launches per launch timing (--points)")
    ap.add_argument("--alternate", default="", help="another checkout (built) to run in turn with this one")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child run (--alternate)")
    ap.add_argument("--out", default="", help="write the --alternate result here as well")
    args = ap.parse_args()
    if args.alternate:
        return run_alternate(args)
    if args.points:
        return run_points(args)
    sys.path.insert(0, str(Path(args.root).resolve()))
    from mvdet_amd import detection_loss, gaussian_kernels
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
