"""``ResProjVariant``'s ground-plane head from the foot planes to the map: the native path (``ProjectThinFuse``: the
thin fused conv1 kernel, then the engine's conv2 -> conv3) against the reference's op order
(``res_proj_variant.py:70-83``: per view the warp of the foot plane, ``torch.cat`` with the coord map, three
``nn.Conv2d`` with their ReLUs) in stock torch on the same GPU, in the same process, on the same tensors (the warp
as ``tools/njc_bench.py`` times it: kornia's steps in torch GPU ops with ``grid_sample``).

Shape: config 2 — 7 foot planes [1,1,270,480], grid (120,360), 512 mid channels.  Timed: (a) the native forward
(the thin kernel alone, and with conv2 -> conv3) and the reference order's, under ``no_grad``, (b) forward +
backward of both from a given map gradient to every plane and every parameter.  Protocol: warm-up, then K steps
between two device events, the variants of a group interleaved, ``--repeats`` rounds; the min and max over the
rounds are reported.  Peak ``torch.cuda.max_memory_allocated`` above what was resident before one step is recorded
for every variant.  The thin kernel's achieved bytes/s over (y1 write + plane reads + weights) stands beside the
6.3 TB/s copy rate of the MI355X.

Usage:  python tools/res_proj_bench.py [--steps 20] [--warmup 5] [--repeats 3]   (prints one JSON line)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from mvdet_amd import ProjectThinFuse, ops, synthetic, thin_fuse  # noqa: E402
from mvdet_amd.geometry import coord_map, projection_matrices  # noqa: E402
from njc_bench import timed, torch_warp  # noqa: E402

VIEWS, B, MID = 7, 1, 512
COPY_RATE = 6.3e12  # bytes/s, the MI355X's measured device copy rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda:0")
    ds = synthetic.wildtrack_like(VIEWS, 4, seed=2)
    up, grid = tuple(ds.upsample_shape), tuple(ds.reducedgrid_shape)
    head = ProjectThinFuse(projection_matrices(ds), up, grid)
    ms = [m.to(dev) for m in head.m_norm_cpu]
    gen = torch.Generator().manual_seed(0)
    planes = [torch.randn((B, 1) + up, generator=gen).to(dev).requires_grad_() for _ in range(VIEWS)]

    def uniform(shape, fan_in):
        return (torch.rand(shape, generator=gen) * 2 - 1).div_(fan_in ** 0.5).to(dev).requires_grad_()

    cin = VIEWS + 2
    w1, b1 = uniform((MID, cin, 3, 3), 9 * cin), uniform((MID,), 9 * cin)
    w2, b2 = uniform((MID, MID, 3, 3), 9 * MID), uniform((MID,), 9 * MID)
    w3 = uniform((1, MID, 3, 3), 9 * MID)
    gmap = torch.randn((B, 1) + grid, generator=gen).to(dev)
    coord = coord_map(*grid).to(dev)
    leaves = planes + [w1, b1, w2, b2, w3]

    def native():
        return head(planes, w1, b1, w2, b2, w3)

    def reference():
        world = [torch_warp(p, m, *grid) for p, m in zip(planes, ms)]
        x = torch.cat(world + [coord.repeat([B, 1, 1, 1])], dim=1)
        y1 = F.relu(F.conv2d(x, w1, b1, padding=1))
        y2 = F.relu(F.conv2d(y1, w2, b2, padding=2, dilation=2))
        return F.conv2d(y2, w3, padding=4, dilation=4)

    y1_fixed = torch.empty(ops.split_shape(B, MID, *grid), dtype=torch.bfloat16, device=dev)
    planes_d, w1_d, b1_d = [p.detach() for p in planes], w1.detach(), b1.detach()

    # the kernel alone: the argument block is built once, so that a step's host time (a few microseconds of ctypes)
    # stays below the kernel's and the events time the GPU
    import ctypes
    from mvdet_amd import _native
    thin_fuse.thin_conv1_forward(planes_d, head.m_norm_cpu, grid, w1_d, b1_d, y1_fixed)  # (checks the arguments)
    arr = (_native.WarpView * VIEWS)()
    for i, p in enumerate(planes_d):
        arr[i].src, arr[i].src_strides = p.data_ptr(), (ctypes.c_int64 * 4)(*p.stride())
        arr[i].m = (ctypes.c_float * 9)(*head.m_norm_cpu[i].reshape(9).tolist())
    fwd, stream = _native.load().mvbev_thin_conv1_forward_f32, torch.cuda.current_stream(dev).cuda_stream

    def thin_only():
        st = fwd(arr, VIEWS, B, up[0], up[1], grid[0], grid[1], w1_d.data_ptr(), b1_d.data_ptr(), MID,
                 y1_fixed.data_ptr(), _native.LAYOUT_SPLIT_BF16, None, stream)
        assert st == 0, st

    def infer(fn):
        def step():
            with torch.no_grad():
                fn()
        return step

    def train(fn):
        def step():
            for t in leaves:
                t.grad = None
            fn().backward(gmap)
        return step

    groups = {
        "forward": {"native": infer(native), "reference_order": infer(reference)},
        "forward_parts": {"native_thin_kernel": infer(thin_only)},
        "forward_backward": {"native": train(native), "reference_order": train(reference)},
    }

    # the two orders agree on the timed tensors
    agree, grads = {}, {}
    for name, step in groups["forward_backward"].items():
        step()
        grads[name] = [t.grad.clone() for t in leaves]
    with torch.no_grad():
        on, ot = native(), reference()
    agree["map"] = ((on - ot).abs().max() / ot.abs().max()).item()
    names = [f"plane{v}" for v in range(VIEWS)] + ["w1", "b1", "w2", "b2", "w3"]
    for n, a, b in zip(names, grads["native"], grads["reference_order"]):
        agree["grad_" + n] = ((a - b).abs().max() / b.abs().max()).item()
    del grads, on, ot

    peak = {}
    for gname in ("forward", "forward_backward"):
        for name, step in groups[gname].items():
            for t in leaves:
                t.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step()
            torch.cuda.synchronize()
            peak[f"{gname}/{name}"] = torch.cuda.max_memory_allocated() - base
            for t in leaves:
                t.grad = None

    npix = grid[0] * grid[1]
    thin_bytes = B * MID * npix * 4 + VIEWS * B * up[0] * up[1] * 4 + w1.numel() * 4
    out = {"bench": "res_proj_bench", "device": torch.cuda.get_device_name(0), "views": VIEWS,
           "plane_shape": [B, 1, *up], "grid_shape": list(grid), "mid": MID, "steps": args.steps,
           "warmup": args.warmup, "repeats": args.repeats,
           "bytes": {"y1": B * MID * npix * 4, "planes": VIEWS * B * up[0] * up[1] * 4, "w1": w1.numel() * 4,
                     "thin_kernel_total": thin_bytes},
           "flop": {"thin_conv1": 2 * B * npix * MID * cin * 9, "conv2": 2 * B * npix * MID * MID * 9},
           "normwise_native_vs_reference_order": agree, "peak_bytes_above_inputs": peak, "results": {}}
    for what, variants in groups.items():
        for step in variants.values():
            for _ in range(args.warmup):
                step()
        runs = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name, step in variants.items():  # interleaved
                runs[name].append(timed(step, args.steps))
        res = {name: {"gpu_ms_min": round(min(r), 4), "gpu_ms_max": round(max(r), 4)} for name, r in runs.items()}
        if "reference_order" in res:
            res["speedup_gpu_min"] = round(res["reference_order"]["gpu_ms_min"] / res["native"]["gpu_ms_max"], 2)
            res["speedup_gpu_max"] = round(res["reference_order"]["gpu_ms_max"] / res["native"]["gpu_ms_min"], 2)
            res["native_faster_beyond_spread"] = res["native"]["gpu_ms_max"] < res["reference_order"]["gpu_ms_min"]
        out["results"][what] = res
        print(f"# {what}: {res}", file=sys.stderr, flush=True)
    t = out["results"]["forward_parts"]["native_thin_kernel"]
    out["thin_kernel_bandwidth"] = {
        "bytes_per_s_at_min": round(thin_bytes / (t["gpu_ms_min"] * 1e-3)),
        "bytes_per_s_at_max": round(thin_bytes / (t["gpu_ms_max"] * 1e-3)),
        "copy_rate_bytes_per_s": COPY_RATE,
        "fraction_of_copy_rate_at_min": round(thin_bytes / (t["gpu_ms_min"] * 1e-3) / COPY_RATE, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
