"""``NoJointConvVariant``'s ground-plane head from the backbone maps to the map: the native path (one batched
GEMM at backbone resolution, then ``ProjectSumHead``'s fused launch) against the reference's op order
(``no_joint_conv_variant.py:64-81``: per view ``F.interpolate`` and the warp, ``torch.cat`` with the coord map,
``Conv2d(512 N + 2, 512, 1)``, ReLU, ``Conv2d(512, 1, 1)``) in stock torch on the same GPU, in the same process,
on the same tensors (the warp as ``bench.py``'s training leg times it: kornia's steps in torch GPU ops).

Shape: config 2 — 7 views, B = 1, maps [1,512,90,160] channels_last -> (270,480), grid (120,360).  Timed:
(a) the native forward, the GEMM and the fused kernel separately and together, (b) the reference order's
forward, both under ``no_grad``, (c) forward + backward of both from a given map gradient to every backbone map
and every parameter.  Protocol: warm-up, then K steps between two device events, the variants of a group
interleaved, ``--repeats`` rounds; the min and max over the rounds are reported.  Peak
``torch.cuda.max_memory_allocated`` above what was resident before one step is recorded for every variant.

Usage:  python tools/njc_bench.py [--steps 20] [--warmup 5] [--repeats 3]   (prints one JSON line)
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

from mvdet_amd import ProjectSumHead, synthetic  # noqa: E402
from mvdet_amd.geometry import coord_map, projection_matrices  # noqa: E402
from mvdet_amd.variants import view_gemm  # noqa: E402

VIEWS, FEAT, CM = 7, (1, 512, 90, 160), 512


def torch_warp(feat, m, ho, wo):
    """kornia's transform_points + grid_sample in torch GPU ops (``m``: the fp32 src_norm <- dst_norm matrix)."""
    B = feat.shape[0]
    xs = (torch.linspace(0, wo - 1, wo, device=feat.device) / (wo - 1) - 0.5) * 2
    ys = (torch.linspace(0, ho - 1, ho, device=feat.device) / (ho - 1) - 0.5) * 2
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    pts = torch.stack([gx, gy, torch.ones_like(gx)], -1) @ m.T
    z = pts[..., 2:]
    scale = torch.where(z.abs() > 1e-8, 1.0 / (z + 1e-8), torch.ones_like(z))
    grid = (scale * pts[..., :2]).unsqueeze(0).expand(B, ho, wo, 2)
    return F.grid_sample(feat, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def timed(step, steps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


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
    head = ProjectSumHead(projection_matrices(ds), up, grid)
    ms = [m.to(dev) for m in head.m_norm_cpu]
    gen = torch.Generator().manual_seed(0)
    feats = [torch.randn(FEAT, generator=gen).clamp_min_(0).to(dev).contiguous(memory_format=torch.channels_last)
             .requires_grad_() for _ in range(VIEWS)]
    cin = FEAT[1] * VIEWS + 2
    w1 = (torch.rand((CM, cin, 1, 1), generator=gen) * 2 - 1).div_(cin ** 0.5).to(dev).requires_grad_()
    b1 = (torch.rand(CM, generator=gen) * 2 - 1).div_(cin ** 0.5).to(dev).requires_grad_()
    w2 = (torch.rand((1, CM, 1, 1), generator=gen) * 2 - 1).div_(CM ** 0.5).to(dev).requires_grad_()
    gmap = torch.randn((FEAT[0], 1) + grid, generator=gen).to(dev)
    coord = coord_map(*grid).to(dev)
    leaves = feats + [w1, b1, w2]

    def native():
        zs = view_gemm(feats, w1, VIEWS)
        return head(zs, b1, w1[:, FEAT[1] * VIEWS:, 0, 0], w2)

    def reference():
        world = [torch_warp(F.interpolate(f, up, mode="bilinear"), m, *grid) for f, m in zip(feats, ms)]
        x = torch.cat(world + [coord.repeat([FEAT[0], 1, 1, 1])], dim=1)
        return F.conv2d(F.relu(F.conv2d(x, w1, b1)), w2)

    with torch.no_grad():
        zs_fixed = [z.contiguous(memory_format=torch.channels_last) for z in view_gemm(feats, w1, VIEWS)]
        wc_fixed = w1[:, FEAT[1] * VIEWS:, 0, 0].contiguous()

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
        "forward_parts": {"native_gemm": infer(lambda: view_gemm(feats, w1, VIEWS)),
                          "native_fused_kernel": infer(lambda: head(zs_fixed, b1, wc_fixed, w2))},
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
    names = [f"feat{v}" for v in range(VIEWS)] + ["w1", "b1", "w2"]
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

    B, C, h, w = FEAT
    out = {"bench": "njc_bench", "device": torch.cuda.get_device_name(0), "views": VIEWS, "feat_shape": list(FEAT),
           "feat_layout": "channels_last", "upsample_shape": list(up), "grid_shape": list(grid), "cm": CM,
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "bytes": {"upsampled_per_view": B * C * up[0] * up[1] * 4, "slab": B * cin * grid[0] * grid[1] * 4,
                     "z_all_views": VIEWS * B * CM * h * w * 4, "hidden": B * CM * grid[0] * grid[1] * 4},
           "flop": {"native_gemm": 2 * VIEWS * B * h * w * C * CM, "reference_conv": 2 * B * grid[0] * grid[1] * cin * CM},
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
