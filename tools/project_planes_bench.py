"""``ProjectPlanes`` (the weighted multi-plane projection, one launch each way) against what the package offers
without it for the same math, and against stock torch, on the same GPU, in the same process, on the same tensors:

(a) ``native``: the op;
(b) ``views``: the D products ``w[:, d:d+1] * feat`` per view, ``ProjectViews(coord_channels=False)`` modules of at
    most 16 (view, plane) pairs each, and the sum over planes of their outputs — the yardstick;
(c) ``torch``: the same in stock torch GPU ops (``F.interpolate`` and ``njc_bench.torch_warp`` per plane).

Shape: config 2 — 7 channels-last maps [1,512,90,160] -> (270,480), grid (120,360), D = 5 planes at z = 0, 30, 60, 90,
120 cm (``geometry.plane_projection_matrices``), softmax weights; fp32 and bf16 maps, no coord channels (side (b)
has none).  Timed: the forward under ``no_grad`` and forward + backward from a fixed random upstream gradient to
every map and every weight.  Protocol: warm-up, then K steps between two device events, the three sides interleaved,
``--repeats`` (>= 5) rounds; median, min and max.  Also recorded: peak ``torch.cuda.max_memory_allocated`` above
what was resident before one step, parity between the sides, and achieved bytes/s from a byte model computed from
the shapes (the op: maps and weights read, result written; backward: upstream gradient, maps and weights read, both
gradients written) against the ~6.3 TB/s a copy reaches on this GPU.  The op counts as faster only where its
slowest round is below (b)'s fastest.

Usage:  python tools/project_planes_bench.py [--steps 10] [--warmup 3] [--repeats 5] [--out profiles/project_planes_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from mvdet_amd import ProjectPlanes, ProjectViews, synthetic  # noqa: E402
from mvdet_amd.geometry import plane_projection_matrices  # noqa: E402
from tools.njc_bench import timed, torch_warp  # noqa: E402
from tools.project_views_bench import torch_warp_16  # noqa: E402

VIEWS, FEAT, HEIGHTS = 7, (1, 512, 90, 160), [0.0, 30.0, 60.0, 90.0, 120.0]
COPY_TBS = 6.3
CL = torch.channels_last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "project_planes_bench.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda:0")
    ds = synthetic.wildtrack_like(VIEWS, 4, seed=2)
    up, grid = tuple(ds.upsample_shape), tuple(ds.reducedgrid_shape)
    pm = plane_projection_matrices(ds, HEIGHTS)
    B, C, h, w = FEAT
    D = len(HEIGHTS)
    gen = torch.Generator().manual_seed(0)
    base = [torch.randn(FEAT, generator=gen).clamp_min_(0) for _ in range(VIEWS)]
    wbase = [torch.softmax(torch.randn((B, D, h, w), generator=gen), 1) for _ in range(VIEWS)]
    out = {"bench": "project_planes_bench", "device": torch.cuda.get_device_name(0), "views": VIEWS, "planes": D,
           "heights": HEIGHTS, "feat_shape": list(FEAT), "feat_layout": "channels_last", "upsample_shape": list(up),
           "grid_shape": list(grid), "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "copy_rate_TBps": COPY_TBS, "yardstick": "views", "results": {}}
    # side (b): (view, plane) pairs in order, at most 16 per ProjectViews module
    pairs = [(v, d) for v in range(VIEWS) for d in range(D)]
    groups_b = [pairs[i:i + 16] for i in range(0, len(pairs), 16)]

    for dtype, dname in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        feats = [t.to(dev, dtype).contiguous(memory_format=CL).requires_grad_() for t in base]
        wts = [t.to(dev).requires_grad_() for t in wbase]
        pp = ProjectPlanes(pm, up, grid, coord_channels=False)
        mods = [ProjectViews([pm[v][d] for v, d in g], up, grid, coord_channels=False) for g in groups_b]
        ms = [[m.to(dev) for m in planes] for planes in pp.m_norm_cpu]
        ctot = VIEWS * C
        gup = torch.randn((B, ctot) + grid, generator=gen).to(dev, dtype).contiguous(memory_format=CL)
        es = feats[0].element_size()

        def native():
            return pp(feats, wts)

        def views():
            prods = [(feats[v] * wts[v][:, d:d + 1].to(dtype)).contiguous(memory_format=CL) for v, d in pairs]
            outs, at = [], 0
            for g, mod in zip(groups_b, mods):
                outs.append(mod(prods[at:at + len(g)]))
                at += len(g)
            world = torch.cat(outs, dim=1)  # [B, N D C, Ho, Wo]: view-major, plane-minor
            return world.reshape(B, VIEWS, D, C, *grid).sum(dim=2).reshape(B, ctot, *grid)

        def stock():
            warp = torch_warp if dtype == torch.float32 else torch_warp_16
            world = []
            for v in range(VIEWS):
                tot = None
                for d in range(D):
                    x = F.interpolate(feats[v] * wts[v][:, d:d + 1].to(dtype), up, mode="bilinear")
                    y = warp(x, ms[v][d], *grid)
                    tot = y if tot is None else tot + y
                world.append(tot)
            return torch.cat(world, dim=1)

        sides = {"native": native, "views": views, "torch": stock}

        def infer(fn):
            def step():
                with torch.no_grad():
                    fn()
            return step

        def train(fn):
            def step():
                for t in feats + wts:
                    t.grad = None
                fn().backward(gup)
            return step

        groups = {"forward": {k: infer(f) for k, f in sides.items()},
                  "forward_backward": {k: train(f) for k, f in sides.items()}}
        grads, worlds = {}, {}
        for name, step in groups["forward_backward"].items():
            step()
            grads[name] = ([t.grad.float() for t in feats], [t.grad.float() for t in wts])
            with torch.no_grad():
                worlds[name] = sides[name]().float()
        nw = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()  # noqa: E731
        agree = {}
        for other in ("views", "torch"):
            agree[f"native_vs_{other}"] = {
                "world": nw(worlds["native"], worlds[other]),
                "grad_feats_worst_view": max(nw(a, b) for a, b in zip(grads["native"][0], grads[other][0])),
                "grad_weights_worst_view": max(nw(a, b) for a, b in zip(grads["native"][1], grads[other][1]))}
        del grads, worlds
        maps_b, wts_b = VIEWS * B * C * h * w * es, VIEWS * B * D * h * w * 4
        world_b = B * ctot * grid[0] * grid[1] * es
        prods_b = VIEWS * D * B * C * h * w * es
        planes_b = D * world_b
        bytes_model = {
            "native": {"forward": maps_b + wts_b + world_b, "backward": world_b + 2 * (maps_b + wts_b)},
            # (b): products written and read, the N D C channels written and read, the sum written; backward: the
            # sum's gradient expanded, read by the adjoints, the products' gradients written and read twice
            "views": {"forward": maps_b + D * wts_b + 2 * prods_b + 2 * planes_b + world_b,
                      "backward": world_b + 2 * planes_b + 3 * prods_b + D * maps_b + 2 * (maps_b + wts_b)},
        }
        res = {"normwise": agree, "bytes_model": bytes_model, "peak_bytes_above_inputs": {}}
        for gname, variants in groups.items():
            for name, step in variants.items():
                for t in feats + wts:
                    t.grad = None
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                resident = torch.cuda.memory_allocated()
                step()
                torch.cuda.synchronize()
                res["peak_bytes_above_inputs"][f"{gname}/{name}"] = torch.cuda.max_memory_allocated() - resident
            for step in variants.values():
                for _ in range(args.warmup):
                    step()
            runs = {name: [] for name in variants}
            for _ in range(args.repeats):
                for name, step in variants.items():  # interleaved
                    runs[name].append(timed(step, args.steps))
            r = {name: {"gpu_ms_median": round(statistics.median(v), 4), "gpu_ms_min": round(min(v), 4),
                        "gpu_ms_max": round(max(v), 4)} for name, v in runs.items()}
            r["native_faster_than_views_beyond_spread"] = r["native"]["gpu_ms_max"] < r["views"]["gpu_ms_min"]
            r["speedup_median_vs_views"] = round(r["views"]["gpu_ms_median"] / r["native"]["gpu_ms_median"], 2)
            r["speedup_median_vs_torch"] = round(r["torch"]["gpu_ms_median"] / r["native"]["gpu_ms_median"], 2)
            peak = res["peak_bytes_above_inputs"]
            r["native_peak_below_views"] = peak[f"{gname}/native"] < peak[f"{gname}/views"]
            for side in ("native", "views"):
                moved = bytes_model[side]["forward"]
                if gname == "forward_backward":
                    moved += bytes_model[side]["backward"]
                tbs = moved / (r[side]["gpu_ms_median"] * 1e-3) / 1e12
                r[f"{side}_model_TBps_median"] = round(tbs, 3)
                r[f"{side}_fraction_of_copy_rate"] = round(tbs / COPY_TBS, 3)
            res[gname] = r
            print(f"# {dname} {gname}: {r}", file=sys.stderr, flush=True)
        out["results"][dname] = res
        del feats, wts, gup, pp, mods
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
