"""``ProjectViews`` (upsample + warp + concat + coord channels, one launch each way) against the reference's op
order in stock torch on the same GPU, in the same process, on the same tensors: per view ``F.interpolate`` and the
warp (``njc_bench.torch_warp``: kornia's steps in torch GPU ops; for bf16 maps its fp32 grid cast to bf16, as
``grid_sample`` demands, which costs torch accuracy, not time), then ``torch.cat`` with the coord map
(``persp_trans_detector.py:65, :69, :77``).

Shape: config 2 — 7 channels-last views [1,512,90,160] -> (270,480), grid (120,360); fp32 and bf16 maps, with and
without the coord channels.  Timed: the forward under ``no_grad`` and forward + backward from a fixed random
upstream gradient to every map.  Protocol: warm-up, then K steps between two device events, the two variants
interleaved, ``--repeats`` (>= 5) rounds; median, min and max over the rounds.  Also recorded: peak
``torch.cuda.max_memory_allocated`` above what was resident before one step, and the op's algorithmic bytes (maps
read + result written; backward: upstream gradient read + map gradients written) per second against the ~6.3 TB/s
a copy reaches on this GPU.  A leg counts as faster only where the op's slowest round is below torch's fastest.

Usage:  python tools/project_views_bench.py [--steps 10] [--warmup 3] [--repeats 5] [--out profiles/project_views_bench.json]
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

from mvdet_amd import ProjectViews, synthetic  # noqa: E402
from mvdet_amd.geometry import coord_map, projection_matrices  # noqa: E402
from tools.njc_bench import timed, torch_warp  # noqa: E402

VIEWS, FEAT = 7, (1, 512, 90, 160)
COPY_TBS = 6.3
CL = torch.channels_last


def torch_warp_16(feat, m, ho, wo):
    """``njc_bench.torch_warp`` for 16-bit maps: the same fp32 grid, cast to the maps' dtype for ``grid_sample``."""
    B = feat.shape[0]
    xs = (torch.linspace(0, wo - 1, wo, device=feat.device) / (wo - 1) - 0.5) * 2
    ys = (torch.linspace(0, ho - 1, ho, device=feat.device) / (ho - 1) - 0.5) * 2
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    pts = torch.stack([gx, gy, torch.ones_like(gx)], -1) @ m.T
    z = pts[..., 2:]
    scale = torch.where(z.abs() > 1e-8, 1.0 / (z + 1e-8), torch.ones_like(z))
    grid = (scale * pts[..., :2]).unsqueeze(0).expand(B, ho, wo, 2).to(feat.dtype)
    return F.grid_sample(feat, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "project_views_bench.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda:0")
    ds = synthetic.wildtrack_like(VIEWS, 4, seed=2)
    up, grid = tuple(ds.upsample_shape), tuple(ds.reducedgrid_shape)
    pm = projection_matrices(ds)
    B, C, h, w = FEAT
    gen = torch.Generator().manual_seed(0)
    base = [torch.randn(FEAT, generator=gen).clamp_min_(0) for _ in range(VIEWS)]
    out = {"bench": "project_views_bench", "device": torch.cuda.get_device_name(0), "views": VIEWS,
           "feat_shape": list(FEAT), "feat_layout": "channels_last", "upsample_shape": list(up),
           "grid_shape": list(grid), "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "copy_rate_TBps": COPY_TBS, "results": {}}

    for dtype, dname in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        for coord in (True, False):
            feats = [t.to(dev, dtype).contiguous(memory_format=CL).requires_grad_() for t in base]
            pv = ProjectViews(pm, up, grid, coord_channels=coord)
            ms = [m.to(dev) for m in pv.m_norm_cpu]
            cmap = coord_map(*grid).to(dev, dtype)
            ctot = VIEWS * C + (2 if coord else 0)
            gup = torch.randn((B, ctot) + grid, generator=gen).to(dev, dtype).contiguous(memory_format=CL)
            es = feats[0].element_size()

            def reference():
                warp = torch_warp if dtype == torch.float32 else torch_warp_16
                world = [warp(F.interpolate(f, up, mode="bilinear"), m, *grid) for f, m in zip(feats, ms)]
                return torch.cat(world + ([cmap.repeat([B, 1, 1, 1])] if coord else []), dim=1)

            def native():
                return pv(feats)

            def infer(fn):
                def step():
                    with torch.no_grad():
                        fn()
                return step

            def train(fn):
                def step():
                    for t in feats:
                        t.grad = None
                    fn().backward(gup)
                return step

            groups = {"forward": {"native": infer(native), "torch": infer(reference)},
                      "forward_backward": {"native": train(native), "torch": train(reference)}}
            grads = {}
            for name, step in groups["forward_backward"].items():
                step()
                grads[name] = [t.grad.float() for t in feats]
            with torch.no_grad():
                on, ot = native().float(), reference().float()
            agree = {"world": ((on - ot).abs().max() / ot.abs().max()).item(),
                     "grad_worst_view": max(((a - b).abs().max() / b.abs().max()).item()
                                            for a, b in zip(grads["native"], grads["torch"]))}
            del grads, on, ot
            fwd_bytes = VIEWS * B * C * h * w * es + B * ctot * grid[0] * grid[1] * es
            bwd_bytes = B * ctot * grid[0] * grid[1] * es + VIEWS * B * C * h * w * es
            res = {"normwise_native_vs_torch": agree, "bytes": {"forward": fwd_bytes, "backward": bwd_bytes},
                   "peak_bytes_above_inputs": {}}
            for gname, variants in groups.items():
                for name, step in variants.items():
                    for t in feats:
                        t.grad = None
                    torch.cuda.synchronize()
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
                r["native_faster_beyond_spread"] = r["native"]["gpu_ms_max"] < r["torch"]["gpu_ms_min"]
                r["speedup_median"] = round(r["torch"]["gpu_ms_median"] / r["native"]["gpu_ms_median"], 2)
                moved = fwd_bytes + (bwd_bytes if gname == "forward_backward" else 0)
                tbs = moved / (r["native"]["gpu_ms_median"] * 1e-3) / 1e12
                r["native_TBps_median"] = round(tbs, 3)
                r["native_fraction_of_copy_rate"] = round(tbs / COPY_TBS, 3)
                res[gname] = r
                print(f"# {dname} coord={coord} {gname}: {r}", file=sys.stderr, flush=True)
            out["results"][f"{dname}/{'coord' if coord else 'nocoord'}"] = res
            del feats, gup
            torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
