"""The image head after its first conv: ``mvdet_amd.upsample_relu_conv1x1`` (one fused launch over the views,
native backward) against the op sequence it replaces (per view ``F.interpolate`` -> ``F.relu`` -> ``F.conv2d``,
torch autograd backward) in stock torch on the same GPU, in the same process, on the same tensors.

Shape: config 2's head — 7 views, B = 1, g [1,64,90,160] channels_last -> (270,480), W [2,64].  Timed: the
forward alone (under ``no_grad``) and one training step (forward, then the backward from given output gradients
to every g and W).  ``normwise_native_vs_torch`` compares the two on the timed tensors: the kernel's pre-activation
has the bits of ``F.interpolate`` on the GPU, so no ReLU decision differs and ``grad_g_elements_over_1e-4`` (the
grad_g elements further than 1e-4 of the maximum from torch's) is 0.
Protocol: warm-up, then K steps between two device events (a host clock around the same steps up to the final
synchronize beside it), the two variants interleaved, ``--repeats`` rounds; the min and max of each over the
rounds are reported.  The training steps also report the peak ``torch.cuda.max_memory_allocated`` above what was
resident before the step.

Usage:  python tools/img_head_bench.py [--steps 50] [--warmup 10] [--repeats 3]   (prints one JSON line)
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from mvdet_amd import upsample_relu_conv1x1  # noqa: E402

VIEWS, G_SHAPE, SIZE, CO = 7, (1, 64, 90, 160), (270, 480), 2


def traffic_bytes():
    """Bytes each variant has to move per view, from the shapes (fp32): the torch forward writes the upsampled
    tensor, reads and rewrites it in the ReLU and reads it in the conv; the fused forward reads g and writes out."""
    B, cm, h, w = G_SHAPE
    g, up, out = B * cm * h * w * 4, B * cm * SIZE[0] * SIZE[1] * 4, B * CO * SIZE[0] * SIZE[1] * 4
    return {"g": g, "upsampled": up, "out": out, "torch_forward": g + 4 * up + out, "native_forward": g + out}


def timed(step, steps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    gs = [torch.randn(G_SHAPE, generator=gen).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_()
          for _ in range(VIEWS)]
    w = (torch.randn(CO, G_SHAPE[1], generator=gen) / 8).to(dev).requires_grad_()
    grs = [torch.randn((G_SHAPE[0], CO) + SIZE, generator=gen).to(dev) for _ in range(VIEWS)]
    leaves = gs + [w]

    def fwd_native():
        return upsample_relu_conv1x1(gs, w, SIZE)

    def fwd_torch():
        w4 = w.view(CO, -1, 1, 1)
        return [F.conv2d(F.relu(F.interpolate(g, SIZE, mode="bilinear")), w4) for g in gs]

    def infer(fwd):
        def step():
            with torch.no_grad():
                fwd()
        return step

    def train(fwd):
        def step():
            for t in leaves:
                t.grad = None
            torch.autograd.backward(fwd(), grs)  # the output gradients are handed in: no loss ops in the timing
        return step

    variants = {"forward": {"native": infer(fwd_native), "torch": infer(fwd_torch)},
                "forward_backward": {"native": train(fwd_native), "torch": train(fwd_torch)}}

    # the two variants agree (the timed work is the same computation)
    agree = {}
    grads = {}
    for name, step in variants["forward_backward"].items():
        step()
        grads[name] = [t.grad.clone() for t in leaves]
    with torch.no_grad():
        on, ot = fwd_native(), fwd_torch()
    agree["out"] = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(on, ot))
    agree["grad_g"] = max(((a - b).abs().max() / b.abs().max()).item()
                          for a, b in zip(grads["native"][:-1], grads["torch"][:-1]))
    agree["grad_g_elements_over_1e-4"] = sum(int(((a - b).abs() > 1e-4 * b.abs().max()).sum().item())
                                              for a, b in zip(grads["native"][:-1], grads["torch"][:-1]))
    agree["grad_g_elements"] = sum(a.numel() for a in grads["native"][:-1])
    agree["grad_w"] = ((grads["native"][-1] - grads["torch"][-1]).abs().max() / grads["torch"][-1].abs().max()).item()
    del grads, on, ot

    # peak memory of one training step above what is resident before it
    peak = {}
    for name, step in variants["forward_backward"].items():
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base

    out = {"bench": "img_head_bench", "device": torch.cuda.get_device_name(0), "views": VIEWS,
           "g_shape": list(G_SHAPE), "g_layout": "channels_last", "size": list(SIZE), "co": CO, "steps": args.steps,
           "warmup": args.warmup, "repeats": args.repeats, "bytes_per_view": traffic_bytes(),
           "normwise_native_vs_torch": agree, "train_step_peak_bytes": peak, "results": {}}
    for what, pair in variants.items():
        for step in pair.values():
            for _ in range(args.warmup):
                step()
        runs = {name: {"gpu_ms": [], "wall_ms": []} for name in pair}
        for _ in range(args.repeats):
            for name, step in pair.items():  # interleaved: native, torch, native, torch, ...
                g_ms, w_ms = timed(step, args.steps)
                runs[name]["gpu_ms"].append(g_ms)
                runs[name]["wall_ms"].append(w_ms)
        res = {}
        for name, r in runs.items():
            res[name] = {"gpu_ms_min": round(min(r["gpu_ms"]), 4), "gpu_ms_max": round(max(r["gpu_ms"]), 4),
                         "wall_ms_min": round(min(r["wall_ms"]), 4), "wall_ms_max": round(max(r["wall_ms"]), 4)}
        # faster by more than the spread of this run's own repeats: the slowest native round against the fastest
        # torch round
        res["speedup_gpu_min"] = round(res["torch"]["gpu_ms_min"] / res["native"]["gpu_ms_max"], 2)
        res["speedup_gpu_max"] = round(res["torch"]["gpu_ms_max"] / res["native"]["gpu_ms_min"], 2)
        res["native_faster_beyond_spread"] = res["native"]["gpu_ms_max"] < res["torch"]["gpu_ms_min"]
        out["results"][what] = res
        print(f"# {what}: {res}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
