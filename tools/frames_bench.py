"""The camera-frame front at config 2 (7 views, decoded ``[1,7,1080,1920,3]`` uint8 -> ``[1,7,3,720,1280]`` fp32):
the native launch (``mvdet_amd.frames``) against the same transform in stock torch on the same GPU, in the same process,
alternating, and against the reference's own host path.

(a) ``native`` / ``native_nchw``: ``resize_normalize`` into a channels-last / NCHW output;
(b) ``torch_gpu``: ``F.interpolate(float image, mode="bilinear", antialias=True)``, then the divide and the normalize.
    Not Pillow's result (fp32 weights, no uint8 rounding between or after the passes): the largest difference from the
    native output is recorded in units of 1/255 of the unnormalized image;
(c) ``pillow_host``: ``Image.resize`` + the torch-CPU ``ToTensor`` / ``Normalize`` ops for the seven views on ONE host
    thread, as ``frameDataset.__getitem__`` runs them (wall clock; only where Pillow is importable).

Protocol: warm-up, then K calls between two device events, the variants interleaved, ``--repeats`` rounds; median, min
and max over the rounds.  One call is tens of microseconds, the order of what the host needs to issue it, so each
variant is timed twice: ``loop`` (K calls issued to an idle GPU: the rate a caller sees, host-bound when the kernel is
shorter than the issue) and ``queued`` (the K calls issued behind ~30 ms of matmuls, so that they run back to back:
the device time per call).  The native kernel's bytes (the uint8 frames read once, the fp32 views written once) over
its ``queued`` time are reported as a fraction of the 6.3 TB/s copy rate of the MI355X.

Usage:  python tools/frames_bench.py [--steps 100] [--warmup 10] [--repeats 7] [--out profiles/frames_bench.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from mvdet_amd import frames  # noqa: E402
from njc_bench import timed  # noqa: E402

VIEWS, B, IN_HW, OUT_HW = 7, 1, (1080, 1920), (720, 1280)
COPY_RATE = 6.3e12  # bytes/s, the measured HBM copy rate (MI355X_MICROARCH)


def timed_queued(step, steps, ballast):
    """ms per call with the calls queued behind ``ballast()`` (GPU work that outlasts their issue)."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ballast()
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def summary(r):
    return {"ms_median": round(statistics.median(r), 5), "ms_min": round(min(r), 5), "ms_max": round(max(r), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "frames_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frames_bench needs a ROCm GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    host = rng.integers(0, 256, size=(B, VIEWS, *IN_HW, 3), dtype=np.uint8)
    u8 = torch.from_numpy(host).to(dev)
    mean = torch.tensor(frames.IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(frames.IMAGENET_STD, device=dev).view(1, 3, 1, 1)
    out_cl = frames.resize_normalize(u8, OUT_HW)
    out_nchw = frames.resize_normalize(u8, OUT_HW, channels_last=False)

    def native():
        return frames.resize_normalize(u8, OUT_HW, out=out_cl)

    def native_nchw():
        return frames.resize_normalize(u8, OUT_HW, channels_last=False, out=out_nchw)

    def torch_gpu():
        x = u8[0].permute(0, 3, 1, 2).float()  # [N,3,H,W]
        y = F.interpolate(x, list(OUT_HW), mode="bilinear", antialias=True)
        return y.div_(255).sub_(mean).div_(std)

    big = torch.randn(8192, 8192, device=dev)

    def ballast():
        for _ in range(4):
            torch.mm(big, big)

    variants = {"native": native, "native_nchw": native_nchw, "torch_gpu": torch_gpu}
    with torch.no_grad():
        ours = native().clone()
        theirs = torch_gpu()[None]
        diff_255 = float(((theirs - ours) * std[None] * 255).abs().max())
        layouts_equal = bool(torch.equal(ours, native_nchw()))
        for step in variants.values():
            for _ in range(args.warmup):
                step()
        ballast()
        torch.cuda.synchronize()
        loop = {k: [] for k in variants}
        queued = {k: [] for k in variants}
        for _ in range(args.repeats):
            for name, step in variants.items():  # interleaved
                loop[name].append(timed(step, args.steps))
                queued[name].append(timed_queued(step, args.steps, ballast))

    moved = u8.numel() + out_cl.numel() * 4
    results = {name: {"loop": summary(loop[name]), "queued": summary(queued[name])} for name in variants}
    for name in ("native", "native_nchw"):
        q = results[name]["queued"]
        results[name]["bytes_over_queued_time_TBps"] = round(moved / (q["ms_median"] * 1e-3) / 1e12, 3)
        results[name]["fraction_of_copy_rate"] = round(moved / (q["ms_median"] * 1e-3) / COPY_RATE, 3)
        results[name]["ms_at_copy_rate"] = round(moved / COPY_RATE * 1e3, 5)
    t = results["torch_gpu"]["queued"]
    results["native"]["torch_over_native_queued_median"] = round(t["ms_median"] / results["native"]["queued"]["ms_median"], 2)

    pillow = None
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        import PIL
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        mean_c, std_c = torch.tensor(frames.IMAGENET_MEAN).view(3, 1, 1), torch.tensor(frames.IMAGENET_STD).view(3, 1, 1)
        images = [Image.fromarray(host[0, v]) for v in range(VIEWS)]

        def host_frame():
            outs = []
            for im in images:
                r = torch.from_numpy(np.array(im.resize((OUT_HW[1], OUT_HW[0]), Image.BILINEAR), copy=True))  # ToTensor's
                outs.append(r.permute(2, 0, 1).contiguous().to(torch.float32).div(255).sub_(mean_c).div_(std_c))
            return torch.stack(outs)

        ref = host_frame()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            host_frame()
            runs.append((time.perf_counter() - t0) * 1e3)
        torch.set_num_threads(threads)
        pillow = {"pillow_version": PIL.__version__, "host_threads": 1, **summary(runs),
                  "native_bitwise_equal": bool(torch.equal(ref, ours.cpu()[0]))}

    out = {"bench": "frames_bench", "device": torch.cuda.get_device_name(0), "views": VIEWS, "batch": B,
           "frames_shape": list(u8.shape), "out_shape": list(out_cl.shape), "tile": list(frames.pick_tile(IN_HW, OUT_HW)),
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "bytes": {"frames_u8": u8.numel(), "views_f32": out_cl.numel() * 4, "moved": moved},
           "copy_rate_TBps": COPY_RATE / 1e12, "layouts_bitwise_equal": layouts_equal,
           "torch_gpu_max_abs_difference_in_1_over_255": round(diff_255, 4), "results": results, "pillow_host": pillow}
    text = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
