"""``ImageProjVariant`` at config 2 (7 views, ``imgs [1,7,3,720,1280]``, 270 x 480 resized, 120 x 360 grid, world
feature ``[1,512,15,45]``): the native paths against the reference's op order in stock torch on the same GPU, in the
same process, alternating.

(a) the fused front (``mvdet_amd.img_proj``, both thread mappings, both output layouts) against N ``F.interpolate``,
    N warps through the project's ``warp_perspective``, the coord repeat and ``torch.cat`` (+ the channels-last copy
    the backbone would make);
(b) the native dense head (``mvdet_amd.dense_head``) against ``map_classifier`` + ``F.interpolate`` in torch, forward
    and forward + backward;
(c) the whole module, forward (``eval``) and forward + backward (``train``), for both values of ``native_map_head``;
(d) peak ``torch.cuda.max_memory_allocated`` above what was resident before one step, for every variant.

Protocol: warm-up, then K steps between two device events, the variants of a group interleaved, ``--repeats`` rounds;
the median, min and max over the rounds are reported, and a native variant counts as faster (not slower) only beyond
the torch side's min-max spread.

Usage:  python tools/img_proj_bench.py [--steps 20] [--warmup 5] [--repeats 5]   (prints one JSON line)
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
sys.path.insert(0, str(Path(__file__).resolve().parent))

from mvdet_amd import DenseFuseHead, ImageProjection, ImageProjVariant, ops, synthetic  # noqa: E402
from mvdet_amd.geometry import coord_map, projection_matrices  # noqa: E402
from njc_bench import timed  # noqa: E402

VIEWS, B, MID, IN_HW = 7, 1, 512, (720, 1280)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda:0")
    ds = synthetic.wildtrack_like(VIEWS, 4, seed=2)
    up, grid = tuple(ds.upsample_shape), tuple(ds.reducedgrid_shape)
    mats = projection_matrices(ds)
    front = ImageProjection(mats, up, grid)
    gen = torch.Generator().manual_seed(0)
    imgs = torch.rand((B, VIEWS, 3) + IN_HW, generator=gen).to(dev)
    coord = coord_map(*grid).to(dev)
    mats_dev = [M.float().reshape(1, 3, 3).repeat(B, 1, 1).to(dev) for M in mats]

    def torch_front(channels_last):
        def step():
            world = []
            for cam in range(VIEWS):
                img_res = F.interpolate(imgs[:, cam], list(up), mode="bilinear")
                world.append(ops.warp_perspective(img_res, mats_dev[cam], grid))
            x = torch.cat(world + [coord.repeat([B, 1, 1, 1])], dim=1)
            return x.contiguous(memory_format=torch.channels_last) if channels_last else x
        return step

    def infer(fn):
        def step():
            with torch.no_grad():
                return fn()
        return step

    # (b) the head on a world feature of the backbone's kind (post-ReLU), channels-last as the backbone leaves it
    wf = torch.relu(torch.randn((B, 512, grid[0] // 8, grid[1] // 8), generator=gen)).to(dev)
    wf = wf.contiguous(memory_format=torch.channels_last).requires_grad_()

    def uniform(shape, fan_in):
        return (torch.rand(shape, generator=gen) * 2 - 1).div_(fan_in ** 0.5).to(dev).requires_grad_()

    w1, b1 = uniform((MID, 512, 3, 3), 9 * 512), uniform((MID,), 9 * 512)
    w2, b2 = uniform((MID, MID, 3, 3), 9 * MID), uniform((MID,), 9 * MID)
    w3 = uniform((1, MID, 3, 3), 9 * MID)
    gmap = torch.randn((B, 1) + grid, generator=gen).to(dev)
    leaves = [wf, w1, b1, w2, b2, w3]
    head = DenseFuseHead(grid)

    def native_head():
        return head(wf, w1, b1, w2, b2, w3)

    def torch_head():
        y1 = F.relu(F.conv2d(wf, w1, b1, padding=1))
        y2 = F.relu(F.conv2d(y1, w2, b2, padding=2, dilation=2))
        return F.interpolate(F.conv2d(y2, w3, padding=4, dilation=4), list(grid), mode="bilinear")

    def train(fn, params):
        def step():
            for t in params:
                t.grad = None
            fn().backward(gmap)
        return step

    # (c) the whole module, the same parameters under both flags
    models = {}
    for flag in (True, False):
        torch.manual_seed(0)
        models[flag] = ImageProjVariant(ds, device=dev, native_map_head=flag)
    models[False].load_state_dict(models[True].state_dict())

    def module_fwd(flag):
        def step():
            models[flag].eval()
            with torch.no_grad():
                return models[flag](imgs)[0]
        return step

    def module_train(flag):
        params = list(models[flag].parameters())

        def step():
            models[flag].train()
            for t in params:
                t.grad = None
            models[flag](imgs)[0].backward(gmap)
        return step

    groups = {
        "front": {"native": infer(lambda: front(imgs, channels_last=True)),  # (the default mapping: per pixel)
                  "native_pixel_view": infer(lambda: front(imgs, channels_last=True, per_pixel=False)),
                  "native_nchw": infer(lambda: front(imgs, channels_last=False)),
                  "native_nchw_pixel_view": infer(lambda: front(imgs, channels_last=False, per_pixel=False)),
                  "torch_order": infer(torch_front(True)), "torch_order_nchw": infer(torch_front(False))},
        "head_forward": {"native": infer(native_head), "torch_order": infer(torch_head)},
        "head_forward_backward": {"native": train(native_head, leaves), "torch_order": train(torch_head, leaves)},
        "module_forward": {"native": module_fwd(True), "torch_order": module_fwd(False)},
        "module_forward_backward": {"native": module_train(True), "torch_order": module_train(False)},
    }

    # the compared paths agree on the timed tensors
    agree = {}
    with torch.no_grad():
        a, b = front(imgs, channels_last=True), torch_front(True)()
        agree["front"] = ((a - b).abs().max() / b.abs().max()).item()
        agree["front_mappings_bitwise"] = bool(torch.equal(a, front(imgs, channels_last=False, per_pixel=False)))
        a, b = native_head(), torch_head()
        agree["head_map"] = ((a - b).abs().max() / b.abs().max()).item()
        a, b = module_fwd(True)(), module_fwd(False)()
        agree["module_map"] = ((a - b).abs().max() / b.abs().max()).item()
    grads = {}
    for name, step in groups["head_forward_backward"].items():
        step()
        grads[name] = [t.grad.clone() for t in leaves]
    for n, a, b in zip(("world_feature", "w1", "b1", "w2", "b2", "w3"), grads["native"], grads["torch_order"]):
        agree["head_grad_" + n] = ((a - b).abs().max() / b.abs().max()).item()
    del grads, a, b

    peak = {}
    for gname, variants in groups.items():
        for name, step in variants.items():
            step()  # (caches: workspaces, weight packs, MIOpen's find)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step()
            torch.cuda.synchronize()
            peak[f"{gname}/{name}"] = torch.cuda.max_memory_allocated() - base
    for t in leaves:
        t.grad = None

    npix = grid[0] * grid[1]
    out = {"bench": "img_proj_bench", "device": torch.cuda.get_device_name(0), "views": VIEWS,
           "imgs_shape": [B, VIEWS, 3, *IN_HW], "resized_shape": list(up), "grid_shape": list(grid),
           "world_feature_shape": list(wf.shape), "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "bytes": {"front_out": B * (3 * VIEWS + 2) * npix * 4, "imgs": imgs.numel() * 4,
                     "resized_images_never_written": B * VIEWS * 3 * up[0] * up[1] * 4,
                     "world_feature": wf.numel() * 4},
           "items": {"pixel_views": B * VIEWS * npix},
           "normwise_native_vs_torch_order": agree, "peak_bytes_above_inputs": peak, "results": {}}
    for what, variants in groups.items():
        for step in variants.values():
            for _ in range(args.warmup):
                step()
        runs = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name, step in variants.items():  # interleaved
                runs[name].append(timed(step, args.steps))
        res = {name: {"gpu_ms_median": round(statistics.median(r), 4), "gpu_ms_min": round(min(r), 4),
                      "gpu_ms_max": round(max(r), 4)} for name, r in runs.items()}
        t = res["torch_order"]
        for name in variants:
            if name.startswith("native"):
                n = res[name]
                n["faster_beyond_torch_spread"] = n["gpu_ms_median"] < t["gpu_ms_median"] - (t["gpu_ms_max"] - t["gpu_ms_min"])
                n["not_slower_beyond_torch_spread"] = n["gpu_ms_median"] <= t["gpu_ms_median"] + (t["gpu_ms_max"] - t["gpu_ms_min"])
                n["torch_over_native_median"] = round(t["gpu_ms_median"] / n["gpu_ms_median"], 2)
        out["results"][what] = res
        print(f"# {what}: {res}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
