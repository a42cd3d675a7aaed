"""The CLEAR MOD evaluation (``mvdet_amd.evaluation``) on the GPU, timed.

(a) per ``update()``: ``DetectionEvaluator.update`` (threshold, NMS and append as three launches, no readback)
    against ``postprocess.threshold_rows`` + ``frame_results`` (the count read back, then the per-frame loop with an
    ``.item()``) on the same config-2 maps (120 x 360) in the same process.  Both sides are timed as wall clock per
    map including a final synchronize: the older path's cost is its host syncs, which device events do not see.
(b) per ``compute()``-style evaluation: ``evaluation.evaluate`` on arrays (pack on the host, upload, ONE matching
    launch, one readback) on the reference's demo case (from ``tests/golden/eval_cases.npz``), on 400 frames x 40 GT
    x 300 detections (an early epoch) and on 40 frames x 40 GT x 2000 detections (what NMS at distance 20 leaves of
    a config-2 map whose every cell is over ``cls_thres``); and the matching launch alone between two device events.

Protocol: warm-up, the variants interleaved, ``--repeats`` rounds; median, min and max over the rounds.  Beside
them the file quotes the reference's host-CPU seconds on the same inputs, measured where the fixtures are made
(``profiles/eval_ref_cpu.json``, written by ``tools/gen_golden_eval.py``): neither the reference nor scipy is
needed here.

Usage:  python tools/eval_bench.py [--steps 20] [--warmup 3] [--repeats 5] [--out profiles/eval_bench.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

GRID = (120, 360)  # config 2's reduced grid
GRID_REDUCE = 4


def synthetic_rows(F, n_gt, n_det, seed=0):
    """``F`` frames of ``n_gt`` GT and ``n_det`` detections as (frame, x, y) rows on config 2's ground plane:
    integer grid cells x 4; three quarters of the GT have a detection within a few cells, the other
    detections are spread over the plane."""
    rng = np.random.default_rng(seed)
    gt, det = [], []
    for f in range(F):
        g = np.column_stack([rng.integers(0, GRID[0], n_gt), rng.integers(0, GRID[1], n_gt)]) * GRID_REDUCE
        d = np.column_stack([rng.integers(0, GRID[0], n_det), rng.integers(0, GRID[1], n_det)]) * GRID_REDUCE
        k = min(n_gt, n_det) * 3 // 4
        d[:k] = g[:k] + rng.integers(-4, 5, (k, 2)) * GRID_REDUCE
        d = d[rng.permutation(n_det)]
        gt.append(np.column_stack([np.full(n_gt, f), g]))
        det.append(np.column_stack([np.full(n_det, f), d]))
    return np.concatenate(gt).astype(np.float64), np.concatenate(det).astype(np.float64)


def blob_maps(n, seed=0):
    """``n`` config-2 maps of smooth blobs (a trained model's output shape), as in tools/gen_golden_nms.py."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:GRID[0], 0:GRID[1]]
    maps = []
    for _ in range(n):
        m = np.zeros(GRID, np.float32)
        for _ in range(25):
            cy, cx = rng.uniform(0, GRID[0]), rng.uniform(0, GRID[1])
            m += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * rng.uniform(1.5, 4) ** 2)).astype(np.float32)
        maps.append(m + rng.uniform(0, 0.05, size=m.shape).astype(np.float32))
    return maps


def summary(r):
    return {"ms_median": round(statistics.median(r), 4), "ms_min": round(min(r), 4), "ms_max": round(max(r), 4)}


def main():
    import torch

    from mvdet_amd import _native, evaluation, postprocess

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "eval_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a ROCm GPU")
    dev = torch.device("cuda:0")

    # ---- (a) per update()
    maps = [torch.from_numpy(m)[None, None].to(dev) for m in blob_maps(args.steps)]
    gt_rows = synthetic_rows(args.steps, 40, 1)[0]
    ev = evaluation.DetectionEvaluator(gt_rows, max_frames=max(args.steps, 1))

    def native_updates():
        ev.reset()
        for f, m in enumerate(maps):
            ev.update(m, f)

    def rows_path():
        rows = [postprocess.threshold_rows(m, f, 0.4, GRID_REDUCE) for f, m in enumerate(maps)]
        return postprocess.frame_results(torch.cat(rows, 0))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(maps)

    variants = {"evaluator_update": native_updates, "threshold_rows_frame_results": rows_path}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    per_update = {k: [] for k in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():  # interleaved
            per_update[name].append(wall(fn))
    native_updates()
    same = bool(torch.equal(ev.results(), rows_path()))
    dets_per_map = ev.results().shape[0] / len(maps)

    # ---- (b) the evaluation
    g = dict(np.load(ROOT / "tests" / "golden" / "eval_cases.npz", allow_pickle=False))
    cases = {"demo": (g["demo_gt"].astype(np.float64), g["demo_det"].astype(np.float64)),
             "400x40x300": synthetic_rows(400, 40, 300), "40x40x2000": synthetic_rows(40, 40, 2000)}
    lib = _native.load()
    evaluate_ms, launch_ms, numbers = {k: [] for k in cases}, {k: [] for k in cases}, {}
    packed = {}
    for name, (gt, det) in cases.items():
        p = evaluation.pack_frames(gt, det)
        n_g, n_d = np.diff(p.gt_off), np.diff(p.det_off)
        packed[name] = dict(gt=torch.from_numpy(p.gt_xy).to(dev), det=torch.from_numpy(p.det_xy).to(dev),
                            go=torch.from_numpy(p.gt_off).to(dev), do=torch.from_numpy(p.det_off).to(dev),
                            F=len(p.frames), small=int(np.minimum(n_g, n_d).max()), large=int(np.maximum(n_g, n_d).max()))
        numbers[name] = list(evaluation.evaluate(det, gt))

    def launch_only(c):
        out = evaluation._launch_matching(c["gt"], c["det"], _native.EVAL_F64, c["go"], c["do"], c["F"], c["small"],
                                          c["large"], evaluation.TD, False, c.get("out"), ws=c.get("ws"))
        c["out"], c["ws"] = out, out.ws

    for _ in range(args.warmup):
        for name, (gt, det) in cases.items():
            evaluation.evaluate(det, gt)
            launch_only(packed[name])
    for _ in range(args.repeats):
        for name, (gt, det) in cases.items():  # interleaved
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evaluation.evaluate(det, gt)
            evaluate_ms[name].append((time.perf_counter() - t0) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch_only(packed[name])
            e1.record()
            torch.cuda.synchronize()
            launch_ms[name].append(e0.elapsed_time(e1))
    assert lib.mvbev_version() == 12500

    ref_cpu = None
    ref_file = ROOT / "profiles" / "eval_ref_cpu.json"
    if ref_file.exists():
        ref_cpu = json.loads(ref_file.read_text())
    out = {"bench": "eval_bench", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "map": list(GRID),
           "per_update_wall_ms": {k: summary(v) for k, v in per_update.items()},
           "update_results_equal_frame_results": same, "detections_per_map": round(dets_per_map, 1),
           "evaluate_wall_ms": {k: summary(v) for k, v in evaluate_ms.items()},
           "matching_launch_ms": {k: summary(v) for k, v in launch_ms.items()},
           "numbers": numbers, "reference_host_cpu_s": ref_cpu}
    text = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
