"""The backbone's dtype at config 2 (Wildtrack, 7 views, 720 x 1280 frames -> 90 x 160 maps, C = 512, grid
120 x 360): what ``PerspTransDetector(backbone_dtype=...)`` buys, measured, not assumed.

Legs, interleaved within every round (each leg once per round, >= 5 rounds; medians and min-max), on real
(non-zero) data, HIP events on the stream:
  backbone   the channels-last ResNet-18 (both halves) over the 7 views as one batch: fp32, bf16 autocast,
             fp16 autocast (MIOpen);
  warp       ``warp_up_wino_cl_kernel`` from fp32, bf16 and fp16 channels-last maps through the engine's own call
             (one launch; CALLS back-to-back launches per event pair, time per launch; map bytes read);
  module     the whole module's inference forward, ``backbone_dtype`` None / bf16 / fp16 (same weights);
and the normwise difference max|a - b| / max|a| of ``map_result`` between the fp32 backbone and each 16-bit one —
on this tool's SYNTHETIC (randomly initialised) weights and random frames: an order of magnitude, not a trained
model's accuracy.  The comparison base of every leg is the fp32 leg of the same run.

Writes ``profiles/backbone_dtype_bench.json`` (and prints it)."""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from mvdet_amd import PerspTransDetector, synthetic  # noqa: E402

DTYPES = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}
CALLS = 20  # back-to-back warp launches per event pair (the launch's host cost hides behind the queue)


def _ms(fn, calls: int = 1) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def _stats(ts):
    s = sorted(ts)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "rounds": len(s)}


def _interleaved(legs: dict, rounds: int) -> dict:
    """``legs``: name -> (callable, calls per event pair).  One warm-up of every leg, then ``rounds`` rounds of
    every leg in turn."""
    for k, (fn, calls) in legs.items():
        for _ in range(2):
            _ms(fn, calls)
        print(f"  warmed {k}", file=sys.stderr, flush=True)
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, calls) in legs.items():
            times[k].append(_ms(fn, calls))
    return {k: _stats(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "backbone_dtype_bench.json"))
    ap.add_argument("--ab-lib", default=None, help="an experimental libmvbev build (make -C mvdet_amd/csrc exp) to "
                    "A/B the fused upsample warp against the built library, interleaved")
    ap.add_argument("--ab-note", default="", help="what the experimental build changes (recorded with its numbers)")
    args = ap.parse_args()
    rounds = max(5, args.rounds)
    dev = torch.device("cuda:0")
    ds = synthetic.CONFIGS[2]["make"]()
    N, B = ds.num_cam, 1
    torch.manual_seed(0)
    models = {}
    for name, dt in DTYPES.items():
        m = PerspTransDetector(ds, backbone_dtype=dt).eval()
        if models:
            m.load_state_dict(models["fp32"].state_dict())
        models[name] = m
    frames = torch.randn(B, N, 3, 720, 1280, device=dev)
    out = {"config": synthetic.CONFIGS[2]["name"], "frames": list(frames.shape), "rounds": rounds,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__}

    with torch.no_grad():
        # -- the backbone alone --------------------------------------------------------------------------
        ref = models["fp32"]
        net = torch.nn.Sequential(ref.base_pt1, ref.base_pt2)
        x = frames[0].contiguous(memory_format=torch.channels_last)

        def backbone(dt):
            def run():
                if dt is None:
                    return net(x)
                with torch.autocast("cuda", dtype=dt):
                    return net(x)
            return run
        y = {k: backbone(dt)() for k, dt in DTYPES.items()}
        out["backbone"] = _interleaved({k: (backbone(dt), 1) for k, dt in DTYPES.items()}, rounds)
        for k in DTYPES:
            out["backbone"][k]["out_dtype"] = str(y[k].dtype)
            out["backbone"][k]["channels_last_out"] = y[k].is_contiguous(memory_format=torch.channels_last)
        out["backbone"]["shape"] = list(y["fp32"].shape)

        # -- the fused upsample warp from each dtype's maps ----------------------------------------------
        eng = ref.engine
        ws = eng.workspace(B, dev)
        cams = list(range(N))
        maps32 = [y["fp32"][v:v + 1].contiguous(memory_format=torch.channels_last) for v in range(N)]
        maps = {"fp32": maps32, "bf16": [m.to(torch.bfloat16) for m in maps32],
                "fp16": [m.to(torch.float16) for m in maps32]}
        for k, ms in maps.items():
            assert all(m.is_contiguous(memory_format=torch.channels_last) and float(m.float().abs().max()) > 0 for m in ms)
            eng.warp_views_upsampled(ws, cams, ms)
            assert ws.t_from_warp, "the fused path did not take these maps"
        out["warp"] = _interleaved({k: ((lambda ms=ms: eng.warp_views_upsampled(ws, cams, ms)), CALLS)
                                    for k, ms in maps.items()}, rounds)
        for k, ms in maps.items():
            out["warp"][k]["map_bytes"] = sum(m.numel() * m.element_size() for m in ms)
        out["warp"]["kernel"] = "warp_up_wino_cl_kernel"
        out["warp"]["form"] = int(ws.t_form)
        out["warp"]["launches_per_event_pair"] = CALLS
        if args.ab_lib:  # an experimental build of the library (make exp) against the built one, the same calls
            from mvdet_amd import _native
            base_lib, exp_lib = _native.load(), _native.load(args.ab_lib)

            def through(lib, ms):
                def run():
                    _native._lib = lib
                    try:
                        eng.warp_views_upsampled(ws, cams, ms)
                    finally:
                        _native._lib = base_lib
                return run
            t_base = {}
            for k in ("bf16", "fp16"):  # the experimental build writes the same T
                through(base_lib, maps[k])()
                t_base[k] = (ws.wino_t43 if ws.t_form == 4 else ws.wino_t).clone()
                through(exp_lib, maps[k])()
                assert torch.equal((ws.wino_t43 if ws.t_form == 4 else ws.wino_t).view(torch.int16),
                                   t_base[k].view(torch.int16)), "the experimental build writes another T"
            legs = {}
            for k in ("fp32", "bf16", "fp16"):
                legs[f"{k}_built"] = (through(base_lib, maps[k]), CALLS)
                legs[f"{k}_ab"] = (through(exp_lib, maps[k]), CALLS)
            out["warp_ab"] = _interleaved(legs, rounds)
            out["warp_ab"]["ab_lib"] = Path(args.ab_lib).name
            out["warp_ab"]["note"] = args.ab_note
        eng.fuse(ws, ref.map_classifier)  # (closes the frame: the workspace's guard state)

        # -- the whole module ----------------------------------------------------------------------------
        res = {k: m(frames)[0].float().clone() for k, m in models.items()}
        out["module"] = _interleaved({k: ((lambda m=m: m(frames)), 1) for k, m in models.items()}, rounds)
        scale = float(res["fp32"].abs().max())
        out["map_result_vs_fp32_backbone"] = {
            "note": "SYNTHETIC weights (random init) and random frames: max|a - b| / max|a| of map_result",
            **{k: float((res[k] - res["fp32"]).abs().max()) / scale for k in ("bf16", "fp16")}}
        out["map_result_finite"] = {k: bool(torch.isfinite(v).all()) for k, v in res.items()}

    text = json.dumps(out, indent=1)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
