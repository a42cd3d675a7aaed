"""The backbone's tail at config 2 (Wildtrack, 7 views, 720 x 1280 frames -> 7 maps [1,256,90,160] channels-last into
layer4): what ``PerspTransDetector(native_tail=True)`` / ``mvdet_amd.ResidualTail`` costs and buys, measured.

Legs, interleaved within every round (each leg once per round, >= 5 rounds; medians and min-max), on real
(non-zero) data, HIP events on the stream:
  a  torch ``base_pt2`` in fp32, per view as the detector calls it (``tail_torch_fp32``), and the whole backbone the
     same way (``backbone_torch_fp32``), which gives the tail's share;
  b  torch ``base_pt2`` under bf16 autocast, per view (``tail_torch_bf16``);
  c  the native tail over all views (``tail_native``), and per round one more run with an event before every launch
     group: the conversion, each conv, the 1x1 GEMMs, the polyphase permutation, the block closes (``native_breakdown``);
  d  the whole module's inference forward with ``native_tail`` off and on (same weights).
Accuracy: the normwise difference max|a - ref| / max|ref| of b's and c's output (and of torch's own fp32) from a
float64 evaluation of the same blocks (float64 GEMMs on the GPU, one per tap; checked here against torch's float64
CPU modules on a crop) — on this tool's SYNTHETIC weights (random init, BatchNorm statistics randomised) and random
frames: the arithmetic's error, not a trained model's accuracy.

The yardstick of every leg is leg a of the same run.  Writes ``profiles/res_tail_bench.json`` (and prints it)."""
import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from mvdet_amd import PerspTransDetector, synthetic  # noqa: E402
from mvdet_amd.res_tail import ResidualTail  # noqa: E402


def _ms(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _stats(ts):
    s = sorted(ts)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "rounds": len(s)}


def _breakdown(tail, xs) -> dict:
    """One run of the native tail with an event before every launch group: name -> ms until the next mark."""
    evs = []

    def mark(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        evs.append((name, e))
    tail.mark = mark
    try:
        tail(xs)
    finally:
        tail.mark = None
    torch.cuda.synchronize()
    return {name: e.elapsed_time(evs[i + 1][1]) for i, (name, e) in enumerate(evs[:-1])}


def _conv64(x, w, dil):
    """3x3 conv (padding = dilation) of x [B,C,h,w] float64 as nine float64 GEMMs on shifted copies."""
    B, C, h, wd = x.shape
    xp = F.pad(x, (dil, dil, dil, dil))
    y = torch.zeros(B, w.shape[0], h * wd, dtype=torch.float64, device=x.device)
    for i in range(3):
        for j in range(3):
            xs = xp[:, :, i * dil:i * dil + h, j * dil:j * dil + wd].reshape(B, C, h * wd)
            y += torch.matmul(w[:, :, i, j], xs)
    return y.view(B, -1, h, wd)


def _bn64(bn, y):
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return y * s.view(1, -1, 1, 1) + (bn.bias.double() - bn.running_mean.double() * s).view(1, -1, 1, 1)


def blocks64(blocks, x):
    """The eval-mode BasicBlocks in float64 without a float64 conv kernel."""
    x = x.double()
    for blk in blocks:
        ident = x
        if blk.downsample is not None:
            wd = blk.downsample[0].weight.double()
            ident = _bn64(blk.downsample[1], torch.einsum("oc,bchw->bohw", wd[:, :, 0, 0], x))
        y = torch.relu(_bn64(blk.bn1, _conv64(x, blk.conv1.weight.double(), blk.conv1.dilation[0])))
        y = _bn64(blk.bn2, _conv64(y, blk.conv2.weight.double(), blk.conv2.dilation[0]))
        x = torch.relu(y + ident)
    return x


def _normwise(a, ref) -> float:
    return float((a.double() - ref).abs().max() / ref.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "res_tail_bench.json"))
    args = ap.parse_args()
    rounds = max(5, args.rounds)
    dev = torch.device("cuda:0")
    ds = synthetic.CONFIGS[2]["make"]()
    N, B = ds.num_cam, 1
    torch.manual_seed(0)
    off = PerspTransDetector(ds).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # BatchNorm statistics, gamma, beta as a trained backbone has them: not the identity
        for m in off.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.running_mean.copy_((torch.randn(c, generator=g) * 0.2).to(dev))
                m.running_var.copy_((0.5 + torch.rand(c, generator=g)).to(dev))
                m.weight.copy_((0.75 + 0.5 * torch.rand(c, generator=g)).to(dev))
                m.bias.copy_((torch.randn(c, generator=g) * 0.2).to(dev))
    on = PerspTransDetector(ds, native_tail=True).eval()
    on.load_state_dict(off.state_dict())
    frames = torch.randn(B, N, 3, 720, 1280, device=dev)
    out = {"config": synthetic.CONFIGS[2]["name"], "frames": list(frames.shape), "rounds": rounds,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__}

    with torch.no_grad():
        cl = torch.channels_last
        views = [frames[:, v].contiguous(memory_format=cl) for v in range(N)]
        mids = [off.base_pt1(x) for x in views]
        assert all(m.is_contiguous(memory_format=cl) and float(m.abs().max()) > 0 for m in mids)
        out["tail_input"] = [N] + list(mids[0].shape)
        blocks = off.base_pt2[0]
        tail = ResidualTail(blocks)
        assert tail.native_applies(mids), tail.why_not(tuple(mids[0].shape), N)

        def tail_fp32():
            return [off.base_pt2(m) for m in mids]

        def tail_bf16():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return [off.base_pt2(m) for m in mids]

        def backbone_fp32():
            return [off.base_pt2(off.base_pt1(x)) for x in views]

        legs = {"tail_torch_fp32": tail_fp32, "backbone_torch_fp32": backbone_fp32, "tail_torch_bf16": tail_bf16,
                "tail_native": lambda: tail(mids), "module_tail_off": lambda: off(frames),
                "module_tail_on": lambda: on(frames)}
        for k, fn in legs.items():
            for _ in range(2):
                _ms(fn)
            print(f"  warmed {k}", file=sys.stderr, flush=True)
        times, parts = {k: [] for k in legs}, {}
        for _ in range(rounds):
            for k, fn in legs.items():
                times[k].append(_ms(fn))
            for name, t in _breakdown(tail, mids).items():
                parts.setdefault(name, []).append(t)
        out["legs"] = {k: _stats(v) for k, v in times.items()}
        out["native_breakdown"] = {k: _stats(v) for k, v in parts.items()}
        out["native_breakdown"]["note"] = ("one event before every launch group of one extra run per round; a group's "
                                           "time runs to the next group's event, host gaps included")
        a, bb = out["legs"]["tail_torch_fp32"], out["legs"]["backbone_torch_fp32"]
        out["tail_share_of_backbone"] = round(a["median_ms"] / bb["median_ms"], 4)
        out["native_faster_than_torch_fp32"] = bool(out["legs"]["tail_native"]["max_ms"] < a["min_ms"])

        # -- accuracy against float64 --------------------------------------------------------------------
        crop = mids[0][:, :, :12, :16].contiguous()
        cpu64 = torch.nn.Sequential(*[b for b in blocks])
        import copy
        cpu64 = copy.deepcopy(cpu64).cpu().double()
        out["float64_reference_self_check"] = _normwise(blocks64(blocks, crop).cpu(), cpu64(crop.cpu().double()))
        refs = [blocks64(blocks, m) for m in mids]
        got = {"torch_fp32": tail_fp32(), "torch_bf16": tail_bf16(), "native": tail(mids)}
        out["normwise_vs_float64"] = {
            "note": "SYNTHETIC weights and random frames: max over the views of max|a - ref| / max|ref| of the tail's output",
            **{k: max(_normwise(o, r) for o, r in zip(v, refs)) for k, v in got.items()}}
        res_off, res_on = off(frames), on(frames)
        out["module_map_result_on_vs_off"] = _normwise(res_on[0], res_off[0].double())
        out["module_imgs_result_on_vs_off"] = max(_normwise(p, q.double()) for p, q in zip(res_on[1], res_off[1]))

    text = json.dumps(out, indent=1)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
