"""Golden vectors for the CLEAR MOD evaluation (``mvdet_amd.evaluation``) from the reference.

Runs ONLY in the build container: needs ``/root/reference`` and scipy.  It imports the reference's own
``evaluation/pyeval/CLEAR_MOD_HUN.py`` and ``evaluateDetection.py`` and records

* the demo pair (``gt-demo.txt`` / ``test-demo.txt`` as integer arrays), the reference's four numbers
  for it and the per-frame counters c, fp, m, g, MODP sums and optimal costs;
* synthetic frames of the sizes the matching kernel's tests need (integer grid coordinates x 4,
  non-integer fp64 coordinates, duplicated detections, a frame with every pair beyond td, isolated
  pairs at exactly td), with the same per-frame expectations.  The whole set, as one multi-frame
  input, is also run through the reference's ``CLEAR_MOD_HUN`` and its four numbers recorded;
* a hand-built ``pack_frames`` case with the ``gtAllMatrix`` / ``detAllMatrix`` the reference's
  ``evaluateDetection_py`` hands to ``CLEAR_MOD_HUN`` (its frame rule and renumbering);
* counter sets with the numbers the reference's closing expressions (``CLEAR_MOD_HUN.py:93-98``,
  executed from its source) give for them: g = 0, c = 0, a negative MODA.

Per-frame counters are not something the reference returns: they are computed here with scipy on the
reference's cost matrix (``tests/eval_ref.py``), and checked by summing them into the reference's four
numbers.  Every frame is probed for ambiguity before it is recorded: two optimal assignments could count
a different number of exactly-td pairs, so the price of every such pair is moved by +-1e-6 and the frame
solved again; the matched count must not change.  A demo frame that fails stops the run, a synthetic one is
regenerated from the next seed.

It also times the reference on the inputs ``tools/eval_bench.py`` runs (host CPU, one thread of Python) and
writes them to ``profiles/eval_ref_cpu.json``, which the bench quotes beside its GPU times.

Usage:  python tools/gen_golden_eval.py        (writes tests/golden/eval_cases.npz)
"""
from __future__ import annotations

import inspect
import json
import math
import sys
import tempfile
import textwrap
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
REF = Path("/root/reference")
OUT = ROOT / "tests" / "golden" / "eval_cases.npz"
CPU_OUT = ROOT / "profiles" / "eval_ref_cpu.json"
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(REF))

import eval_ref  # noqa: E402
from eval_bench import synthetic_rows  # noqa: E402
from multiview_detector.evaluation.pyeval import evaluateDetection as ref_ed  # noqa: E402
from multiview_detector.evaluation.pyeval.CLEAR_MOD_HUN import CLEAR_MOD_HUN as ref_hun  # noqa: E402

TD = 20.0
SIZES = [(0, 3), (3, 0), (1, 1), (1, 70), (70, 1), (3, 5), (5, 3), (40, 33), (63, 64), (64, 65), (65, 64), (130, 70),
         (7, 300), (12, 3000), (200, 200), (1024, 1030)]
EXTRA = {"float": [(3, 5), (40, 33), (130, 70), (7, 300), (12, 3000), (200, 200)],
         "dup": [(5, 3), (40, 33), (64, 65)], "far": [(3, 5)], "exact": [(1, 1), (3, 5)]}


def make_frame(kind, ng, nd, seed):
    rng = np.random.default_rng(seed)
    if kind == "exact":  # isolated pairs at exactly td (12-16-20), one clear match, the rest far away
        gt = np.array([[0, 0], [400, 400], [800, 0]], np.float64)[:ng]
        det = np.array([[12, 16], [404, 400], [800, 2000], [1600, 20], [816, 12]], np.float64)[:nd]
        return gt, det
    side = max(8, int(math.sqrt(max(ng, nd, 1)) * 6))  # about two detections within td of a GT
    gt = rng.integers(0, side, (ng, 2)) * 4.0
    k = min(ng, nd) * 3 // 4
    det = rng.integers(0, side, (nd, 2)) * 4.0
    det[:k] = gt[rng.permutation(ng)[:k]] + rng.integers(-5, 6, (k, 2)) * 4.0  # up to td per axis, exact pairs among them
    if kind == "float":
        gt = gt + rng.uniform(-2, 2, gt.shape)
        det = det + rng.uniform(-2, 2, det.shape)
    if kind == "dup" and nd >= 2:
        det[1::2] = det[0:2 * (nd // 2):2]  # exact cost ties
    if kind == "far":
        det = det + 5000.0
    return gt, det[rng.permutation(nd)]


def unambiguous(gt, det):
    c = eval_ref.frame_expect(gt, det, TD)[0]
    if not (eval_ref.distances(gt, det) == TD).any():
        return True
    return all(eval_ref.frame_expect(gt, det, TD, bump=b)[0] == c for b in (1e-6, -1e-6))


def hun_rows(off, xy):
    """CSR point lists -> the reference's [n, 4] rows (frame index, id, x, y)."""
    n = np.diff(off)
    frame = np.repeat(np.arange(len(n)), n)
    ident = np.concatenate([np.arange(k) for k in n] + [np.zeros(0, np.int64)])
    return np.column_stack([frame, ident, xy]).astype(np.float64)


def closing_expressions():
    """CLEAR_MOD_HUN.py:93-98 as a callable (c, fp, m, g, distances, td) -> the four numbers, from its source."""
    src = inspect.getsource(ref_hun).splitlines()
    first = next(i for i, ln in enumerate(src) if ln.strip().startswith("MODP ="))
    last = next(i for i, ln in enumerate(src) if ln.strip().startswith("return"))
    body = textwrap.dedent("\n".join(src[first:last]))

    def run(c, fp, m, g, distances, td):
        env = {"np": np, "c": c, "fp": fp, "m": m, "g": g, "distances": distances, "td": td, "sum": sum}
        with np.errstate(all="ignore"):
            exec(body, env)  # noqa: S102
        return [float(env[k]) for k in ("recall", "precision", "MODA", "MODP")]
    return run


def main():
    out = {}
    # ---- the demo pair
    ev = REF / "multiview_detector" / "evaluation"
    gt, det = np.loadtxt(ev / "gt-demo.txt"), np.loadtxt(ev / "test-demo.txt")
    assert (gt == np.round(gt)).all() and (det == np.round(det)).all()
    want = [float(v) for v in ref_ed.evaluateDetection_py(str(ev / "test-demo.txt"), str(ev / "gt-demo.txt"), "Wildtrack")]
    frames = np.unique(det[:, 0])
    cs, ss, costs, gs, ds, exact = [], [], [], [], [], []
    for t in frames:
        g_xy, d_xy = gt[gt[:, 0] == t, 1:3], det[det[:, 0] == t, 1:3]
        assert unambiguous(g_xy, d_xy), f"demo frame {t:g} is ambiguous"
        c, s, cost, _ = eval_ref.frame_expect(g_xy, d_xy, TD)
        if (eval_ref.distances(g_xy, d_xy) == TD).any():
            exact.append(int(t))
        cs.append(c), ss.append(s), costs.append(cost), gs.append(len(g_xy)), ds.append(len(d_xy))
    cs, gs, ds = np.array(cs), np.array(gs), np.array(ds)
    got = eval_ref.metrics_expect(cs, ds - cs, gs - cs, gs, ss)
    assert list(got[:3]) == want[:3] and abs(got[3] - want[3]) <= 1e-12 * want[3], (got, want)
    print("demo:", want, "frames with exact-td pairs:", exact)
    out.update(demo_gt=gt.astype(np.int32), demo_det=det.astype(np.int32), demo_metrics=np.array(want),
               demo_frames=frames.astype(np.int32), demo_c=cs, demo_fp=ds - cs, demo_m=gs - cs, demo_g=gs,
               demo_modp_sum=np.array(ss), demo_cost=np.array(costs), demo_exact_frames=np.array(exact, np.int32))

    # ---- synthetic frames
    todo = [("grid", s) for s in SIZES] + [(k, s) for k, sizes in EXTRA.items() for s in sizes]
    kinds, g_all, d_all, cs, ss, costs, seeds = [], [], [], [], [], [], []
    for idx, (kind, (ng, nd)) in enumerate(todo):
        seed = 1000 * idx
        while True:
            g_xy, d_xy = make_frame(kind, ng, nd, seed)
            if unambiguous(g_xy, d_xy):
                break
            assert kind != "exact"
            seed += 1
        c, s, cost, _ = eval_ref.frame_expect(g_xy, d_xy, TD)
        kinds.append(kind), g_all.append(g_xy), d_all.append(d_xy), cs.append(c), ss.append(s), costs.append(cost)
        seeds.append(seed)
        n_exact = int((eval_ref.distances(g_xy, d_xy) == TD).sum())
        print(f"{kind:6s} ({ng},{nd}) seed {seed}: c = {c}, exact-td pairs {n_exact}, cost {cost:.6f}")
    g_off = np.concatenate([[0], np.cumsum([len(a) for a in g_all])]).astype(np.int32)
    d_off = np.concatenate([[0], np.cumsum([len(a) for a in d_all])]).astype(np.int32)
    g_xy, d_xy = np.concatenate(g_all), np.concatenate(d_all)
    cs, n_g, n_d = np.array(cs), np.diff(g_off), np.diff(d_off)
    t0 = time.perf_counter()
    want = [float(v) for v in ref_hun(hun_rows(g_off, g_xy), hun_rows(d_off, d_xy))]
    print(f"reference CLEAR_MOD_HUN on the synthetic set: {time.perf_counter() - t0:.1f} s ->", want)
    # the last frames could hold no GT, which ends the reference's frame range early: they do not
    assert n_g[-1] > 0
    got = eval_ref.metrics_expect(cs, n_d - cs, n_g - cs, n_g, ss)
    assert list(got[:3]) == want[:3] and abs(got[3] - want[3]) <= 1e-12 * max(want[3], 1), (got, want)
    out.update(syn_kind=np.array(kinds), syn_seed=np.array(seeds), syn_gt_off=g_off, syn_det_off=d_off, syn_gt_xy=g_xy,
               syn_det_xy=d_xy, syn_c=cs, syn_modp_sum=np.array(ss), syn_cost=np.array(costs),
               syn_metrics=np.array(want))

    # ---- pack_frames: what evaluateDetection_py hands to CLEAR_MOD_HUN
    pg = np.array([[1810, 40, 44], [1800, 8, 12], [1805, 100, 60], [1800, 52, 48], [1820, 4, 4], [1805, 16, 20],
                   [1800, 200, 200], [1810, 44, 40]], np.float64)  # 1820: GT without detections
    pd = np.array([[1805, 100, 64], [1815, 300, 300], [1800, 8, 16], [1810, 40, 40], [1800, 48, 48], [1815, 8, 8],
                   [1805, 400, 400]], np.float64)  # 1815: detections without GT
    seen = {}

    def recorder(gt_all, det_all):
        seen["gt"], seen["det"] = np.array(gt_all), np.array(det_all)
        return ref_hun(gt_all, det_all)
    keep = ref_ed.CLEAR_MOD_HUN
    ref_ed.CLEAR_MOD_HUN = recorder
    try:
        with tempfile.TemporaryDirectory() as tmp:
            np.savetxt(f"{tmp}/gt.txt", pg, "%d")
            np.savetxt(f"{tmp}/res.txt", pd, "%d")
            pm = ref_ed.evaluateDetection_py(f"{tmp}/res.txt", f"{tmp}/gt.txt", "Wildtrack")
    finally:
        ref_ed.CLEAR_MOD_HUN = keep
    out.update(pack_gt=pg, pack_det=pd, pack_gt_all=seen["gt"], pack_det_all=seen["det"],
               pack_metrics=np.array([float(v) for v in pm]))

    # ---- counter sets through the reference's closing expressions
    close = closing_expressions()
    sets = [  # per-frame c, fp, m, g and the matched distances per frame
        ([2, 1], [1, 0], [0, 2], [2, 3], [[3.0, 12.5], [7.25]]),
        ([0, 0], [2, 1], [3, 1], [3, 1], [[], []]),           # c = 0
        ([0, 0], [2, 0], [0, 0], [0, 0], [[], []]),           # g = 0
        ([1, 1], [6, 4], [1, 0], [2, 1], [[19.5], [0.0]]),    # MODA < 0 -> 0
        ([0], [0], [0], [0], [[]]),                            # nothing at all
    ]
    cnt, exp, msum = [], [], []
    for c, fp, m, g, dist in sets:
        F = len(c)
        width = max(max((len(d) for d in dist), default=0), 1)
        dm = np.inf * np.ones((F, width))
        for f, d in enumerate(dist):
            dm[f, :len(d)] = d
        exp.append(close(np.array([c], np.float64), np.array([fp], np.float64), np.array([m], np.float64),
                         np.array([g], np.float64), dm, TD))
        per = [float(sum(1 - np.array(d) / TD)) if len(d) else 0.0 for d in dist]
        cnt.append(np.array([c, fp, m, g], np.float64).T.reshape(-1))
        msum.append(per)
    out.update(metric_sets=np.array([len(s[0]) for s in sets]),
               metric_counters=np.concatenate(cnt), metric_modp_sum=np.concatenate([np.array(p) for p in msum]),
               metric_expect=np.array(exp))
    print("counter sets ->", exp)

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, OUT.stat().st_size, "bytes")

    # ---- the reference's host time on the bench inputs
    cpu = {"scipy": __import__("scipy").__version__, "what": "reference CLEAR_MOD_HUN, host CPU seconds (one run)"}
    t0 = time.perf_counter()
    ref_ed.evaluateDetection_py(str(ev / "test-demo.txt"), str(ev / "gt-demo.txt"), "Wildtrack")
    cpu["demo"] = round(time.perf_counter() - t0, 4)
    for name, (F, ng, nd) in {"400x40x300": (400, 40, 300), "40x40x2000": (40, 40, 2000)}.items():
        g_rows, d_rows = synthetic_rows(F, ng, nd)
        to4 = lambda r, n: np.column_stack([r[:, 0], np.arange(len(r)) % n, r[:, 1:3]]).astype(np.float64)  # noqa: E731
        t0 = time.perf_counter()
        res = ref_hun(to4(g_rows, ng), to4(d_rows, nd))
        cpu[name] = round(time.perf_counter() - t0, 4)
        cpu[name + "_metrics"] = [float(v) for v in res]
    CPU_OUT.write_text(json.dumps(cpu) + "\n")
    print("wrote", CPU_OUT, cpu)


if __name__ == "__main__":
    main()
