"""CPU tests of the CLEAR MOD evaluation's host side (``mvdet_amd.evaluation``): the frame rule and the
metric expressions against what the reference recorded (``tests/golden/eval_cases.npz``, made by
``tools/gen_golden_eval.py``), the fixture itself against the metric's definition (``eval_ref``, with scipy),
and the new ABI's argument validation (no launch)."""
import ctypes

import numpy as np
import pytest

import eval_ref
from helpers import load_golden
from mvdet_amd import _native, evaluation


@pytest.fixture(scope="module")
def g():
    return load_golden("eval_cases")


def test_pack_frames_gives_the_reference_renumbering(g):
    """Unsorted rows, frames 1800, 1805, ..., a GT frame without detections (dropped), a detection frame
    without GT (kept, empty): frame k of ``pack_frames`` holds the rows the reference renumbered to k."""
    p = evaluation.pack_frames(g["pack_gt"], g["pack_det"])
    np.testing.assert_array_equal(p.frames, [1800, 1805, 1810, 1815])
    ref_gt, ref_det = g["pack_gt_all"], g["pack_det_all"]  # [n, 4]: frame index, id, x, y
    for off, xy, ref in ((p.gt_off, p.gt_xy, ref_gt), (p.det_off, p.det_xy, ref_det)):
        assert off.dtype == np.int32 and off[0] == 0 and off[-1] == len(xy) == len(ref)
        frame = np.repeat(np.arange(len(off) - 1), np.diff(off))
        ident = np.concatenate([np.arange(n) for n in np.diff(off)])
        np.testing.assert_array_equal(np.column_stack([frame, ident, xy]), ref)
    assert list(np.diff(p.gt_off)) == [3, 2, 2, 0] and list(np.diff(p.det_off)) == [2, 2, 1, 2]
    # tensors and lists are taken too; an [n, 3] of no rows packs to no frames
    import torch
    q = evaluation.pack_frames(torch.from_numpy(g["pack_gt"]), g["pack_det"].tolist())
    assert all(np.array_equal(a, b) for a, b in zip(p, q))
    assert len(evaluation.pack_frames(g["pack_gt"], np.zeros((0, 3))).frames) == 0


def test_pack_frames_refuses_non_finite_coordinates(g):
    bad = g["pack_det"].copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or inf"):
        evaluation.pack_frames(g["pack_gt"], bad)
    bad = g["pack_gt"].copy()
    bad[0, 2] = np.inf
    with pytest.raises(ValueError, match="NaN or inf"):
        evaluation.pack_frames(bad, g["pack_det"])


def test_metrics_give_the_reference_numbers_on_recorded_counters(g):
    """Counter sets through the reference's closing expressions, g = 0, c = 0 and a negative MODA among
    them; and the demo's per-frame counters summed to its four numbers."""
    at = 0
    seen = []
    for F, want in zip(g["metric_sets"], g["metric_expect"]):
        c, fp, m, gg = g["metric_counters"][4 * at:4 * (at + F)].reshape(F, 4).T
        s = g["metric_modp_sum"][at:at + F]
        at += F
        got = evaluation.metrics(c, fp, m, gg, s)
        assert list(got[:3]) == list(want[:3])
        assert got[3] == pytest.approx(want[3], rel=1e-12, abs=0)
        seen.append((gg.sum() == 0, c.sum() == 0, (m + fp).sum() > gg.sum() > 0 and want[2] == 0))
    assert any(s[0] for s in seen) and any(s[1] and not s[0] for s in seen) and any(s[2] for s in seen)
    got = evaluation.metrics(g["demo_c"], g["demo_fp"], g["demo_m"], g["demo_g"], g["demo_modp_sum"])
    assert list(got[:3]) == list(g["demo_metrics"][:3])
    assert got[3] == pytest.approx(g["demo_metrics"][3], rel=1e-12)
    assert list(g["demo_metrics"]) == [94.9579831932773, 93.58178053830227, 88.4453781512605, 75.60477898846455]


def test_fixture_matches_the_metric_definition(g):
    """``eval_ref`` (the metric from its definition, scipy's assignment) reproduces every per-frame
    expectation of the fixture: the demo's and the synthetic frames'."""
    pytest.importorskip("scipy")
    p = evaluation.pack_frames(g["demo_gt"], g["demo_det"])
    np.testing.assert_array_equal(p.frames, g["demo_frames"])
    np.testing.assert_array_equal(np.diff(p.gt_off), g["demo_g"])
    c, s, cost = eval_ref.case_expect(p.gt_off, p.gt_xy, p.det_off, p.det_xy)
    np.testing.assert_array_equal(c, g["demo_c"])
    np.testing.assert_array_equal(np.diff(p.det_off) - c, g["demo_fp"])
    np.testing.assert_array_equal(np.diff(p.gt_off) - c, g["demo_m"])
    np.testing.assert_allclose(s, g["demo_modp_sum"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(cost, g["demo_cost"], rtol=1e-12, atol=0)
    # the four frames the reference's demo holds a pair at exactly td in
    exact = [int(t) for f, t in enumerate(p.frames)
             if (eval_ref.distances(p.gt_xy[p.gt_off[f]:p.gt_off[f + 1]],
                                    p.det_xy[p.det_off[f]:p.det_off[f + 1]]) == eval_ref.TD).any()]
    assert exact == [1970, 1975, 1985, 1990] == list(g["demo_exact_frames"])
    c, s, cost = eval_ref.case_expect(g["syn_gt_off"], g["syn_gt_xy"], g["syn_det_off"], g["syn_det_xy"])
    np.testing.assert_array_equal(c, g["syn_c"])
    np.testing.assert_allclose(s, g["syn_modp_sum"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(cost, g["syn_cost"], rtol=1e-12, atol=0)
    n_g, n_d = np.diff(g["syn_gt_off"]), np.diff(g["syn_det_off"])
    got = eval_ref.metrics_expect(c, n_d - c, n_g - c, n_g, s)
    assert list(got[:3]) == list(g["syn_metrics"][:3]) and got[3] == pytest.approx(g["syn_metrics"][3], rel=1e-12)


def test_clear_mod_abi_validation_codes():
    """``mvbev_clear_mod_frames`` and the sync-free detection entries return the documented codes before
    any launch (the pointers are never dereferenced)."""
    lib = _native.load()
    p = ctypes.c_void_p(64)

    def frames(gt=p, det=p, dtype=_native.EVAL_F64, go=p, do=p, F=1, Ng=8, Nd=8, small=4, large=8, outs=(p,) * 5,
               ws=None, ws_bytes=0):
        return lib.mvbev_clear_mod_frames(gt, det, dtype, go, do, F, Ng, Nd, small, large, 20.0, *outs, None, ws,
                                          ws_bytes, None)
    assert frames(go=None) == -5 and frames(gt=None) == -5 and frames(outs=(p, p, None, p, p)) == -5
    assert frames(F=0) == -1 and frames(Ng=-1) == -1
    assert frames(dtype=3) == -2
    assert frames(small=_native.CLEAR_MOD_MAX_SMALL + 1, large=2000) == -2  # smaller side 1025
    assert frames(large=_native.CLEAR_MOD_MAX_LARGE + 1) == -2
    assert frames(small=9, large=8) == -2
    # up to 2048 columns live in LDS: no workspace; beyond, 24 bytes per point
    assert lib.mvbev_clear_mod_workspace_bytes(100, 5000, 2048) == 0
    need = lib.mvbev_clear_mod_workspace_bytes(100, 5000, 2049)
    assert need == 24 * 5100
    big = dict(Ng=100, Nd=5000, small=100, large=2049)
    assert frames(**big, ws=None) == -5
    assert frames(**big, ws=p, ws_bytes=need - 1) == -2  # too small
    assert frames(**big, ws=ctypes.c_void_p(68), ws_bytes=need) == -4  # misaligned
    # the sync-free detection entries
    assert lib.mvbev_threshold_points_xy(None, 4, 4, 0.4, 4.0, 0, p, p, p, 16, None) == -5
    assert lib.mvbev_threshold_points_xy(p, 0, 4, 0.4, 4.0, 0, p, p, p, 16, None) == -1
    assert lib.mvbev_threshold_points_xy(p, 4, 4, 0.4, 4.0, 0, p, p, p, 15, None) == -2  # capacity < H * W
    nws = lib.mvbev_point_nms_workspace_bytes(16, 16)
    assert lib.mvbev_point_nms_dev(p, p, None, 16, 20.0, 16, p, p, p, nws, None) == -5
    assert lib.mvbev_point_nms_dev(p, p, p, 0, 20.0, 16, p, p, p, nws, None) == -1
    assert lib.mvbev_point_nms_dev(p, p, p, 16, 20.0, 16, p, p, p, nws - 1, None) == -2
    assert lib.mvbev_point_nms_dev(p, p, p, 16, 20.0, 16, p, p, ctypes.c_void_p(66), nws, None) == -4
    assert lib.mvbev_detections_append(p, p, p, 16, p, 8, p, p, None, None) == -5
    assert lib.mvbev_detections_append(p, p, p, 16, p, 0, p, p, p, None) == -1


def test_evaluator_and_entry_points_refuse_bad_input_on_the_host():
    import torch
    with pytest.raises(ValueError, match="NaN or inf"):
        evaluation.DetectionEvaluator(np.array([[0, 1.0, np.nan]]))
    ev = evaluation.DetectionEvaluator(np.array([[0, 1.0, 2.0]]))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ev.update(torch.zeros(1, 1, 4, 4), 0)
    assert ev.compute() == (0, 0, 0, 0)
    assert evaluation.evaluate(np.zeros((0, 3)), np.array([[0, 1.0, 2.0]])) == (0, 0, 0, 0)
    with pytest.raises(ValueError):
        evaluation.CLEAR_MOD_HUN(np.zeros((0, 4)), np.zeros((0, 4)))
