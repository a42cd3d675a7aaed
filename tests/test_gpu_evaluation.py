"""GPU tests of the CLEAR MOD evaluation (``mvdet_amd.evaluation``): the matching kernel against the
per-frame expectations of ``tests/golden/eval_cases.npz`` (the reference's demo and synthetic frames; nothing is
imported from the reference or scipy), the drop-in entry points on the demo, and ``DetectionEvaluator`` against
``postprocess.threshold_rows`` + ``frame_results`` and ``evaluate``.

Tolerance of the fp64 sums: a frame sums at most 1024 terms and a case at most 10^6, each within fp64's
eps = 1.1e-16 of its value, so N eps <= 1.1e-10 relative; the bound is 1e-9 (x10 margin)."""
import numpy as np
import pytest
import torch

from helpers import load_golden

pytestmark = pytest.mark.gpu

TD = 20.0
RTOL = 1e-9
SIZES = [(0, 3), (3, 0), (1, 1), (1, 70), (70, 1), (3, 5), (5, 3), (40, 33), (63, 64), (64, 65), (65, 64), (130, 70),
         (7, 300), (12, 3000), (200, 200), (1024, 1030)]
INTEGER_KINDS = ("grid", "dup", "far", "exact")


@pytest.fixture(scope="module")
def g():
    return load_golden("eval_cases")


def csr(g, idx, perm_seed=None):
    """The fixture's synthetic frames ``idx`` (repeats allowed) as one CSR input; ``perm_seed``: the detections
    shuffled inside each frame."""
    go, do = g["syn_gt_off"], g["syn_det_off"]
    gt = [g["syn_gt_xy"][go[f]:go[f + 1]] for f in idx]
    det = [g["syn_det_xy"][do[f]:do[f + 1]] for f in idx]
    if perm_seed is not None:
        rng = np.random.default_rng(perm_seed)
        det = [d[rng.permutation(len(d))] for d in det]
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)  # noqa: E731
    return np.concatenate(gt), off(gt), np.concatenate(det), off(det)


def launch(g, idx, dtype=np.float64, perm_seed=None):
    from mvdet_amd import evaluation
    gt, go, det, do = csr(g, idx, perm_seed)
    r = evaluation.clear_mod_frames(gt.astype(dtype), go, det.astype(dtype), do, TD, want_match=True)
    return r, (gt, go, det, do)


def check(g, idx, r, data):
    """Counts exact, sums within RTOL of the fixture's, and ``match`` an injective map of pairs with d < td
    whose recomputed sums are the outputs."""
    gt, go, det, do = data
    idx = np.asarray(idx)
    np.testing.assert_array_equal(r["n_gt"], np.diff(go))
    np.testing.assert_array_equal(r["n_det"], np.diff(do))
    np.testing.assert_array_equal(r["matched"], g["syn_c"][idx])
    np.testing.assert_allclose(r["modp_sum"], g["syn_modp_sum"][idx], rtol=RTOL, atol=0)
    np.testing.assert_allclose(r["cost"], g["syn_cost"][idx], rtol=RTOL, atol=0)
    assert r["match"].shape == (len(gt),)
    for f in range(len(idx)):
        mt = r["match"][go[f]:go[f + 1]]
        hit = np.flatnonzero(mt >= 0)
        assert (mt >= -1).all() and (mt < do[f + 1] - do[f]).all()
        assert len(set(mt[hit].tolist())) == len(hit) == r["matched"][f]  # injective
        d = gt[go[f]:go[f + 1]][hit] - det[do[f]:do[f + 1]][mt[hit]]
        d = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        assert (d < TD).all()
        s = 0.0
        for v in d:  # GT order
            s += 1 - v / TD
        assert s == pytest.approx(r["modp_sum"][f], rel=1e-12, abs=0)


def test_fixture_covers_the_sizes_and_data_cases(g):
    sizes = list(zip(np.diff(g["syn_gt_off"]).tolist(), np.diff(g["syn_det_off"]).tolist()))
    kinds = g["syn_kind"].tolist()
    assert [s for s, k in zip(sizes, kinds) if k == "grid"] == SIZES
    assert {"float", "dup", "far", "exact"} <= set(kinds)
    far = kinds.index("far")
    assert g["syn_c"][far] == 0 and g["syn_cost"][far] == 1e6 * min(sizes[far])  # every pair beyond td
    ex = [i for i, k in enumerate(kinds) if k == "exact"]
    assert sizes[ex[0]] == (1, 1) and g["syn_c"][ex[0]] == 0 and g["syn_cost"][ex[0]] == TD  # matched at td, not counted


def test_every_frame_alone(g):
    """F = 1 launches: each size (LDS column state up to 2048 columns, the workspace for (12, 3000)) and each
    data case on its own."""
    for f in range(len(g["syn_c"])):
        r, data = launch(g, [f])
        check(g, [f], r, data)


@pytest.mark.parametrize("F", [None, 67, 300])
def test_mixed_sizes_in_one_launch(g, F):
    """All frames in one launch of mixed sizes (both column-state paths side by side); F = 67 and F = 300
    (more frames than CUs) repeat them cyclically."""
    n = len(g["syn_c"])
    idx = list(range(n)) if F is None else [(3 * k) % n for k in range(F)]
    r, data = launch(g, idx)
    check(g, idx, r, data)


def test_fp32_and_fp64_inputs_of_integer_points_agree_bitwise(g):
    idx = [i for i, k in enumerate(g["syn_kind"].tolist()) if k in INTEGER_KINDS]
    a, data = launch(g, idx, np.float64)
    b, _ = launch(g, idx, np.float32)
    check(g, idx, a, data)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    # fp64 GT with fp32 detections (the evaluator's launch)
    from mvdet_amd import evaluation
    gt, go, det, do = data
    c = evaluation.clear_mod_frames(gt, go, det.astype(np.float32), do, TD, want_match=True)
    for k in a:
        assert a[k].tobytes() == c[k].tobytes(), k


def test_shuffled_detections_change_only_the_match(g):
    idx = list(range(len(g["syn_c"])))
    r, data = launch(g, idx, perm_seed=5)
    check(g, idx, r, data)


def test_two_launches_are_bitwise_equal(g):
    idx = [(5 * k) % len(g["syn_c"]) for k in range(40)]
    a, _ = launch(g, idx)
    b, _ = launch(g, idx)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_frames_past_the_stated_bounds_are_reported_not_run(g):
    """A frame larger than the bounds the caller stated (here: more columns than LDS holds, no workspace) is
    flagged with matched = -1 and left alone; its neighbours are solved."""
    from mvdet_amd import _native, evaluation
    kinds = g["syn_kind"].tolist()
    sizes = list(zip(np.diff(g["syn_gt_off"]).tolist(), np.diff(g["syn_det_off"]).tolist()))
    big, small = sizes.index((12, 3000)), sizes.index((3, 5))
    assert kinds[big] == "grid"
    gt, go, det, do = csr(g, [small, big, small])
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    out = evaluation._launch_matching(t(gt), t(det), _native.EVAL_F64, t(go), t(do), 3, 12, 2048, TD, False, None)
    r = out.read()
    assert r["matched"].tolist() == [g["syn_c"][small], -1, g["syn_c"][small]]
    assert r["n_det"].tolist() == [5, 3000, 5]


def test_demo_through_the_drop_in_entry_points(g, tmp_path):
    """The reference's demo: recall, precision and MODA are the same fp64 expression on integer counts (==),
    MODP within RTOL; from arrays, from tensors on the GPU and from text files."""
    from mvdet_amd import evaluation
    want = g["demo_metrics"].tolist()
    gt, det = g["demo_gt"], g["demo_det"]
    np.savetxt(tmp_path / "gt.txt", gt, "%d")
    np.savetxt(tmp_path / "res.txt", det, "%d")
    for got in (evaluation.evaluate(det, gt),
                evaluation.evaluate(torch.from_numpy(det).cuda(), torch.from_numpy(gt).cuda()),
                evaluation.evaluateDetection_py(str(tmp_path / "res.txt"), str(tmp_path / "gt.txt"), "Wildtrack"),
                evaluation.evaluate(str(tmp_path / "res.txt"), tmp_path / "gt.txt")):
        assert list(got[:3]) == want[:3]
        assert got[3] == pytest.approx(want[3], rel=RTOL, abs=0)
    # per frame, the four frames with a pair at exactly td included
    p = evaluation.pack_frames(gt, det)
    r = evaluation.clear_mod_frames(p.gt_xy, p.gt_off, p.det_xy, p.det_off)
    np.testing.assert_array_equal(r["matched"], g["demo_c"])
    np.testing.assert_array_equal(r["n_gt"], g["demo_g"])
    np.testing.assert_array_equal(r["n_det"] - r["matched"], g["demo_fp"])
    np.testing.assert_allclose(r["modp_sum"], g["demo_modp_sum"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(r["cost"], g["demo_cost"], rtol=RTOL, atol=0)
    (tmp_path / "empty.txt").write_text("")
    assert evaluation.evaluate(str(tmp_path / "empty.txt"), str(tmp_path / "gt.txt")) == (0, 0, 0, 0)


def test_clear_mod_hun_on_the_synthetic_set(g):
    """``CLEAR_MOD_HUN`` itself ([n, 4] rows; its frames are 0 .. max GT frame, so frames with GT and no
    detection count) against the reference's numbers for the synthetic frames as one input."""
    from mvdet_amd import evaluation

    def rows(off, xy):
        n = np.diff(off)
        return np.column_stack([np.repeat(np.arange(len(n)), n), np.concatenate([np.arange(k) for k in n]), xy])
    gt, det = rows(g["syn_gt_off"], g["syn_gt_xy"]), rows(g["syn_det_off"], g["syn_det_xy"])
    want = g["syn_metrics"].tolist()
    for got in (evaluation.CLEAR_MOD_HUN(gt, det), evaluation.CLEAR_MOD_HUN(torch.from_numpy(gt).cuda(), det)):
        assert list(got[:3]) == want[:3]
        assert got[3] == pytest.approx(want[3], rel=RTOL, abs=0)


def blob_map(H, W, centres, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = rng.uniform(0, 0.05, size=(H, W)).astype(np.float32)
    for cy, cx in centres:
        m += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 2.0 ** 2)).astype(np.float32)
    return m


@pytest.fixture(scope="module")
def epoch():
    """(frame, map) in update order: the two trainer-style maps of nms_cases.npz and three small blob maps, one of
    them with no cell over the threshold; frame numbers unsorted."""
    n = load_golden("nms_cases")
    maps = [(1805, n["map0"]), (1800, n["map1"]), (1815, blob_map(23, 37, [(5, 6), (17, 30), (6.5, 8)], 1)),
            (1795, np.zeros((23, 37), np.float32)), (1810, blob_map(40, 29, [(20, 14), (0, 0), (39, 28), (22, 15)], 2))]
    return [(f, torch.from_numpy(m)[None, None].cuda()) for f, m in maps]


@pytest.mark.parametrize("indexing", ["ij", "xy"])
def test_detection_evaluator_matches_the_row_path(epoch, indexing):
    from mvdet_amd import evaluation, postprocess
    want = torch.cat([postprocess.frame_results(postprocess.threshold_rows(m, f, 0.4, 4, indexing))
                      for f, m in sorted(epoch, key=lambda e: e[0])], 0)
    assert want.shape[0] > 30 and 1795 not in want[:, 0].tolist()
    # GT: most detections displaced by less than td, some by more, some GT nowhere near; a GT frame never updated
    rng = np.random.default_rng(9)
    w = want.cpu().numpy().astype(np.float64)
    gt = w[rng.random(len(w)) < 0.8]
    gt[:, 1:] += rng.integers(-4, 5, (len(gt), 2)) * 4.0
    gt = np.concatenate([gt, [[1805, 4000, 4000], [1795, 8, 8], [1795, 40, 40], [1990, 0, 0]]])
    gt = gt[rng.permutation(len(gt))]
    ev = evaluation.DetectionEvaluator(gt, cls_thres=0.4, grid_reduce=4, indexing=indexing, max_frames=8,
                                       max_dets=4096)
    strict = hasattr(torch.cuda, "set_sync_debug_mode")
    for rounds in range(2):  # the second epoch after reset(): the same again
        if strict:
            torch.cuda.set_sync_debug_mode("error")
        try:
            for f, m in epoch:
                ev.update(m, f)
        finally:
            if strict:
                torch.cuda.set_sync_debug_mode("default")
        res = ev.results()
        assert res.dtype == want.dtype and torch.equal(res, want)
        got = ev.compute()
        assert got == evaluation.evaluate(res, gt)  # the empty frame 1795 is left out of both
        assert got == evaluation.evaluate(want.cpu().numpy(), gt) and got[0] > 0 and got[3] > 0
        ev.reset()
    with pytest.raises(ValueError, match="already updated"):
        ev.update(epoch[0][1], 7)
        ev.update(epoch[0][1], 7)


def test_detection_evaluator_of_empty_maps_gives_zeros(epoch):
    from mvdet_amd import evaluation
    ev = evaluation.DetectionEvaluator(np.array([[1, 8.0, 8.0], [2, 4.0, 4.0]]))
    assert ev.compute() == (0, 0, 0, 0)
    empty = epoch[3][1]
    ev.update(empty, 1)
    ev.update(empty * 0 + 0.3, 2)
    assert ev.compute() == (0, 0, 0, 0)
    assert ev.results().shape == (0, 3)


def test_detection_evaluator_overflow_is_an_error_and_stays_in_bounds(epoch):
    from mvdet_amd import _native, evaluation
    ev = evaluation.DetectionEvaluator(np.array([[1805, 8.0, 8.0]]), max_dets=3, max_frames=4)
    ev.update(epoch[0][1], 1805)
    with pytest.raises(RuntimeError, match="max_dets"):
        ev.compute()
    with pytest.raises(RuntimeError, match="max_dets"):
        ev.results()
    # the append itself, with a guard region behind the buffer
    lib, dev = _native.load(), torch.device("cuda:0")
    pts = torch.arange(20, dtype=torch.float32, device=dev).reshape(10, 2)
    keep = torch.tensor([7, 2, 9, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int64, device=dev)
    count = torch.tensor([3], dtype=torch.int32, device=dev)
    max_dets, guard = 5, 16
    buf = torch.full((max_dets + guard, 2), -7.0, device=dev)
    state = torch.tensor([2, 0, -1, -1], dtype=torch.int32, device=dev)  # cursor, overflow, two frame ends
    st = torch.cuda.current_stream().cuda_stream

    def append(slot):
        return lib.mvbev_detections_append(pts.data_ptr(), keep.data_ptr(), count.data_ptr(), 10, buf.data_ptr(),
                                           max_dets, state.data_ptr(), state.data_ptr() + 4 * (2 + slot),
                                           state.data_ptr() + 4, st)
    assert append(0) == 0  # 2 + 3 = 5: fits exactly
    assert state.tolist() == [5, 0, 5, -1]
    assert torch.equal(buf[2:5], pts[[7, 2, 9]]) and (buf[:2] == -7).all() and (buf[5:] == -7).all()
    count.fill_(1)
    before = buf.clone()
    assert append(1) == 0  # one more does not
    assert state.tolist() == [5, 1, 5, 5]
    assert torch.equal(buf, before)
