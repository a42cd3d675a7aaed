"""The CLEAR MOD detection metrics from their definition (numpy, scipy for the assignment): the
reference side of the evaluation tests, stated independently of the reference's loop.

Per frame, with GT points g_o and detections e_e on the ground plane and the threshold td:
  * the distance D[o, e] = sqrt(dx^2 + dy^2) in fp64; a pair may be assigned at price D if D <= td,
    any other pair costs 1e6;
  * the one-to-one assignment of the smaller set into the larger of minimum total price
    (``scipy.optimize.linear_sum_assignment``);
  * an assigned pair with D < td is a match: c matches, fp = n_det - c false positives,
    m = n_gt - c misses; the frame's MODP sum is the sum over matched GT of 1 - D / td.
Over the frames:  recall = c / g,  precision = c / (c + fp),  N-MODA = 1 - (m + fp) / g,
N-MODP = (sum of the MODP sums) / c,  each in percent and 0 unless positive.
"""
import numpy as np

TD = 20.0
BEYOND = 1e6


def distances(gt_xy, det_xy):
    gt_xy, det_xy = np.asarray(gt_xy, np.float64).reshape(-1, 2), np.asarray(det_xy, np.float64).reshape(-1, 2)
    dx = gt_xy[:, None, 0] - det_xy[None, :, 0]
    dy = gt_xy[:, None, 1] - det_xy[None, :, 1]
    return np.sqrt(dx * dx + dy * dy)


def frame_expect(gt_xy, det_xy, td=TD, bump=None):
    """(c, modp_sum, cost, pairs) of one frame; ``bump`` is added to the price of every pair at exactly td
    (the fixture generator's ambiguity probe)."""
    from scipy.optimize import linear_sum_assignment
    D = distances(gt_xy, det_xy)
    price = np.where(D <= td, D, BEYOND)
    if bump is not None:
        price = price + np.where(D == td, bump, 0.0)
    if D.size == 0:
        return 0, 0.0, 0.0, np.zeros((0, 2), np.int64)
    rows, cols = linear_sum_assignment(price)
    hit = D[rows, cols] < td
    pairs = np.stack([rows[hit], cols[hit]], 1)
    pairs = pairs[np.argsort(pairs[:, 0])]
    modp = 0.0
    for o, e in pairs:  # GT order
        modp += 1 - D[o, e] / td
    return int(hit.sum()), modp, float(np.where(D <= td, D, BEYOND)[rows, cols].sum()), pairs


def case_expect(gt_off, gt_xy, det_off, det_xy, td=TD):
    """Per-frame arrays (c, modp_sum, cost) of CSR point lists."""
    out = [frame_expect(gt_xy[gt_off[f]:gt_off[f + 1]], det_xy[det_off[f]:det_off[f + 1]], td)[:3]
           for f in range(len(gt_off) - 1)]
    c, s, cost = zip(*out)
    return np.array(c, np.int64), np.array(s, np.float64), np.array(cost, np.float64)


def metrics_expect(c, fp, m, g, modp_sum):
    """(recall, precision, MODA, MODP) in percent from the totals, 0 unless positive."""
    c, fp, m, g, s = (float(np.sum(np.asarray(a, np.float64))) for a in (c, fp, m, g, modp_sum))

    def pct(num, den):
        v = num / den * 100 if den else float("nan")
        return v if v > 0 else 0
    recall, precision, modp = pct(c, g), pct(c, fp + c), pct(s, c)
    moda = (1 - (m + fp) / g) * 100 if g else float("nan")
    return recall, precision, moda if moda > 0 else 0, modp
