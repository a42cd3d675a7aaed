"""GPU tests of point-list targets in the native criterion (``mvdet_amd.targets`` through
``mvdet_amd.loss`` on ``mvbev_gaussian_mse_points_f32``).

Every case runs the criterion twice on the same ``x`` and kernel, once on a ``PointTargets`` and once
on its ``dense()``, and requires ``torch.equal`` on the loss, the transformed target, the kernel's
``diff`` buffer and ``x.grad``: the point path stages, word for word, the tile the dense path stages
after pooling.  So that the check does not rest on the dense GPU path alone, the point path is also
held against the CPU restatement (``tests/loss_ref.py``) at ``test_gpu_loss.py``'s gate: normwise
``5e-6``, the loss relative ``5e-6`` (fp32 sums of at most 1681 taps that differ in order only)."""
import numpy as np
import pytest
import torch

import loss_ref
from mvdet_amd import loss
from mvdet_amd.targets import PointTargets, pack_step, pooled_range

pytestmark = pytest.mark.gpu

TOL = 5e-6
DEV = "cuda:0"
TH, TW = loss.TILE_H, loss.TILE_W

_kernels = {}


def kernels():
    if not _kernels:
        _kernels["map"], _kernels["img"] = loss.gaussian_kernels(4, 4)
    return _kernels["map"], _kernels["img"]


def rand_x(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-0.2, 1.0, size=shape).astype(np.float32))


def rand_cells(shape, n, seed):
    flat = np.random.default_rng(seed).choice(int(np.prod(shape)), size=n, replace=False)
    return [tuple(int(v) for v in c) for c in np.stack(np.unravel_index(flat, shape), axis=1)]


class Coo:
    def __init__(self):
        self.row, self.col, self.data = [], [], []


def from_cells(shape, cells, vals=None):
    """PointTargets through ``from_coo`` from (b, c, row, col) cells; repeated cells stay duplicates."""
    B, C, Ht, Wt = shape
    mats = [[Coo() for _ in range(C)] for _ in range(B)]
    for i, (b, c, r, q) in enumerate(cells):
        m = mats[b][c]
        m.row.append(r), m.col.append(q), m.data.append(1.0 if vals is None else vals[i])
    return PointTargets.from_coo(mats, (Ht, Wt))


def close(got, ref, what):
    nw = loss_ref.normwise(got, ref)
    print(f"{what}: normwise {nw:.3e}")
    assert nw <= TOL, (what, nw)


def run_single(xd, target, kernel):
    """(loss, t_out, diff, grad, launch) of one criterion call and one ``_traget_transform``."""
    crit = loss.GaussianMSE()
    xd = xd.detach().requires_grad_()
    ls = crit(xd, target, kernel)
    launch = ls.grad_fn.launch
    diff = launch.diff[0]
    ls.backward()
    return ls.detach(), crit._traget_transform(xd, target, kernel), diff, xd.grad, launch


def check_points(x, pt, kernel, x_dev=None, finite=True):
    """The point path bitwise against the dense GPU path on ``pt.dense()`` and within the gate of the
    restatement.  Returns the point path's (loss, t_out, diff, grad, launch)."""
    assert pt.device.type == "cpu"
    xd = x.to(DEV) if x_dev is None else x_dev
    pd = pt.to(DEV)
    got = run_single(xd, pd, kernel)
    ref = run_single(xd, pd.dense(), kernel)
    assert got[4].n_pooled == 0 and got[4].launches == ["mse", "finalize"]
    for a, b, what in zip(got[:4], ref[:4], ("loss", "t_out", "diff", "grad_x")):
        assert a.shape == b.shape and a.dtype == b.dtype
        if finite:
            assert torch.equal(a, b), what
        else:  # the same NaN pattern, the finite values bitwise equal
            assert torch.equal(torch.isnan(a), torch.isnan(b)), what
            assert torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)]), what
    if finite:
        t_ref, d_ref, l_ref, g_ref = loss_ref.single(x, pt.dense(), kernel)
        close(got[1], t_ref, "t_out")
        close(got[2], d_ref, "diff")
        close(got[3], g_ref, "grad_x")
        rel = abs(got[0].item() - float(l_ref)) / abs(float(l_ref))
        print(f"loss: native {got[0].item():.9g} ref {float(l_ref):.9g} rel {rel:.3e}")
        assert rel <= TOL
    return got


@pytest.mark.parametrize("cells", [
    [(0, 0, 0, 0), (0, 0, 0, 149), (0, 0, 39, 0), (0, 0, 39, 149)],  # the image's corners
    [(0, 0, TH, TW)], [(0, 0, TH - 1, TW - 1)],                       # a tile corner: the stamp spans four tiles
    [(0, 0, TH, 2 * TW)],
], ids=["corners", "tile_corner", "tile_corner_m1", "tile_corner_2"])
def test_same_size_map_kernel_tile_corners(cells):
    """h = 40 and w = 150 are no multiples of the 16 x 64 tile: 3 x 3 tiles, the last ones partial; the
    41 x 41 stamp of each cell is clipped by the halo of every tile around it."""
    mk, _ = kernels()
    check_points(rand_x((1, 1, 40, 150), 21), from_cells((1, 1, 40, 150), cells), mk)


def test_same_size_as_the_stats_item():
    """The same cells through ``detection_loss``: the counts read the raw target from the tile's centre."""
    mk, ik = kernels()
    x = rand_x((1, 1, 40, 150), 21)
    cells = [(0, 0, 0, 0), (0, 0, 39, 149), (0, 0, TH, TW), (0, 0, TH - 1, TW - 1), (0, 0, TH, 2 * TW)]
    pt = from_cells((1, 1, 40, 150), cells)
    for _, _, r, q in cells[::2]:
        x[0, 0, r, q] = 0.9
    xd, pd = x.to(DEV), pt.to(DEV)
    ls, stats = loss.detection_loss(xd, [], pd, [], mk, ik, cls_thres=0.4)
    ls2, stats2 = loss.detection_loss(xd, [], pd.dense(), [], mk, ik, cls_thres=0.4)
    assert torch.equal(ls, ls2) and torch.equal(stats, stats2)
    l_ref, _, counts = loss_ref.step(x, [], pt.dense(), [None], mk, ik, 1.0, 0.4)
    assert abs(ls.item() - l_ref.item()) <= TOL * l_ref.item()
    assert tuple(stats.tolist()) == tuple(float(c) for c in counts) and stats[0].item() >= 3


def test_factor4_pool_max_wins_and_duplicates_sum():
    _, ik = kernels()
    shape = (2, 2, 108, 192)
    cells = rand_cells(shape, 14, 4)
    vals = [1.0] * 14
    cells += [(1, 0, 41, 82), (1, 0, 43, 80)]   # one 4 x 4 window (rows 40..43, columns 80..83): the max wins
    vals += [1.0, 3.0]
    cells += [(0, 1, 70, 101), (0, 1, 70, 101)]  # coo duplicates: summed to 2
    vals += [1.0, 1.0]
    pt = from_cells(shape, cells, vals)
    assert len(pt) == 17 and pt.dense()[0, 1, 70, 101] == 2
    _, t, _, _, _ = check_points(rand_x((2, 2, 27, 48), 3), pt, ik)
    assert t[1, 0, 10, 20].item() >= 3.0  # the window's pooled value is 3, under the kernel's centre tap of 1


def test_uneven_overlapping_windows():
    _, ik = kernels()
    shape, h, w = (2, 2, 50, 77), 12, 36
    first_r, last_r = pooled_range(50, h)
    first_c, last_c = pooled_range(77, w)
    rows2, cols2 = np.flatnonzero(last_r > first_r), np.flatnonzero(last_c > first_c)
    assert len(rows2) and len(cols2)  # rows and columns that belong to two windows
    cells = rand_cells(shape, 26, 6)
    extra = [(0, 0, int(rows2[0]), int(cols2[0])), (1, 1, int(rows2[-1]), int(cols2[-1])),
             (0, 1, int(rows2[1]), 3), (1, 0, 4, int(cols2[2]))]
    cells += [c for c in extra if c not in cells]
    starts, ends = loss.pool_windows(50, h)
    assert any(((starts <= r) & (r < ends)).sum() == 2 for _, _, r, _ in cells)
    starts, ends = loss.pool_windows(77, w)
    assert any(((starts <= q) & (q < ends)).sum() == 2 for _, _, _, q in cells)
    check_points(rand_x((2, 2, h, w), 5), from_cells(shape, cells), ik)


def test_target_smaller_than_x():
    """Each cell covers a run of pooled cells; from 5 x 9 to 40 x 150 the runs cross tile borders."""
    mk, _ = kernels()
    check_points(rand_x((1, 1, 7, 9), 7), from_cells((1, 1, 3, 5), rand_cells((1, 1, 3, 5), 3, 8)), mk)
    cells = [(0, 0, 1, 3), (0, 0, 2, 4), (0, 0, 4, 8), (0, 0, 0, 0)]
    _, t, _, _, _ = check_points(rand_x((1, 1, 40, 150), 9), from_cells((1, 1, 5, 9), cells, [1.0, 2.0, 1.0, 0.5]), mk)
    assert torch.count_nonzero(t).item() > 0


def test_empty_list_and_an_empty_frame():
    mk, ik = kernels()
    x = rand_x((1, 1, 40, 150), 20)
    ls, t, _, grad, _ = check_points(x, from_cells((1, 1, 40, 150), []), mk)
    assert torch.count_nonzero(t).item() == 0  # exactly 0
    ref = (x.double() ** 2).mean().item()
    assert abs(ls.item() - ref) <= TOL * ref
    close(grad, 2 * x / x.numel(), "grad_x")
    shape = (2, 2, 108, 192)
    pt = from_cells(shape, [(1,) + c[1:] for c in rand_cells(shape, 9, 10)])  # frame 0 holds nothing
    assert pt.offsets.tolist() == [0, 0, 9]
    x = rand_x((2, 2, 27, 48), 11)
    ls, t, _, _, _ = check_points(x, pt, ik)
    assert torch.count_nonzero(t[0]).item() == 0 and torch.count_nonzero(t[1]).item() > 0


def test_more_cells_than_lanes():
    """600 cells in one (item, b): the 256 lanes walk the list in strides."""
    mk, _ = kernels()
    shape = (1, 1, 24, 72)
    cells = rand_cells(shape, 600, 12)
    vals = np.random.default_rng(13).integers(1, 4, size=600).astype(np.float32)
    pt = from_cells(shape, cells, list(vals))
    assert len(pt) == 600
    check_points(rand_x(shape, 14), pt, mk)


def test_general_kernel_and_k1():
    gen = torch.Generator().manual_seed(15)
    dense_k = torch.randn(2, 2, 3, 3, generator=gen)
    t = torch.from_numpy(np.random.default_rng(16).uniform(0, 1, size=(2, 2, 9, 11)).astype(np.float32))
    t[t < 0.3] = 0
    check_points(rand_x((2, 2, 9, 11), 17), PointTargets.from_dense(t), dense_k)
    pt = from_cells((1, 1, 12, 140), rand_cells((1, 1, 12, 140), 20, 19))
    check_points(rand_x((1, 1, 6, 70), 18), pt, torch.full((1, 1, 1, 1), 0.75))


def test_kernel_with_a_nan_tap():
    _, ik = kernels()
    bad = ik.clone()
    bad[0, 1, 4, 6] = float("nan")  # in a slice that is otherwise all zero
    x = rand_x((1, 2, 40, 150), 28)
    pt = from_cells((1, 2, 40, 150), [(0, 0, 5, 5), (0, 1, 30, 140)])
    _, got, _, _, _ = check_points(x, pt, bad, finite=False)
    got = got.cpu()
    ref = loss_ref.target_transform(x, pt.dense(), bad)
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    nan = torch.isnan(ref)
    assert nan[0, 0].sum().item() == (40 - 6) * (150 - 4) and not nan[0, 1].any()
    close(got[~nan], ref[~nan], "the finite outputs")


def test_non_contiguous_x():
    _, ik = kernels()
    big = rand_x((2, 5, 27, 50), 24)
    x = big[:, 1:4:2, :, 1:49]
    assert not x.is_contiguous() and x.shape == (2, 2, 27, 48)
    bd = big.to(DEV)
    pt = from_cells((2, 2, 108, 192), rand_cells((2, 2, 108, 192), 14, 25))
    check_points(x.contiguous(), pt, ik, x_dev=bd[:, 1:4:2, :, 1:49])


def test_from_dense_on_the_gpu():
    _, ik = kernels()
    pt = from_cells((2, 2, 108, 192), rand_cells((2, 2, 108, 192), 14, 26))
    pd = PointTargets.from_dense(pt.dense().to(DEV))
    assert pd.device.type == "cuda" and len(pd) == 14
    for a, b in zip((pd.offsets, pd.cells, pd.values), (pt.offsets, pt.cells, pt.values)):
        assert torch.equal(a.cpu(), b)
    xd = rand_x((2, 2, 27, 48), 27).to(DEV)
    for a, b in zip(run_single(xd, pd, ik)[:4], run_single(xd, pt.to(DEV), ik)[:4]):
        assert torch.equal(a, b)


def make_step(B, seed, n_pts=8):
    """map [B,1,24,72] with a cell of value 2 that is predicted, 3 views [B,2,27,48] from 108 x 192."""
    ms, vs = (B, 1, 24, 72), (B, 2, 108, 192)
    map_res = rand_x(ms, seed + 1)
    cells = rand_cells(ms, n_pts * B, seed)
    for b, c, y, x in cells[::2]:
        map_res[b, c, y, x] = 0.9
    map_pt = from_cells(ms, cells + [cells[0]])  # two people in cells[0]: value 2, and predicted
    imgs_res = [rand_x((B, 2, 27, 48), seed + 10 + v) for v in range(3)]
    imgs_pt = [from_cells(vs, rand_cells(vs, n_pts * B, seed + 20 + v)) for v in range(3)]
    return map_res, imgs_res, map_pt, imgs_pt


def run_step(map_res, imgs_res, map_gt, imgs_gt, alpha, thres):
    mk, ik = kernels()
    xm = map_res.to(DEV).requires_grad_()
    xv = [v.to(DEV).requires_grad_() for v in imgs_res]
    ls, stats = loss.detection_loss(xm, xv, map_gt, imgs_gt, mk, ik, alpha=alpha, cls_thres=thres)
    launch = ls.grad_fn.launch
    ls.backward()
    return ls.detach(), stats, [x.grad for x in [xm] + xv], launch


@pytest.mark.parametrize("B", [1, 2])
def test_detection_loss_end_to_end(B):
    map_res, imgs_res, map_pt, imgs_pt = make_step(B, 40 + B)
    map_d, imgs_d = map_pt.dense(), [t.dense() for t in imgs_pt]
    assert (map_d == 2).sum() == 1
    mk, ik = kernels()
    l_ref, g_ref, counts = loss_ref.step(map_res, imgs_res, map_d, imgs_d, mk, ik, 0.7, 0.4)
    dense = run_step(map_res, imgs_res, map_d.to(DEV), [t.to(DEV) for t in imgs_d], 0.7, 0.4)
    assert dense[3].n_pooled == 3 and dense[3].launches == ["pool", "mse", "finalize"]

    pm, pvs = pack_step(map_pt, imgs_pt)
    dm = pm.to(DEV, non_blocking=True)
    dvs = [t.to(DEV, non_blocking=True) for t in pvs]
    assert all(t.buffer is dm.buffer for t in dvs) and dm.buffer.is_cuda  # one device buffer, one copy
    assert dm.buffer.numel() == pm.buffer.numel() and dm.buffer.numel() * 4 < 4096
    packed = run_step(map_res, imgs_res, dm, dvs, 0.7, 0.4)
    assert packed[3].n_pooled == 0 and packed[3].launches == ["mse", "finalize"]
    apart = run_step(map_res, imgs_res, map_pt.to(DEV), [t.to(DEV) for t in imgs_pt], 0.7, 0.4)  # own uploads
    mixed = run_step(map_res, imgs_res, map_d.to(DEV), dvs, 0.7, 0.4)  # the map dense, the views as points
    assert mixed[3].n_pooled == 0 and mixed[3].launches == ["mse", "finalize"]
    views_dense = run_step(map_res, imgs_res, dm, [t.to(DEV) for t in imgs_d], 0.7, 0.4)
    assert views_dense[3].n_pooled == 3 and views_dense[3].launches == ["pool", "mse", "finalize"]
    for got in (packed, apart, mixed, views_dense):
        assert torch.equal(got[0], dense[0]) and torch.equal(got[1], dense[1])
        for a, b in zip(got[2], dense[2]):
            assert torch.equal(a, b)
    ls, stats, grads, _ = packed
    rel = abs(ls.item() - float(l_ref)) / abs(float(l_ref))
    print(f"loss: native {ls.item():.9g} ref {float(l_ref):.9g} rel {rel:.3e}; stats {stats.tolist()} ref {counts}")
    assert rel <= TOL
    for i, (got, g) in enumerate(zip(grads, g_ref)):
        close(got, g, f"grad {i}")
    assert tuple(stats.tolist()) == tuple(float(c) for c in counts)
    # the cell of value 2 is predicted: it counts in fn's gt_sum and not in tp (gt == 1 is false there)
    two = map_d == 2
    assert (map_res[two] > 0.4).all()
    tp = ((map_res > 0.4) & (map_d == 1)).sum().item()
    assert stats[0].item() == tp and stats[2].item() == (8 * B + 1) - tp


def test_two_calls_are_bitwise_equal():
    args = make_step(2, 50)
    pm, pvs = pack_step(args[2], args[3])
    dm, dvs = pm.to(DEV), [t.to(DEV) for t in pvs]
    a = run_step(args[0], args[1], dm, dvs, 1.0, 0.4)
    b = run_step(args[0], args[1], dm, dvs, 1.0, 0.4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)


def test_no_pooling_launch_and_no_scratch_for_point_items():
    _, ik = kernels()
    x = rand_x((2, 2, 27, 48), 30).to(DEV)
    pt = from_cells((2, 2, 108, 192), rand_cells((2, 2, 108, 192), 14, 31)).to(DEV)
    launch = loss._Launch([x], [pt], [ik], [1.0])
    assert launch.n_pooled == 0 and launch.pool_items is None and launch.points is not None
    launch.forward()
    assert launch.launches == ["mse", "finalize"]
    dense = loss._Launch([x], [pt.dense()], [ik], [1.0])
    assert dense.n_pooled == 1 and dense.points is None
    dense.forward()
    assert dense.launches == ["pool", "mse", "finalize"]
    # a device mismatch is refused as for a dense target
    with pytest.raises(ValueError):
        loss.GaussianMSE()(x, pt.to("cpu"), ik)
