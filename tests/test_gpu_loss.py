"""GPU tests of the native criterion (``mvdet_amd.loss`` on ``mvdet_amd/csrc/loss.hip``) against the
fp32 CPU restatement of the reference (``tests/loss_ref.py``) and the reference's own golden outputs.

Gates: the transformed target, ``x - t`` and the x-gradient normwise ``max|d| / max|ref| <= 5e-6``,
the loss relative ``5e-6`` — both sides are fp32 sums of at most 1681 Ci taps that differ only in
summation order (a sequential fp32 tap loop and torch's CPU conv were measured <= 2e-7 apart on dense
41 x 41 inputs, either within 1.7e-6 of fp64 for a flat kernel on a dense target) — and the counts
exactly: both sides threshold the same fp32 ``x``."""
import math

import numpy as np
import pytest
import torch

import loss_ref
from mvdet_amd import loss

pytestmark = pytest.mark.gpu

TOL = 5e-6
DEV = "cuda:0"
TH, TW = loss.TILE_H, loss.TILE_W
SINGLES = ["halo", "pool4", "uneven", "grow", "general", "k1", "dense", "wide_sigma"]
STEPS = ["step_b1", "step_b2", "step_wt"]

_kernels = {}


def kernels():
    if not _kernels:
        _kernels["map"], _kernels["img"] = loss.gaussian_kernels(4, 4)
    return _kernels["map"], _kernels["img"]


def rand_x(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-0.2, 1.0, size=shape).astype(np.float32))


def rand_points(shape, n, seed):
    rng = np.random.default_rng(seed)
    flat = rng.choice(int(np.prod(shape)), size=n, replace=False)
    pts = np.stack(np.unravel_index(flat, shape), axis=1)
    return loss_ref.dense(shape, pts, np.ones(n, np.float32))


def close(got, ref, what):
    nw = loss_ref.normwise(got, ref)
    print(f"{what}: normwise {nw:.3e}")
    assert nw <= TOL, (what, nw)


def check_single(x, target, kernel, upstream=1.0, x_dev=None, ref=None):
    """One criterion call on the GPU against the restatement (or a golden dict): t_out, the kernel's own
    diff buffer, loss, x-gradient.  Returns the native (t, loss, grad)."""
    crit = loss.GaussianMSE()
    t_ref, d_ref, l_ref, g_ref = loss_ref.single(x, target, kernel, upstream) if ref is None else ref
    xd = (x.to(DEV) if x_dev is None else x_dev).detach().requires_grad_()
    td = target.to(DEV)
    ls = crit(xd, td, kernel)
    assert ls.dim() == 0 and ls.dtype == torch.float32 and ls.grad_fn is not None
    diff = ls.grad_fn.launch.diff[0]  # the buffer the conv + MSE kernel wrote for the backward
    assert diff.shape == x.shape
    (upstream * ls).backward()
    t = crit._traget_transform(xd, td, kernel)
    assert t.shape == x.shape and not t.requires_grad
    close(t, t_ref, "t_out")
    close(diff, d_ref, "diff")
    close(xd.grad, g_ref, "grad_x")
    rel = abs(ls.item() - float(l_ref)) / abs(float(l_ref))
    print(f"loss: native {ls.item():.9g} ref {float(l_ref):.9g} rel {rel:.3e}")
    assert rel <= TOL
    return t, ls, xd.grad


def test_image_smaller_than_the_halo():
    mk, _ = kernels()
    check_single(rand_x((1, 1, 23, 37), 1), rand_points((1, 1, 23, 37), 5, 2), mk)


def test_factor4_pool_block_diagonal_kernel():
    _, ik = kernels()
    check_single(rand_x((2, 2, 27, 48), 3), rand_points((2, 2, 108, 192), 14, 4), ik)


def test_uneven_overlapping_windows():
    _, ik = kernels()
    check_single(rand_x((2, 2, 12, 36), 5), rand_points((2, 2, 50, 77), 30, 6), ik)


def test_target_smaller_than_x():
    mk, _ = kernels()
    check_single(rand_x((1, 1, 7, 9), 7), rand_points((1, 1, 3, 5), 3, 8), mk)


def test_pool_chunks_and_the_direct_window_walk():
    """More than one 256-output chunk per row (w = 300 from 700), and a source span past the 1024
    columns of the staged column maxima (2100 -> 2: the windows are walked directly)."""
    k3 = torch.zeros(1, 1, 3, 3)
    k3[0, 0, 1, 1] = 1.0
    k3[0, 0, 0, 2] = 0.25
    t = torch.from_numpy(np.random.default_rng(9).standard_normal((1, 1, 9, 700)).astype(np.float32))
    check_single(rand_x((1, 1, 4, 300), 10), t, k3)
    t = torch.from_numpy(np.random.default_rng(11).standard_normal((1, 1, 6, 2100)).astype(np.float32))
    check_single(rand_x((1, 1, 2, 2), 12), t, k3)


def test_pool_nan_wins_a_window():
    k1 = torch.ones(1, 1, 1, 1)
    t = torch.from_numpy(np.random.default_rng(13).standard_normal((1, 1, 8, 12)).astype(np.float32))
    t[0, 0, 5, 7] = float("nan")
    x = rand_x((1, 1, 4, 4), 14)
    got = loss.GaussianMSE()._traget_transform(x.to(DEV), t.to(DEV), k1).cpu()
    ref = loss_ref.target_transform(x, t, k1)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.isnan(got).sum() == 1
    assert torch.equal(got[~torch.isnan(got)], ref[~torch.isnan(ref)])


def test_general_kernel_and_k1():
    gen = torch.Generator().manual_seed(15)
    dense_k = torch.randn(2, 2, 3, 3, generator=gen)
    assert loss.plan_slices(dense_k)[0] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    t = torch.from_numpy(np.random.default_rng(16).uniform(0, 1, size=(2, 2, 9, 11)).astype(np.float32))
    check_single(rand_x((2, 2, 9, 11), 17), t, dense_k)
    check_single(rand_x((1, 1, 6, 70), 18), rand_points((1, 1, 12, 140), 20, 19), torch.full((1, 1, 1, 1), 0.75))


def test_all_zero_target_skips_every_tile():
    mk, _ = kernels()
    x = rand_x((1, 1, 40, 150), 20)
    xd = x.to(DEV).requires_grad_()
    crit = loss.GaussianMSE()
    z = torch.zeros(1, 1, 40, 150, device=DEV)
    t = crit._traget_transform(xd, z, mk)
    assert torch.count_nonzero(t).item() == 0  # exactly 0
    ls = crit(xd, z, mk)
    ls.backward()
    ref = (x.double() ** 2).mean().item()
    assert abs(ls.item() - ref) <= TOL * ref
    close(xd.grad, 2 * x / x.numel(), "grad_x")


@pytest.mark.parametrize("cells", [
    [(0, 0, 0, 0)], [(0, 0, 39, 149)],                        # the image's corners
    [(0, 0, TH, TW)], [(0, 0, TH - 1, TW - 1)],               # a tile corner: the stamp spans four tiles
    [(0, 0, 0, 0), (0, 0, 39, 149), (0, 0, TH, 2 * TW)],
], ids=["first", "last", "tile_corner", "tile_corner_m1", "mixed"])
def test_single_points_and_tile_corners(cells):
    """h = 40 and w = 150 are no multiples of the 16 x 64 tile: 3 x 3 tiles, the last ones partial."""
    mk, _ = kernels()
    check_single(rand_x((1, 1, 40, 150), 21), loss_ref.points((1, 1, 40, 150), cells), mk)


def test_dense_random_target():
    mk, _ = kernels()
    t = torch.from_numpy(np.random.default_rng(22).uniform(0, 1, size=(1, 1, 40, 70)).astype(np.float32))
    check_single(rand_x((1, 1, 40, 70), 23), t, mk)


def test_largest_tile_that_fits_the_lds():
    """k = 89 at C = 1 is the largest kernel whose staged tile (104 rows x 153 floats, 63.6 kB of dynamic
    LDS beside the static 104 B) is admitted; k = 91 is refused.  A few points under a wide Gaussian: each
    output sums at most 6 non-zero products, so the 5e-6 gate holds as for the small kernels."""
    r = torch.arange(-44, 45, dtype=torch.float64)
    k89 = torch.exp(-(r[:, None] ** 2 + r[None, :] ** 2) / (2 * 150.0)).float()[None, None]
    target = loss_ref.points((1, 1, 20, 70), [(0, 0, 0, 0), (0, 0, 19, 69), (0, 0, 9, 30), (0, 0, 16, 64),
                                              (0, 0, 3, 66), (0, 0, 15, 2)])
    check_single(rand_x((1, 1, 20, 70), 33), target, k89)
    from mvdet_amd import _native
    with pytest.raises(_native.NativeError):
        k91 = torch.ones(1, 1, 91, 91)
        loss.GaussianMSE()(rand_x((1, 1, 20, 70), 33).to(DEV), target.to(DEV), k91)


def test_non_contiguous_x():
    _, ik = kernels()
    big = rand_x((2, 5, 27, 50), 24)
    x = big[:, 1:4:2, :, 1:49]
    assert not x.is_contiguous() and x.shape == (2, 2, 27, 48)
    bd = big.to(DEV)
    check_single(x.contiguous(), rand_points((2, 2, 108, 192), 14, 25), ik, x_dev=bd[:, 1:4:2, :, 1:49])


def test_non_contiguous_target():
    """Column-sliced targets: rows that start off a 16-byte boundary, and a column stride of 2."""
    _, ik = kernels()
    big = rand_points((2, 2, 108, 390), 60, 31)
    x = rand_x((2, 2, 27, 48), 32)
    bd = big.to(DEV)
    crit = loss.GaussianMSE()
    for sl in (slice(1, 193), slice(4, 388, 2)):
        t = big[..., sl]
        assert t.shape == (2, 2, 108, 192) and not t.is_contiguous()
        t_ref, _, l_ref, _ = loss_ref.single(x, t, ik)
        close(crit._traget_transform(x.to(DEV), bd[..., sl], ik), t_ref, "t_out")
        assert abs(crit(x.to(DEV), bd[..., sl], ik).item() - l_ref.item()) <= TOL * l_ref.item()


def test_nan_in_x_at_one_pixel():
    mk, _ = kernels()
    x = rand_x((1, 1, 30, 90), 26)
    x[0, 0, 17, 65] = float("nan")
    gt = rand_points((1, 1, 30, 90), 8, 27)
    xd = x.to(DEV).requires_grad_()
    ls, stats = loss.detection_loss(xd, [], gt.to(DEV), [], mk, kernels()[1], cls_thres=0.4)
    ls.backward()
    assert math.isnan(ls.item())
    nan = torch.isnan(xd.grad.cpu())
    assert nan.sum().item() == 1 and nan[0, 0, 17, 65]
    clean = torch.nan_to_num(x, nan=0.0)
    _, _, _, g_ref = loss_ref.single(clean, gt, mk)
    close(torch.nan_to_num(xd.grad.cpu(), nan=0.0)[~nan], g_ref[~nan], "grad_x off the NaN")
    pred = (x > 0.4).int()
    tp = (pred.eq(gt) * pred.eq(1)).sum().item()
    assert stats.tolist() == [tp, pred.sum().item() - tp, gt.sum().item() - tp]  # the NaN is not in pred


def test_kernel_with_a_nan_tap():
    _, ik = kernels()
    bad = ik.clone()
    bad[0, 1, 4, 6] = float("nan")  # in a slice that is otherwise all zero
    assert loss.plan_slices(bad) == ([(0, 0), (0, 1), (1, 0), (1, 1)], False)
    x = rand_x((1, 2, 40, 150), 28)
    target = loss_ref.points((1, 2, 40, 150), [(0, 0, 5, 5), (0, 1, 30, 140)])
    got = loss.GaussianMSE()._traget_transform(x.to(DEV), target.to(DEV), bad).cpu()
    ref = loss_ref.target_transform(x, target, bad)
    # 0 * NaN wherever the tap reads a cell of the image (torch never multiplies the padding)
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    nan = torch.isnan(ref)
    assert nan[0, 0].sum().item() == (40 - 6) * (150 - 4) and not nan[0, 1].any()
    close(got[~nan], ref[~nan], "the finite outputs")


def test_upstream_gradient():
    mk, _ = kernels()
    check_single(rand_x((1, 1, 23, 37), 29), rand_points((1, 1, 23, 37), 5, 30), mk, upstream=3.0)


def make_step(B, n_views, map_shape, view_shape, view_t_shape, seed, n_pts=8):
    rng = np.random.default_rng(seed)
    ms = (B, 1) + map_shape
    map_res = rand_x(ms, seed + 1)
    flat = rng.choice(int(np.prod(ms)), size=n_pts * B, replace=False)
    pts = np.stack(np.unravel_index(flat, ms), axis=1)
    vals = np.ones(len(pts), np.float32)
    vals[3] = 2.0  # a cell holding two people
    map_gt = loss_ref.dense(ms, pts, vals)
    for b, c, y, x in pts[::2]:
        map_res[b, c, y, x] = 0.9
    imgs_res = [rand_x((B, 2) + view_shape, seed + 10 + v) for v in range(n_views)]
    imgs_gt = [rand_points((B, 2) + view_t_shape, n_pts * B, seed + 20 + v) for v in range(n_views)]
    return map_res, imgs_res, map_gt, imgs_gt


def run_step(map_res, imgs_res, map_gt, imgs_gt, alpha, thres, mk, ik):
    xm = map_res.to(DEV).requires_grad_()
    xv = [v.to(DEV).requires_grad_() for v in imgs_res]
    ls, stats = loss.detection_loss(xm, xv, map_gt.to(DEV), [t.to(DEV) for t in imgs_gt], mk, ik, alpha=alpha,
                                    cls_thres=thres)
    assert ls.dim() == 0 and ls.dtype == torch.float32 and ls.grad_fn is not None
    assert stats.shape == (3,) and stats.is_cuda and not stats.requires_grad
    ls.backward()
    return ls.detach(), stats, [x.grad for x in [xm] + xv]


def check_step(map_res, imgs_res, map_gt, imgs_gt, alpha, thres, ref=None, mk=None, ik=None):
    mk, ik = (mk, ik) if mk is not None else kernels()
    if ref is None:
        ref = loss_ref.step(map_res, imgs_res, map_gt, imgs_gt, mk, ik, alpha, thres)
    l_ref, g_ref, counts = ref
    ls, stats, grads = run_step(map_res, imgs_res, map_gt, imgs_gt, alpha, thres, mk, ik)
    rel = abs(ls.item() - float(l_ref)) / abs(float(l_ref))
    print(f"loss: native {ls.item():.9g} ref {float(l_ref):.9g} rel {rel:.3e}; stats {stats.tolist()} ref {counts}")
    assert rel <= TOL
    for i, (got, g) in enumerate(zip(grads, g_ref)):
        close(got, g, f"grad {i}")
    assert tuple(stats.tolist()) == tuple(float(c) for c in counts)
    return ls, stats, grads


@pytest.mark.parametrize("B", [1, 2])
def test_detection_loss_end_to_end(B):
    args = make_step(B, 3, (30, 90), (27, 48), (108, 192), 40 + B)
    _, stats, _ = check_step(*args, alpha=0.7, thres=0.4)
    assert (args[2] == 2).any() and stats[0].item() > 0 and stats[2].item() > 0


def test_wildtrack_size_step_and_repeatability():
    """cfg2's map and two full-size views (1080 x 1920 ground truth), 40 points each; a second call on
    the same inputs gives bitwise the same loss, stats and gradients."""
    args = make_step(1, 2, (120, 360), (270, 480), (1080, 1920), 50, n_pts=40)
    ls, stats, grads = check_step(*args, alpha=1.0, thres=0.4)
    ls2, stats2, grads2 = run_step(*args, 1.0, 0.4, *kernels())
    assert torch.equal(ls, ls2) and torch.equal(stats, stats2)
    for a, b in zip(grads, grads2):
        assert torch.equal(a, b)


def test_repeatability_dense():
    mk, _ = kernels()
    t = torch.from_numpy(np.random.default_rng(60).uniform(0, 1, size=(2, 1, 40, 150)).astype(np.float32)).to(DEV)
    x = rand_x((2, 1, 40, 150), 61).to(DEV)
    outs = []
    for _ in range(2):
        xd = x.clone().requires_grad_()
        ls, stats = loss.detection_loss(xd, [], t, [], mk, kernels()[1])
        ls.backward()
        outs.append((ls.detach(), stats, xd.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_kernel_cache():
    mk = loss.gaussian_kernels(4, 4)[0].clone()  # a host kernel of this test's own
    x, gt = rand_x((1, 1, 23, 37), 62), rand_points((1, 1, 23, 37), 5, 63)
    crit = loss.GaussianMSE()
    xd, td = x.to(DEV), gt.to(DEV)
    n0 = loss.kernel_cache.uploads
    first = crit(xd, td, mk).item()
    assert loss.kernel_cache.uploads == n0 + 1
    assert crit(xd, td, mk).item() == first
    crit._traget_transform(xd, td, mk)
    assert loss.kernel_cache.uploads == n0 + 1  # unchanged: not uploaded again
    v = mk._version
    mk.mul_(0.5)  # in place: _version bumps
    assert mk._version > v
    second = crit(xd, td, mk).item()
    assert loss.kernel_cache.uploads == n0 + 2
    ref = loss_ref.gaussian_mse(x, gt, mk).item()
    assert abs(second - ref) <= TOL * abs(ref) and second != first


@pytest.mark.parametrize("name", SINGLES)
def test_golden_single(name):
    c = loss_ref.golden_single(name)
    ref = (c["t"], c["x"] - c["t"], c["loss"], c["grad"])
    check_single(c["x"], c["target"], c["kernel"], ref=ref)


@pytest.mark.parametrize("name", STEPS)
def test_golden_step(name):
    c = loss_ref.golden_step(name)
    check_step(c["xs"][0], c["xs"][1:], c["targets"][0], c["targets"][1:], c["alpha"], c["thres"],
               ref=(c["loss"], c["grads"], c["counts"]), mk=c["map_kernel"], ik=c["img_kernel"])
