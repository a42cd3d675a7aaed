"""CPU tests of the training criterion's host side (``mvdet_amd.loss``, the loss entry points of
``include/mvbev.h``): the CPU restatement the GPU tests compare against reproduces the reference's
golden outputs, the closed-form kernels equal scipy's, the pooling windows equal torch's, the
kernel plan, the C ABI's refusals before any launch, and the Python argument errors."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref
from mvdet_amd import _native, loss

SINGLES = ["halo", "pool4", "uneven", "grow", "general", "k1", "dense", "wide_sigma"]
STEPS = ["step_b1", "step_b2", "step_wt"]


def test_golden_lists_the_cases():
    g = loss_ref.golden()
    assert list(g["singles"]) == SINGLES and list(g["steps"]) == STEPS
    assert loss_ref.GOLDEN.stat().st_size < (1 << 20)


@pytest.mark.parametrize("name", SINGLES)
def test_restatement_reproduces_golden_single(name):
    c = loss_ref.golden_single(name)
    t, diff, ls, grad = loss_ref.single(c["x"], c["target"], c["kernel"])
    assert loss_ref.normwise(t, c["t"]) <= 1e-6
    assert loss_ref.normwise(grad, c["grad"]) <= 1e-6
    assert abs(ls.item() - c["loss"]) <= 1e-6 * abs(c["loss"])


@pytest.mark.parametrize("name", STEPS)
def test_restatement_reproduces_golden_step(name):
    c = loss_ref.golden_step(name)
    ls, grads, counts = loss_ref.step(c["xs"][0], c["xs"][1:], c["targets"][0], c["targets"][1:], c["map_kernel"],
                                      c["img_kernel"], c["alpha"], c["thres"])
    assert abs(ls.item() - c["loss"]) <= 1e-6 * abs(c["loss"])
    for got, ref in zip(grads, c["grads"]):
        assert loss_ref.normwise(got, ref) <= 1e-6
    assert tuple(float(v) for v in counts) == c["counts"]
    assert c["counts"][0] > 0 and c["counts"][1] > 0 and c["counts"][2] > 0
    assert (c["targets"][0] == 2).any()


def test_gaussian_kernels_equal_the_golden_kernels():
    g = loss_ref.golden()
    mk4, ik4 = loss.gaussian_kernels(4, 4)
    mk1, _ = loss.gaussian_kernels(1, 4)
    assert mk4.shape == (1, 1, 41, 41) and ik4.shape == (2, 2, 21, 21) and mk4.dtype == torch.float32
    for got, name in ((mk4, "map_kernel_4"), (ik4, "img_kernel_4"), (mk1, "map_kernel_1")):
        assert np.abs(got.numpy().astype(np.float64) - g[name].astype(np.float64)).max() <= 1e-7, name
    assert not ik4[0, 1].any() and not ik4[1, 0].any()


@pytest.mark.parametrize("n_in,n_out", [(50, 12), (77, 36), (1080, 270), (5, 5), (3, 7)])
def test_pool_windows_equal_torch(n_in, n_out):
    rng = np.random.default_rng(n_in * 1000 + n_out)
    src = rng.standard_normal((n_in, n_in + 3)).astype(np.float32)
    rs, re_ = loss.pool_windows(n_in, n_out)
    cs, ce = loss.pool_windows(n_in + 3, n_out + 1)
    got = np.array([[src[rs[i]:re_[i], cs[j]:ce[j]].max() for j in range(n_out + 1)] for i in range(n_out)])
    ref = F.adaptive_max_pool2d(torch.from_numpy(src)[None, None], (n_out, n_out + 1))[0, 0].numpy()
    assert np.array_equal(got, ref)


def test_kernel_plan():
    _, ik = loss.gaussian_kernels()
    assert loss.plan_slices(ik) == ([(0, 0), (1, 1)], True)
    off = ik.clone()
    off[0, 1, 3, 4] = 0.5
    assert loss.plan_slices(off) == ([(0, 0), (0, 1), (1, 1)], True)
    bad = ik.clone()
    bad[1, 1, 0, 0] = float("nan")
    assert loss.plan_slices(bad) == ([(0, 0), (0, 1), (1, 0), (1, 1)], False)
    inf = ik.clone()
    inf[0, 0, 2, 2] = float("inf")
    assert loss.plan_slices(inf)[1] is False
    plan = loss.KernelPlan(off, "cpu")
    assert plan.mask == 0b1011 and plan.C == 2 and plan.k == 21 and plan.finite


def test_kernel_cache_never_serves_a_freed_kernels_plan():
    """Transient kernels of one shape: a freed host tensor's address may go to the next one, whose
    ``_version`` is 0 again.  Every cached plan keeps its kernel alive, so the key ``(data_ptr,
    _version, ...)`` cannot come to name another tensor.  fp64 kernels: the plan's fp32 copy does not
    alias them, as a device copy does not alias a host kernel."""
    cache = loss._PlanCache()
    for i in range(40):
        k = torch.full((1, 1, 1, 1), float(i + 1), dtype=torch.float64)
        plan = cache.get(k, "cpu")
        assert plan.dev.item() == float(i + 1), i
        assert plan.source is k
        del k, plan
    for i in range(12):
        k = loss.gaussian_kernels(4 + i, 4)[0].double()
        plan = cache.get(k, "cpu")
        assert torch.equal(plan.dev, k.float()), i
        del k, plan
    assert cache.uploads == 52 and len(cache.plans) <= cache.capacity
    k = torch.full((1, 1, 1, 1), 3.0)
    assert cache.get(k, "cpu") is cache.get(k, "cpu") and cache.uploads == 53  # unchanged: one plan
    k.mul_(2.0)
    assert cache.get(k, "cpu").dev.item() == 6.0 and cache.uploads == 54       # changed in place: a new one


def _item(fake, C=1, h=8, w=8, Ht=8, Wt=8, kernel_id=0):
    s = _native._i64x4(C * h * w, h * w, w, 1)
    st = _native._i64x4(C * Ht * Wt, Ht * Wt, Wt, 1)
    return _native.LossItem(fake, s, fake, st, C, h, w, Ht, Wt, fake, fake, fake, kernel_id, 1.0)


def test_c_abi_refuses_before_any_launch():
    lib = _native.load()
    fake = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    items = (_native.LossItem * 1)(_item(fake))
    kern = lambda k, C=1: (_native.LossKernel * 1)(_native.LossKernel(fake, C, k, 1, 1))  # noqa: E731
    mse = lambda it, n, kn, stats=-1, np_=1 << 20: lib.mvbev_gaussian_mse_f32(  # noqa: E731
        it, n, 1, kn, 1, 0.4, stats, fake, np_, None)
    assert mse(items, 1, kern(4)) == -2          # even k
    assert mse(items, 1, kern(40)) == -2
    assert mse(items, 0, kern(3)) == -1          # n <= 0
    assert mse(items, -1, kern(3)) == -1
    assert mse(None, 1, kern(3)) == -5           # null item array
    assert mse(items, 1, None) == -5
    assert mse(items, 1, kern(3, C=2)) == -2     # kernel channels != item channels
    assert mse(items, 1, kern(129)) == -2        # the tile does not fit the LDS
    assert mse(items, 1, kern(3), np_=3) == -2   # partials too small
    assert mse(items, 1, kern(3), stats=1) == -2
    assert mse(items, 17, kern(3)) == -2         # more than 16 items
    neg = _item(fake)
    neg.x_strides[2] = -8
    assert mse((_native.LossItem * 1)(neg), 1, kern(3)) == -3
    assert mse((_native.LossItem * 1)(_item(fake, h=0)), 1, kern(3)) == -1
    assert mse((_native.LossItem * 1)(_item(fake, C=9)), 1, kern(3, C=9)) == -2
    pooled = (_native.LossItem * 1)(_item(fake, Ht=16, Wt=16))
    assert mse(pooled, 1, kern(3), stats=0) == -2  # the stats item's target must have x's size
    assert lib.mvbev_adaptive_max_pool_f32(None, 1, 1, None) == -5
    assert lib.mvbev_adaptive_max_pool_f32(items, 0, 1, None) == -1
    assert lib.mvbev_adaptive_max_pool_f32(items, 1, 0, None) == -1
    assert lib.mvbev_adaptive_max_pool_f32(items, 1, 1, None) == 0  # equal sizes: nothing to launch
    nopool = _item(fake, Ht=16, Wt=16)
    nopool.pooled = None
    assert lib.mvbev_adaptive_max_pool_f32((_native.LossItem * 1)(nopool), 1, 1, None) == -5
    assert lib.mvbev_gaussian_mse_blocks(items, 1, 3) == 3
    assert lib.mvbev_gaussian_mse_blocks((_native.LossItem * 1)(_item(fake, h=17, w=65)), 1, 2) == 8
    assert lib.mvbev_gaussian_mse_blocks(None, 1, 1) == 0
    assert lib.mvbev_loss_finalize_f32(None, 1, 1, fake, 4, -1, fake, None, None) == -5
    assert lib.mvbev_loss_finalize_f32(items, 0, 1, fake, 4, -1, fake, None, None) == -1
    assert lib.mvbev_loss_finalize_f32(items, 1, 1, fake, 3, -1, fake, None, None) == -2
    assert lib.mvbev_loss_finalize_f32(items, 1, 1, fake, 4, -1, None, None, None) == -5
    ptrs = (ctypes.c_void_p * 1)(16)
    assert lib.mvbev_gaussian_mse_backward_f32(None, 1, 1, fake, ptrs, None) == -5
    assert lib.mvbev_gaussian_mse_backward_f32(items, 0, 1, fake, ptrs, None) == -1
    assert lib.mvbev_gaussian_mse_backward_f32(items, 1, 1, None, ptrs, None) == -5
    nodiff = _item(fake)
    nodiff.diff = None
    assert lib.mvbev_gaussian_mse_backward_f32((_native.LossItem * 1)(nodiff), 1, 1, fake, ptrs, None) == -5


def test_python_argument_errors():
    crit = loss.GaussianMSE()
    mk, ik = loss.gaussian_kernels()
    x, t = torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 16, 16)
    bad = [
        (torch.zeros(1, 8, 8), t, mk),                       # x not 4-D
        (x, torch.zeros(16, 16), mk),                        # target not 4-D
        (x, torch.zeros(2, 1, 16, 16), mk),                  # batch mismatch
        (x, torch.zeros(1, 2, 16, 16), mk),                  # channel mismatch
        (x, t, ik),                                          # kernel channels != x's
        (x, t, torch.zeros(1, 1, 4, 4)),                     # even k
        (x, t, torch.zeros(1, 1, 3, 5)),                     # not square
        (x, t, torch.zeros(1, 2, 3, 3)),                     # not [C,C,k,k]
        (x, t, torch.zeros(3, 3)),                           # not 4-D
        (x.double(), t, mk),                                 # dtype
        (x.half(), t, mk),
        (x, t.double(), mk),
        (x, t, torch.zeros(1, 1, 3, 3, dtype=torch.int32)),
        (x, torch.zeros(1, 1, 16, 16, device="meta"), mk),   # target on another device than x
        ("x", t, mk),
    ]
    for args in bad:
        with pytest.raises((ValueError, TypeError)):
            crit(*args)
        with pytest.raises((ValueError, TypeError)):
            crit._traget_transform(*args)
    with pytest.raises((ValueError, TypeError)):
        loss.detection_loss(x, [torch.zeros(1, 2, 8, 8)], x, [], mk, ik)
    with pytest.raises((ValueError, TypeError)):
        loss.detection_loss(x, [torch.zeros(1, 2, 8, 8)], x, [torch.zeros(1, 1, 32, 32)], mk, ik)
    # valid arguments on the host: there is no CPU fallback
    with pytest.raises(RuntimeError):
        crit(x, t, mk)
    with pytest.raises(ValueError):  # trainer.py:51-54 compares map_res and map_gt cell by cell
        loss.detection_loss(x, [], t, [], mk, ik)


def test_public_surface():
    import mvdet_amd
    assert mvdet_amd.GaussianMSE is loss.GaussianMSE and mvdet_amd.detection_loss is loss.detection_loss
    assert mvdet_amd.gaussian_kernels is loss.gaussian_kernels
    assert hasattr(loss.GaussianMSE, "_traget_transform")
    for name in ("mvbev_adaptive_max_pool_f32", "mvbev_gaussian_mse_f32", "mvbev_loss_finalize_f32",
                 "mvbev_gaussian_mse_backward_f32"):
        assert name in _native.EXPORTS
    assert _native.load().mvbev_version() == 12500
