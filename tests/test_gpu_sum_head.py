"""``ProjectSumHead`` on the GPU (``mvbev_warp_sum_head_*``) against fp64 CPU autograd of the reference-order
restatement (``variant_ref.reference_order``: interpolate, warp, cat with the coord map, conv 1x1, ReLU, conv 1x1)
from the same fp32 values.  The op's inputs are the ``z_v``; the restatement takes them as the views' features
with a first conv of N identity blocks plus the coord columns (``variant_ref.head_weight``), which is the same
function.  Gate: ``helpers.assert_parity`` at 5e-5 normwise.  Gradients use ``masked_relu`` with the GPU's own
activation pattern (``return_hidden=True``) under ``test_gpu_backward.py``'s flip rule."""
import functools

import numpy as np
import pytest
import torch

import variant_ref as vr
from helpers import assert_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5


def _rand_h(rng, H, W, ho, wo):
    A = np.eye(3)
    A[0, 0] = wo / W * rng.uniform(0.6, 1.4)
    A[1, 1] = ho / H * rng.uniform(0.6, 1.4)
    A[0, 1], A[1, 0] = rng.uniform(-0.2, 0.2, 2)
    A[0, 2], A[1, 2] = rng.uniform(-3, 3, 2)
    A[2, 0], A[2, 1] = rng.uniform(-2e-3, 2e-3, 2)
    return A


class Case:
    def __init__(self, N, B, Cm, hw, up, grid, seed, Ms=None):
        rng = np.random.default_rng(seed)
        self.N, self.B, self.Cm, self.hw, self.up, self.grid = N, B, Cm, hw, up, grid
        self.Ms = Ms if Ms is not None else [_rand_h(rng, *up, *grid) for _ in range(N)]
        self.zs = [torch.from_numpy(rng.standard_normal((B, Cm, *hw)).astype(np.float32)) for _ in range(N)]
        self.bias = torch.from_numpy(rng.uniform(-0.5, 0.5, Cm).astype(np.float32))
        self.w_coord = torch.from_numpy(rng.uniform(-0.5, 0.5, (Cm, 2)).astype(np.float32))
        self.w2 = torch.from_numpy((rng.uniform(-1, 1, Cm) / np.sqrt(Cm)).astype(np.float32))
        self.dmap = torch.from_numpy(rng.standard_normal((B, 1, *grid)).astype(np.float32))

    def head(self):
        from mvdet_amd import ProjectSumHead
        return ProjectSumHead([torch.from_numpy(M) for M in self.Ms], self.up, self.grid)

    def gpu_inputs(self, layouts=None):
        """The z_v on the GPU: 'cl' channels-last, 'nchw' (the op makes it channels-last), 'slice' a
        non-contiguous slice with channel stride 1 of a larger channels-last tensor (unaligned base)."""
        out = []
        for i, z in enumerate(self.zs):
            kind = (layouts or ["cl"] * self.N)[i]
            if kind == "nchw":
                t = z.to(DEV)
            elif kind == "cl":
                t = z.to(DEV).contiguous(memory_format=torch.channels_last)
            else:
                B, Cm, h, w = z.shape
                big = torch.zeros((B, Cm + 3, h, w + 2), device=DEV).contiguous(memory_format=torch.channels_last)
                big[:, 1:1 + Cm, :, 1:-1] = z.to(DEV)
                t = big[:, 1:1 + Cm, :, 1:-1]
                assert t.stride(1) == 1 and not t.is_contiguous(memory_format=torch.channels_last)
            out.append(t.detach())
        return out

    def run(self, layouts=None, grad=("z", "bias", "w_coord", "w2"), z_grad=None, head=None):
        """One forward (+ backward when ``grad``) on the GPU: dict of CPU tensors."""
        head = head or self.head()
        zs = self.gpu_inputs(layouts)
        z_grad = z_grad if z_grad is not None else [("z" in grad)] * self.N
        zs = [z.requires_grad_() if gz else z for z, gz in zip(zs, z_grad)]
        p = dict(bias=self.bias.to(DEV), w_coord=self.w_coord.to(DEV), w2=self.w2.to(DEV))
        for k in p:
            if k in grad:
                p[k].requires_grad_()
        out, hidden = head(zs, p["bias"], p["w_coord"], p["w2"], return_hidden=True)
        res = dict(map=out.detach().cpu(), hidden=hidden.detach().cpu(), grad_fn=out.grad_fn)
        if out.grad_fn is not None:
            out.backward(self.dmap.to(DEV))
        torch.cuda.synchronize()
        res["gz"] = [None if z.grad is None else z.grad.cpu() for z in zs]
        res.update({"g" + k: (None if t.grad is None else t.grad.cpu()) for k, t in p.items()})
        return res

    def reference(self, pattern=None, backward=True):
        """fp64 CPU autograd of the reference order: dict(map, pre, gz, gbias, gw_coord, gw2)."""
        zs = [z.double().requires_grad_() for z in self.zs]
        b, wc, w2 = (t.double().requires_grad_() for t in (self.bias, self.w_coord, self.w2))
        out, pre = vr.reference_order(zs, self.Ms, self.up, self.grid, vr.head_weight(self.Cm, self.N, wc), b,
                                      w2.reshape(1, self.Cm, 1, 1), dtype=torch.float64, pattern=pattern)
        res = dict(map=out.detach(), pre=pre.detach())
        if backward:
            out.backward(self.dmap.double())
            res.update(gz=[z.grad for z in zs], gbias=b.grad, gw_coord=wc.grad, gw2=w2.grad)
        return res

    def check(self, got, what, grads=True):
        """Forward against plain ReLU, the flip rule, then every gradient given the GPU's pattern."""
        plain = self.reference(backward=False)
        assert_parity(got["map"], plain["map"], f"{what}: map", normwise_tol=TOL)
        assert_parity(got["hidden"], torch.relu(plain["pre"]), f"{what}: hidden", normwise_tol=TOL)
        if not grads:
            return
        pattern = (got["hidden"] > 0).double()
        vr.relu_flips(pattern, plain["pre"])
        ref = self.reference(pattern=pattern)
        for i in range(self.N):
            assert_parity(got["gz"][i], ref["gz"][i], f"{what}: d z_{i}", normwise_tol=TOL)
        for k in ("bias", "w_coord", "w2"):
            assert_parity(got["g" + k], ref["g" + k], f"{what}: d {k}", normwise_tol=TOL)


@functools.lru_cache(maxsize=None)
def _general():
    """Case 1: N = 3, B = 2, Cm = 5 (no multiple of 4), 7 x 9 -> 20 x 31, grid 12 x 17 (two blocks per row, a
    partial group of pixels), one NCHW view, one channels-last view, one unaligned slice."""
    case = Case(3, 2, 5, (7, 9), (20, 31), (12, 17), seed=1)
    return case, case.run(layouts=["nchw", "cl", "slice"])


def test_general_case_forward_and_every_gradient():
    case, got = _general()
    assert type(got["grad_fn"]).__name__.startswith("WarpSumHead")
    assert tuple(got["map"].shape) == (2, 1, 12, 17) and tuple(got["hidden"].shape) == (2, 5, 12, 17)
    assert all(tuple(g.shape) == (2, 5, 7, 9) for g in got["gz"])
    case.check(got, "general")


def test_full_channel_mapping_512_wide_reduction():
    """Case 2: Cm = 512 (both channel halves of every lane, the 16-B loads, the whole-wave dot), exact 3x
    upsample (taps of weight 0), grid 16 x 24 (16-B hidden stores)."""
    case = Case(2, 1, 512, (6, 8), (18, 24), (16, 24), seed=2)
    case.check(case.run(), "Cm=512")


def test_frustum_edge_cases():
    """Case 3: view 0's source lies entirely off the grid, view 1 covers every grid pixel, view 2 is general."""
    up, grid = (20, 31), (12, 17)
    rng = np.random.default_rng(3)
    off = _rand_h(rng, *up, *grid)
    off[0, 2] += 1.0e4   # the source lands 10^4 grid pixels to the right of the grid
    full = np.diag([grid[1] / up[1] * 1.5, grid[0] / up[0] * 1.5, 1.0])  # the grid is the source's top-left 2/3
    case = Case(3, 2, 8, (7, 9), up, grid, seed=3, Ms=[off, full, _rand_h(rng, *up, *grid)])
    for v, want in ((0, 0.0), (1, 1.0)):
        g = vr.sample_grid(torch.from_numpy(case.Ms[v]).reshape(1, 3, 3).float(), up, grid)[0]
        ix, iy = (g[..., 0] + 1) / 2 * (up[1] - 1), (g[..., 1] + 1) / 2 * (up[0] - 1)
        inside = (ix > -1) & (ix < up[1]) & (iy > -1) & (iy < up[0])
        assert float(inside.float().mean()) == want  # the case is what it says
    head = case.head()
    got = case.run(head=head)
    case.check(got, "frustum")
    assert torch.count_nonzero(got["gz"][0]) == 0, "the off-grid view's gradient must be exactly 0"
    assert torch.count_nonzero(got["gz"][1]) > 0
    case.zs[0] = case.zs[0] * -3.0 + 7.0  # other data in the view that reaches no pixel
    again = case.run(head=head, grad=())
    assert torch.equal(again["map"], got["map"]), "the off-grid view's data changed the map"


def test_degenerate_homography_nan_pattern():
    """Case 4: view 1's homography overflows fp32 on part of the grid (kornia's transform gives non-finite
    coordinates there, grid_sample NaN): the map is NaN on exactly the restatement's pixels.  Forward only."""
    up, grid = (20, 31), (12, 17)
    rng = np.random.default_rng(4)
    Ms = [_rand_h(rng, *up, *grid) for _ in range(3)]
    # view 1's source pixel coordinates scaled by s = 4e37: the normalised coordinate becomes s (x + 1) - 1, and
    # grid_sample's pixel coordinate ((x + 1) / 2) (W - 1) overflows fp32 where it passes 2 * 3.4e38 / 30 = 2.3e37,
    # i.e. right of source column 0.57 * 15 = 8.5 (rows likewise).  _rand_h maps the grid onto 0.7 to 1.7 times
    # the source around its centre, so the grid holds pixels on both sides of that line whatever the draw
    Ms[1] = Ms[1] @ np.diag([1 / 4e37, 1 / 4e37, 1.0])
    case = Case(3, 1, 8, (7, 9), up, grid, seed=4, Ms=Ms)
    ref = case.reference(backward=False)
    n_nan = int(torch.isnan(ref["map"]).sum())
    assert 0 < n_nan < ref["map"].numel(), "the case should be partly NaN"
    got = case.run(grad=())
    assert got["grad_fn"] is None
    assert torch.equal(torch.isnan(got["map"]), torch.isnan(ref["map"]))
    assert_parity(got["map"], ref["map"], "degenerate: map (NaN pattern included)", normwise_tol=TOL)
    assert_parity(got["hidden"], torch.relu(ref["pre"]), "degenerate: hidden", normwise_tol=TOL)


NONFINITE_PARAMS = [("w2", (2,), float("-inf")), ("w2", (2,), float("nan")), ("bias", (1,), float("-inf")),
                    ("bias", (1,), float("inf")), ("w_coord", (3, 0), float("inf")), ("w_coord", (3, 1), float("nan"))]


@pytest.mark.parametrize("which,idx,val", NONFINITE_PARAMS)
def test_nonfinite_parameters_forward_pattern(which, idx, val):
    """A NaN / inf in w2, the bias or a coord weight (a diverging ``optimizer.step()``) with finite features, on the
    general case's 12 x 17 grid (odd width: the x coord is exactly 0 on the middle column, where 0 * inf = NaN):
    ``hidden`` and the map have the fp64 reference's NaN, +inf and -inf patterns — w2 = -inf gives -inf where the
    ReLU passes and NaN where it gives 0, a -inf bias a dead channel and a finite map — and the finite entries
    pass the gate."""
    case = Case(3, 2, 5, (7, 9), (20, 31), (12, 17), seed=1)
    getattr(case, which)[idx] = val
    got = case.run(layouts=["nchw", "cl", "slice"], grad=())
    ref = case.reference(backward=False)
    for name, g, r in (("map", got["map"], ref["map"]), ("hidden", got["hidden"], torch.relu(ref["pre"]))):
        assert torch.equal(torch.isposinf(g), torch.isposinf(r)), f"{name}: +inf pattern differs"
        assert torch.equal(torch.isneginf(g), torch.isneginf(r)), f"{name}: -inf pattern differs"
        assert_parity(g, r, f"{which}{idx} = {val}: {name}", normwise_tol=TOL)  # (NaN pattern included)
    nf = int((~torch.isfinite(ref["map"])).sum())
    if which == "bias" and val < 0:
        assert nf == 0 and torch.count_nonzero(got["hidden"][:, idx[0]]) == 0
    else:
        assert nf > 0


@pytest.mark.parametrize("subset", ["params", "zs", "one_z_off"])
def test_needs_input_grad_subsets(subset):
    """Case 5: what needs no gradient gets None, and what does is bitwise what the full backward gave."""
    case, full = _general()
    layouts = ["nchw", "cl", "slice"]
    if subset == "params":
        got = case.run(layouts, grad=("bias", "w_coord", "w2"))
        assert all(g is None for g in got["gz"])
        want_z = [False] * 3
    elif subset == "zs":
        got = case.run(layouts, grad=("z",))
        assert got["gbias"] is None and got["gw_coord"] is None and got["gw2"] is None
        want_z = [True] * 3
    else:
        want_z = [True, False, True]
        got = case.run(layouts, z_grad=want_z)
        assert got["gz"][1] is None
    for i, wz in enumerate(want_z):
        if wz:
            assert torch.equal(got["gz"][i], full["gz"][i]), f"d z_{i} changed"
    if subset != "zs":
        for k in ("gbias", "gw_coord", "gw2"):
            assert torch.equal(got[k], full[k]), f"{k} changed"
    assert torch.equal(got["map"], full["map"])


def test_two_runs_are_bitwise_equal():
    """Case 6: no float atomics anywhere."""
    case, first = _general()
    second = case.run(layouts=["nchw", "cl", "slice"])
    for k in ("map", "hidden", "gbias", "gw_coord", "gw2"):
        assert torch.equal(first[k], second[k]), k
    for a, b in zip(first["gz"], second["gz"]):
        assert torch.equal(a, b)


def test_inference_writes_nothing_of_slab_size():
    """Case 7: under no_grad the peak above the inputs stays below a quarter of the concatenated slab
    (N Cm Ho Wo fp32) the reference order builds; the design's own footprint is the map."""
    case = Case(3, 1, 64, (6, 8), (18, 24), (40, 60), seed=7)
    head = case.head()
    zs = case.gpu_inputs()
    b, wc, w2 = case.bias.to(DEV), case.w_coord.to(DEV), case.w2.to(DEV)
    with torch.no_grad():
        head(zs, b, wc, w2)  # the geometry-only boxes are built once per rig, outside the measured call
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = head(zs, b, wc, w2)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    slab = case.N * case.Cm * 40 * 60 * 4
    assert peak < slab // 4, (peak, slab)
    assert out.grad_fn is None
    assert_parity(out.cpu(), case.reference(backward=False)["map"], "inference map", normwise_tol=TOL)
