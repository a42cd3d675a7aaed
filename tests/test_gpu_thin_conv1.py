"""The thin fused conv1 on the GPU (``mvbev_thin_conv1_*`` through ``mvdet_amd.thin_fuse``'s kernel-level wrappers)
against a torch-CPU restatement in fp64 with fp32 geometry: ``variant_ref.warp`` (the oracle's kornia warp) of every
plane, cat with the coord map, ``F.conv2d(padding=1)``, ReLU.  Gate: ``helpers.assert_parity`` at 5e-5 normwise.
The backward kernels take the gradient of the pre-activation as given (the caller masks it), so their reference is
fp64 autograd of the pre-activation itself: no activation pattern is involved at this level."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import variant_ref as vr
from helpers import assert_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5


def _rand_h(rng, H, W, ho, wo):
    """A mild random homography from H x W source pixels to ho x wo grid pixels (``test_gpu_sum_head``'s)."""
    A = np.eye(3)
    A[0, 0] = wo / W * rng.uniform(0.6, 1.4)
    A[1, 1] = ho / H * rng.uniform(0.6, 1.4)
    A[0, 1], A[1, 0] = rng.uniform(-0.2, 0.2, 2)
    A[0, 2], A[1, 2] = rng.uniform(-3, 3, 2)
    A[2, 0], A[2, 1] = rng.uniform(-2e-3, 2e-3, 2)
    return A


def _m_norms(Ms, src, grid):
    from mvdet_amd.geometry import kornia_src_norm_from_dst_norm
    return [kornia_src_norm_from_dst_norm(torch.from_numpy(np.asarray(M)).float().reshape(1, 3, 3), src, grid)[0]
            for M in Ms]


class Case:
    def __init__(self, N, B, cout, src, grid, seed, Ms=None, bias=True):
        rng = np.random.default_rng(seed)
        self.N, self.B, self.cout, self.src, self.grid = N, B, cout, src, grid
        self.Ms = Ms if Ms is not None else [_rand_h(rng, *src, *grid) for _ in range(N)]
        self.planes = [torch.from_numpy(rng.standard_normal((B, 1, *src)).astype(np.float32)) for _ in range(N)]
        k = 1.0 / np.sqrt(9 * (N + 2))
        self.w1 = torch.from_numpy(rng.uniform(-k, k, (cout, N + 2, 3, 3)).astype(np.float32))
        self.b1 = torch.from_numpy(rng.uniform(-k, k, cout).astype(np.float32)) if bias else None
        self.dpre = torch.from_numpy(rng.standard_normal((B, cout, *grid)).astype(np.float32))

    def gpu_planes(self, sliced=False):
        """The planes on the GPU; ``sliced``: channel 1 of a [B,2,H+1,W+3] tensor, columns 1 .. W (non-contiguous
        batch, channel and row strides, an unaligned base)."""
        if not sliced:
            return [p.to(DEV) for p in self.planes]
        out = []
        H, W = self.src
        for p in self.planes:
            big = torch.full((self.B, 2, H + 1, W + 3), 9.0, device=DEV)
            big[:, 1:2, :H, 1:W + 1] = p.to(DEV)
            t = big[:, 1:2, :H, 1:W + 1]
            assert not t.is_contiguous() and t.stride(3) == 1
            out.append(t)
        return out

    def forward(self, split=False, want_xw=True, sliced=False):
        from mvdet_amd import ops, thin_fuse
        B, (Ho, Wo) = self.B, self.grid
        if split:
            y1 = torch.full(ops.split_shape(B, self.cout, Ho, Wo), 7.0, dtype=torch.bfloat16, device=DEV)
        else:
            y1 = torch.full((B, self.cout, Ho, Wo), 7.0, device=DEV)
        xw = torch.full((B, self.N, Ho, Wo), 7.0, device=DEV) if want_xw else None
        thin_fuse.thin_conv1_forward(self.gpu_planes(sliced), _m_norms(self.Ms, self.src, self.grid), self.grid,
                                     self.w1.to(DEV), None if self.b1 is None else self.b1.to(DEV), y1, xw)
        torch.cuda.synchronize()
        y = ops.split_decode(y1, self.cout) if split else y1
        return y.cpu(), None if xw is None else xw.cpu()

    def backward(self, xw, need_dx=True, need_dw=True, coord=True):
        """dxw, dw1 (view channels from the new kernels, coord channels from the existing one), db1 on the GPU."""
        from mvdet_amd import ops, thin_fuse
        dpre, w1 = self.dpre.to(DEV), self.w1.to(DEV)
        dw = torch.zeros_like(w1) if need_dw else None
        db = torch.empty(self.cout, device=DEV) if coord else None
        if coord:
            ops.conv3x3_bias_coord_grad(dpre, 1, db=db, dw=dw, coord_ch=self.N)
        dxw = thin_fuse.thin_conv1_backward(dpre, w1, xw.to(DEV), self.N, need_dx=need_dx, dw=dw)
        torch.cuda.synchronize()
        return (None if dxw is None else dxw.cpu(), None if dw is None else dw.cpu(), None if db is None else db.cpu())

    def reference(self, backward=False):
        """fp64 CPU: dict(xw, pre, y1 [, dxw, dw1, db1])."""
        xw = torch.cat([vr.warp(p.double(), M, self.grid) for p, M in zip(self.planes, self.Ms)], 1)
        xw = xw.detach().requires_grad_()
        with np.errstate(all="ignore"):  # (a 1-pixel grid side: kornia's and the coord map's 0 / 0)
            coord = vr.coord_map(*self.grid).double().repeat([self.B, 1, 1, 1])
        w1 = self.w1.double().requires_grad_()
        b1 = None if self.b1 is None else self.b1.double().requires_grad_()
        pre = F.conv2d(torch.cat([xw, coord], 1), w1, b1, padding=1)
        res = dict(xw=xw.detach(), pre=pre.detach(), y1=torch.relu(pre.detach()))
        if backward:
            pre.backward(self.dpre.double())
            res.update(dxw=xw.grad, dw1=w1.grad, db1=None if b1 is None else b1.grad)
        return res


@functools.lru_cache(maxsize=None)
def _general(cout):
    """N = 3, B = 2, source 24 x 32, grid 19 x 45: ragged against 4-, 8-, 12- and 16-row and 16- and 32-column
    tiles, several tiles in both directions."""
    case = Case(3, 2, cout, (24, 32), (19, 45), seed=10 + cout)
    return case, case.reference(backward=True)


@pytest.mark.parametrize("cout", [128, 512])
@pytest.mark.parametrize("split", [False, True])
def test_general_case_forward(cout, split):
    case, ref = _general(cout)
    y1, xw = case.forward(split=split)
    assert tuple(y1.shape) == (2, cout, 19, 45)
    assert_parity(xw, ref["xw"], "xw against the warp alone", normwise_tol=TOL)
    assert_parity(y1, ref["y1"], f"y1 (split={split})", normwise_tol=TOL)
    assert float((y1 == 0).float().mean()) > 0.2  # the ReLU is there
    y1b, none = case.forward(split=split, want_xw=False)
    assert none is None and torch.equal(y1b, y1)


@pytest.mark.parametrize("N", [1, 7, 16])
def test_view_counts(N):
    case = Case(N, 1, 16, (24, 32), (19, 45), seed=20 + N)
    ref = case.reference()
    y1, xw = case.forward()
    assert_parity(xw, ref["xw"], f"N={N}: xw", normwise_tol=TOL)
    assert_parity(y1, ref["y1"], f"N={N}: y1", normwise_tol=TOL)


def test_channel_slices_with_non_contiguous_strides():
    case, ref = _general(128)
    y1, xw = case.forward()
    y1s, xws = case.forward(sliced=True)
    assert torch.equal(y1s, y1) and torch.equal(xws, xw)
    assert_parity(y1s, ref["y1"], "sliced planes: y1", normwise_tol=TOL)


def _inside_share(M, src, grid):
    g = vr.sample_grid(torch.from_numpy(M).reshape(1, 3, 3).float(), src, grid)[0]
    ix, iy = (g[..., 0] + 1) / 2 * (src[1] - 1), (g[..., 1] + 1) / 2 * (src[0] - 1)
    return float(((ix > -1) & (ix < src[1]) & (iy > -1) & (iy < src[0])).float().mean())


def test_frustum_edge_cases():
    """View 0's source lies entirely off the grid (exact zeros, its data is not read), view 1 covers every grid
    pixel, view 2 is general."""
    src, grid = (24, 32), (19, 45)
    rng = np.random.default_rng(3)
    off = _rand_h(rng, *src, *grid)
    off[0, 2] += 1.0e4  # the source lands 10^4 grid pixels to the right of the grid
    full = np.diag([grid[1] / src[1] * 1.5, grid[0] / src[0] * 1.5, 1.0])  # the grid is the source's top-left 2/3
    case = Case(3, 2, 16, src, grid, seed=3, Ms=[off, full, _rand_h(rng, *src, *grid)])
    assert _inside_share(off, src, grid) == 0.0 and _inside_share(full, src, grid) == 1.0
    ref = case.reference(backward=True)
    y1, xw = case.forward()
    assert torch.count_nonzero(xw[:, 0]) == 0, "the off-grid view's warped plane must be exactly 0"
    assert torch.count_nonzero(xw[:, 1] == 0) == 0
    assert_parity(xw, ref["xw"], "frustum: xw", normwise_tol=TOL)
    assert_parity(y1, ref["y1"], "frustum: y1", normwise_tol=TOL)
    dxw, dw, db = case.backward(xw)
    assert_parity(dxw, ref["dxw"], "frustum: dxw", normwise_tol=TOL)
    assert_parity(dw, ref["dw1"], "frustum: dw1", normwise_tol=TOL)
    assert torch.count_nonzero(dw[:, 0]) == 0, "the off-grid view's weight gradient must be exactly 0"
    case.planes[0] = case.planes[0] * -3.0 + 7.0  # other data in the view that reaches no pixel
    again, _ = case.forward()
    assert torch.equal(again, y1), "the off-grid view's data changed y1"


@pytest.mark.parametrize("grid", [(1, 37), (19, 1)])
def test_one_pixel_grid_side(grid):
    """kornia's meshgrid and the coord map divide by (size - 1): a 1-pixel side makes every sample coordinate and
    one coord channel NaN, so y1 is NaN wherever the reference's is (everywhere)."""
    case = Case(2, 1, 8, (24, 32), grid, seed=5)
    ref = case.reference()
    assert torch.isnan(ref["y1"]).all()
    y1, xw = case.forward()
    assert torch.equal(torch.isnan(xw), torch.isnan(ref["xw"]))
    assert torch.equal(torch.isnan(y1), torch.isnan(ref["y1"]))


def test_degenerate_homography_nan_pattern():
    """View 1's homography overflows fp32 on part of the grid (non-finite sample coordinates, NaN samples): y1 is
    NaN on exactly the reference conv's pixels, the 3 x 3 neighbourhoods of the NaN samples, in every channel."""
    src, grid = (24, 32), (19, 45)
    rng = np.random.default_rng(4)
    Ms = [_rand_h(rng, *src, *grid) for _ in range(3)]
    Ms[1] = Ms[1] @ np.diag([1 / 4e37, 1 / 4e37, 1.0])  # (as test_gpu_sum_head's degenerate case)
    for split in (False, True):
        case = Case(3, 1, 16, src, grid, seed=4, Ms=Ms)
        ref = case.reference()
        n_nan = int(torch.isnan(ref["xw"][:, 1]).sum())
        assert 0 < n_nan < grid[0] * grid[1], "the case should be partly NaN"
        y1, xw = case.forward(split=split)
        assert torch.equal(torch.isnan(xw), torch.isnan(ref["xw"]))
        assert torch.equal(torch.isnan(y1), torch.isnan(ref["y1"]))
        assert 0 < int(torch.isnan(y1[0, 0]).sum()) < grid[0] * grid[1]
        assert_parity(y1, ref["y1"], f"degenerate: y1 (split={split})", normwise_tol=TOL)


def test_no_bias():
    case = Case(3, 1, 16, (24, 32), (19, 45), seed=6, bias=False)
    y1, _ = case.forward()
    assert_parity(y1, case.reference()["y1"], "b1 = NULL: y1", normwise_tol=TOL)


@functools.lru_cache(maxsize=None)
def _general_backward():
    case, ref = _general(128)
    _, xw = case.forward()
    return xw, case.backward(xw)


def test_backward_against_fp64_autograd():
    case, ref = _general(128)
    _, (dxw, dw, db) = _general_backward()
    assert_parity(dxw, ref["dxw"], "dxw", normwise_tol=TOL)
    assert_parity(dw[:, :3], ref["dw1"][:, :3], "dw1, view channels", normwise_tol=TOL)
    assert_parity(dw[:, 3:], ref["dw1"][:, 3:], "dw1, coord channels", normwise_tol=TOL)
    assert_parity(db, ref["db1"], "db1", normwise_tol=TOL)


@pytest.mark.parametrize("N,cout", [(7, 264), (16, 8)])
def test_backward_view_groups_and_channel_slices(N, cout):
    """More views than one weight-gradient block takes (4), a partial last group, Cout past one 256-channel block
    and no multiple of 16."""
    case = Case(N, 1, cout, (24, 32), (19, 45), seed=30 + N)
    ref = case.reference(backward=True)
    _, xw = case.forward()
    dxw, dw, _ = case.backward(xw)
    assert_parity(dxw, ref["dxw"], f"N={N}: dxw", normwise_tol=TOL)
    assert_parity(dw, ref["dw1"], f"N={N}: dw1", normwise_tol=TOL)


def test_null_outputs_leave_the_others_bitwise_unchanged():
    case, _ = _general(128)
    xw, (dxw, dw, db) = _general_backward()
    only_dx, none_dw, _ = case.backward(xw, need_dw=False, coord=False)
    assert none_dw is None and torch.equal(only_dx, dxw)
    none_dx, only_dw, _ = case.backward(xw, need_dx=False)
    assert none_dx is None and torch.equal(only_dw, dw)


def test_two_runs_are_bitwise_equal():
    case, _ = _general(128)
    xw, first = _general_backward()
    for split in (False, True):
        a, b = case.forward(split=split), case.forward(split=split)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    second = case.backward(xw)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_bad_arguments_return_the_documented_codes():
    """With real device pointers: the checks come before any launch."""
    import ctypes
    from mvdet_amd import _native
    lib = _native.load()
    x = torch.zeros(1, 1, 24, 32, device=DEV)
    w1, y1 = torch.zeros(12, 3, 3, 3, device=DEV), torch.zeros(1, 16, 19, 45, device=DEV)
    arr = (_native.WarpView * 1)()
    arr[0].src, arr[0].src_strides = x.data_ptr(), (ctypes.c_int64 * 4)(*x.stride())
    arr[0].m = (1, 0, 0, 0, 1, 0, 0, 0, 1)
    fn = lib.mvbev_thin_conv1_forward_f32
    assert fn(arr, 1, 1, 24, 32, 19, 45, w1.data_ptr(), None, 12, y1.data_ptr(), 0, None, None) == -2  # Cout % 8
    assert fn(arr, 1, 1, 24, 32, 19, 45, w1.data_ptr(), None, 8, y1.data_ptr() + 4, 2, None, None) == -4
    assert fn(arr, 1, 1, 24, 32, 19, 45, None, None, 8, y1.data_ptr(), 0, None, None) == -5
    arr[0].src_strides = (ctypes.c_int64 * 4)(768, 768, 32, 2)
    assert fn(arr, 1, 1, 24, 32, 19, 45, w1.data_ptr(), None, 8, y1.data_ptr(), 0, None, None) == -3
    torch.cuda.synchronize()
    assert torch.count_nonzero(y1) == 0  # nothing was launched
