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

    def forward(self, split=False, want_xw=True, sliced=False, mask=False):
        """``mask``: with the weight word of ``thin_conv1_weight_mask`` (as ``ProjectThinFuse`` calls the kernel)."""
        from mvdet_amd import ops, thin_fuse
        B, (Ho, Wo) = self.B, self.grid
        if split:
            y1 = torch.full(ops.split_shape(B, self.cout, Ho, Wo), 7.0, dtype=torch.bfloat16, device=DEV)
        else:
            y1 = torch.full((B, self.cout, Ho, Wo), 7.0, device=DEV)
        xw = torch.full((B, self.N, Ho, Wo), 7.0, device=DEV) if want_xw else None
        w1 = self.w1.to(DEV)
        self.mask_word = int(thin_fuse.thin_conv1_weight_mask(w1, self.N).item()) if mask else None
        thin_fuse.thin_conv1_forward(self.gpu_planes(sliced), _m_norms(self.Ms, self.src, self.grid), self.grid,
                                     w1, None if self.b1 is None else self.b1.to(DEV), y1, xw,
                                     w_mask=thin_fuse.thin_conv1_weight_mask(w1, self.N) if mask else None)
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


def _frustum_case():
    """``test_frustum_edge_cases``'s rig: view 0 entirely off the grid, view 1 covering it, view 2 general."""
    src, grid = (24, 32), (19, 45)
    rng = np.random.default_rng(3)
    off = _rand_h(rng, *src, *grid)
    off[0, 2] += 1.0e4
    full = np.diag([grid[1] / src[1] * 1.5, grid[0] / src[0] * 1.5, 1.0])
    return Case(3, 2, 16, src, grid, seed=3, Ms=[off, full, _rand_h(rng, *src, *grid)])


NONFINITE_PARAMS = {
    # name: (tensor, index, value, bit of the weight word, output channel, what that channel of y1 is)
    "w1_dead_view_nan": ("w1", (3, 0, 1, 1), float("nan"), 1, 3, "nan"),
    "w1_dead_view_ninf": ("w1", (3, 0, 1, 1), float("-inf"), 1, 3, "nan"),  # 0 * -inf
    "w1_general_view_ninf": ("w1", (3, 2, 1, 1), float("-inf"), 4, 3, "mixed"),
    "b1_ninf": ("b1", (5,), float("-inf"), 0, 5, "zero"),  # a dead channel
    "w1_coord_x_nan": ("w1", (6, 3, 1, 1), float("nan"), 0, 6, "nan"),
    "w1_coord_y_pinf": ("w1", (6, 4, 1, 1), float("inf"), 0, 6, "mixed"),  # 0 on the middle row: 0 * inf = NaN
}


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", sorted(NONFINITE_PARAMS))
def test_nonfinite_conv1_parameters(name, split):
    """A NaN / inf at a centre tap of w1 (a view entirely off the grid, whose tiles the kernel skips when its
    weights are finite: the reference multiplies 0 * NaN = NaN at every pixel; a general view; a coord channel, on
    a grid with odd sides whose coord value is exactly 0 on the middle row / column) or in b1: y1's NaN / inf
    pattern is the fp64 reference's, fp32 layout and split-bf16 (which keeps NaN and the finite values; its
    hi / lo pair of +inf decodes as NaN, so there the non-finite entries are compared as such), the other
    channels untouched.  The weight word marks exactly the views whose w1 columns are non-finite."""
    case = _frustum_case()
    base, _ = case.forward(split=split, mask=True)
    assert case.mask_word == 0
    plain, _ = case.forward(split=split)
    assert torch.equal(base, plain), "finite weights: the weight word must not change y1"
    which, idx, val, bit, co, kind = NONFINITE_PARAMS[name]
    getattr(case, which)[idx] = val
    ref = case.reference()["y1"]
    y1, _ = case.forward(split=split, mask=True)
    assert case.mask_word == bit
    r = ref[:, co]
    if kind == "nan":
        assert torch.isnan(r).all()
    elif kind == "zero":
        assert torch.count_nonzero(r) == 0
    else:
        assert 0 < int(torch.isnan(r).sum()) < r.numel() and int(torch.isposinf(r).sum()) > 0
    others = [c for c in range(case.cout) if c != co]
    assert torch.isfinite(ref[:, others]).all() and torch.equal(y1[:, others], base[:, others])
    assert torch.equal(~torch.isfinite(y1), ~torch.isfinite(ref)), "non-finite pattern differs"
    if split:
        assert torch.isnan(y1[torch.isnan(ref)]).all()
        fin = torch.isfinite(ref)
        assert_parity(y1[fin], ref[fin], f"{name}: finite entries of y1 (split)", normwise_tol=TOL)
    else:
        assert torch.equal(torch.isposinf(y1), torch.isposinf(ref)) and not torch.isneginf(y1).any()
        assert_parity(y1, ref, f"{name}: y1", normwise_tol=TOL)


@pytest.mark.parametrize("train", [False, True])
def test_head_weight_word_follows_w1_in_place(train):
    """``ProjectThinFuse`` itself (inference, and the training forward of ``ThinFuseFunction``): its cached weight
    word (``w1_mask``, keyed on w1's ``(data_ptr, _version, strides)``) follows w1 poisoned and restored IN PLACE —
    finite: word 0; ``w1[3, 0] = NaN`` at the centre tap of the off-grid view: bit 0, and (inference) channel 3 of
    the head's y1 all NaN as the reference's; restored: word 0 again and y1 bitwise the first one."""
    from mvdet_amd import ProjectThinFuse, ops
    case = _frustum_case()
    mid = 128
    rng = np.random.default_rng(7)
    k = 1.0 / np.sqrt(9 * (case.N + 2))
    w1 = torch.from_numpy(rng.uniform(-k, k, (mid, case.N + 2, 3, 3)).astype(np.float32)).to(DEV)
    b1 = torch.from_numpy(rng.uniform(-k, k, mid).astype(np.float32)).to(DEV)
    w2 = torch.from_numpy((rng.uniform(-1, 1, (mid, mid, 3, 3)) / np.sqrt(9 * mid)).astype(np.float32)).to(DEV)
    b2 = torch.zeros(mid, device=DEV)
    w3 = torch.from_numpy((rng.uniform(-1, 1, (1, mid, 3, 3)) / np.sqrt(9 * mid)).astype(np.float32)).to(DEV)
    if train:
        w1.requires_grad_()
    head = ProjectThinFuse([torch.from_numpy(np.asarray(M)) for M in case.Ms], case.src, case.grid, mid_channels=mid)
    planes = case.gpu_planes()

    def run():
        out = head(planes, w1, b1, w2, b2, w3)
        assert (out.grad_fn is not None) == train
        word = int(head.w1_mask(w1.detach(), w1.detach()).item())
        y1 = None if train else ops.split_decode(head.engine.workspace(case.B, DEV).y1, mid).clone()
        return word, y1, out.detach().clone()

    word0, y0, out0 = run()
    assert word0 == 0 and torch.isfinite(out0).all()
    with torch.no_grad():
        old = w1[3, 0, 1, 1].item()
        w1[3, 0, 1, 1] = float("nan")
    word1, y1, _ = run()
    assert word1 == 1
    if not train:
        assert torch.isnan(y1[:, 3]).all() and torch.isfinite(y1[:, :3]).all() and torch.isfinite(y1[:, 4:]).all()
    with torch.no_grad():
        w1[3, 0, 1, 1] = old
    word2, y2, out2 = run()
    assert word2 == 0 and torch.equal(out2, out0)
    if not train:
        assert torch.equal(y2, y0)


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
