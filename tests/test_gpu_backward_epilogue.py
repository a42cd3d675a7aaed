"""The small kernels of the training backward, each on its own against a plain reference: the ReLU masks
(``relu_backward_``, ``relu_backward_split_``), the bias / coord-channel reduction
(``conv3x3_bias_coord_grad``), conv3's backward (``conv3x3_cout1_backward``), the gated activation store
(``store_gated_``) and the gated fp32 pack / row transform.  The end-to-end training tests gate a whole
network at 1e-3 normwise and cannot see a dropped tail element; these can.

Rules of this file:
  * elementwise results are BITWISE the reference (signed zeros and denormals included; a NaN's payload is
    compared as NaN-ness, as ``helpers`` does);
  * a sum is compared with float64 under the forward-error bound of fp32 summation in ANY order, with or
    without fma contraction:  |got - ref64| <= (N + 2) * 2^-24 * sum|terms|  (N summed products, sum|terms|
    from the float64 reference over absolute values), and under ``helpers.assert_parity``;
  * that bound cannot see one dropped element, so every reduction also runs impulse inputs (all zero but
    single 1.0s, one per channel, at the first / last pixel, the end of a row, the first pixel of a second
    wave / thread / batch trip and the tail positions): one non-zero term per sum, so the result must be
    EXACT (a single fp32 product, 1.0 for the bias);
  * the ReLU masks follow ``torch.ops.aten.threshold_backward(grad, y, 0)`` on the CPU, the op ``nn.ReLU``
    differentiates to: 0 where y <= 0, else grad — the gradient passes at a NaN activation."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_parity
from oracle import cpu_path

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24  # fp32 unit roundoff
NAN, INF = float("nan"), float("inf")
# activations: NaN, +-inf, +-0, denormals, tiny normals (between them: ordinary values)
SPECIAL = [NAN, INF, -INF, 0.0, -0.0, 1e-40, 1e-30, -1e-40, -1e-30]


# ------------------------------------------------------------------------------------------ helpers

def _bits_equal(got, ref, what):
    """Bitwise equality of two tensors of one float dtype; NaN payloads compared as NaN-ness."""
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    nr = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nr), f"{what}: NaN pattern differs"
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    bad = (got.view(it) != ref.view(it)) & ~nr
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} entries differ, first at "
                           f"{bad.nonzero()[0].tolist()}: {got[bad][0].item()!r} vs {ref[bad][0].item()!r}")


def _check_sum(got, ref64, abs64, n, what, exact=False):
    """A reduction of ``n`` products: the NaN / inf pattern (signs included) and the parity gate, the derived
    bound (n + 2) * 2^-24 * sum|terms|, and with ``exact`` (impulse inputs: one non-zero term) equality."""
    got = got.detach().cpu()
    assert_parity(got, ref64, what)
    inf = torch.isinf(ref64)
    assert torch.equal(got.double()[inf], ref64[inf]), f"{what}: infinities differ in sign"
    fin = torch.isfinite(ref64)
    err = (got.double() - ref64).abs()[fin]
    bound = (n + 2) * U * abs64[fin]
    assert (err <= bound).all(), f"{what}: |err| over the bound by {float((err - bound).max()):.3e} (N = {n})"
    if exact:
        assert torch.equal(got.double()[fin], ref64[fin]), \
            f"{what}: impulse result not exact, max |err| {float(err.max()):.3e}"


def _split_encode(x, keep_nonfinite=False):
    """fp32 [B, C, H, W] -> the split-bf16 blocked layout [B, ceil(C / 8), H, W, 2, 8], channels past C zero:
    hi = bf16(x) (round to nearest even), lo = bf16(x - hi); ``keep_nonfinite``: ``store_gated_``'s encoding,
    lo = 0 where x is not finite (hi + lo keeps the value)."""
    B, C, H, W = x.shape
    G = -(-C // 8)
    if 8 * G != C:
        x = torch.cat([x, torch.zeros((B, 8 * G - C, H, W))], 1)
    hi = x.to(torch.bfloat16)
    d = x - hi.float()
    if keep_nonfinite:
        d = torch.where(torch.isfinite(x), d, torch.zeros_like(d))
    t = torch.stack([hi, d.to(torch.bfloat16)], 0).reshape(2, B, G, 8, H, W)
    return t.permute(1, 2, 4, 5, 0, 3).contiguous()


def _sprinkle(t, values, every, phase=0):
    """In place over the flattened ``t``: every ``every``-th element (from ``phase``) takes the next of
    ``values`` in turn."""
    f = t.view(-1)
    idx = torch.arange(phase, max(f.numel(), phase), every)
    f[idx] = torch.tensor(values, dtype=t.dtype)[torch.arange(idx.numel()) % len(values)]
    return t


def _impulses(B, C, H, W, flat_positions):
    """[B, C, H, W] zeros with one 1.0 per channel: channel c at flat pixel ``flat_positions[c % len]`` of
    batch item c % B."""
    t = torch.zeros((B, C, H * W))
    for c in range(C):
        t[c % B, c, flat_positions[c % len(flat_positions)]] = 1.0
    return t.view(B, C, H, W)


def _positions(HW, W, extra=()):
    """Flat pixels where a reduction's loop can drop or double an element: the first, the last, the end of
    the first row, and around each trip boundary of 1024 threads x 4 pixels."""
    cand = [0, HW - 1, W - 1, 1023, 1024, 4095, 4096, HW - 3073, HW - 3072, HW - 1025, HW - 1024, *extra]
    return sorted({p for p in cand if 0 <= p < HW})


# ------------------------------------------------------------------------------ (a) relu_backward_

def _relu_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    y = _sprinkle(torch.randn(n, generator=g), SPECIAL, 3)
    dy = _sprinkle(torch.randn(n, generator=g), [NAN, INF, -INF], 5, 2)
    # the last elements (the scalar tail's where n % 4): a NaN activation under a finite gradient, -inf under
    # a NaN gradient (masked to 0), +inf under an infinite one
    for k, (yv, gv) in enumerate([(NAN, 3.0), (-INF, NAN), (INF, -INF)]):
        if n > k:
            y[n - 1 - k], dy[n - 1 - k] = yv, gv
    return y, dy


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 256 * 3 + 1, 4 * 256 * 3 + 2,
                               4 * 256 * 3 + 3])
def test_relu_backward_bitwise_vs_threshold_backward(n):
    """The float4 body and the scalar tail (n % 4 elements of the last thread), non-finite activations and
    gradients in both.  Before the fix the kernel masked with y > 0 and dropped the gradient at a NaN."""
    from mvdet_amd import ops
    y, dy = _relu_inputs(n, 100 + n)
    ref = torch.ops.aten.threshold_backward(dy, y, 0)
    assert ref[n - 1] == 3.0  # torch passes the gradient at a NaN activation
    got = ops.relu_backward_(dy.clone().to(DEV), y.to(DEV))
    _bits_equal(got, ref, f"relu_backward_ n={n}")


# ------------------------------------------------------------------------ (b) relu_backward_split_

@pytest.mark.parametrize("with_split", [False, True])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 51), (16, 16), (1, 257)])
def test_relu_backward_split_bitwise_vs_threshold_backward(H, W, C, B, with_split):
    """y = hi + lo in the split layout (HW = 1, 255, 256, 257: one thread, a partial block, a full one, a
    second block): the fast path's split of a non-finite value (lo = NaN), ``store_gated_``'s (hi = value,
    lo = 0), a positive value with a negative lo, hi + lo = 0 exactly; the split copy of the masked gradient
    is the test's own encoding of it."""
    from mvdet_amd import ops
    g = torch.Generator().manual_seed(7 * H * W + C + B)
    y = _sprinkle(torch.randn((B, C, H, W), generator=g), SPECIAL, 3)
    dy = _sprinkle(torch.randn((B, C, H, W), generator=g), [NAN, INF, -INF], 5, 2)
    ys = _split_encode(y)  # NaN -> (NaN, NaN), +-inf -> (+-inf, NaN): what the fast path's split leaves
    last = H * W - 1

    def put(b, c, p, hi, lo):
        ys[b, c // 8, p // W, p % W, 0, c % 8] = hi
        ys[b, c // 8, p // W, p % W, 1, c % 8] = lo
        dy[b, c, p // W, p % W] = 3.0

    put(0, 1, last, NAN, 0.0)                    # store_gated_'s NaN: passes
    put(0, 2, last, 1.0, NAN)                    # a NaN left in lo alone: y is NaN, passes
    put(B - 1, 3, 0, INF, 0.0)                   # store_gated_'s +inf: passes
    put(B - 1, 4, 0, -INF, 0.0)                  # store_gated_'s -inf: no gradient
    put(B - 1, 5, last, 1.0078125, -2.0 ** -12)  # positive, lo negative: passes
    put(0, 6, 0, 2.0 ** -10, -2.0 ** -10)        # hi + lo = 0 exactly: no gradient
    put(0, 7, 0, -1.0, 2.0 ** -9)                # negative, lo positive: no gradient
    ydec = ops.split_decode(ys, C)               # plain torch on the CPU: hi + lo in fp32
    assert torch.isnan(ydec[0, 1].view(-1)[last]) and torch.isnan(ydec[0, 2].view(-1)[last])
    assert ydec[B - 1, 5].view(-1)[last] > 0 and ydec[0, 6, 0, 0] == 0 and ydec[0, 7, 0, 0] < 0
    ref = torch.ops.aten.threshold_backward(dy, ydec, 0)
    assert ref[0, 1].view(-1)[last] == 3.0 and ref[B - 1, 4, 0, 0] == 0 and ref[0, 6, 0, 0] == 0
    out = torch.full(ops.split_shape(B, C, H, W), 7.0, dtype=torch.bfloat16, device=DEV) if with_split else None
    got = ops.relu_backward_split_(dy.clone().to(DEV), ys.to(DEV), out)
    _bits_equal(got, ref, "relu_backward_split_")
    if with_split:
        _bits_equal(out, _split_encode(ref), "relu_backward_split_: dy_split")


# -------------------------------------------------------------------- (c) conv3x3_bias_coord_grad

def _coord_ref(dy, H, W, dil):
    """float64 [Cout, 2, 3, 3]: ``torch.nn.grad.conv2d_weight`` on ``cpu_path.coord_map`` (NaN where H == 1 /
    W == 1: create_coord_map divides 0 by 0), and the same over absolute values."""
    B, Co = dy.shape[:2]
    with np.errstate(invalid="ignore", divide="ignore"):
        cm = cpu_path.coord_map(H, W).double().repeat(B, 1, 1, 1)
    ref = torch.nn.grad.conv2d_weight(cm, (Co, 2, 3, 3), dy.double(), padding=dil, dilation=dil)
    ab = torch.nn.grad.conv2d_weight(cm.abs(), (Co, 2, 3, 3), dy.double().abs(), padding=dil, dilation=dil)
    return ref, ab


def _bias_coord_check(dy, dil, with_db, with_dw, coord_ch=0, cin_w=5, exact=False, what=""):
    from mvdet_amd import ops
    B, Co, H, W = dy.shape
    what = f"{what} B={B} Cout={Co} H={H} W={W} dil={dil} coord_ch={coord_ch}"
    db = torch.full((Co,), 5.0, device=DEV) if with_db else None
    dw = torch.full((Co, cin_w, 3, 3), 4.0, device=DEV) if with_dw else None
    ops.conv3x3_bias_coord_grad(dy.to(DEV), dil, db=db, dw=dw, coord_ch=coord_ch)
    n = B * H * W
    if with_db:
        _check_sum(db, dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3)), n, what + ": db", exact)
    if with_dw:
        ref, ab = _coord_ref(dy, H, W, dil)
        got = dw.cpu()
        _check_sum(got[:, coord_ch:coord_ch + 2], ref, ab, n, what + ": coord dw", exact)
        other = [c for c in range(cin_w) if c not in (coord_ch, coord_ch + 1)]
        assert (got[:, other] == 4.0).all(), what + ": dw written outside the coord channels"
        return got[:, coord_ch:coord_ch + 2]


@pytest.mark.parametrize("H", [1, 2, 13, 16, 17, 33])
def test_bias_coord_grad_with_dw_shapes(H):
    """Training's conv1 call (db + dw) at dilation 1 and 2: one row, a partial / full / second trip of the 16
    waves over the rows (H = 13, 16, 17, 33), a partial / full / second trip of the 256-column loop (W = 29
    .. 300), W == 1 / H == 1 (NaN coords, the reference's pattern), B 1 and 3, the coord channels first and
    last of 5.  Random dy under the bound; impulses (end of a row, column 256, row 16, the last pixel) exact."""
    k = 0
    for W in (1, 2, 29, 64, 65, 256, 257, 300):
        for dil in (1, 2):
            k += 1
            B, ch = (1, 3)[k % 2], (0, 3)[(k // 2) % 2]
            g = torch.Generator().manual_seed(1000 * H + 10 * W + dil)
            _bias_coord_check(torch.randn((B, 3, H, W), generator=g), dil, True, True, ch, what="random")
            pos = _positions(H * W, W, (256, 16 * W, 16 * W + W - 1, H * W - W))
            _bias_coord_check(_impulses(B, len(pos), H, W, pos), dil, True, True, ch, exact=True, what="impulse")


@pytest.mark.parametrize("dil", [1, 2])
def test_bias_coord_grad_dw_alone(dil):
    """``db=None``: the coord gradient alone (a pre-filled db-less call), random and impulse."""
    for B, H, W, ch in ((1, 17, 65, 0), (3, 13, 257, 3)):
        g = torch.Generator().manual_seed(H + W + dil)
        _bias_coord_check(torch.randn((B, 4, H, W), generator=g), dil, False, True, ch, what="random, dw alone")
        pos = _positions(H * W, W, (256, 16 * W))
        _bias_coord_check(_impulses(B, len(pos), H, W, pos), dil, False, True, ch, exact=True,
                          what="impulse, dw alone")


@pytest.mark.parametrize("H,W", [(1, 1), (3, 341), (32, 32), (25, 41), (65, 63), (64, 64), (17, 241), (50, 100)])
def test_bias_grad_db_alone(H, W):
    """Training's conv2 call (db alone: the 4x unrolled loop over 1024 threads + its scalar tail) at HW = 1,
    1023, 1024, 1025, 4095, 4096, 4097, 5000, dilation 1 and 2 (unused there), B 1 and 3; every impulse
    (around each 1024 / 4096 boundary and the boundary between unrolled and tail threads) sums to 1.0."""
    for B, dil in ((1, 2), (3, 1)):
        g = torch.Generator().manual_seed(H * W + B)
        _bias_coord_check(torch.randn((B, 3, H, W), generator=g), dil, True, False, what="random, db alone")
        pos = _positions(H * W, W)
        _bias_coord_check(_impulses(B, max(3, len(pos)), H, W, pos), dil, True, False, exact=True,
                          what="impulse, db alone")


@pytest.mark.parametrize("H,W,dil", [(1, 1, 1), (2, 2, 2), (13, 29, 29), (13, 29, 40), (1, 29, 29), (13, 1, 13),
                                     (13, 29, 13)])
def test_bias_coord_grad_taps_outside_are_exact_zeros(H, W, dil):
    """A dilation of at least W (H): every off-centre column (row) tap has no pixel inside, so its gradient is
    exactly 0 — also where the coord itself is NaN (H == 1 / W == 1): 0 terms, not NaN * 0."""
    g = torch.Generator().manual_seed(H + 31 * W + dil)
    got = _bias_coord_check(torch.randn((2, 3, H, W), generator=g), dil, True, True, 3, what="far taps")
    if dil >= W:
        assert (got[:, :, :, [0, 2]] == 0).all()
    if dil >= H:
        assert (got[:, :, [0, 2], :] == 0).all()
    centre = got[:, :, 1, 1]
    assert torch.equal(torch.isnan(centre[:, 0]), torch.full((3,), W == 1))
    assert torch.equal(torch.isnan(centre[:, 1]), torch.full((3,), H == 1))


def test_bias_coord_grad_table_limit():
    """The coord tables hold 4096 rows / columns: H = 4096 is served, H or W = 4097 with dw is refused with
    MVBEV_ERR_SHAPE and nothing written, and the same shapes with db alone (no table) are served."""
    from mvdet_amd import _native, ops
    g = torch.Generator().manual_seed(4096)
    _bias_coord_check(torch.randn((1, 1, 4096, 2), generator=g), 1, True, True, 0, cin_w=2, what="H = 4096")
    _bias_coord_check(_impulses(1, 1, 4096, 2, [4096 * 2 - 1]), 2, True, True, 0, cin_w=2, exact=True,
                      what="H = 4096, impulse")
    for H, W in ((4097, 2), (2, 4097)):
        dy = torch.randn((1, 3, H, W), generator=g)
        db, dw = torch.full((3,), 5.0, device=DEV), torch.full((3, 4, 3, 3), 4.0, device=DEV)
        with pytest.raises(_native.NativeError, match=rf"status {_native.ERR_SHAPE}\)"):
            ops.conv3x3_bias_coord_grad(dy.to(DEV), 1, db=db, dw=dw, coord_ch=2)
        torch.cuda.synchronize()
        assert (db == 5.0).all() and (dw == 4.0).all()
        _bias_coord_check(dy, 1, True, False, what="4097, db alone")
        pos = _positions(H * W, W)
        _bias_coord_check(_impulses(1, len(pos), H, W, pos), 2, True, False, exact=True,
                          what="4097, db alone, impulse")


# --------------------------------------------------------------------- (d) conv3x3_cout1_backward

def _cout1_ref(x, w, dmap, dil, relu_mask):
    """float64 autograd through F.conv2d: (dx, dw) and the same sums over absolute values; with
    ``relu_mask`` dx under ``threshold_backward`` on x (the ReLU's output)."""
    out = []
    for f in (lambda t: t.double(), lambda t: t.double().abs()):
        xr, wr = f(x).requires_grad_(), f(w).requires_grad_()
        F.conv2d(xr, wr, padding=dil, dilation=dil).backward(f(dmap))
        dx = torch.ops.aten.threshold_backward(xr.grad, x.double(), 0) if relu_mask else xr.grad
        out += [dx, wr.grad]
    return out[0], out[1], out[2], out[3]


def _cout1_check(x, w, dmap, dil, relu_mask, split=False, need_dx=True, need_dw=True, exact_dx=False,
                 exact_dw=False, what=""):
    from mvdet_amd import ops
    B, C, H, W = x.shape
    what = f"{what} B={B} C={C} H={H} W={W} dil={dil} relu_mask={relu_mask}"
    dxs = torch.full(ops.split_shape(B, C, H, W), 7.0, dtype=torch.bfloat16, device=DEV) if split else None
    dx, dw = ops.conv3x3_cout1_backward(x.to(DEV), w.to(DEV), dmap.to(DEV), dil, relu_mask=relu_mask,
                                        need_dx=need_dx, need_dw=need_dw, dx_split=dxs)
    rdx, rdw, adx, adw = _cout1_ref(x, w, dmap, dil, relu_mask)
    assert (dx is None) == (not need_dx) and (dw is None) == (not need_dw)
    if need_dx:
        _check_sum(dx, rdx, adx, 9, what + ": dx", exact_dx)
        if split:
            _bits_equal(dxs, _split_encode(dx.cpu()), what + ": dx_split")
    if need_dw:
        _check_sum(dw, rdw, adw, B * H * W, what + ": dw", exact_dw)


def _cout1_inputs(B, C, H, W, seed, relu):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, C, H, W), generator=g)
    return (F.relu(x) if relu else x), torch.randn((1, C, 3, 3), generator=g) * 0.1, \
        torch.randn((B, 1, H, W), generator=g)


@pytest.mark.parametrize("relu_mask", [False, True])
@pytest.mark.parametrize("C", [1, 7, 33, 40])
def test_cout1_backward_shapes(C, relu_mask):
    """C = 1, 7 (one partial block of 32), 33 (a full block + 1), 40 (+ 8: with ``dx_split``, whole groups of 8
    from the partial block); HW = 15 (3 x 5, smaller than dilation 4: of the off-centre taps only column 0 <-> 4 lands), 1024, 4096
    (one batch of 4 x 1024 pixels), 4097 (one pixel past it); dilation 1, 2, 4; B 1 and 3.  Random inputs
    under the bound; an x of impulses (exact dw) and a dmap of one impulse (exact dx and dw)."""
    k = 0
    for H, W in ((3, 5), (32, 32), (64, 64), (17, 241)):
        for dil in (1, 2, 4):
            k += 1
            B = (1, 3)[k % 2]
            x, w, dmap = _cout1_inputs(B, C, H, W, 100 * C + 10 * k + relu_mask, relu_mask)
            split = C % 8 == 0
            _cout1_check(x, w, dmap, dil, relu_mask, split, what="random")
            pos = _positions(H * W, W)
            _cout1_check(_impulses(B, C, H, W, pos[k % len(pos):] + pos[:k % len(pos)]), w, dmap, dil, relu_mask,
                         split, exact_dw=True, what="x impulses")
            d1 = torch.zeros_like(dmap)
            d1[B - 1].view(-1)[pos[k % len(pos)]] = 1.0
            _cout1_check(x, w, d1, dil, relu_mask, split, exact_dx=True, exact_dw=True, what="dmap impulse")


def test_cout1_backward_grid_smaller_than_the_dilation():
    """Dilation 4 on a 3 x 5 grid: the row taps fall outside (dw's rows ky = 0, 2 exactly 0; the column taps
    still pair column 0 with column 4); on 3 x 4 only the centre tap lands: the other 8 entries of dw are
    exactly 0 and dx is w's centre tap times dmap, one fp32 product."""
    from mvdet_amd import ops
    x, w, dmap = _cout1_inputs(2, 7, 3, 5, 5, True)
    dx, dw = ops.conv3x3_cout1_backward(x.to(DEV), w.to(DEV), dmap.to(DEV), 4, relu_mask=False)
    assert (dw.cpu()[0, :, [0, 2], :] == 0).all() and (dw.cpu()[0, :, 1, :] != 0).all()
    x, w, dmap = _cout1_inputs(2, 7, 3, 4, 6, True)
    dx, dw = ops.conv3x3_cout1_backward(x.to(DEV), w.to(DEV), dmap.to(DEV), 4, relu_mask=False)
    off = torch.ones(9, dtype=torch.bool)
    off[4] = False
    assert (dw.cpu().view(7, 9)[:, off] == 0).all() and (dw.cpu().view(7, 9)[:, 4] != 0).all()
    assert torch.equal(dx.cpu(), w[0, :, 1, 1].view(1, 7, 1, 1) * dmap)


@pytest.mark.parametrize("C", [7, 40])
def test_cout1_backward_one_output_alone(C):
    """``need_dx`` alone (with the split copy at C = 40) and ``need_dw`` alone: one launch each."""
    x, w, dmap = _cout1_inputs(3, C, 17, 33, C, True)
    _cout1_check(x, w, dmap, 2, True, C % 8 == 0, need_dw=False, what="dx alone")
    _cout1_check(x, w, dmap, 2, True, need_dx=False, what="dw alone")
    _cout1_check(_impulses(3, C, 17, 33, _positions(17 * 33, 33)), w, dmap, 4, False, need_dx=False, exact_dw=True,
                 what="dw alone, x impulses")


def test_cout1_backward_nonfinite_activations():
    """NaN and +-inf in x under ``relu_mask``: dx passes at NaN and +inf and is 0 at -inf
    (``threshold_backward``; the kernel's y > 0 dropped the NaN); dw is non-finite exactly in the reference's
    entries, signs included — a non-finite x in a corner reaches only the taps that land inside (torch's zero
    padding contributes no term, not x * 0)."""
    B, C, H, W = 2, 40, 13, 29
    x, w, dmap = _cout1_inputs(B, C, H, W, 77, True)
    x[0, 0, 0, 0] = NAN          # corner: 4 of 9 taps under dilation 4
    x[0, 1, 6, 14] = INF         # interior: every tap
    x[1, 2, 12, 28] = -INF       # the opposite corner
    x[1, 3, 5, 2] = NAN          # left edge
    x[1, 33, 0, 28] = INF        # the partial channel block
    rdx, rdw, _, _ = _cout1_ref(x, w, dmap, 4, True)
    assert torch.isfinite(rdx).all() and rdx[0, 0, 0, 0] != 0 and rdx[0, 1, 6, 14] != 0 and rdx[1, 2, 12, 28] == 0
    nf = ~torch.isfinite(rdw[0])
    assert int(nf[0].sum()) == 4 and nf[1].all() and int(nf[2].sum()) == 4 and int(nf[3].sum()) == 6 \
        and int(nf[33].sum()) == 4 and not nf[4:33].any()
    _cout1_check(x, w, dmap, 4, True, True, what="non-finite x")


# -------------------------------------------------------------------------------- (e) store_gated_

def _gate(open_):
    flag = torch.tensor([41], dtype=torch.int32, device=DEV)
    return (flag, 41 if open_ else 42)


def _store_src(B, C, H, W, seed, denormals):
    """A strided fp32 source view (every second channel, a row and column window) with non-finite values,
    signed zeros, tiny and huge ones."""
    g = torch.Generator().manual_seed(seed)
    big = torch.randn((B, 2 * C, H + 1, W + 3), generator=g)
    _sprinkle(big, [NAN, INF, -INF, 0.0, -0.0, 1e-30, -3e30] + ([1e-40, -1e-40] if denormals else []), 7, 1)
    src = big.to(DEV)[:, ::2, 1:, 2:2 + W]
    assert not src.is_contiguous() and src.stride(3) == 1
    return src


@pytest.mark.parametrize("open_", [True, False])
def test_store_gated_fp32_slice(open_):
    """A strided source into a channel slice and row window of a larger fp32 tensor: a bitwise copy with the
    gate open, the destination byte-identical to its pre-fill with the gate closed; the surroundings
    untouched either way."""
    from mvdet_amd import ops
    B, C, H, W = 2, 5, 7, 19
    src = _store_src(B, C, H, W, 1, denormals=True)
    big = torch.full((B, C + 3, H + 4, W), 7.0, device=DEV)
    ops.store_gated_(src, big[:, 1:1 + C, 2:2 + H], _gate(open_))
    want = torch.full((B, C + 3, H + 4, W), 7.0)
    if open_:
        want[:, 1:1 + C, 2:2 + H] = src.cpu()
    _bits_equal(big, want, f"store_gated_ fp32 slice, gate open={open_}")


@pytest.mark.parametrize("open_", [True, False])
@pytest.mark.parametrize("C", [8, 13, 24])
def test_store_gated_split_slab_slice(C, open_):
    """Into the split layout, as group / row slices of a larger slab: finite values in the test's own split
    encoding, non-finite ones as hi = value, lo = 0, the channels past C of the last group (C = 13) zero;
    closed gate and surroundings untouched."""
    from mvdet_amd import ops
    B, H, W = 2, 6, 11
    G = -(-C // 8)
    src = _store_src(B, C, H, W, C, denormals=False)
    slab = torch.full((B, G + 2, H + 3, W, 2, 8), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.store_gated_(src, slab[:, 1:1 + G, 2:2 + H], _gate(open_))
    want = torch.full((B, G + 2, H + 3, W, 2, 8), 7.0, dtype=torch.bfloat16)
    if open_:
        enc = _split_encode(src.cpu(), keep_nonfinite=True)
        nonfin = ~torch.isfinite(enc[..., 0, :].float())
        assert nonfin.any() and (enc[..., 1, :][nonfin] == 0).all()
        if C % 8:
            assert (enc[:, -1, :, :, :, C % 8:] == 0).all()
        want[:, 1:1 + G, 2:2 + H] = enc
    _bits_equal(slab, want, f"store_gated_ split C={C}, gate open={open_}")
    if open_:  # hi + lo is the value wherever it is not finite: the backward's mask reads it
        dec = ops.split_decode(slab[:, 1:1 + G, 2:2 + H].contiguous(), C).cpu()
        s = src.cpu()
        bad = ~torch.isfinite(s)
        assert torch.equal(torch.isnan(dec[bad]), torch.isnan(s[bad]))
        assert torch.equal(dec[bad & ~torch.isnan(s)], s[bad & ~torch.isnan(s)])


def test_store_gated_grid_stride_wrap():
    """More than 8192 x 256 stored elements (the launch is capped at 8192 blocks): the grid-stride loop's
    second trip stores the rest."""
    from mvdet_amd import ops
    B, C, H, W = 1, 8, 520, 512
    assert B * C * H * W > 8192 * 256
    src = torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(3)).to(DEV)
    dst = torch.full((B, C, H, W), 7.0, device=DEV)
    ops.store_gated_(src, dst, _gate(True))
    assert torch.equal(dst.view(torch.int32), src.view(torch.int32))


def test_store_gated_refusals():
    """By status code: a source whose column stride is not 1, a split destination off its 16-byte alignment,
    a NULL gate; nothing is written."""
    from mvdet_amd import _native, ops
    B, C, H, W = 1, 8, 4, 6
    src2 = torch.randn((B, C, H, 2 * W), device=DEV)
    dst = torch.full((B, C, H, W), 7.0, device=DEV)
    flag, tag = _gate(True)
    lib = _native.load()
    st = lib.mvbev_store_gated_f32(src2.data_ptr(), _native._i64x4(*src2[..., ::2].stride()), dst.data_ptr(),
                                   _native._i64x4(*dst.stride()), B, C, H, W, _native.LAYOUT_F32, flag.data_ptr(),
                                   tag, None)
    assert st == -3  # MVBEV_ERR_STRIDE
    src = src2[..., :W]
    buf = torch.full((B * H * W * 16 + 8,), 7.0, dtype=torch.bfloat16, device=DEV)
    off = buf[4:4 + B * H * W * 16].view(ops.split_shape(B, C, H, W))  # 8 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 8
    with pytest.raises(_native.NativeError, match=r"status -4\)"):  # MVBEV_ERR_ALIGN
        ops.store_gated_(src, off, (flag, tag))
    with pytest.raises(_native.NativeError, match=r"status -5\)"):  # MVBEV_ERR_NULL
        ops.store_gated_(src, dst, None)
    torch.cuda.synchronize()
    assert (dst == 7.0).all() and (buf == 7.0).all()


# ------------------------------------------------------- (f) the gated fp32 pack and row transform

def test_gated_fp32_pack():
    """``PackedConv3x3.get_gated``: the ungated pack bit for bit with the gate open, the buffer untouched with
    it closed."""
    from mvdet_amd import ops
    g = torch.Generator().manual_seed(9)
    w = (torch.randn((128, 11, 3, 3), generator=g) * 0.1).to(DEV)
    cmap = [10, 3, -1, 7, 0, 5, 1, 2, 9]
    want = ops.PackedConv3x3(cmap, "fp32").get(w).clone()
    pk = ops.PackedConv3x3(cmap, "fp32")
    got = pk.get_gated(w, _gate(True))
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))
    got.fill_(7.0)
    w2 = (torch.randn((128, 11, 3, 3), generator=g) * 0.1).to(DEV)
    again = pk.get_gated(w2, _gate(False))
    assert again.data_ptr() == got.data_ptr() and (again == 7.0).all()


def test_gated_wino_rows():
    """The gated row transform: the ungated call's T bit for bit with the gate open, T untouched with it
    closed."""
    from mvdet_amd import ops
    g = torch.Generator().manual_seed(10)
    B, C, H, W = 2, 16, 13, 40
    xs = _split_encode(torch.randn((B, C, H, W), generator=g)).to(DEV)
    d = ops.conv_desc(B, C, H, W, group=C, group_stride=0, batch_stride=C * H * W)
    n = (ops.wino_rows_bytes(d) + 1) // 2
    want = ops.wino_rows(xs, d, torch.zeros(n, dtype=torch.bfloat16, device=DEV))
    got = ops.wino_rows(xs, d, torch.zeros(n, dtype=torch.bfloat16, device=DEV), gate=_gate(True))
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and (want != 0).any()
    kept = ops.wino_rows(xs, d, torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV), gate=_gate(False))
    assert (kept == 7.0).all()
