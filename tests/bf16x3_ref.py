"""The 3xbf16 arithmetic of the backward conv kernels restated on the CPU, with its localized lapses.

No GPU and nothing from the library under test.  An operand is split ``x = hi + lo`` (``split``: round to
nearest even, ``hi = bf16(x)``, ``lo = bf16(x - hi)``, the encoding ``mvbev_split_rows_bf16`` pins) and a
product of two operands is the three bf16 passes ``hi*lo + lo*hi + hi*hi``; a product of two bf16 values
is exact in fp32, so the only rounding is the fp32 accumulation, as in the kernels.  Each ``emulate_*``
sums three fp32 torch-CPU evaluations of the same linear map, one per pass.  The row-Winograd forms run
their transforms (``F33``: B^T on the data rows, A^T on the gradient rows, G on the weights) in fp32 before
the split and fold the 5 transformed points back afterwards, as the kernels do.

``lapse`` names one localized defect, applied by zeroing a part of ONE ``lo`` operand (the pass that reads
it then misses there):

=========  ==========================================================================================
lapse      what is zeroed
=========  ==========================================================================================
tap        the ``lo`` weight of tap (0, 0) (dgrad); the whole ``lo`` of the transformed point xi = 0 (Winograd
           forms: of G w in a data gradient, of B^T x in a weight gradient)
kstep      the ``lo`` weight of the last 16 reduction channels (dgrad forms)
row        the ``lo`` of the last image row (of the row tile that holds it: Winograd forms)
segment    the ``lo`` of the last ``W % 32 or 32`` columns
batch      the ``lo`` of the last batch item (wgrad forms, B > 1)
lolo       ``lo*lo`` where ``lo*hi`` belongs: in tap (0, 0) / point 0 (dgrad forms), in the last row
           (tile) (wgrad forms)
=========  ==========================================================================================

In a weight gradient the lapsed operand is the activation x (the ``lo*hi`` pass); in a data gradient the
weight for tap / kstep / lolo and dy for row / segment.

``GATES`` pins, per kernel form and case of the GPU tests, the normwise gate that
``test_backward_gates_host.py`` proves discriminating on the GPU tests' own inputs:
``3 * e_int <= GATE <= min(e_lapse) / 3`` with ``e_int`` the error of the intended emulation against float64
torch and ``e_lapse`` that of each lapse that applies (both max|d| / max|ref|, per slice where the GPU test
gates per slice).  The GPU tests look the number up (``pinned_gate``) and compute no emulation.

Measured windows (``python -m pytest tests/test_backward_gates_host.py -s`` prints them):

key                                    e_int     min(e_lapse)          GATE
wgrad/1-64-12-36-d1                    5.5e-06   0.000747 (segment)    5e-5
wgrad/2-136-17-37-d2                   5.94e-06  0.00075 (row)         5e-5
wgrad/1-512-30-90-d2                   5.86e-06  0.00052 (lolo)        5e-5
wgrad/1-24-5-70-d1                     5.66e-06  0.000846 (segment)    5e-5
wgrad/2-72-13-44-d2                    5.03e-06  0.000715 (row)        5e-5
wgrad/2-72-13-44-d1                    5.44e-06  0.000781 (row)        5e-5
wgrad_presplit/1-64-12-40-d1           5.2e-06   0.000664 (lolo)       5e-5
wgrad_presplit/2-72-13-48-d2           5.24e-06  0.00058 (lolo)        5e-5
wgrad_presplit/2-192-37-96-d1          5.67e-06  0.000405 (row)        5e-5
wgrad_grouped                          6.06e-06  0.000742 (row)        5e-5
wgrad_frustum                          6.03e-06  0.000396 (row)        5e-5
dgrad/1-128-40-12-36-d1                4.1e-06   0.00057 (tap)         5e-5
dgrad/2-512-512-17-37-d2               4.65e-06  0.000346 (kstep)      5e-5
dgrad/1-256-200-9-64-d1                5.69e-06  0.000564 (kstep)      5e-5
dgrad_ring/1-128-40-25-36-d1           4.65e-06  0.000609 (tap)        5e-5
dgrad_ring/2-512-512-17-37-d2          4.48e-06  0.00031 (kstep)       5e-5
dgrad_ring/1-256-200-9-64-d1           4.09e-06  0.00044 (kstep)       5e-5
dgrad_ring/1-128-72-14-37-d1           4.26e-06  0.000561 (tap)        5e-5
dgrad_ring/1-128-72-14-37-d2           4.6e-06   0.000595 (kstep)      5e-5
dgrad_ring_pieces/0                    6.98e-06  0.000638 (tap)        5e-5
dgrad_ring_pieces/3                    6.86e-06  0.000644 (kstep)      5e-5
dgrad_chanmap                          5.66e-06  0.000592 (kstep)      5e-5
wino_dgrad2/1-128-25-36-w0             1.4e-05   0.00117 (row)         8e-5
wino_dgrad2/1-128-25-36-w1             1.62e-05  0.00124 (row)         8e-5
wino_dgrad2/2-512-17-70-w0             1.48e-05  0.00115 (kstep)       8e-5
wino_dgrad2/2-512-17-70-w1             1.42e-05  0.00135 (kstep)       8e-5
wino_dgrad2/1-128-14-40-w0             1.53e-05  0.00138 (tap)         8e-5
wino_dgrad2/1-128-14-40-w1             1.94e-05  0.00138 (lolo)        8e-5
wino_dgrad1/1-128-256-25-70-split      1.44e-05  0.00128 (row)         8e-5
wino_dgrad1/1-128-256-25-70-f32        1.61e-05  0.00136 (row)         8e-5
wino_dgrad1/2-256-384-14-40-split      1.49e-05  0.00139 (tap)         8e-5
wino_dgrad1/2-256-384-14-40-f32        1.47e-05  0.0014 (lolo)         8e-5
wino_dgrad1/1-512-256-13-40-split      1.55e-05  0.00106 (kstep)       8e-5
wino_dgrad1/1-512-256-13-40-f32        1.51e-05  0.00104 (kstep)       8e-5
wino_wgrad/1-64-12-64-d1               1.71e-05  0.00154 (tap)         8e-5
wino_wgrad/2-72-17-40-d1               1.22e-05  0.00111 (lolo)        8e-5
wino_wgrad/1-256-31-96-d1              1.27e-05  0.000433 (lolo)       8e-5
wino_wgrad/2-128-25-200-d1             1.45e-05  0.000458 (row)        8e-5
wino_wgrad/1-64-5-40-d1                1.25e-05  0.00159 (tap)         8e-5
wino_wgrad/1-64-12-64-d2               1.47e-05  0.00151 (tap)         8e-5
wino_wgrad/2-72-17-40-d2               1.34e-05  0.00166 (tap)         8e-5
wino_wgrad/1-256-31-96-d2              1.52e-05  0.000451 (lolo)       8e-5
wino_wgrad/2-128-25-200-d2             1.37e-05  0.00045 (lolo)        8e-5
wino_wgrad/1-64-5-40-d2                1.36e-05  0.00242 (tap)         8e-5
wino_wgrad_grouped                     1.67e-05  0.000425 (lolo)       8e-5

The direct forms share the project's forward 3xbf16 gate, 5e-5; their window over all keys is [2.1e-5, 1.0e-4].
The Winograd forms' transforms add about twice the rounding again (e_int 1.2 - 1.9e-5, as
``tools/wino_error.py`` shows for the forward): their window is [5.9e-5, 1.4e-4] and they are pinned at 8e-5.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

# ------------------------------------------------------------------ shared with tools/wino_error.py

F33 = dict(
    m=3,
    BT=np.array([[2, -1, -2, 1, 0], [0, -2, -1, 1, 0], [0, 2, -3, 1, 0], [0, -1, 0, 1, 0], [0, 2, -1, -2, 1]], float),
    G=np.array([[1 / 2, 0, 0], [-1 / 2, -1 / 2, -1 / 2], [-1 / 6, 1 / 6, -1 / 6], [1 / 6, 1 / 3, 2 / 3], [0, 0, 1]]),
    AT=np.array([[1, 1, 1, 1, 0], [0, 1, -1, 2, 0], [0, 1, 1, 4, 1]], float),
)
F43 = dict(
    m=4,
    BT=np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0],
                 [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], float),
    G=np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
                [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]),
    AT=np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], float),
)


def bf16_np(x):
    """Round-to-nearest-even fp32 -> bf16 (as float32 values), numpy."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split_np(x):
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_np(x)
    return hi, bf16_np(x - hi)


def mm3(a_hi, a_lo, b_hi, b_lo):
    """[M, K] x [K, N] as the 3 bf16 products accumulated in fp32 (16-deep MFMA chunks, in K order)."""
    K = a_hi.shape[1]
    acc = np.zeros((a_hi.shape[0], b_hi.shape[1]), np.float32)
    for k0 in range(0, K, 16):
        s = slice(k0, k0 + 16)
        for a, b in ((a_hi, b_lo), (a_lo, b_hi), (a_hi, b_hi)):  # the kernels' pass order
            acc = (acc + (a[:, s].astype(np.float64) @ b[s].astype(np.float64)).astype(np.float32)).astype(np.float32)
    return acc


# ------------------------------------------------------------------ the split and the three passes (torch)

def split(x: torch.Tensor):
    """x -> (hi, lo), both bf16 values held in fp32: hi = bf16(x), lo = bf16(x - hi), round to nearest even."""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def _three(op, a, b, a_lolo=None):
    """op(a, b) of the split pairs a = (hi, lo), b = (hi, lo) in the kernels' pass order hi*lo + lo*hi + hi*hi,
    each pass one fp32 evaluation.  ``a_lolo``: a part of a's lo that multiplies b's lo instead of b's hi (the
    "lolo" lapse; the caller has removed that part from a's lo)."""
    r = op(a[0], b[1]) + op(a[1], b[0])
    if a_lolo is not None:
        r = r + op(a_lolo, b[1])
    return r + op(a[0], b[0])


def _zeroed(t, index):
    t = t.clone()
    t[index] = 0
    return t


def _only(t, index):
    r = torch.zeros_like(t)
    r[index] = t[index]
    return r


def _seg(W):
    return slice(W - (W % 32 or 32), W)


def _check(lapse, allowed):
    if lapse is not None and lapse not in allowed:
        raise ValueError(f"lapse {lapse!r} does not apply here (one of {allowed})")


WGRAD_LAPSES = ("row", "segment", "batch", "lolo")
DGRAD_LAPSES = ("tap", "kstep", "row", "segment", "lolo")
WINO_WGRAD_LAPSES = ("tap", "row", "segment", "batch", "lolo")
WINO_DGRAD_LAPSES = DGRAD_LAPSES


def emulate_wgrad(x, dy, dil, lapse=None):
    """dw [Cout, K, 3, 3] of a 3x3 conv (padding = dilation = dil) from x [B, K, H, W] and dy [B, Cout, H, W]."""
    _check(lapse, WGRAD_LAPSES)
    B, K, H, W = x.shape
    cout = dy.shape[1]
    (xh, xl), d = split(x), split(dy)
    lolo = None
    if lapse == "row":
        xl = _zeroed(xl, (..., H - 1, slice(None)))
    elif lapse == "segment":
        xl = _zeroed(xl, (..., _seg(W)))
    elif lapse == "batch":
        if B < 2:
            raise ValueError("the batch lapse needs B > 1")
        xl = _zeroed(xl, (B - 1,))
    elif lapse == "lolo":
        idx = (..., H - 1, slice(None))
        lolo, xl = _only(xl, idx), _zeroed(xl, idx)
    return _three(lambda a, b: conv2d_weight(a, (cout, K, 3, 3), b, padding=dil, dilation=dil), (xh, xl), d, lolo)


def emulate_dgrad(w, dy, dil, lapse=None, split_out=False):
    """dx [B, K, H, W] from the forward weight w [Cw, K, 3, 3] and dy [B, Cw, H, W]; ``split_out``: the result
    rounded to the split-bf16 encoding (hi + lo), as a kernel writing that layout leaves it."""
    _check(lapse, DGRAD_LAPSES)
    B, Cw, H, W = dy.shape
    K = w.shape[1]
    (wh, wl), (dh, dl) = split(w), split(dy)
    lolo = None
    if lapse == "tap":
        wl = _zeroed(wl, (..., 0, 0))
    elif lapse == "kstep":
        wl = _zeroed(wl, (slice(Cw - 16, Cw),))
    elif lapse == "row":
        dl = _zeroed(dl, (..., H - 1, slice(None)))
    elif lapse == "segment":
        dl = _zeroed(dl, (..., _seg(W)))
    elif lapse == "lolo":
        lolo, wl = _only(wl, (..., 0, 0)), _zeroed(wl, (..., 0, 0))
    r = _three(lambda a, b: conv2d_input((B, K, H, W), a, b, padding=dil, dilation=dil), (wh, wl), (dh, dl), lolo)
    return sum(split(r)) if split_out else r


# ------------------------------------------------------------------ row-Winograd F(3,3) forms

def wino_tile_bases(H, dil):
    """First output row of every 3-row tile: rows base + dil * i (i < 3).  Dilation 2 interleaves two pairs of
    tiles in each 12 rows (bases 0, 1, 6, 7)."""
    if dil == 1:
        return [3 * r for r in range(-(-H // 3))]
    return [12 * (r // 4) + (0, 1, 6, 7)[r % 4] for r in range(4 * (-(-H // 12)))]


def _gather_rows(x, rows):
    """x [..., H, W] -> [..., len(rows), W], zero where a row is outside the image."""
    H = x.shape[-2]
    ok = torch.tensor([0 <= r < H for r in rows])
    g = x[..., [min(max(r, 0), H - 1) for r in rows], :]
    return g * ok.to(x.dtype)[:, None]


def _apply(mat_row, parts):
    """sum_m mat_row[m] * parts[m] in fp32, left to right, zero coefficients skipped."""
    acc = None
    for c, p in zip(mat_row, parts):
        if c == 0:
            continue
        t = p * np.float32(c)
        acc = t if acc is None else acc + t
    return acc


def _bt_rows(d, bases, dil):
    """T[xi] [B, C, R3, W] = (B^T d)[xi] in fp32 over the 5 input rows base + dil * (m - 1) of every tile."""
    rows = [_gather_rows(d, [b + dil * (m - 1) for b in bases]) for m in range(5)]
    return [_apply(F33["BT"][xi], rows) for xi in range(5)]


def _at_rows(dy, bases, dil):
    """D[xi] [B, C, R3, W] = sum_j A^T[j][xi] dy[base + dil * j] in fp32."""
    rows = [_gather_rows(dy, [b + dil * j for b in bases]) for j in range(3)]
    return [_apply(F33["AT"][:, xi], rows) for xi in range(5)]


def _last_tile(H, bases, dil):
    return next(i for i, b in enumerate(bases) if (H - 1 - b) % dil == 0 and 0 <= (H - 1 - b) // dil < 3)


def emulate_wino_conv(wt, x, dil, lapse=None, split_out=False):
    """The row-Winograd conv y [B, O, H, W] of x [B, C, H, W] (given split: hi + lo) with wt [O, C, 3, 3],
    padding = dilation = dil: T = B^T x per 3-row tile, U = G wt (float64, rounded to fp32), both split, the
    three passes per point as a 1 x 3 conv along the columns, then A^T."""
    _check(lapse, WINO_DGRAD_LAPSES)
    B, C, H, W = x.shape
    bases = wino_tile_bases(H, dil)
    T = _bt_rows(sum(split(x)), bases, dil)
    U = torch.einsum("xh,ochw->xocw", torch.from_numpy(F33["G"]), wt.double()).float()  # [5, O, C, 3]
    last = _last_tile(H, bases, dil)
    M = []
    for xi in range(5):
        (th, tl), (uh, ul) = split(T[xi]), split(U[xi][:, :, None, :])
        lolo = None
        if lapse == "tap" and xi == 0:
            ul = torch.zeros_like(ul)
        elif lapse == "kstep":
            ul = _zeroed(ul, (slice(None), slice(C - 16, C)))
        elif lapse == "row":
            tl = _zeroed(tl, (..., last, slice(None)))
        elif lapse == "segment":
            tl = _zeroed(tl, (..., _seg(W)))
        elif lapse == "lolo" and xi == 0:
            lolo, ul = ul, torch.zeros_like(ul)
        M.append(_three(lambda a, b: F.conv2d(b, a, padding=(0, dil), dilation=(1, dil)), (uh, ul), (th, tl), lolo))
    y = torch.zeros((B, wt.shape[0], H, W))
    for i in range(3):
        yi = _apply(F33["AT"][i], M)
        for r3, b in enumerate(bases):
            if b + dil * i < H:
                y[:, :, b + dil * i] = yi[:, :, r3]
    return sum(split(y)) if split_out else y


def emulate_wino_dgrad(w, dy, dil, lapse=None, split_out=False):
    """The data gradient as the row-Winograd conv of dy with the forward weight w [Cw, K, 3, 3] swapped and its
    taps reversed."""
    return emulate_wino_conv(w.flip(2, 3).transpose(0, 1), dy, dil, lapse, split_out)


def emulate_wino_wgrad(x, dy, dil, lapse=None):
    """dw from T = B^T x (x given split) and D = A^T-transformed dy rows, both split: M[xi][kw] the three passes
    summed over batch, tiles and columns, folded with G in float64 and rounded once."""
    _check(lapse, WINO_WGRAD_LAPSES)
    B, K, H, W = x.shape
    cout = dy.shape[1]
    bases = wino_tile_bases(H, dil)
    T = _bt_rows(sum(split(x)), bases, dil)
    D = _at_rows(dy.float(), bases, dil)
    last = _last_tile(H, bases, dil)
    M = []
    for xi in range(5):
        (th, tl), d = split(T[xi]), split(D[xi])
        lolo = None
        if lapse == "tap" and xi == 0:
            tl = torch.zeros_like(tl)
        elif lapse == "row":
            tl = _zeroed(tl, (..., last, slice(None)))
        elif lapse == "segment":
            tl = _zeroed(tl, (..., _seg(W)))
        elif lapse == "batch":
            if B < 2:
                raise ValueError("the batch lapse needs B > 1")
            tl = _zeroed(tl, (B - 1,))
        elif lapse == "lolo":
            idx = (..., last, slice(None))
            lolo, tl = _only(tl, idx), _zeroed(tl, idx)
        M.append(_three(lambda a, b: conv2d_weight(a, (cout, K, 1, 3), b, padding=(0, dil), dilation=(1, dil)),
                        (th, tl), d, lolo))
    Mx = torch.stack(M).double()[:, :, :, 0]  # [5, Cout, K, kw]
    return torch.einsum("xh,xocw->ochw", torch.from_numpy(F33["G"]), Mx).float()


# ------------------------------------------------------------------ the pinned gates

DIRECT = 5e-5  # the project's forward 3xbf16 gate (tests/test_gpu_parity.py CONV_TOL["bf16x3"])
# the Winograd forms' own window is [5.9e-5, 1.4e-4] over their keys (3 * max e_int, min e_lapse / 3): its middle
WINO = 8e-5

GATES = {
    "wgrad/1-64-12-36-d1": DIRECT,
    "wgrad/2-136-17-37-d2": DIRECT,
    "wgrad/1-512-30-90-d2": DIRECT,
    "wgrad/1-24-5-70-d1": DIRECT,
    "wgrad/2-72-13-44-d2": DIRECT,
    "wgrad/2-72-13-44-d1": DIRECT,
    "wgrad_presplit/1-64-12-40-d1": DIRECT,
    "wgrad_presplit/2-72-13-48-d2": DIRECT,
    "wgrad_presplit/2-192-37-96-d1": DIRECT,
    "wgrad_grouped": DIRECT,
    "wgrad_frustum": DIRECT,
    "dgrad/1-128-40-12-36-d1": DIRECT,
    "dgrad/2-512-512-17-37-d2": DIRECT,
    "dgrad/1-256-200-9-64-d1": DIRECT,
    "dgrad_ring/1-128-40-25-36-d1": DIRECT,
    "dgrad_ring/2-512-512-17-37-d2": DIRECT,
    "dgrad_ring/1-256-200-9-64-d1": DIRECT,
    "dgrad_ring/1-128-72-14-37-d1": DIRECT,
    "dgrad_ring/1-128-72-14-37-d2": DIRECT,
    "dgrad_ring_pieces/0": DIRECT,
    "dgrad_ring_pieces/3": DIRECT,
    "dgrad_chanmap": DIRECT,
    "wino_dgrad2/1-128-25-36-w0": WINO,
    "wino_dgrad2/1-128-25-36-w1": WINO,
    "wino_dgrad2/2-512-17-70-w0": WINO,
    "wino_dgrad2/2-512-17-70-w1": WINO,
    "wino_dgrad2/1-128-14-40-w0": WINO,
    "wino_dgrad2/1-128-14-40-w1": WINO,
    "wino_dgrad1/1-128-256-25-70-split": WINO,
    "wino_dgrad1/1-128-256-25-70-f32": WINO,
    "wino_dgrad1/2-256-384-14-40-split": WINO,
    "wino_dgrad1/2-256-384-14-40-f32": WINO,
    "wino_dgrad1/1-512-256-13-40-split": WINO,
    "wino_dgrad1/1-512-256-13-40-f32": WINO,
    "wino_wgrad/1-64-12-64-d1": WINO,
    "wino_wgrad/2-72-17-40-d1": WINO,
    "wino_wgrad/1-256-31-96-d1": WINO,
    "wino_wgrad/2-128-25-200-d1": WINO,
    "wino_wgrad/1-64-5-40-d1": WINO,
    "wino_wgrad/1-64-12-64-d2": WINO,
    "wino_wgrad/2-72-17-40-d2": WINO,
    "wino_wgrad/1-256-31-96-d2": WINO,
    "wino_wgrad/2-128-25-200-d2": WINO,
    "wino_wgrad/1-64-5-40-d2": WINO,
    "wino_wgrad_grouped": WINO,
}


def pinned_gate(key: str) -> float:
    return GATES[key]
