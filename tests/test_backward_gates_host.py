"""Host proof that the gates of the backward conv tests discriminate (no GPU).

For every (kernel form, case) that ``test_gpu_backward.py`` and ``test_gpu_wgrad_wino.py`` gate with
``bf16x3_ref.pinned_gate``, on the very inputs of the GPU test (``backward_cases``):

    3 * e_int <= GATE <= min(e_lapse) / 3

``e_int``: the intended 3xbf16 arithmetic (``bf16x3_ref.emulate_*``) against float64 torch; ``e_lapse``: the same
with one localized lapse (a ``lo`` pass missing in a tap, a K step, the last row, the last column segment, the
last batch item, or ``lo*lo`` where ``lo*hi`` belongs).  Both in the measure the GPU test uses: max|d| / max|ref|
over the tensor, or per (channel slot, tap) / per channel where the GPU test gates per slice.  A correct kernel
therefore passes with a factor 3 to spare and a kernel with any of these lapses fails by a factor 3.
``-s`` shows the window of every key.
"""
import pytest
import torch
from torch.nn.grad import conv2d_input, conv2d_weight

import backward_cases as bc
import bf16x3_ref as br
from helpers import parity_stats, parity_stats_sliced


def _global(got, ref):
    return parity_stats(got, ref)["normwise"]


def _window(key, ref, emulate, lapses, measure):
    gate = br.pinned_gate(key)
    e_int = measure(emulate(None), ref)
    e_lapse = {l: measure(emulate(l), ref) for l in lapses}
    worst = min(e_lapse, key=e_lapse.get)
    print(f"\n[window] {key}: e_int {e_int:.3g}  3*e_int {3 * e_int:.3g} <= GATE {gate:.3g} <= "
          f"min(e_lapse)/3 {e_lapse[worst] / 3:.3g}  (min e_lapse {e_lapse[worst]:.3g}: {worst}; " +
          ", ".join(f"{l} {e:.3g}" for l, e in e_lapse.items()) + ")")
    assert 3 * e_int <= gate <= e_lapse[worst] / 3, (key, e_int, gate, e_lapse)


def _wgrad_ref(x, dy, dil):
    return conv2d_weight(x.double(), (dy.shape[1], x.shape[1], 3, 3), dy.double(), padding=dil, dilation=dil)


def _dgrad_ref(w, dy, dil):
    B, _, H, W = dy.shape
    return conv2d_input((B, w.shape[1], H, W), w.double(), dy.double(), padding=dil, dilation=dil)


def _wgrad_lapses(B, wino=False):
    names = br.WINO_WGRAD_LAPSES if wino else br.WGRAD_LAPSES
    return [l for l in names if l != "batch" or B > 1]


# ------------------------------------------------------------------ direct weight gradients

@pytest.mark.parametrize("B,K,H,W,dil", bc.WGRAD_CASES)
def test_wgrad_window(B, K, H, W, dil):
    x, dy = bc.wgrad_inputs(B, K, H, W, dil)
    slots = bc.channel_tiles(K)
    _window(bc.key_wgrad(B, K, H, W, dil), _wgrad_ref(x, dy, dil), lambda l: br.emulate_wgrad(x, dy, dil, l),
            _wgrad_lapses(B), lambda a, b: bc.wgrad_error(a, b, slots))


@pytest.mark.parametrize("B,K,H,W,dil,lists", bc.PRESPLIT_CASES)
def test_wgrad_presplit_window(B, K, H, W, dil, lists):
    x, dy = bc.presplit_inputs(B, K, H, W, dil)
    slots = bc.channel_tiles(K)
    _window(bc.key_presplit(B, K, H, W, dil, lists), _wgrad_ref(x, dy, dil),
            lambda l: br.emulate_wgrad(x, dy, dil, l), _wgrad_lapses(B), lambda a, b: bc.wgrad_error(a, b, slots))


def test_wgrad_grouped_window():
    (S, B, C, Cs, H, W), _, x, dy = bc.grouped_inputs()
    slots = [slice(s * C, (s + 1) * C) for s in range(S)]  # per camera slot, in the module's column order
    _window(bc.KEY_GROUPED, _wgrad_ref(x, dy, 1), lambda l: br.emulate_wgrad(x, dy, 1, l), _wgrad_lapses(B),
            lambda a, b: bc.wgrad_error(a, b, slots))


def test_wgrad_frustum_window():
    (S, B, Cs, H, W), _, x, dy = bc.frustum_inputs()
    slots = [slice(s * Cs, (s + 1) * Cs) for s in range(S)]
    _window(bc.KEY_FRUSTUM, _wgrad_ref(x, dy, 1), lambda l: br.emulate_wgrad(x, dy, 1, l), _wgrad_lapses(B),
            lambda a, b: bc.wgrad_error(a, b, slots))


# ------------------------------------------------------------------ direct data gradients

@pytest.mark.parametrize("B,Cw,K,H,W,dil", bc.DGRAD_CASES)
def test_dgrad_window(B, Cw, K, H, W, dil):
    w, dy = bc.dgrad_inputs(B, Cw, K, H, W, dil)
    _window(bc.key_dgrad(B, Cw, K, H, W, dil), _dgrad_ref(w, dy, dil), lambda l: br.emulate_dgrad(w, dy, dil, l),
            br.DGRAD_LAPSES, _global)


@pytest.mark.parametrize("B,Cw,K,H,W,dil", bc.DGRAD_RING_CASES)
def test_dgrad_ring_window(B, Cw, K, H, W, dil):
    w, dy = bc.dgrad_inputs(B, Cw, K, H, W, dil, ring=True)
    _window(bc.key_dgrad_ring(B, Cw, K, H, W, dil), _dgrad_ref(w, dy, dil),
            lambda l: br.emulate_dgrad(w, dy, dil, l), br.DGRAD_LAPSES, _global)


@pytest.mark.parametrize("pieces", [p for p in bc.RING_PIECES if p != 1])  # pieces = 1 is compared bitwise
def test_dgrad_ring_pieces_window(pieces):
    """The split-bf16 output of the scheduled ring kernel (the GPU test compares it with the plain launch's, both
    within this error of the float64 result)."""
    _, dy, w = bc.ring_pieces_inputs(pieces)
    _window(bc.key_ring_pieces(pieces), _dgrad_ref(w, dy, 1),
            lambda l: br.emulate_dgrad(w, dy, 1, l, split_out=True), br.DGRAD_LAPSES, _global)


def test_dgrad_chanmap_window():
    w, dy, cmap = bc.chanmap_inputs()
    cols = [c for c in cmap if c >= 0]
    _window(bc.KEY_CHANMAP, _dgrad_ref(w, dy, 1)[:, cols], lambda l: br.emulate_dgrad(w, dy, 1, l)[:, cols],
            br.DGRAD_LAPSES, lambda a, b: parity_stats_sliced(a, b, dims=(0, 2, 3))["normwise"])


# ------------------------------------------------------------------ row-Winograd forms

@pytest.mark.parametrize("B,C,H,W", bc.CONV2_WINO_DGRAD_CASES)
def test_conv2_wino_dgrad_window(B, C, H, W):
    for it, (w, dy) in enumerate(bc.conv2_wino_dgrad_inputs(B, C, H, W)):
        _window(bc.key_conv2_wino_dgrad(B, C, H, W, it), _dgrad_ref(w, dy, 2),
                lambda l: br.emulate_wino_dgrad(w, dy, 2, l), br.WINO_DGRAD_LAPSES, _global)


@pytest.mark.parametrize("B,Cw,K,H,W", bc.CONV1_WINO_DGRAD_CASES)
def test_conv1_wino_dgrad_window(B, Cw, K, H, W):
    w, dy, _, _, keep = bc.conv1_wino_dgrad_inputs(B, Cw, K, H, W)
    ref = _dgrad_ref(w, dy, 1)
    _window(bc.key_conv1_wino_dgrad(B, Cw, K, H, W, True), ref[keep],
            lambda l: br.emulate_wino_dgrad(w, dy, 1, l, split_out=True)[keep], br.WINO_DGRAD_LAPSES, _global)
    _window(bc.key_conv1_wino_dgrad(B, Cw, K, H, W, False), ref, lambda l: br.emulate_wino_dgrad(w, dy, 1, l),
            br.WINO_DGRAD_LAPSES, _global)


@pytest.mark.parametrize("B,K,H,W", bc.WINO_WGRAD_CASES)
@pytest.mark.parametrize("dil", [1, 2])
def test_wino_wgrad_window(B, K, H, W, dil):
    x, dy = bc.wino_wgrad_inputs(B, K, H, W, dil)
    slots = bc.channel_tiles(K)
    _window(bc.key_wino_wgrad(B, K, H, W, dil), _wgrad_ref(x, dy, dil),
            lambda l: br.emulate_wino_wgrad(x, dy, dil, l), _wgrad_lapses(B, wino=True),
            lambda a, b: bc.wgrad_error(a, b, slots))


def test_wino_wgrad_grouped_window():
    (S, B, C, Cs, H, W, cout), _, x, dy = bc.wino_grouped_inputs()
    slots = [slice(s * C, (s + 1) * C) for s in range(S)]
    ref = _wgrad_ref(x, dy, 1)[:, :S * C]
    _window(bc.KEY_WINO_GROUPED, ref, lambda l: br.emulate_wino_wgrad(x[:, :S * C], dy, 1, l),
            _wgrad_lapses(B, wino=True), lambda a, b: bc.wgrad_error(a, b, slots))


# ------------------------------------------------------------------ the warp adjoints' reference floors

def _floor(Ms, gouts, B, C, H, W, ho, wo, feats=None):
    """max|d| / max|ref| between CPU fp32 grid_sample autograd (the GPU tests' reference) and the float64
    evaluation of the same restatement from the same fp32 matrix, worst view."""
    import torch.nn.functional as F
    from oracle import kornia_warp
    worst = 0.0
    for i, (M, g) in enumerate(zip(Ms, gouts)):
        mn = kornia_warp.src_norm_from_dst_norm(M, (H, W), (ho, wo))[0]
        grads = []
        for dt in (torch.float32, torch.float64):
            src = (torch.zeros((B, C, H, W)) if feats is None else feats[i]).to(dt).clone().requires_grad_()
            up = src if feats is None else F.interpolate(src, (H, W), mode="bilinear")
            y = (kornia_warp.warp_perspective(up, M.repeat(B, 1, 1), (ho, wo)) if dt == torch.float32
                 else kornia_warp.warp_from_norm(up, mn, (ho, wo)))
            y.backward(g.to(dt))
            grads.append(src.grad)
        worst = max(worst, _global(grads[0], grads[1]))
    return worst


def _check_floor(what, case, pinned, measured):
    print(f"\n[floor] {what} {case}: measured {measured:.3g}, pinned {pinned:.3g}, gate {4 * pinned:.3g}")
    assert measured <= 1.05 * pinned and pinned <= 1.15 * measured and 4 * pinned <= 2e-4, (what, case, pinned, measured)


def test_warp_adjoint_floors_are_the_measured_ones():
    """The floors pinned beside the adjoint cases of ``test_gpu_backward.py`` are this reference's own distance
    from float64, rounded up by at most 15 % (5 % the other way allowed for another CPU's fp32 roundings), and
    every gate (4 x floor) is tighter than the forward's 2e-4."""
    import test_gpu_backward as tb
    for case, pinned in tb._ATOMIC_FLOOR.items():
        B, C, H, W, ho, wo = case
        Ms, gouts, _ = tb._adjoint_inputs(100 * B + C, 3, B, C, H, W, ho, wo)
        _check_floor("atomic", case, pinned, _floor(Ms, gouts, B, C, H, W, ho, wo))
    for case, pinned in tb._GATHER_FLOOR.items():
        B, C, H, W, ho, wo = case
        Ms, gouts, _ = tb._adjoint_inputs(7 * B + C, 2, B, C, H, W, ho, wo)
        _check_floor("gather", case, pinned, _floor(Ms, gouts, B, C, H, W, ho, wo))
    for case, pinned in tb._UPSAMPLED_FLOOR.items():
        B, C, h, w, H, W, ho, wo = case
        Ms, gouts, feats = tb._adjoint_inputs(3 * C + h, 2, B, C, H, W, ho, wo, feat_hw=(h, w))
        _check_floor("upsampled", case, pinned, _floor(Ms, gouts, B, C, H, W, ho, wo, feats))


# ------------------------------------------------------------------ the emulations themselves

def test_split_is_the_pinned_encoding():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((3, 5, 24), generator=g) * torch.logspace(-8, 8, 24)
    hi, lo = br.split(x)
    assert torch.equal(hi, x.to(torch.bfloat16).float())
    assert torch.equal(lo, (x - x.to(torch.bfloat16).float()).to(torch.bfloat16).float())
    nh, nl = br.split_np(x.numpy())
    assert torch.equal(hi, torch.from_numpy(nh)) and torch.equal(lo, torch.from_numpy(nl))


@pytest.mark.parametrize("dil,H", [(1, 7), (1, 8), (2, 13), (2, 17)])
def test_wino_emulations_are_the_conv_in_exact_arithmetic(dil, H):
    """With small-integer operands, which the bf16 split holds exactly, the direct emulations are exact to fp32
    rounding and the Winograd ones to the split of G's sixths (hi + lo keeps 2^-17 of them, amplified by the
    transforms' cancellation: below 3e-5), where a misplaced row, tile or interleaved dilation-2 tile or a wrong
    fold would show at 1e-2 and more."""
    g = torch.Generator().manual_seed(H + dil)
    B, C, O, W = 2, 16, 8, 11
    x = torch.randint(-3, 4, (B, C, H, W), generator=g).float()
    dy = torch.randint(-3, 4, (B, O, H, W), generator=g).float()
    w = torch.randint(-3, 4, (O, C, 3, 3), generator=g).float()
    ref_d = conv2d_input((B, C, H, W), w.double(), dy.double(), padding=dil, dilation=dil)
    ref_w = conv2d_weight(x.double(), (O, C, 3, 3), dy.double(), padding=dil, dilation=dil)
    assert _global(br.emulate_wino_dgrad(w, dy, dil), ref_d) < 3e-5
    assert _global(br.emulate_wino_wgrad(x, dy, dil), ref_w) < 3e-5
    assert _global(br.emulate_dgrad(w, dy, dil), ref_d) < 1e-6
    assert _global(br.emulate_wgrad(x, dy, dil), ref_w) < 1e-6
