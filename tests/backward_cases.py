"""The inputs of the gated backward conv tests, built once for the GPU tests (``test_gpu_backward.py``,
``test_gpu_wgrad_wino.py``) and for the host proof of their gates (``test_backward_gates_host.py``): same
generator, same seed, same draw order, so the two cannot drift.  CPU tensors only; a builder makes every draw
its GPU test needs, the masks and extra weights included.  ``key_*`` name the ``bf16x3_ref.GATES`` entries."""
import torch
import torch.nn.functional as F

COUT = 128

# W % 4 == 0 with split input takes wgrad_dma_kernel (LDS-DMA staging): (12, 36, d1), (13, 44, d2) and
# (13, 44, d1): a partial 64-channel tile, B = 2 and a partial last row segment at both dilations; the
# others wgrad_kernel
WGRAD_CASES = [(1, 64, 12, 36, 1), (2, 136, 17, 37, 2), (1, 512, 30, 90, 2), (1, 24, 5, 70, 1), (2, 72, 13, 44, 2),
               (2, 72, 13, 44, 1)]
PRESPLIT_CASES = [(1, 64, 12, 40, 1, False), (2, 72, 13, 48, 2, False), (2, 192, 37, 96, 1, True)]
DGRAD_CASES = [(1, 128, 40, 12, 36, 1), (2, 512, 512, 17, 37, 2), (1, 256, 200, 9, 64, 1)]
# the ring kernel (split dy, 12-row tiles); the last two: H % 12 != 0 and W % 32 != 0 together with a K that is
# no multiple of 128, at both dilations
DGRAD_RING_CASES = [(1, 128, 40, 25, 36, 1), (2, 512, 512, 17, 37, 2), (1, 256, 200, 9, 64, 1),
                    (1, 128, 72, 14, 37, 1), (1, 128, 72, 14, 37, 2)]
CONV2_WINO_DGRAD_CASES = [(1, 128, 25, 36), (2, 512, 17, 70), (1, 128, 14, 40)]  # the last: H % 3 == 2
CONV1_WINO_DGRAD_CASES = [(1, 128, 256, 25, 70), (2, 256, 384, 14, 40), (1, 512, 256, 13, 40)]  # 14: H % 3 == 2
# H % 3 == 2: 17 and the one-and-a-partial-tile 5
WINO_WGRAD_CASES = [(1, 64, 12, 64), (2, 72, 17, 40), (1, 256, 31, 96), (2, 128, 25, 200), (1, 64, 5, 40)]
RING_PIECES = (0, 1, 3)
FRUSTUM_RECTS = [(0, 12, 0, 40), (10, 37, 30, 100), (5, 9, 60, 75)]  # each camera's footprint; the last 4 x 15


def _key(form, *dims):
    return form + "/" + "-".join(str(d) for d in dims)


def key_wgrad(B, K, H, W, dil):
    return _key("wgrad", B, K, H, W, f"d{dil}")


def key_presplit(B, K, H, W, dil, lists):
    return _key("wgrad_presplit", B, K, H, W, f"d{dil}")


def key_dgrad(B, Cw, K, H, W, dil):
    return _key("dgrad", B, Cw, K, H, W, f"d{dil}")


def key_dgrad_ring(B, Cw, K, H, W, dil):
    return _key("dgrad_ring", B, Cw, K, H, W, f"d{dil}")


def key_ring_pieces(pieces):
    return _key("dgrad_ring_pieces", pieces)


def key_conv2_wino_dgrad(B, C, H, W, it):
    return _key("wino_dgrad2", B, C, H, W, f"w{it}")


def key_conv1_wino_dgrad(B, Cw, K, H, W, split_out):
    return _key("wino_dgrad1", B, Cw, K, H, W, "split" if split_out else "f32")


def key_wino_wgrad(B, K, H, W, dil):
    return _key("wino_wgrad", B, K, H, W, f"d{dil}")


KEY_GROUPED = "wgrad_grouped"
KEY_FRUSTUM = "wgrad_frustum"
KEY_CHANMAP = "dgrad_chanmap"
KEY_WINO_GROUPED = "wino_wgrad_grouped"


def wgrad_inputs(B, K, H, W, dil):
    g = torch.Generator().manual_seed(K + H + dil)
    x = F.relu(torch.randn((B, K, H, W), generator=g))
    dy = torch.randn((B, COUT, H, W), generator=g)
    return x, dy


def grouped_inputs():
    """conv1's view-major grouped slab: S groups of C channels padded to Cs, and the module-order x."""
    g = torch.Generator().manual_seed(7)
    S, B, C, Cs, H, W = 3, 2, 13, 16, 11, 40
    slab = torch.zeros((S, B, Cs, H, W))
    slab[:, :, :C] = F.relu(torch.randn((S, B, C, H, W), generator=g))
    x = torch.cat([slab[s][:, :C] for s in range(S)] + [torch.zeros((B, 2, H, W))], 1)
    dy = torch.randn((B, COUT, H, W), generator=g)
    return (S, B, C, Cs, H, W), slab, x, dy


def presplit_inputs(B, K, H, W, dil):
    g = torch.Generator().manual_seed(K + W)
    x = F.relu(torch.randn((B, K, H, W), generator=g))
    dy = torch.randn((B, COUT, H, W), generator=g)
    return x, dy


def _footprints(slab, H, W):
    for s_, (r0, r1, c0, c1) in enumerate(FRUSTUM_RECTS):
        keep = torch.zeros((H, W))
        keep[r0:r1, c0:c1] = 1
        slab[s_] *= keep
    return slab


def frustum_inputs():
    g = torch.Generator().manual_seed(21)
    S, B, Cs, H, W = 3, 2, 64, 37, 100
    slab = _footprints(F.relu(torch.randn((S, B, Cs, H, W), generator=g)), H, W)
    dy = torch.randn((B, COUT, H, W), generator=g)
    x = torch.cat([slab[s_] for s_ in range(S)], 1)
    return (S, B, Cs, H, W), slab, x, dy


def ring_pieces_inputs(pieces):
    """dy [B, K, H, W], forward weight w [K, Cw, 3, 3] (the data gradient has Cw channels)."""
    g = torch.Generator().manual_seed(11 + pieces)
    B, Cw, K, H, W = 2, 256, 128, 29, 70
    dy = torch.randn((B, K, H, W), generator=g)
    w = torch.randn((K, Cw, 3, 3), generator=g) * 0.05
    return (B, Cw, K, H, W), dy, w


def dgrad_inputs(B, Cw, K, H, W, dil, ring=False):
    g = torch.Generator().manual_seed(Cw + K + dil + (1 if ring else 0))
    w = torch.randn((Cw, K, 3, 3), generator=g) * 0.05
    dy = torch.randn((B, Cw, H, W), generator=g)
    return w, dy


def conv2_wino_dgrad_inputs(B, C, H, W):
    """Two (w, dy) pairs from one generator: the GPU test changes the weight in place between them."""
    g = torch.Generator().manual_seed(C + H)
    out = []
    for _ in range(2):
        w = torch.randn((C, C, 3, 3), generator=g) * 0.05
        dy = torch.randn((B, C, H, W), generator=g)
        out.append((w, dy))
    return out


def conv1_wino_dgrad_inputs(B, Cw, K, H, W):
    """w, dy, two extra (coord) weight inputs past K, the random output mask (a bit per 128-channel group and
    12 x 32 tile, tile 0 full) and the elements [B, K, H, W] it keeps."""
    g = torch.Generator().manual_seed(Cw + K + H)
    w = torch.randn((Cw, K, 3, 3), generator=g) * 0.05
    dy = torch.randn((B, Cw, H, W), generator=g)
    extra = torch.randn((Cw, 2, 3, 3), generator=g)
    ty, tx = -(-H // 12), -(-W // 32)
    ngroups = K // 128
    mask = torch.randint(0, 1 << ngroups, (ty * tx,), generator=g, dtype=torch.int32)
    mask[0] = (1 << ngroups) - 1
    keep = torch.zeros((K, H, W), dtype=torch.bool)
    for i in range(ty):
        for j in range(tx):
            for gi in range(ngroups):
                if (int(mask[i * tx + j]) >> gi) & 1:
                    keep[gi * 128:(gi + 1) * 128, 12 * i:12 * i + 12, 32 * j:32 * j + 32] = True
    return w, dy, extra, mask, keep.expand(B, K, H, W)


def chanmap_inputs():
    g = torch.Generator().manual_seed(3)
    w = torch.randn((128, 30, 3, 3), generator=g) * 0.1
    dy = torch.randn((1, 128, 10, 20), generator=g)
    return w, dy, [29, 3, -1, 7, 0]


def wino_wgrad_inputs(B, K, H, W, dil):
    g = torch.Generator().manual_seed(K + H + W + dil)
    x = F.relu(torch.randn((B, K, H, W), generator=g))
    dy = torch.randn((B, COUT, H, W), generator=g)
    return x, dy


def wino_grouped_inputs():
    g = torch.Generator().manual_seed(11)
    S, B, C, Cs, H, W = 3, 2, 128, 128, 37, 104
    slab = _footprints(F.relu(torch.randn((S, B, Cs, H, W), generator=g)), H, W)
    cout = 256
    x = torch.cat([slab[s_] for s_ in range(S)] + [torch.zeros((B, 2, H, W))], 1)
    dy = torch.randn((B, cout, H, W), generator=g)
    return (S, B, C, Cs, H, W, cout), slab, x, dy


def channel_tiles(K, tile=64):
    return [slice(k0, min(K, k0 + tile)) for k0 in range(0, K, tile)]


# ------------------------------------------------------------------ the sliced measure of a weight gradient

def wgrad_error(got, ref, slots):
    """Worst normwise error of dw [Cout, K, 3, 3] over the slices (channel slot, tap), each on its own scale."""
    from helpers import parity_stats_sliced
    return max(parity_stats_sliced(got[:, s], ref[:, s], dims=(0, 1))["normwise"] for s in slots)


def assert_gated(got, ref, what, normwise_tol):
    """``helpers.assert_parity`` at a pinned gate, the measured figure printed beside it."""
    from helpers import assert_parity, parity_stats
    print(f"[gate] {what}: normwise {parity_stats(got, ref)['normwise']:.3g} <= {normwise_tol:.3g}")
    return assert_parity(got, ref, what, normwise_tol=normwise_tol)


def assert_wgrad_parity(got, ref, slots, what, normwise_tol):
    """The gate per (channel slot, tap): ``helpers.assert_parity_sliced`` on every slot's columns."""
    from helpers import assert_parity_sliced
    print(f"[gate] {what}: worst (slot, tap) normwise {wgrad_error(got, ref, slots):.3g} <= {normwise_tol:.3g}")
    for s in slots:
        assert_parity_sliced(got[:, s], ref[:, s], (0, 1), f"{what}, channels {s.start}:{s.stop}", normwise_tol)
