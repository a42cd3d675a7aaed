"""Each warp adjoint against the forward it is the adjoint of, at fp32 rounding.

``test_gpu_backward.py`` compares the adjoints with CPU ``grid_sample`` autograd, whose coordinates round on their
own (1e-6 ... 2e-5).  Forward and adjoint of this library share one coordinate and weight code, so between them
the only slack is fp32 summation:

    <warp(x), y> = <x, adjoint(y)>                                      (dot-product identity, random x, y)
    adjoint(y)[p] = <warp(e_p), y>                                      (impulses e_p at border pixels)

both sides formed in float64 from the GPU's fp32 outputs, within

    (n_max + 8) * 2^-24 * sum |x| . |S|^T |y|

the bound ``test_gpu_backward_epilogue.py`` derives for its sums: a source pixel's gradient is a sum of n <= n_max
products (n - 1 additions, one rounding per product: n * 2^-24 of the absolute sum), a forward sample is 4 (fused
upsample: 9) weighted corners, and the weights themselves carry a few roundings that the two sides share; ``+ 8``
covers the forward's products and additions.  ``n_max`` and ``|S|`` come from the CPU restatement of the plan
(``oracle.kornia_warp.sampling_matrix``), never from the GPU.

| adjoint                                   | forward                       |
|-------------------------------------------|-------------------------------|
| ``ops.warp_views_backward`` (atomic)      | ``ops.warp_views_into``       |
| ``ops.warp_views_adjoint`` (planned)      | ``ops.warp_views_into``       |
| ``ops.warp_views_adjoint``, upsampled plan| ``ops.warp_views_upsampled_into`` |

Geometries: 9 x 11 -> 20 x 30 (magnifying: ~24 output samples per source pixel) and 27 x 48 -> 12 x 36
(minifying), 3 views each, the last with a strong perspective row (m[6], m[7] = +-0.3): part of its grid lands
outside the source and part in the (-1, 0) and (W - 1, W) bands, where a sample keeps only its in-bounds corners.
Split-bf16 ``grad_out`` variants are fed y = decode(encode(y)), which carries no quantization of its own.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import kornia_warp
from test_gpu_backward import _rand_h, _split_encode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
B = 2
# (source, grid); the fused upsample's source is the same map, upsampled 3x before the warp (the matrices act on
# normalized coordinates, so one set serves both)
GEOMETRIES = {"magnify": ((9, 11), (20, 30)), "minify": ((27, 48), (12, 36))}
SEEDS = {"magnify": 31, "minify": 12}  # of the matrices: draws whose perspective view meets both column bands
FORMS = ["atomic", "gather", "gather_split", "upsampled", "upsampled_split"]


def _quantized(y):
    hi = y.to(torch.bfloat16).float()
    return hi + (y - hi).to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def _geometry(name):
    """The 3 matrices (src_norm <- dst_norm, fp32) of a geometry and, per view and for the plain and the
    upsampled source, the CPU restatement's |S| [O, P] (float64) and each source pixel's entry count."""
    from mvdet_amd.geometry import kornia_src_norm_from_dst_norm
    (H, W), (ho, wo) = GEOMETRIES[name]
    rng = np.random.default_rng(SEEDS[name])
    mns = [kornia_src_norm_from_dst_norm(torch.from_numpy(_rand_h(rng, H, W, ho, wo)).float()[None], (H, W),
                                         (ho, wo))[0].clone() for _ in range(3)]
    mns[2][2, 0], mns[2][2, 1] = 0.3, -0.3
    # the perspective view reaches outside the source and into both one-corner-pair bands
    grid = kornia_warp.transform_points(mns[2][None, None, None], kornia_warp.create_meshgrid(ho, wo))[0]
    ix, iy = (grid[..., 0] + 1) / 2 * (W - 1), (grid[..., 1] + 1) / 2 * (H - 1)
    in_y = (iy > -1) & (iy < H)
    assert ((ix <= -1) | (ix >= W) | ~in_y).any() and ((ix > 0) & (ix < W - 1) & (iy > 0) & (iy < H - 1)).any()
    assert ((ix > -1) & (ix < 0) & in_y).any() and ((ix > W - 1) & (ix < W) & in_y).any()
    mats = {}
    for up in (False, True):
        S = [kornia_warp.sampling_matrix(m, (3 * H, 3 * W), (ho, wo), backbone_hw=(H, W)) if up else
             kornia_warp.sampling_matrix(m, (H, W), (ho, wo)) for m in mns]
        mats[up] = [(s.abs().double(), (s != 0).sum(0)) for s in S]
    return mns, mats


def _forward(form, xs, mns, name):
    from mvdet_amd import ops
    (H, W), (ho, wo) = GEOMETRIES[name]
    dsts = [torch.full((x.shape[0], x.shape[1], ho, wo), float("nan"), device=DEV) for x in xs]
    if form.startswith("upsampled"):
        ops.warp_views_upsampled_into(xs, (3 * H, 3 * W), mns, dsts)
    else:
        ops.warp_views_into(xs, mns, dsts)
    return dsts


def _adjoint(form, ys, mns, name, C, prefill=None):
    """adjoint(y) per view; ``prefill``: accumulated into buffers holding that value."""
    from mvdet_amd import ops
    (H, W), (ho, wo) = GEOMETRIES[name]
    up = form.startswith("upsampled")
    outs = [torch.full((B, C, H, W), float("nan") if prefill is None else prefill, device=DEV) for _ in ys]
    if form == "atomic":
        if prefill is None:
            for o in outs:
                o.zero_()
        ops.warp_views_backward(ys, mns, outs)
        return outs
    plans = [ops.WarpAdjointPlan(m, (3 * H, 3 * W), (ho, wo), DEV, backbone_hw=(H, W)) if up else
             ops.WarpAdjointPlan(m, (H, W), (ho, wo), DEV) for m in mns]
    gs = [_split_encode(y) for y in ys] if form.endswith("split") else ys
    ops.warp_views_adjoint(gs, plans, outs, accumulate=prefill is not None)
    return outs


def _inputs(form, name, C, seed):
    (H, W), (ho, wo) = GEOMETRIES[name]
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn((B, C, H, W), generator=g) for _ in range(3)]
    ys = [torch.randn((B, C, ho, wo), generator=g) for _ in range(3)]
    if form.endswith("split"):
        ys = [_quantized(y) for y in ys]
    return xs, ys


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_dot_product_identity(name, form):
    mns, mats = _geometry(name)
    C = 8
    xs, ys = _inputs(form, name, C, seed=1)
    fw = _forward(form, [x.to(DEV) for x in xs], mns, name)
    ad = _adjoint(form, [y.to(DEV) for y in ys], mns, name, C)
    for v in range(3):
        absS, cnt = mats[form.startswith("upsampled")][v]
        lhs = (fw[v].cpu().double() * ys[v].double()).sum().item()
        rhs = (xs[v].double() * ad[v].cpu().double()).sum().item()
        spread = torch.einsum("op,bco->bcp", absS, ys[v].abs().double().flatten(2))  # |S|^T |y|
        bound = (int(cnt.max()) + 8) * U * (xs[v].abs().double().flatten(2) * spread).sum().item()
        print(f"[identity] {name} {form} view {v}: |lhs - rhs| {abs(lhs - rhs):.3g} <= {bound:.3g} "
              f"(n_max {int(cnt.max())}, lhs {lhs:.6g})")
        assert abs(lhs - rhs) <= bound, (name, form, v, lhs, rhs, bound)


def _impulse_pixels(h, w, counts):
    """16 source pixels, one per channel: the four corners, the middles of the four edges, one interior pixel,
    and the 7 other border pixels that the restated plans of the views touch most (a minifying warp leaves
    many border pixels untouched: those must come out exactly zero, these carry the border weights)."""
    px = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1),
          (h // 2, w // 2)]
    total = sum(counts).reshape(h, w)
    border = [(r, q) for r in range(h) for q in range(w) if r in (0, h - 1) or q in (0, w - 1)]
    border.sort(key=lambda p: -int(total[p]))  # (stable: ties in raster order)
    px += [p for p in border if p not in px][:7]
    assert len(set(px)) == 16
    return px


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_boundary_impulses(name, form):
    """x = e_p per channel: adjoint(y)[p] equals sum warp(e_p) . y, the few samples that touch p — the corner
    weights at the zero-padding border, which random data at a global scale cannot see."""
    mns, mats = _geometry(name)
    C = 16
    _, ys = _inputs(form, name, C, seed=2)
    h, w = GEOMETRIES[name][0]
    px = _impulse_pixels(h, w, [cnt for _, cnt in mats[form.startswith("upsampled")]])
    x = torch.zeros((B, C, h, w))
    for c, (r, q) in enumerate(px):
        x[:, c, r, q] = 1.0
    fw = _forward(form, [x.to(DEV)] * 3, mns, name)
    ad = _adjoint(form, [y.to(DEV) for y in ys], mns, name, C)
    touched = 0
    for v in range(3):
        _, cnt = mats[form.startswith("upsampled")][v]
        f, y, a = fw[v].cpu().double(), ys[v].double(), ad[v].cpu().double()
        want = (f * y).sum((2, 3))                       # [B, C]
        absum = (f.abs() * y.abs()).sum((2, 3))
        worst = 0.0
        for c, (r, q) in enumerate(px):
            n = int(cnt[r * w + q])
            touched += n
            for b in range(B):
                bound = (n + 8) * U * absum[b, c].item()
                err = abs(a[b, c, r, q].item() - want[b, c].item())
                worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else float("inf")))
                assert err <= bound, (name, form, v, (r, q), b, a[b, c, r, q].item(), want[b, c].item(), bound)
        print(f"[impulse] {name} {form} view {v}: worst |adjoint(y)[p] - <warp(e_p), y>| / bound {worst:.3g}")
    assert touched > 0


@pytest.mark.parametrize("form", ["atomic", "gather", "upsampled_split"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_accumulation_into_a_prefilled_buffer(name, form):
    """Accumulating onto 0.5 adds exactly the adjoint: elementwise within the n + 2 roundings of a sum of n terms
    that starts from the prefill, (n + 2) * 2^-24 * (0.5 + |S|^T |y|), twice for the atomic form, whose two runs
    add in different orders."""
    mns, mats = _geometry(name)
    C = 8
    _, ys = _inputs(form, name, C, seed=3)
    ydev = [y.to(DEV) for y in ys]
    plain = _adjoint(form, ydev, mns, name, C)
    acc = _adjoint(form, ydev, mns, name, C, prefill=0.5)
    for v in range(3):
        absS, cnt = mats[form.startswith("upsampled")][v]
        spread = torch.einsum("op,bco->bcp", absS, ys[v].abs().double().flatten(2))
        bound = (1 + (form == "atomic")) * (cnt.double() + 2) * U * (0.5 + spread)
        err = (acc[v].cpu().double() - 0.5 - plain[v].cpu().double()).flatten(2).abs()
        print(f"[accumulate] {name} {form} view {v}: worst err / bound {(err / bound).max().item():.3g}")
        assert (err <= bound).all(), (name, form, v, (err / bound).max().item())
