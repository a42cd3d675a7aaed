"""CPU reference of ``mvdet_amd.ProjectPlanes`` and the shared inputs of its tests.  TEST INFRASTRUCTURE ONLY.

``project_planes`` is the op's formula in the oracle's stock torch-CPU ops, per plane: ``feat * weight[:, d:d+1]``,
``F.interpolate(bilinear)`` when the map is smaller than ``upsample_shape``, ``oracle.kornia_warp.warp_perspective``;
the planes summed in order, the views concatenated, ``cpu_path.coord_map`` appended.  It is differentiable in the
maps and in the weights.

``CASES`` are ``project_views_ref.CASES``' shapes (a short last unit, whole units, both tap counts, several tiles
both ways) with a plane count each, N = 2 views.  ``inputs`` builds a case's matrices, upstream gradients, maps and
weights once; ``reference`` and ``floors`` are computed once per case and never modified."""
import functools

import numpy as np
import torch

from oracle import cpu_path, kornia_warp

# (seed, B, C, D, source (h, w), upsample (H, W) or None for the plain warp, grid (Ho, Wo))
CASES = [
    (921, 2, 40, 3, (10, 14), (27, 48), (17, 23)),
    (922, 1, 64, 4, (9, 16), (27, 48), (12, 36)),
    (923, 1, 5, 2, (27, 48), None, (12, 36)),
    (924, 2, 36, 1, (9, 11), None, (20, 30)),
    (925, 1, 72, 5, (7, 20), (20, 57), (15, 40)),
]
N_VIEWS = 2


def case_id(case):
    seed, B, C, D, src, up, grid = case
    return (f"{seed}-B{B}-C{C}-D{D}-{src[0]}x{src[1]}-{'plain' if up is None else f'{up[0]}x{up[1]}'}-"
            f"{grid[0]}x{grid[1]}")


def project_planes(feats, weights, proj_mats, upsample_shape, reducedgrid_shape, coord_channels=True, warp=None):
    """feats: N x [B,C,h,w], weights: N x [B,D,h,w], proj_mats: N x D 3x3 (CPU tensors) -> [B, N*C (+2), Ho, Wo].
    ``warp(up, M)``: the warp of one plane (default: kornia's, the fp32 reference)."""
    if warp is None:
        def warp(up, M):
            m = torch.as_tensor(np.asarray(M)).reshape(1, 3, 3).repeat([up.shape[0], 1, 1]).float()
            return kornia_warp.warp_perspective(up, m, list(reducedgrid_shape))
    views = []
    for f, w, mats in zip(feats, weights, proj_mats):
        total = None
        for d, M in enumerate(mats):
            x = f * w[:, d:d + 1]
            if tuple(x.shape[2:]) != tuple(upsample_shape):
                x = cpu_path.upsample(x, upsample_shape)
            y = warp(x, M)
            total = y if total is None else total + y
        views.append(total)
    if coord_channels:
        B = feats[0].shape[0]
        views = views + [cpu_path.coord_map(*reducedgrid_shape).to(feats[0].dtype).repeat([B, 1, 1, 1])]
    return torch.cat(views, dim=1)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(Ms: N lists of D [3,3] fp32, gouts: N x [B,C,Ho,Wo], feats: N x [B,C,h,w], weights {"softmax", "raw"}: N x
    [B,D,h,w], up_hw) of a case.  Plane (v, d) takes matrix v D + d of ``test_gpu_backward._adjoint_inputs``."""
    import test_gpu_backward as tb
    seed, B, C, D, src, up, grid = case
    H, W = src if up is None else up
    Ms, gouts, _ = tb._adjoint_inputs(seed, N_VIEWS * D, B, C, H, W, grid[0], grid[1])
    Ms = [[Ms[v * D + d][0] for d in range(D)] for v in range(N_VIEWS)]
    rng = np.random.default_rng(seed + 1000)
    feats = [torch.from_numpy(rng.standard_normal((B, C, *src)).astype(np.float32)) for _ in range(N_VIEWS)]
    raw = [torch.from_numpy(rng.standard_normal((B, D, *src)).astype(np.float32)) for _ in range(N_VIEWS)]
    weights = {"raw": raw, "softmax": [torch.softmax(r, 1) for r in raw]}
    return Ms, gouts[:N_VIEWS], feats, weights, (H, W)


def _run(case, kind, dtype):
    """world and both gradients in ``dtype``; float64: the same steps from the same fp32 normalised matrices with no
    fp32 rounding anywhere (``kornia_warp.warp_from_norm``, the ``_floor`` idiom of ``test_backward_gates_host``)."""
    Ms, gouts, feats, weights, up_hw = inputs(case)
    grid = case[6]
    warp = None
    if dtype == torch.float64:
        def warp(up, M):
            mn = kornia_warp.src_norm_from_dst_norm(M.reshape(1, 3, 3), up_hw, grid)[0]
            return kornia_warp.warp_from_norm(up, mn, grid)
    fl = [f.to(dtype).clone().requires_grad_() for f in feats]
    wl = [w.to(dtype).clone().requires_grad_() for w in weights[kind]]
    world = project_planes(fl, wl, Ms, up_hw, grid, warp=warp)
    n, C = len(feats), case[2]
    world[:, :n * C].backward(torch.cat(gouts, 1).to(dtype))
    return world.detach(), [t.grad for t in fl], [t.grad for t in wl]


@functools.lru_cache(maxsize=None)
def reference(case, kind="softmax"):
    """(world with the coord channels, grad_feats, grad_weights) of the fp32 CPU reference under the upstream
    gradient cat(gouts) (the coord channels pass none); ``kind``: "softmax" or "raw" weights."""
    return _run(case, kind, torch.float32)


@functools.lru_cache(maxsize=None)
def floors(case):
    """The fp32 reference's own normwise distance from its float64 evaluation (softmax weights): (forward, worst
    view's grad_feats, worst view's grad_weights)."""
    from helpers import parity_stats
    w32, gf32, gw32 = reference(case)
    w64, gf64, gw64 = _run(case, "softmax", torch.float64)
    nw = lambda a, b: parity_stats(a, b)["normwise"]  # noqa: E731
    return (nw(w32, w64), max(nw(a, b) for a, b in zip(gf32, gf64)), max(nw(a, b) for a, b in zip(gw32, gw64)))
