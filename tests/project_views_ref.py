"""CPU reference of ``mvdet_amd.ProjectViews`` and the shared inputs of its tests.  TEST INFRASTRUCTURE ONLY.

``project_views`` is ``persp_trans_detector.py:65, :69, :77`` with the oracle's stock torch-CPU ops
(``cpu_path.upsample``, ``cpu_path.warp_views``, ``cpu_path.coord_map``); it is differentiable.  On
``tests/golden/module_wt2`` it reproduces the reference-made ``warp_out`` and ``coord_map`` exactly
(``test_project_views_host.py``).

``CASES`` are the shapes of ``test_gpu_project_views.py``, the smallest that reach every path of the kernels:
fused upsample and plain warp, B = 1 and 2, C = 5 and 40 (a short last unit / lane round), 36 and 64 (whole
16-B units), and (1, 72, 7x20 -> 20x57 -> 15x40) with several tiles in both grid directions.  ``inputs`` builds
a case's matrices, upstream gradients and maps once (``test_gpu_backward._adjoint_inputs``, 3 views), for the GPU
tests and for the host check of the pinned adjoint floors alike."""
import functools

import numpy as np
import torch

from oracle import cpu_path

# (seed, B, C, source (h, w), upsample (H, W) or None for the plain warp, grid (Ho, Wo))
CASES = [
    (911, 2, 40, (10, 14), (27, 48), (17, 23)),
    (912, 1, 64, (9, 16), (27, 48), (12, 36)),
    (913, 1, 5, (27, 48), None, (12, 36)),
    (914, 2, 36, (9, 11), None, (20, 30)),
    (915, 1, 72, (7, 20), (20, 57), (15, 40)),
]
N_VIEWS = 3


def case_id(case):
    seed, B, C, src, up, grid = case
    return f"{seed}-B{B}-C{C}-{src[0]}x{src[1]}-{'plain' if up is None else f'{up[0]}x{up[1]}'}-{grid[0]}x{grid[1]}"


def project_views(feats, proj_mats, upsample_shape, reducedgrid_shape, coord_channels=True):
    """feats: N x [B,C,h,w] CPU tensors -> [B, N*C (+2), Ho, Wo]; (h, w) == upsample_shape: the warp alone."""
    up = [f if tuple(f.shape[2:]) == tuple(upsample_shape) else cpu_path.upsample(f, upsample_shape) for f in feats]
    warped = cpu_path.warp_views(up, proj_mats, reducedgrid_shape)
    if coord_channels:
        B = feats[0].shape[0]
        warped = warped + [cpu_path.coord_map(*reducedgrid_shape).to(feats[0].dtype).repeat([B, 1, 1, 1])]
    return torch.cat(warped, dim=1)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(Ms [1,3,3] fp32 per view, gouts [B,C,Ho,Wo] per view, feats [B,C,h,w] per view, up_hw) of a case."""
    import test_gpu_backward as tb
    seed, B, C, src, up, grid = case
    H, W = src if up is None else up
    Ms, gouts, feats = tb._adjoint_inputs(seed, N_VIEWS, B, C, H, W, grid[0], grid[1],
                                          feat_hw=None if up is None else src)
    if feats is None:
        rng = np.random.default_rng(seed + 1000)
        feats = [torch.from_numpy(rng.standard_normal((B, C, *src)).astype(np.float32)) for _ in range(N_VIEWS)]
    return Ms, gouts, feats, (H, W)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The CPU reference of a case, computed once and never modified: ``world`` with the coord channels and each
    view's gradient under the upstream gradient cat(gouts) (the coord channels pass none)."""
    Ms, gouts, feats, up_hw = inputs(case)
    grid = case[5]
    leaves = [f.clone().requires_grad_() for f in feats]
    world = project_views(leaves, [M[0] for M in Ms], up_hw, grid)
    n, C = len(feats), case[2]
    world[:, :n * C].backward(torch.cat(gouts, 1))
    return world.detach(), [l.grad for l in leaves]
