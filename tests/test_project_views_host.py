"""Host checks of ``mvdet_amd.ProjectViews`` (no GPU): its CPU reference against the reference module's own golden
tensors, the argument errors, and the adjoint floors that ``test_gpu_project_views.py`` pins."""
import pytest
import torch

import project_views_ref as pr
from helpers import load_golden, parity_stats


def test_reference_helper_is_the_reference_modules_projection():
    """``project_views_ref.project_views`` on module_wt2's inputs gives the fixture's ``warp_out`` and ``coord_map``
    exactly: the op's definition is the reference's own module."""
    g = load_golden("module_wt2")
    m = g["meta"]
    x = torch.from_numpy(g["feat_in"])
    N, C = x.shape[1], x.shape[2]
    with torch.no_grad():
        world = pr.project_views([x[:, v] for v in range(N)], list(g["proj_mats"]), m["upsample_shape"],
                                 m["reducedgrid_shape"])
    assert parity_stats(world[:, :N * C], torch.from_numpy(g["warp_out"]).flatten(1, 2))["normwise"] == 0.0
    assert torch.equal(world[:, N * C:], torch.from_numpy(g["coord_map"]).repeat(x.shape[0], 1, 1, 1))


def test_reference_helper_is_differentiable():
    case = pr.CASES[2]
    world, grads = pr.reference(case)
    assert world.shape[1] == pr.N_VIEWS * case[2] + 2
    assert all(g is not None and g.shape == f.shape and g.abs().max() > 0 for g, f in zip(grads, pr.inputs(case)[2]))


def test_constructor_and_argument_errors():
    import mvdet_amd
    eye = [torch.eye(3)] * 2
    pv = mvdet_amd.ProjectViews(eye, (27, 48), (12, 36))
    assert isinstance(pv, torch.nn.Module) and not list(pv.parameters())
    for grid in ((1, 36), (12, 1)):
        with pytest.raises(ValueError, match="grid side of 1"):
            mvdet_amd.ProjectViews(eye, (27, 48), grid)
    for bad in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(TypeError, match="out_dtype"):
            mvdet_amd.ProjectViews(eye, (27, 48), (12, 36), out_dtype=bad)
    f = torch.zeros((1, 4, 9, 16))
    with pytest.raises(ValueError, match="3 views for a rig of 2"):
        pv([f, f, f])
    with pytest.raises(TypeError, match="sequence of tensors"):
        pv(f)
    with pytest.raises(TypeError, match="share one dtype"):
        pv([f, f.half()])
    with pytest.raises(ValueError, match="differs from"):
        pv([f, f[:, :3]])
    with pytest.raises(ValueError, match="larger than the upsampled size"):
        pv([torch.zeros((1, 4, 28, 16))] * 2)
    with pytest.raises(ValueError, match="larger than the upsampled size"):
        pv([torch.zeros((1, 4, 9, 49))] * 2)
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        pv([f.double()] * 2)
    with pytest.raises(ValueError, match="no CPU fallback"):
        pv([f, f])
    with pytest.raises(ValueError, match="no CPU fallback"):
        pv([f.contiguous(memory_format=torch.channels_last)] * 2)


def test_mixed_memory_formats_and_nchw_out_dtype_raise():
    """The format checks come before any launch; meta tensors stand in for the GPU's."""
    import mvdet_amd
    from mvdet_amd import project_views as mod
    eye = [torch.eye(3)] * 2
    pv = mvdet_amd.ProjectViews(eye, (27, 48), (12, 36))
    f = torch.zeros((1, 4, 9, 16))
    cl = f.contiguous(memory_format=torch.channels_last)

    class OnGpu(torch.Tensor):  # a CPU tensor that reports a ROCm device: only the host-side checks run
        is_cuda = True

    fake = lambda t: t.as_subclass(OnGpu)  # noqa: E731
    with pytest.raises(ValueError, match="share one memory format"):
        mod._check(pv, [fake(f), fake(cl)])
    with pytest.raises(ValueError, match="share one memory format"):
        mod._check(pv, [fake(f.half()), fake(f.half())])  # 16-bit NCHW views are out of scope
    assert mod._check(pv, [fake(f), fake(f)]) is False and mod._check(pv, [fake(cl), fake(cl)]) is True
    pv32 = mvdet_amd.ProjectViews(eye, (27, 48), (12, 36), out_dtype=torch.float32)
    assert mod._check(pv32, [fake(cl.half()), fake(cl.half())]) is True


def test_adjoint_floors_are_the_measured_ones():
    """As ``test_backward_gates_host.test_warp_adjoint_floors_are_the_measured_ones`` for the existing adjoints: the
    floors pinned in ``test_gpu_project_views.py`` are the CPU fp32 reference's own distance from float64 on that
    file's inputs, rounded up by at most 15 %, and every gate (4 x floor) is below 2e-4."""
    import test_gpu_project_views as tp
    from test_backward_gates_host import _check_floor, _floor
    assert set(tp.FLOORS) == set(pr.CASES)
    for case, pinned in tp.FLOORS.items():
        _, B, C, _, up, (ho, wo) = case
        Ms, gouts, feats, (H, W) = pr.inputs(case)
        _check_floor("project_views", pr.case_id(case), pinned,
                     _floor(Ms, gouts, B, C, H, W, ho, wo, None if up is None else feats))
