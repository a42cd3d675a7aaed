"""Host checks of ``mvdet_amd.ProjectPlanes`` (no GPU): its CPU reference against ``ProjectViews``' reference, the
floors that ``test_gpu_project_planes.py`` pins, the argument errors and ``geometry.plane_projection_matrices``."""
import numpy as np
import pytest
import torch

import project_planes_ref as pr
import project_views_ref as pvr

CL = torch.channels_last


def test_reference_with_one_unit_plane_is_project_views_reference():
    case = pr.CASES[0]
    Ms, _, feats, _, up_hw = pr.inputs(case)
    ones = [torch.ones((f.shape[0], 1, *f.shape[2:])) for f in feats]
    mats = [planes[0] for planes in Ms]
    with torch.no_grad():
        a = pr.project_planes(feats, ones, [[M] for M in mats], up_hw, case[6])
        b = pvr.project_views(feats, mats, up_hw, case[6])
    assert torch.equal(a, b)


def test_reference_is_differentiable_in_both_inputs():
    case = pr.CASES[2]
    world, gf, gw = pr.reference(case)
    _, _, feats, weights, _ = pr.inputs(case)
    assert world.shape[1] == pr.N_VIEWS * case[2] + 2
    assert all(g is not None and g.shape == f.shape and g.abs().max() > 0 for g, f in zip(gf, feats))
    assert all(g is not None and g.shape == w.shape and g.abs().max() > 0 for g, w in zip(gw, weights["softmax"]))


@pytest.mark.parametrize("case", pr.CASES, ids=pr.case_id)
def test_floors_are_the_measured_ones(case):
    """The floors pinned in ``test_gpu_project_planes.py`` are the CPU fp32 reference's own distance from its float64
    evaluation on that file's inputs, rounded up by at most 15 % (5 % the other way allowed for another CPU's fp32
    roundings), and every gate (4 x floor) is below 2e-4."""
    import test_gpu_project_planes as tp
    from test_backward_gates_host import _check_floor
    assert set(tp.FLOORS) == set(pr.CASES)
    for what, pinned, measured in zip(("forward", "grad_feats", "grad_weights"), tp.FLOORS[case], pr.floors(case)):
        _check_floor(f"project_planes {what}", pr.case_id(case), pinned, measured)
    world, _, gw = pr.reference(case)
    zero = (world == 0).float().mean().item()
    nonzero_gw = torch.cat([g.flatten() for g in gw]).ne(0).float().mean().item()
    print(f"[cases] {pr.case_id(case)}: {zero:.0%} of outputs exactly zero, {nonzero_gw:.0%} of weight gradients "
          f"non-zero")
    assert zero < 0.5 and nonzero_gw > 0.4  # the case exercises both the gather and the planes' gradients


def _planes(n, d):
    return [[torch.eye(3)] * d for _ in range(n)]


def test_constructor_errors():
    import mvdet_amd
    pp = mvdet_amd.ProjectPlanes(_planes(2, 3), (27, 48), (12, 36))
    assert isinstance(pp, torch.nn.Module) and not list(pp.parameters())
    assert (pp.num_views, pp.num_planes) == (2, 3) and tuple(pp.m_norm_cpu.shape) == (2, 3, 3, 3)
    for n in (0, 17):
        with pytest.raises(ValueError, match="1 .. 16 views"):
            mvdet_amd.ProjectPlanes(_planes(n, 2), (27, 48), (12, 36))
    for d in (0, 9):
        with pytest.raises(ValueError, match="1 .. 8 planes"):
            mvdet_amd.ProjectPlanes(_planes(2, d), (27, 48), (12, 36))
    with pytest.raises(ValueError, match="same number of planes"):
        mvdet_amd.ProjectPlanes([[torch.eye(3)] * 2, [torch.eye(3)] * 3], (27, 48), (12, 36))
    with pytest.raises(ValueError, match="must be 3x3"):
        mvdet_amd.ProjectPlanes([[torch.eye(3), torch.eye(4)]], (27, 48), (12, 36))
    with pytest.raises(TypeError, match="sequences of D 3x3"):
        mvdet_amd.ProjectPlanes(torch.eye(3), (27, 48), (12, 36))
    with pytest.raises(ValueError, match="grid side of 1"):
        mvdet_amd.ProjectPlanes(_planes(2, 2), (27, 48), (1, 36))
    for bad in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(TypeError, match="out_dtype"):
            mvdet_amd.ProjectPlanes(_planes(2, 2), (27, 48), (12, 36), out_dtype=bad)


def test_argument_errors():
    """Every check comes before any launch; CPU tensors that report a ROCm device stand in for the GPU's."""
    import mvdet_amd
    from mvdet_amd import project_planes as mod
    pp = mvdet_amd.ProjectPlanes(_planes(2, 3), (27, 48), (12, 36))

    class OnGpu(torch.Tensor):  # a CPU tensor that reports a ROCm device: only the host-side checks run
        is_cuda = True

    fake = lambda t: t.as_subclass(OnGpu)  # noqa: E731
    f = fake(torch.zeros((1, 4, 9, 16)).contiguous(memory_format=CL))
    w = fake(torch.zeros((1, 3, 9, 16)))
    mod._check(pp, [f, f], [w, w])  # the good call
    with pytest.raises(ValueError, match="3 feats for a rig of 2"):
        pp([f, f, f], [w, w])
    with pytest.raises(ValueError, match="1 weights for a rig of 2"):
        pp([f, f], [w])
    with pytest.raises(TypeError, match="sequence of tensors"):
        pp(f, [w, w])
    with pytest.raises(ValueError, match="has 2 planes, the rig 3"):
        pp([f, f], [w, fake(torch.zeros((1, 2, 9, 16)))])
    for bad in ((2, 3, 9, 16), (1, 3, 8, 16), (1, 3, 9, 15)):
        with pytest.raises(ValueError, match="does not match"):
            pp([f, f], [w, fake(torch.zeros(bad))])
    with pytest.raises(TypeError, match=r"weights\[1\] must be float32"):
        pp([f, f], [w, fake(torch.zeros((1, 3, 9, 16)).half())])
    with pytest.raises(ValueError, match=r"weights\[0\] must be contiguous"):
        pp([f, f], [fake(torch.zeros((1, 3, 16, 9)).transpose(2, 3)), w])
    with pytest.raises(ValueError, match="channels_last"):
        pp([fake(torch.zeros((1, 4, 9, 16)))] * 2, [w, w])  # contiguous fp32 maps with C > 1
    with pytest.raises(TypeError, match="share one dtype"):
        pp([f, fake(f.half())], [w, w])
    with pytest.raises(ValueError, match="differs from"):
        pp([f, fake(f[:, :3])], [w, w])
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        pp([fake(f.double())] * 2, [w, w])
    with pytest.raises(ValueError, match="larger than the upsampled size"):
        pp([fake(torch.zeros((1, 4, 28, 16)).contiguous(memory_format=CL))] * 2, [w, w])
    cpu_f, cpu_w = torch.zeros((1, 4, 9, 16)).contiguous(memory_format=CL), torch.zeros((1, 3, 9, 16))
    with pytest.raises(ValueError, match="no CPU fallback"):
        pp([cpu_f, cpu_f], [w, w])
    with pytest.raises(ValueError, match=r"weights\[0\] is on cpu.*no CPU fallback"):
        pp([f, f], [cpu_w, w])


@pytest.mark.parametrize("cfg", [1, 2])
def test_ground_plane_is_projection_matrices(cfg):
    from mvdet_amd import geometry, synthetic
    ds = synthetic.CONFIGS[cfg]["make"]()
    planes = geometry.plane_projection_matrices(ds, [0.0])
    base = geometry.projection_matrices(ds)
    assert len(planes) == ds.num_cam and all(len(p) == 1 for p in planes)
    for p, b in zip(planes, base):
        assert p[0].dtype == torch.float64 and np.array_equal(p[0].numpy(), b.numpy())


@pytest.mark.parametrize("cfg", [1, 2])
def test_plane_matrices_map_the_projection_of_a_raised_point_to_its_grid_cell(cfg):
    """A world point (X, Y, z) above grid cell g, projected with K [R | t] and taken to upsampled-image pixels, is
    mapped by plane z's matrix back to g's reduced-grid pixel: 1e-9 relative in float64."""
    from mvdet_amd import geometry, synthetic
    ds = synthetic.CONFIGS[cfg]["make"]()
    unit = 100.0 if cfg == 2 else 1.0  # Wildtrack's world is in cm, MultiviewX's in m
    heights = [0.3 * unit, 0.9 * unit, 1.7 * unit]
    mats = geometry.plane_projection_matrices(ds, heights)
    base = ds.base
    ups = geometry.upsample_shape(ds.img_shape, ds.img_reduce)
    img_zoom = np.diag(np.append(np.array(ds.img_shape) / np.array(ups), [1]))
    map_zoom = np.diag(np.append(np.ones([2]) / ds.grid_reduce, [1]))
    rng = np.random.default_rng(cfg)
    worst = 0.0
    for cam in range(ds.num_cam):
        for d, z in enumerate(heights):
            g = np.append(rng.uniform(0, 1, 2) * np.array(base.worldgrid_shape), 1.0)
            xy = base.worldgrid2worldcoord_mat @ g
            xy = xy / xy[2]
            cam_pt = np.asarray(base.extrinsic_matrices[cam]) @ np.array([xy[0], xy[1], z, 1.0])
            img = base.intrinsic_matrices[cam] @ cam_pt
            up_px = np.linalg.inv(img_zoom) @ (img / img[2])
            got = mats[cam][d].numpy() @ up_px
            got = got / got[2]
            want = map_zoom @ (geometry.PERMUTATION @ g)
            worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print(f"[planes] config {cfg}: worst relative distance from the grid cell {worst:.3g}")
    assert worst <= 1e-9
