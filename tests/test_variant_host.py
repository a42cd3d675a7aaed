"""CPU tests of ``NoJointConvVariant``'s host side: the test-side restatement is pinned to the reference's own
outputs (the ``variant_njc`` fixture), the commuted order the native path rests on equals the reference's order
in fp64, the drop-in module has the reference's ``state_dict``, the new entry points are exported and refuse bad
arguments with the documented codes before any launch (the pointers are never dereferenced), and
``ProjectSumHead`` raises on arguments it cannot run."""
import subprocess

import numpy as np
import pytest
import torch

import variant_ref as vr
from helpers import assert_parity
from mvdet_amd import _native

P = 16  # a pointer value that is never dereferenced: validation fails first


def _fixture_case(dtype):
    fx = vr.fixture()
    g, p = fx["g"], fx["params"]
    m = g["meta"]
    feats = [fx["feats"][:, v] for v in range(m["num_cam"])]
    args = (feats, list(g["proj_mats"]), m["upsample_shape"], m["reducedgrid_shape"], p["map_classifier.0.weight"],
            p["map_classifier.0.bias"], p["map_classifier.2.weight"])
    return g, p, feats, args


def test_restatement_equals_the_reference_golden():
    """fp32, the reference's order: 1e-6 normwise against what the reference class itself produced.

    Measured: 0 (bit for bit) on the CPU that generated the fixture with two or more threads, 9.3e-7 there with
    one thread, and 1.55e-6 — over the bound — on the MI355X host's CPU: the fp32 1x1 conv over 1538 channels sums
    in another order there.  The fixture's own fp32 rounding against the fp64 restatement is 1.63e-6, so the
    bound sits inside the reference's noise and holds only where the conv blocks its sum as the generating run
    did; ``imgs_result`` (64-channel sums) stays below 6e-7 everywhere."""
    g, p, feats, args = _fixture_case(torch.float32)
    with torch.no_grad():
        got, _ = vr.reference_order(*args)
        imgs = vr.img_head(feats, g["meta"]["upsample_shape"], p)
    assert_parity(got, g["map_result"], "restatement map_result", normwise_tol=1e-6)
    for v, r in enumerate(imgs):
        assert_parity(r, g["imgs_result"][v], f"restatement imgs_result {v}", normwise_tol=1e-6)
    assert np.array_equal(vr.coord_map(*g["meta"]["reducedgrid_shape"]).numpy(), g["coord_map"])


def test_fixture_rig_discriminates():
    g = vr.fixture()["g"]
    assert all(0.05 <= s <= 0.95 for s in g["meta"]["inside_share"]), g["meta"]["inside_share"]


def test_fp64_warp_is_the_oracle_warp_with_fp32_geometry():
    """The lines ``variant_ref.warp`` runs for fp64 values are the oracle's ``warp_perspective`` (bitwise in fp32)."""
    import torch.nn.functional as F
    from oracle import kornia_warp
    g = vr.fixture()["g"]
    src = torch.from_numpy(np.random.default_rng(0).standard_normal((2, 3, 24, 32)).astype(np.float32))
    grid_hw = g["meta"]["reducedgrid_shape"]
    pm = torch.from_numpy(g["proj_mats"][1]).reshape(1, 3, 3).repeat([2, 1, 1]).float()
    ref = kornia_warp.warp_perspective(src, pm, grid_hw)
    got = F.grid_sample(src, vr.sample_grid(pm, (24, 32), grid_hw), align_corners=True)
    assert torch.equal(got, ref)
    # fp32 grid_sample forms its weights from coordinates up to 32 in fp32 (half an ulp: 2e-6 of a pixel), four
    # of them per sample: 1e-5 of the value range bounds what the fp32 sample may lose against the fp64 one
    assert_parity(vr.warp(src.double(), g["proj_mats"][1], grid_hw), ref, "fp64 values", normwise_tol=1e-5)


def test_commuted_order_equals_reference_order_fp64():
    """The algebra the design rests on: the first 1x1 conv commutes with the upsample and the warp."""
    _, _, _, args = _fixture_case(torch.float64)
    with torch.no_grad():
        ref, pre_ref = vr.reference_order(*args, dtype=torch.float64)
        got, pre = vr.commuted_order(*args, dtype=torch.float64)
    assert_parity(pre, pre_ref, "pre-activation, commuted vs reference order", normwise_tol=1e-12)
    assert_parity(got, ref, "map, commuted vs reference order", normwise_tol=1e-12)


def test_relu_pattern_of_the_fp32_restatement_stays_inside_the_cap():
    """The tests on the GPU take the activation pattern from fp32 arithmetic: fp32 against fp64 on the CPU already
    has to stay inside the flip rule, or the seeds are badly chosen."""
    _, _, _, args = _fixture_case(torch.float32)
    with torch.no_grad():
        _, pre32 = vr.reference_order(*args)
        _, pre64 = vr.reference_order(*args, dtype=torch.float64)
    vr.relu_flips((pre32 > 0).float(), pre64)


def test_state_dict_is_the_reference_class():
    from mvdet_amd import NoJointConvVariant
    g = vr.fixture()["g"]
    model = NoJointConvVariant(vr.ds_from_golden(g), device="cpu")
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == g["meta"]["state_dict_shapes"]
    assert list(got) == list(g["meta"]["state_dict_shapes"])  # the same order
    N = g["meta"]["num_cam"]
    assert got["map_classifier.0.weight"] == [512, 512 * N + 2, 1, 1] and got["map_classifier.2.weight"] == [1, 512, 1, 1]
    assert model.upsample_shape == g["meta"]["upsample_shape"] and model.reducedgrid_shape == g["meta"]["reducedgrid_shape"]
    for a, b in zip(model.proj_mats, g["proj_mats"]):
        assert np.allclose(a.numpy(), b, rtol=1e-12, atol=0)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        model(torch.zeros(1, N, 3, 96, 128))


def test_entry_points_are_exported_and_the_version_stays():
    names = ("mvbev_warp_sum_head_forward_f32", "mvbev_warp_sum_head_backward_f32",
             "mvbev_warp_sum_head_grad_params_f32", "mvbev_warp_sum_head_backward_blocks")
    for n in names:
        assert n in _native.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    for n in names:
        assert f" T {n}\n" in out, n
    assert _native.load().mvbev_version() == 12500


def _views(n=1, src=P, cstride=1, stride=8):
    arr = (_native.WarpView * n)()
    for i in range(n):
        arr[i].src = src
        arr[i].src_strides = _native._i64x4(stride * 64, cstride, stride * 8, stride)
        arr[i].m = (1, 0, 0, 0, 1, 0, 0, 0, 1)
    return arr


# (nviews, B, Cm, h, w, H, W, Ho, Wo)
GOOD = (1, 1, 8, 6, 8, 18, 24, 10, 14)


def test_forward_validation_codes():
    fn = _native.load().mvbev_warp_sum_head_forward_f32
    n, *dims = GOOD
    tail = (P, P, P, P, None, None, None)  # bias, w_coord, w2, map, hidden, boxes, stream
    assert fn(None, n, *dims, *tail) == -5
    for k in range(4):  # bias, w_coord, w2, map
        t = list(tail)
        t[k] = None
        assert fn(_views(), n, *dims, *t) == -5, k
    assert fn(_views(src=None), n, *dims, *tail) == -5
    assert fn(_views(cstride=2), n, *dims, *tail) == -3    # channel stride != 1
    assert fn(_views(stride=-1), n, *dims, *tail) == -3
    bad = [((1, 1, 0, 6, 8, 18, 24, 10, 14), -1),     # Cm = 0
           ((1, 1, 513, 6, 8, 18, 24, 10, 14), -2),   # Cm = 513
           ((17, 1, 8, 6, 8, 18, 24, 10, 14), -2),    # 17 views
           ((0, 1, 8, 6, 8, 18, 24, 10, 14), -1),     # no view
           ((1, 0, 8, 6, 8, 18, 24, 10, 14), -1),     # empty batch
           ((1, 1, 8, 6, 8, 5, 24, 10, 14), -2),      # H < h
           ((1, 1, 8, 6, 8, 18, 7, 10, 14), -2),      # W < w
           ((1, 1, 8, 6, 8, 18, 24, 0, 14), -1)]      # empty grid
    for (n, *dims), status in bad:
        assert fn(_views(max(n, 1)), n, *dims, *tail) == status, (n, dims)


def test_backward_validation_codes():
    lib = _native.load()
    fn = lib.mvbev_warp_sum_head_backward_f32
    dims = (1, 8, 10, 14)  # B, Cm, Ho, Wo
    assert fn(None, P, P, *dims, P, P, None) == -5
    assert fn(P, None, P, *dims, P, P, None) == -5
    assert fn(P, P, None, *dims, P, P, None) == -5
    assert fn(P, P, P, 1, 0, 10, 14, P, P, None) == -1
    assert fn(P, P, P, 1, 513, 10, 14, P, P, None) == -2
    assert fn(P, P, P, 0, 8, 10, 14, P, P, None) == -1
    assert fn(P, P, P, *dims, None, None, None) == 0  # nothing is wanted: nothing launched
    assert lib.mvbev_warp_sum_head_backward_blocks(*dims) == 1
    assert lib.mvbev_warp_sum_head_backward_blocks(2, 512, 120, 360) == 2 * 11  # 43,200 pixels in chunks of 4096
    assert lib.mvbev_warp_sum_head_backward_blocks(1, 513, 10, 14) == 0
    gp = lib.mvbev_warp_sum_head_grad_params_f32
    assert gp(None, 4, 8, P, P, P, None) == -5
    assert gp(P, 0, 8, P, P, P, None) == -1
    assert gp(P, 4, 513, P, P, P, None) == -2
    assert gp(P, 4, 0, P, P, P, None) == -1
    assert gp(P, 4, 8, None, None, None, None) == 0  # nothing is wanted


def test_project_sum_head_refuses_arguments_it_cannot_run():
    from mvdet_amd import ProjectSumHead
    eye = [torch.eye(3, dtype=torch.float64)] * 2
    head = ProjectSumHead(eye, (18, 24), (10, 14))
    assert head.num_views == 2 and tuple(head.m_norm_cpu.shape) == (2, 3, 3) and head.m_norm_cpu.dtype == torch.float32
    z = torch.zeros(1, 8, 6, 8)
    b, wc, w2 = torch.zeros(8), torch.zeros(8, 2), torch.zeros(8)
    with pytest.raises(ValueError, match="cpu"):  # a CPU tensor: there is no CPU fallback
        head([z, z], b, wc, w2)
    with pytest.raises(TypeError, match="float16"):
        head([z.half(), z], b, wc, w2)
    with pytest.raises(TypeError, match="float64"):
        head([z, z], b.double(), wc, w2)
    with pytest.raises(ValueError, match=r"\(1, 8, 6, 9\)"):  # mismatched view shapes
        head([z, torch.zeros(1, 8, 6, 9)], b, wc, w2)
    with pytest.raises(ValueError, match="4-D"):
        head([z[0], z], b, wc, w2)
    with pytest.raises(ValueError, match="views per call"):
        head([], b, wc, w2)
    with pytest.raises(ValueError, match="views per call"):
        head([z] * 17, b, wc, w2)
    with pytest.raises(ValueError, match="built for 2"):
        head([z], b, wc, w2)
    with pytest.raises(TypeError, match="sequence"):
        head(z, b, wc, w2)
    with pytest.raises(TypeError, match="tensor"):
        head([None, z], b, wc, w2)
    with pytest.raises(ValueError, match="views, got 17"):
        ProjectSumHead([torch.eye(3)] * 17, (18, 24), (10, 14))
    with pytest.raises(ValueError, match="3x3"):
        ProjectSumHead([torch.eye(4)], (18, 24), (10, 14))
    with pytest.raises(ValueError, match="positive"):
        ProjectSumHead(eye, (18, 0), (10, 14))
    # checks that come after the device check, on meta tensors' shapes
    from mvdet_amd.sum_head import _check
    zc = torch.zeros(1, 8, 6, 8, device="cuda") if torch.cuda.is_available() else None
    if zc is not None:
        with pytest.raises(ValueError, match="bias must be"):
            _check(1, [zc], torch.zeros(7, device="cuda"), wc.cuda(), w2.cuda())
        with pytest.raises(ValueError, match="w_coord must be"):
            _check(1, [zc], b.cuda(), torch.zeros(8, 3, device="cuda"), w2.cuda())
        with pytest.raises(ValueError, match="Cm <= 512"):
            _check(1, [torch.zeros(1, 513, 2, 2, device="cuda")], b.cuda(), wc.cuda(), w2.cuda())
