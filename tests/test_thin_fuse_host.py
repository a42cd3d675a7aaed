"""CPU tests of ``ResProjVariant``'s host side: the test-side restatement is pinned to the reference's own outputs
(the ``variant_res_proj`` fixture), the drop-in module has the reference's ``state_dict``, the new entry points are
exported and refuse bad arguments with the documented codes before any launch (the pointers are never
dereferenced), and ``ProjectThinFuse`` / ``ResProjVariant`` raise on arguments they cannot run."""
import subprocess

import numpy as np
import pytest
import torch

import res_proj_ref as rr
from helpers import assert_parity, parity_stats
from mvdet_amd import _native

P = 16  # a pointer value that is never dereferenced: validation fails first
NAMES = ("mvbev_thin_conv1_forward_f32", "mvbev_thin_conv1_backward_blocks", "mvbev_thin_conv1_backward_f32",
         "mvbev_thin_conv1_grad_weight_f32")


def _fixture_args():
    fx = rr.fixture()
    g, m = fx["g"], fx["g"]["meta"]
    feats = [fx["feats"][:, v] for v in range(m["num_cam"])]
    return g, (feats, list(g["proj_mats"]), m["upsample_shape"], m["reducedgrid_shape"], fx["params"])


def test_restatement_equals_the_reference_golden():
    """fp32, the reference's order, against what the reference class itself produced.

    Measured on the CPU that generated the fixture: 0 (bit for bit) with four threads; with one thread 3.5e-7
    normwise on ``map_result`` and 5.2e-7 on ``imgs_result`` (the convs block their sums differently).  The
    fixture's own fp32 rounding, measured against the fp64 restatement, is 3.8e-7 (``map_result``) and 5.2e-7
    (``imgs_result``) — so two fp32 evaluations in different summation orders already differ by the rounding level
    itself.  The gate is therefore not a constant but that level, measured here: each of the two fp32 results
    (the golden, and this CPU's restatement in whatever order its convs sum) may sit one rounding level r from
    the exact value, and another summation order may double a result's own error, so the bound is 4 r with r =
    the normwise difference of the golden to the fp64 restatement of the same tensor."""
    g, args = _fixture_args()
    with torch.no_grad():
        got, imgs, _ = rr.reference_order(*args)
        ref64, imgs64, _ = rr.reference_order(*args, dtype=torch.float64)
    r = parity_stats(g["map_result"], ref64)["normwise"]
    s = parity_stats(got, g["map_result"])
    print(f"map_result: restatement vs golden {s['normwise']:.3e}, golden vs fp64 {r:.3e}")
    assert 0 < r < 5e-6, r  # an fp32 rounding level for sums of at most 4608 terms, not an error in the restatement
    assert_parity(got, g["map_result"], "restatement map_result", normwise_tol=4 * r)
    for v, res in enumerate(imgs):
        rv = parity_stats(g["imgs_result"][v], imgs64[v])["normwise"]
        sv = parity_stats(res, g["imgs_result"][v])
        print(f"imgs_result {v}: restatement vs golden {sv['normwise']:.3e}, golden vs fp64 {rv:.3e}")
        assert 0 < rv < 5e-6, rv
        assert_parity(res, g["imgs_result"][v], f"restatement imgs_result {v}", normwise_tol=4 * rv)
    assert np.array_equal(rr.coord_map(*g["meta"]["reducedgrid_shape"]).numpy(), g["coord_map"])


def test_fixture_rig_discriminates():
    m = rr.fixture()["g"]["meta"]
    assert all(0.05 <= s <= 0.95 for s in m["inside_share"]), m["inside_share"]
    assert all(s > 0 for s in m["foot_spread"]), m["foot_spread"]


def test_relu_patterns_of_the_fp32_restatement_stay_inside_the_cap():
    """The GPU tests take both activation patterns from fp32 arithmetic: fp32 against fp64 on the CPU already has
    to stay inside the flip rule, or the seeds are badly chosen."""
    _, args = _fixture_args()
    with torch.no_grad():
        _, _, pre32 = rr.reference_order(*args)
        _, _, pre64 = rr.reference_order(*args, dtype=torch.float64)
    for a, b in zip(pre32, pre64):
        rr.relu_flips((a > 0).float(), b)


def test_state_dict_is_the_reference_class():
    from mvdet_amd import ResProjVariant
    g = rr.fixture()["g"]
    model = ResProjVariant(rr.ds_from_golden(g), device="cpu")
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == g["meta"]["state_dict_shapes"]
    assert list(got) == list(g["meta"]["state_dict_shapes"])  # the same order
    N = g["meta"]["num_cam"]
    assert got["map_classifier.0.weight"] == [512, N + 2, 3, 3] and got["map_classifier.4.weight"] == [1, 512, 3, 3]
    assert model.upsample_shape == g["meta"]["upsample_shape"] and model.reducedgrid_shape == g["meta"]["reducedgrid_shape"]
    assert model.num_cam == N and np.array_equal(model.coord_map.numpy(), g["coord_map"])
    for a, b in zip(model.proj_mats, g["proj_mats"]):
        assert np.allclose(a.numpy(), b, rtol=1e-12, atol=0)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        model(torch.zeros(1, N, 3, 96, 128))


def test_entry_points_are_exported_and_the_version_stays():
    for n in NAMES:
        assert n in _native.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    for n in NAMES:
        assert f" T {n}\n" in out, n
    assert _native.load().mvbev_version() == 12500


def _views(n=1, src=P, colstride=1, stride=32):
    arr = (_native.WarpView * n)()
    for i in range(n):
        arr[i].src = src
        arr[i].src_strides = _native._i64x4(stride * 48, stride * 24, stride, colstride)
        arr[i].m = (1, 0, 0, 0, 1, 0, 0, 0, 1)
    return arr


def test_forward_validation_codes():
    fn = _native.load().mvbev_thin_conv1_forward_f32
    F32, SPLIT = _native.LAYOUT_F32, _native.LAYOUT_SPLIT_BF16

    def call(views=None, n=1, dims=(1, 24, 32, 10, 14), w1=P, b1=P, cout=8, y1=P, layout=F32, xw=None):
        return fn(_views(max(n, 1)) if views is None else views, n, *dims, w1, b1, cout, y1, layout, xw, None)

    assert fn(None, 1, 1, 24, 32, 10, 14, P, P, 8, P, F32, None, None) == -5
    assert call(w1=None) == -5 and call(y1=None) == -5
    assert call(views=_views(src=None)) == -5
    assert call(views=_views(colstride=2)) == -3   # column stride != 1
    assert call(views=_views(stride=-1)) == -3
    assert call(n=0) == -1 and call(n=17) == -2
    assert call(dims=(0, 24, 32, 10, 14)) == -1     # empty batch
    assert call(dims=(1, 0, 32, 10, 14)) == -1      # empty source
    assert call(dims=(1, 24, 32, 10, 0)) == -1      # empty grid
    assert call(cout=0) == -1 and call(cout=12) == -2  # Cout % 8
    assert call(dims=(1, 24, 32, 1 << 16, 1 << 16)) == -2  # y1 past 2^31 elements
    assert call(layout=_native.LAYOUT_F16) == -2 and call(layout=7) == -2
    assert call(y1=24, layout=SPLIT) == -4          # split y1 not 16-B aligned


def test_backward_validation_codes():
    lib = _native.load()
    fn = lib.mvbev_thin_conv1_backward_f32
    dims = (1, 1, 8, 10, 14)  # nviews, B, Cout, Ho, Wo
    assert fn(None, P, P, *dims, P, P, 1 << 20, None) == -5
    assert fn(P, None, P, *dims, P, None, 0, None) == -5   # dxw needs w1
    assert fn(P, P, None, *dims, None, P, 1 << 20, None) == -5  # the partials need xw
    assert fn(P, P, P, 0, 1, 8, 10, 14, P, P, 1 << 20, None) == -1
    assert fn(P, P, P, 17, 1, 8, 10, 14, P, P, 1 << 20, None) == -2
    assert fn(P, P, P, 1, 1, 12, 10, 14, P, P, 1 << 20, None) == -2
    assert fn(P, P, P, 1, 0, 8, 10, 14, P, P, 1 << 20, None) == -1
    assert fn(P, P, P, *dims, None, P, 8 * 9 * 2 - 1, None) == -2  # partials too small (2 blocks)
    assert fn(P, P, P, *dims, None, None, 0, None) == 0  # nothing is wanted: nothing launched
    assert lib.mvbev_thin_conv1_backward_blocks(1, 10, 14) == 2
    assert lib.mvbev_thin_conv1_backward_blocks(2, 120, 360) == 2 * 15 * 12
    assert lib.mvbev_thin_conv1_backward_blocks(1, 0, 14) == 0
    gw = lib.mvbev_thin_conv1_grad_weight_f32
    assert gw(None, 2, 1, 8, P, None) == -5 and gw(P, 2, 1, 8, None, None) == -5
    assert gw(P, 0, 1, 8, P, None) == -1 and gw(P, 2, 0, 8, P, None) == -1
    assert gw(P, 2, 17, 8, P, None) == -2 and gw(P, 2, 1, 12, P, None) == -2


def test_project_thin_fuse_refuses_arguments_it_cannot_run():
    from mvdet_amd import ProjectThinFuse
    eye = [torch.eye(3, dtype=torch.float64)] * 2
    head = ProjectThinFuse(eye, (18, 24), (10, 14))
    assert head.num_views == 2 and tuple(head.m_norm_cpu.shape) == (2, 3, 3) and head.m_norm_cpu.dtype == torch.float32
    x = torch.zeros(1, 1, 18, 24)
    w1, b1, w2, b2, w3 = (torch.zeros(512, 4, 3, 3), torch.zeros(512), torch.zeros(512, 512, 3, 3), torch.zeros(512),
                          torch.zeros(1, 512, 3, 3))
    with pytest.raises(ValueError, match="cpu"):  # a CPU tensor: there is no CPU fallback
        head([x, x], w1, b1, w2, b2, w3)
    with pytest.raises(TypeError, match="float16"):
        head([x.half(), x], w1, b1, w2, b2, w3)
    with pytest.raises(TypeError, match="float64"):
        head([x, x], w1, b1.double(), w2, b2, w3)
    with pytest.raises(ValueError, match=r"\(1, 1, 18, 25\)"):  # mismatched view shapes
        head([x, torch.zeros(1, 1, 18, 25)], w1, b1, w2, b2, w3)
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        head([torch.zeros(1, 2, 18, 24), x], w1, b1, w2, b2, w3)
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        head([x[0], x], w1, b1, w2, b2, w3)
    with pytest.raises(ValueError, match="views per call"):
        head([], w1, b1, w2, b2, w3)
    with pytest.raises(ValueError, match="views per call"):
        head([x] * 17, w1, b1, w2, b2, w3)
    with pytest.raises(ValueError, match="built for 2"):
        head([x], w1, b1, w2, b2, w3)
    with pytest.raises(TypeError, match="sequence"):
        head(x, w1, b1, w2, b2, w3)
    with pytest.raises(TypeError, match="tensor"):
        head([None, x], w1, b1, w2, b2, w3)
    with pytest.raises(ValueError, match="views, got 17"):
        ProjectThinFuse([torch.eye(3)] * 17, (18, 24), (10, 14))
    with pytest.raises(ValueError, match="3x3"):
        ProjectThinFuse([torch.eye(4)], (18, 24), (10, 14))
    with pytest.raises(ValueError, match="positive"):
        ProjectThinFuse(eye, (18, 0), (10, 14))
    # the checks that come after the device check run on meta tensors: only shapes are read
    from mvdet_amd.thin_fuse import _check

    class FakeCuda(torch.Tensor):
        is_cuda = True

    def fake(*shape):
        return torch.zeros(*shape).as_subclass(FakeCuda)

    good = dict(planes=[fake(1, 1, 18, 24)] * 2, w1=fake(512, 4, 3, 3), b1=fake(512), w2=fake(512, 512, 3, 3),
                b2=fake(512), w3=fake(1, 512, 3, 3))
    _check(2, (18, 24), **good)
    for key, bad, msg in (("w1", fake(512, 5, 3, 3), "w1 must be"), ("w1", fake(12, 4, 3, 3), "w1 must be"),
                          ("w2", fake(512, 256, 3, 3), "w2 must be"), ("w3", fake(2, 512, 3, 3), "w3 must be"),
                          ("b1", fake(511), "b1 must be"), ("b2", fake(1, 512), "b2 must be"),
                          ("planes", [fake(1, 1, 18, 20)] * 2, "built for")):
        with pytest.raises(ValueError, match=msg):
            _check(2, (18, 24), **{**good, key: bad})
