"""``ImageProjVariant`` on the host: the export, the module's ``state_dict`` against what the reference class itself
recorded in the ``variant_img_proj`` fixture, the parameter recipe, the restatement (``img_proj_ref``) pinned bit for
bit to the reference's arrays, the unchanged 3-channel backbone, the library's new symbols and the argument checks
of the new ops — no GPU compute."""
import numpy as np
import pytest
import torch

import img_proj_ref as ir
from mvdet_amd import _native

NEW_SYMBOLS = ("mvbev_img_proj_forward_f32", "mvbev_upsample_map_f32", "mvbev_upsample_map_backward_f32")


def test_the_variant_is_exported():
    import mvdet_amd
    assert hasattr(mvdet_amd, "ImageProjVariant"), "mvdet_amd.ImageProjVariant is missing"
    from mvdet_amd import DenseFuseHead, ImageProjection, ImageProjVariant  # noqa: F401
    assert "ImageProjVariant" in mvdet_amd.__all__


def test_state_dict_is_the_reference_class_s():
    from mvdet_amd import ImageProjVariant
    fx = ir.fixture()
    g, m = fx["g"], fx["g"]["meta"]
    model = ImageProjVariant(ir.ds_from_golden(g), device="cpu")
    sd = model.state_dict()
    want = m["state_dict_shapes"]
    assert len(want) == 125 and list(sd) == list(want)
    assert {k: list(v.shape) for k, v in sd.items()} == want
    assert list(ir.param_shapes(m["num_cam"])) == list(want)
    # the reference's attributes and helpers
    assert model.num_cam == m["num_cam"] and model.img_shape == m["img_shape"]
    assert model.reducedgrid_shape == m["reducedgrid_shape"] and model.upsample_shape == m["upsample_shape"]
    assert np.array_equal(model.coord_map.numpy(), g["coord_map"])
    assert np.array_equal(torch.stack(list(model.proj_mats)).numpy(), g["proj_mats"])
    assert torch.equal(model.create_coord_map(m["reducedgrid_shape"] + [1]), model.coord_map)
    mats = model.get_imgcoord2worldgrid_matrices(tuple(g["K"]), tuple(g["E"]), g["G"])
    assert sorted(mats) == list(range(m["num_cam"]))
    assert [type(c).__name__ for c in model.children()] == ["Sequential"] * 3
    assert [n for n, _ in model.named_children()] == ["base_pt1", "base_pt2", "map_classifier"]
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        model(torch.zeros(1, m["num_cam"], 3, 8, 8))


def test_recipe_gives_the_fixture_s_parameters():
    fx = ir.fixture()  # (asserts the sha256)
    m = fx["g"]["meta"]
    ps = ir.params(m["num_cam"], m["weight_seed"])
    assert ir.params_sha256(ps) == m["weights_sha256"]
    assert sum(v.size for v in ps.values() if v.dtype == np.float32) > 15_000_000


def test_restatement_is_the_reference():
    """fp32, the reference's order, against what the reference class itself produced.

    Bit for bit on the CPU that generated the fixture, with 1, 4 and 16 threads, and ``tools/gen_golden_img_proj.py``
    asserts exactly that before it writes the file: there the restatement IS the reference.  It is not a property
    of every host: on another CPU model torch's own ``F.interpolate`` / ``grid_sample`` / conv kernels give other
    fp32 bits for the same ops (``torch.equal`` was seen to fail on one), as the reference class itself would.  So, as in ``test_thin_fuse_host.py``, the gate here is the fp32 rounding level of these very tensors,
    measured: r = the normwise difference of the golden to the fp64 restatement (2.1e-6 for ``projected_imgs``,
    whose resize weights come from fp32 source coordinates of up to 86 pixels: 86 x 2^-24 = 5e-6 of a weight;
    5.1e-7 for ``map_result``); each of the two fp32 results may sit r from the exact value and another evaluation
    order may double a result's own error: the bound is 4 r.  The coord channels are bitwise everywhere."""
    from helpers import assert_parity, parity_stats
    fx = ir.fixture()
    g, m = fx["g"], fx["g"]["meta"]
    args = (fx["imgs"], list(g["proj_mats"]), m["upsample_shape"], m["reducedgrid_shape"])
    proj = ir.front(*args)
    r = parity_stats(g["projected_imgs"], ir.front(*args, dtype=torch.float64))["normwise"]
    s = parity_stats(proj, g["projected_imgs"])
    print(f"projected_imgs: restatement vs golden {s['normwise']:.3e}, golden vs fp64 {r:.3e}")
    assert 0 < r < 1e-5, r  # an fp32 rounding level of bilinear weights at these sizes, not an error
    assert_parity(proj, g["projected_imgs"], "restatement projected_imgs", normwise_tol=4 * r)
    N = m["num_cam"]
    assert torch.equal(proj[:, 3 * N:], torch.from_numpy(g["projected_imgs"][:, 3 * N:]))
    wf = torch.from_numpy(g["world_feature"])
    with torch.no_grad():
        out, _ = ir.head(wf, fx["params"], m["reducedgrid_shape"])
        out64, _ = ir.head(wf, fx["params"], m["reducedgrid_shape"], dtype=torch.float64)
    r = parity_stats(g["map_result"], out64)["normwise"]
    s = parity_stats(out, g["map_result"])
    print(f"map_result: restatement vs golden {s['normwise']:.3e}, golden vs fp64 {r:.3e}")
    assert 0 < r < 5e-6, r  # an fp32 rounding level for sums of at most 4608 terms
    assert_parity(out, g["map_result"], "restatement map_result", normwise_tol=4 * r)
    assert list(g["world_feature"].shape[2:]) == m["world_feature_hw"] == [5, 7]
    assert m["imgs_result_shape"] == [m["num_cam"], m["B"], 2, *m["input_hw"]]


def test_three_channel_backbone_is_unchanged():
    from mvdet_amd.backbone import build_backbone, resnet18_trunk, vgg11_features
    torch.manual_seed(3)
    a1, a2, ca = build_backbone("resnet18")
    torch.manual_seed(3)
    b1, b2, cb = build_backbone("resnet18", in_channels=3)
    assert ca == cb == 512
    for x, y in ((a1, b1), (a2, b2)):
        sx, sy = x.state_dict(), y.state_dict()
        assert list(sx) == list(sy) and all(torch.equal(sx[k], sy[k]) for k in sx)
    assert a1[0].weight.shape == (64, 3, 7, 7)
    assert resnet18_trunk(in_channels=11)[0].weight.shape == (64, 11, 7, 7)
    assert vgg11_features()[0].weight.shape == (64, 3, 3, 3) and vgg11_features(11)[0].weight.shape == (64, 11, 3, 3)
    p1, _, _ = build_backbone("vgg11", in_channels=23)
    assert p1[0].weight.shape == (64, 23, 3, 3)


def test_library_exports_the_new_symbols():
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTS, f"{name} is not declared in _native.EXPORTS"
        assert hasattr(lib, name), f"libmvbev.so does not export {name}"
    assert lib.mvbev_version() == 12500
    # validation codes before any launch (the pointers are never dereferenced)
    import ctypes
    p = ctypes.c_void_p(16)
    s4 = _native._i64x4(1, 1, 1, 1)
    view = (_native.WarpView * 1)()
    view[0].src, view[0].src_strides = 16, _native._i64x4(12, 4, 2, 1)
    assert lib.mvbev_img_proj_forward_f32(None, 1, 1, 2, 2, 2, 2, 2, 2, p, s4, 0, None) == -5
    assert lib.mvbev_img_proj_forward_f32(view, 0, 1, 2, 2, 2, 2, 2, 2, p, s4, 0, None) == -1
    assert lib.mvbev_img_proj_forward_f32(view, 17, 1, 2, 2, 2, 2, 2, 2, p, s4, 0, None) == -2
    assert lib.mvbev_img_proj_forward_f32(view, 1, 1, 2, 2, 2, 2, 2, 2, p, s4, 2, None) == -2  # unknown flag
    view[0].src_strides = _native._i64x4(12, 4, 2, 2)
    assert lib.mvbev_img_proj_forward_f32(view, 1, 1, 2, 2, 2, 2, 2, 2, p, s4, 0, None) == -3  # column stride
    assert lib.mvbev_upsample_map_f32(None, 1, 2, 2, 4, 4, p, None) == -5
    assert lib.mvbev_upsample_map_f32(p, 1, 0, 2, 4, 4, p, None) == -1
    assert lib.mvbev_upsample_map_f32(p, 1, 4, 4, 2, 8, p, None) == -2  # a ratio < 1
    assert lib.mvbev_upsample_map_backward_f32(p, 1, 4, 4, 8, 2, p, None) == -2


def test_front_argument_errors():
    from mvdet_amd import ImageProjection
    from mvdet_amd.img_proj import img_proj_forward
    eye = [torch.eye(3, dtype=torch.float64)] * 2
    front = ImageProjection(eye, (6, 8), (5, 7))
    ok = [torch.zeros(1, 3, 12, 16) for _ in range(2)]
    with pytest.raises(ValueError, match="2 views|3 views|built for"):
        front(ok + ok[:1])
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        front([torch.zeros(1, 4, 12, 16)] * 2)  # wrong channel count
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        front([torch.zeros(3, 12, 16)] * 2)  # wrong rank
    with pytest.raises(ValueError, match=r"\[B,N,3,H,W\]"):
        front(torch.zeros(1, 3, 12, 16))  # a tensor that is not [B,N,3,H,W]
    with pytest.raises((TypeError, ValueError), match="float32"):
        front([t.double() for t in ok])
    with pytest.raises(ValueError, match="differs"):
        front([ok[0], torch.zeros(1, 3, 12, 18)])
    with pytest.raises(ValueError, match="ROCm GPU"):
        front(ok)  # CPU tensors: no fallback
    with pytest.raises(ValueError, match="1 .. 16"):
        img_proj_forward([ok[0]] * 17, [torch.eye(3)] * 17, (6, 8), (5, 7))
    with pytest.raises(ValueError, match="1 .. 16"):
        ImageProjection([torch.eye(3, dtype=torch.float64)] * 17, (6, 8), (5, 7))
    with pytest.raises(ValueError, match="positive"):
        img_proj_forward(ok, eye, (0, 8), (5, 7))


def test_upsample_and_dense_head_argument_errors():
    from mvdet_amd import DenseFuseHead, ops
    x = torch.zeros(2, 1, 5, 7)
    assert ops.upsample_map(x, (5, 7)) is x and ops.upsample_map_backward(x, (5, 7)) is x  # the elided identity
    with pytest.raises(ValueError, match=r"\[B,1,h,w\]"):
        ops.upsample_map(torch.zeros(2, 2, 5, 7), (40, 56))
    with pytest.raises(ValueError, match="ratio"):
        ops.upsample_map(x, (4, 56))
    with pytest.raises(ValueError, match="ratio"):
        ops.upsample_map_backward(torch.zeros(2, 1, 4, 56), (5, 7))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.upsample_map(x, (40, 56))
    head = DenseFuseHead((40, 56))
    w1, w2, w3 = torch.zeros(512, 512, 3, 3), torch.zeros(512, 512, 3, 3), torch.zeros(1, 512, 3, 3)
    f = torch.zeros(2, 512, 5, 7)
    with pytest.raises(ValueError, match="w1 must be"):
        head(f, torch.zeros(512, 64, 3, 3), None, w2, None, w3)
    with pytest.raises(ValueError, match="w3 must be"):
        head(f, w1, None, w2, None, torch.zeros(2, 512, 3, 3))
    with pytest.raises(ValueError, match="ROCm GPU"):
        head(f, w1, None, w2, None, w3)
    with pytest.raises(ValueError, match="larger than the grid"):
        DenseFuseHead((4, 4))(f, w1, None, w2, None, w3)
