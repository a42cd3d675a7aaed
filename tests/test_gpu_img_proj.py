"""``ImageProjVariant`` on the GPU: the fused front (resize + warp + concat + coord channels) against what the
reference class itself produced (``variant_img_proj``) and against the restatement (``img_proj_ref.front``) at
further small shapes; the map upsample and its adjoint against ``F.interpolate``; the dense head against the
fixture and, for one training step, against fp64 CPU autograd of the restatement (gate 5e-5 normwise with
``test_gpu_backward.py``'s ReLU flip rule on the GPU's own y1 / y2 patterns); the whole module in inference and in
training, with both values of ``native_map_head``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import img_proj_ref as ir
from helpers import assert_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5        # the variants' gate; CONV_TOL['bf16x3'] of the conv tests
F32_TOL = 2e-5    # the suite's tolerance for fp32 kernels


def _front(fx):
    from mvdet_amd import ImageProjection
    g, m = fx["g"], fx["g"]["meta"]
    return ImageProjection([torch.from_numpy(M) for M in g["proj_mats"]], m["upsample_shape"], m["reducedgrid_shape"])


def test_front_matches_the_reference_golden_in_both_layouts():
    fx = ir.fixture()
    g, m = fx["g"], fx["g"]["meta"]
    front = _front(fx)
    imgs = fx["imgs"].to(DEV)
    cl = front(imgs, channels_last=True)
    nchw = front(imgs, channels_last=False)
    pp = front(imgs, channels_last=True, per_pixel=False)
    N = m["num_cam"]
    assert tuple(cl.shape) == g["projected_imgs"].shape and cl.grad_fn is None
    assert cl.is_contiguous(memory_format=torch.channels_last) and nchw.is_contiguous()
    s = assert_parity(cl.cpu(), g["projected_imgs"], "projected_imgs vs the reference's", normwise_tol=TOL)
    print("front normwise", s["normwise"])
    assert torch.equal(cl, nchw), "channels-last and NCHW outputs differ"
    assert torch.equal(cl, pp), "the two thread mappings differ"
    assert np.array_equal(cl[:, 3 * N:].cpu().numpy(), np.repeat(g["coord_map"], m["B"], 0)), "coord channels"


def _rig_case(n_views, in_hw, B=2, seed=5):
    """The fixture rig's matrices (reused cyclically for ``n_views``), its resized and grid sizes, random images of
    ``in_hw``."""
    fx = ir.fixture()
    g, m = fx["g"], fx["g"]["meta"]
    mats = [torch.from_numpy(g["proj_mats"][v % m["num_cam"]]) for v in range(n_views)]
    imgs = torch.from_numpy(ir.feature_input((B, n_views, 3, *in_hw), seed)) - 0.3
    return mats, tuple(m["upsample_shape"]), tuple(m["reducedgrid_shape"]), imgs


@pytest.mark.parametrize("n_views,in_hw", [(3, (20, 30)), (3, (24, 32)), (1, (64, 86)), (16, (37, 41))],
                         ids=["upscaling-resize", "equal-size", "one-view", "sixteen-views"])
def test_front_matches_the_restatement(n_views, in_hw):
    from mvdet_amd import ImageProjection
    mats, up, grid, imgs = _rig_case(n_views, in_hw)
    ref = ir.front(imgs, mats, up, grid)
    got = ImageProjection(mats, up, grid)(imgs.to(DEV))
    assert_parity(got.cpu(), ref, f"front, {n_views} views of {in_hw}", normwise_tol=TOL)
    assert torch.equal(got[:, 3 * n_views:].cpu(), ref[:, 3 * n_views:])


def test_front_reads_a_strided_slice_in_place_and_has_no_backward():
    from mvdet_amd import ImageProjection
    mats, up, grid, imgs = _rig_case(3, (33, 47), B=4)
    wide = torch.zeros(4, 3, 3, 33, 60)
    wide[..., :47] = imgs
    sl = wide.to(DEV)[::2, :, :, :, :47]  # batch-strided, rows padded: not contiguous
    assert not sl.is_contiguous()
    ref = ir.front(imgs[::2], mats, up, grid)
    front = ImageProjection(mats, up, grid)
    got = front(sl)
    assert_parity(got.cpu(), ref, "front on a strided slice", normwise_tol=TOL)
    assert torch.equal(got, front([sl[:, v].contiguous() for v in range(3)]))
    x = imgs.to(DEV).requires_grad_()
    with pytest.raises(NotImplementedError, match="no backward"):
        front(x)
    with torch.no_grad():
        assert front(x).grad_fn is None


def test_front_materialises_no_resized_image():
    """imgs [1,4,3,360,640] -> 270 x 480 -> grid 30 x 90: the resized images would be 6.2 MB, the output is 151 KB."""
    from mvdet_amd import ImageProjection
    fx = ir.fixture()
    mats = [torch.from_numpy(fx["g"]["proj_mats"][v % 3]) for v in range(4)]
    front = ImageProjection(mats, (270, 480), (30, 90))
    imgs = torch.rand(1, 4, 3, 360, 640, device=DEV)
    first = front(imgs)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = front(imgs)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert peak < (1 << 20), peak
    assert torch.equal(out, first)


@pytest.mark.parametrize("lo,hi", [((5, 7), (40, 56)), ((15, 45), (120, 360)), ((20, 32), (160, 250))])
def test_upsample_map_forward_and_adjoint(lo, hi):
    from mvdet_amd import ops
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal((2, 1, *lo)).astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal((2, 1, *hi)).astype(np.float32))
    xd = x.double().requires_grad_()
    ref = F.interpolate(xd, list(hi), mode="bilinear")
    ref.backward(gy.double())
    got = ops.upsample_map(x.to(DEV), hi)
    assert_parity(got.cpu(), F.interpolate(x, list(hi), mode="bilinear"), f"upsample {lo}->{hi} vs F.interpolate",
                  normwise_tol=F32_TOL)
    assert_parity(got.cpu(), ref.detach(), f"upsample {lo}->{hi} vs fp64", normwise_tol=F32_TOL)
    gx = ops.upsample_map_backward(gy.to(DEV), lo)
    assert_parity(gx.cpu(), xd.grad, f"upsample adjoint {hi}->{lo} vs fp64 autograd", normwise_tol=F32_TOL)
    assert torch.equal(gx, ops.upsample_map_backward(gy.to(DEV), lo)), "the adjoint is not repeatable"
    same = x.to(DEV)
    assert ops.upsample_map(same, lo) is same and ops.upsample_map_backward(same, lo) is same


def _head_args(p, dev=DEV, grad=False):
    return [p[k].to(dev).requires_grad_(grad) for k in ir.HEAD_KEYS]


def test_dense_head_matches_the_reference_golden():
    from mvdet_amd import DenseFuseHead
    fx = ir.fixture()
    g, m = fx["g"], fx["g"]["meta"]
    head = DenseFuseHead(m["reducedgrid_shape"])
    x = torch.from_numpy(g["world_feature"]).to(DEV)
    with torch.no_grad():
        out = head(x, *_head_args(fx["params"]))
        out_cl = head(x.contiguous(memory_format=torch.channels_last), *_head_args(fx["params"]))
    s = assert_parity(out.cpu(), g["map_result"], "dense head vs the reference's map_result", normwise_tol=TOL)
    print("dense head normwise", s["normwise"])
    assert torch.equal(out, out_cl)


def test_dense_head_training_step_matches_fp64_autograd():
    from mvdet_amd import DenseFuseHead, ops
    fx = ir.fixture()
    g, m = fx["g"], fx["g"]["meta"]
    grid = m["reducedgrid_shape"]
    head = DenseFuseHead(grid)
    wf = torch.from_numpy(g["world_feature"])
    x = wf.to(DEV).requires_grad_()
    params = _head_args(fx["params"], grad=True)
    out = head(x, *params)
    fn = out.grad_fn
    assert type(fn).__name__.startswith("DenseFuseFunction")
    assert_parity(out.detach().cpu(), g["map_result"], "training-mode forward vs golden", normwise_tol=TOL)
    y1 = ops.split_decode(fn.ws.y1, 512) if fn.ws.y1.dtype == torch.bfloat16 else fn.ws.y1
    patterns = ((y1 > 0).double().cpu(), (fn.ws.y2 > 0).double().cpu())
    rng = np.random.default_rng(0)
    gmap = torch.from_numpy(rng.standard_normal(out.shape).astype(np.float32))
    out.backward(gmap.to(DEV))
    torch.cuda.synchronize()
    # a second backward through a released graph raises, as the other functions' does
    again = head(x.detach(), *params)
    grads = torch.autograd.grad(again.sum(), [params[4]], retain_graph=True)
    assert torch.isfinite(grads[0]).all()
    with pytest.raises(RuntimeError, match="second time"):
        torch.autograd.grad(again.sum(), [params[4]])

    def ref(pats):
        xr = wf.double().requires_grad_()
        p = {k: fx["params"][k].double().requires_grad_() for k in ir.HEAD_KEYS}
        o, pre = ir.head(xr, p, grid, dtype=torch.float64, patterns=pats)
        (o * gmap.double()).sum().backward()
        return [t.detach() for t in pre], xr.grad, p

    pre, _, _ = ref((None, None))
    for pat, pr in zip(patterns, pre):
        ir.relu_flips(pat, pr)
    _, gx, gp = ref(patterns)
    assert_parity(x.grad.cpu(), gx, "d world feature", normwise_tol=TOL)
    for k, t in zip(ir.HEAD_KEYS, params):
        assert_parity(t.grad.cpu(), gp[k].grad, f"d {k}", normwise_tol=TOL)


def test_dense_head_at_the_config2_size():
    """15 x 45 at B = 1 (16 conv workgroups on 256 CUs) against fp64 ``F.conv2d``: the forward and the
    world-feature gradient, through the 8x upsample to 120 x 360."""
    from mvdet_amd import DenseFuseHead, ops
    rng = np.random.default_rng(7)
    grid = (120, 360)
    wf = torch.from_numpy(np.maximum(rng.standard_normal((1, 512, 15, 45)).astype(np.float32), 0))
    p = {k: torch.from_numpy(v) for k, v in ir.params(1, 9).items() if k in ir.HEAD_KEYS}
    head = DenseFuseHead(grid)
    with torch.no_grad():
        inf = head(wf.to(DEV), *_head_args(p))
    x = wf.to(DEV).requires_grad_()
    out = head(x, *_head_args(p))
    fn = out.grad_fn
    y1 = ops.split_decode(fn.ws.y1, 512) if fn.ws.y1.dtype == torch.bfloat16 else fn.ws.y1
    patterns = ((y1 > 0).double().cpu(), (fn.ws.y2 > 0).double().cpu())
    gmap = torch.from_numpy(rng.standard_normal(out.shape).astype(np.float32))
    out.backward(gmap.to(DEV))
    xr = wf.double().requires_grad_()
    pd = {k: v.double() for k, v in p.items()}
    plain, pre = ir.head(xr, pd, grid, dtype=torch.float64)
    for pat, pr in zip(patterns, pre):
        ir.relu_flips(pat, pr.detach())
    o, _ = ir.head(xr, pd, grid, dtype=torch.float64, patterns=patterns)
    (o * gmap.double()).sum().backward()
    assert_parity(inf.cpu(), plain.detach(), "config-2 size inference forward", normwise_tol=TOL)
    assert_parity(out.detach().cpu(), plain.detach(), "config-2 size training forward", normwise_tol=TOL)
    assert_parity(x.grad.cpu(), xr.grad, "config-2 size d world feature", normwise_tol=TOL)


def _model(native_map_head=True):
    from mvdet_amd import ImageProjVariant
    fx = ir.fixture()
    model = ImageProjVariant(ir.ds_from_golden(fx["g"]), device=DEV, native_map_head=native_map_head)
    model.load_state_dict(fx["params"])
    return fx, model


def test_module_inference_matches_the_reference_golden():
    fx, model = _model(True)
    g, m = fx["g"], fx["g"]["meta"]
    model.eval()
    with torch.no_grad():
        map_res, imgs_res = model(fx["imgs"])
    assert map_res.grad_fn is None and tuple(map_res.shape) == g["map_result"].shape
    s = assert_parity(map_res.cpu(), g["map_result"], "map_result vs the reference's")  # the project gate, 1e-3
    print("module normwise", s["normwise"])
    assert len(imgs_res) == m["imgs_result_shape"][0]
    for r in imgs_res:
        assert list(r.shape) == m["imgs_result_shape"][1:] and r.grad_fn is None and not r.requires_grad
        assert r.device.type == "cuda" and float(r.abs().max()) == 0
    _, torch_head = _model(False)
    torch_head.eval()
    with torch.no_grad():
        other, _ = torch_head(fx["imgs"])
    assert_parity(other.cpu(), map_res.cpu(), "native_map_head=False vs True")
    assert_parity(other.cpu(), g["map_result"], "native_map_head=False vs the reference's")


@pytest.mark.parametrize("native", [True, False], ids=["native-head", "torch-head"])
def test_module_training_step(native):
    fx, model = _model(native)
    model.train()
    map_res, imgs_res = model(fx["imgs"])
    if native:
        assert type(map_res.grad_fn).__name__.startswith("DenseFuseFunction")
    assert all(r.grad_fn is None for r in imgs_res)
    rng = np.random.default_rng(1)
    gmap = torch.from_numpy(rng.standard_normal(map_res.shape).astype(np.float32)).to(DEV)
    (map_res * gmap).sum().backward()
    torch.cuda.synchronize()
    for name, p in model.named_parameters():
        assert name.split(".")[0] in ("base_pt1", "base_pt2", "map_classifier")
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert float(p.grad.abs().max()) > 0, name
