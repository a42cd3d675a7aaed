"""The fused image head (``mvdet_amd.upsample_relu_conv1x1``: bilinear upsample -> ReLU -> 1x1 conv for all
views in one launch, native backward) against torch-CPU fp64 autograd of
``F.conv2d(F.relu(F.interpolate(g, size, mode="bilinear")), W)`` from the same fp32 values, at the suite's
5e-5 normwise gate (``helpers.assert_parity``; torch-CPU fp32 interpolate sits at <= 7e-7 of fp64 here).

A ReLU whose pre-activation is within rounding of zero may fall either way, and one flip moves a grad_g
element by far more than the gate, so every case with random data asserts on the fp64 reference that no
``|pre| <= 1e-5 max|pre|`` (``_margin``): a condition on the data (the seeds are chosen for it), not a
tolerance.  Every case runs with ``g`` as NCHW planes and as torch channels_last."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from helpers import assert_parity, parity_stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 5e-5
LAYOUTS = ["nchw", "channels_last"]


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def _offset_randn(shape, seed):
    """0.5 N(0,1) around +-1 by channel parity: both ReLU branches inside every channel (about 1 upsampled value
    in 200 on the minority side, spread over the whole map), few values near 0 (at 490 k upsampled values per
    view plain N(0,1) data always has some within 1e-5 of zero, and so had every seed tried at +-0.75)."""
    off = torch.tensor([1.0, -1.0]).repeat((shape[1] + 1) // 2)[:shape[1]].view(1, -1, 1, 1)
    return (0.5 * _randn(shape, seed).double() + off.double()).float()


def _weight(co, cm, seed):
    return _randn((co, cm), 1000 + seed)


def _to_layout(t, layout):
    t = t.to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else t.contiguous()


def _sliced(t, layout):
    """``t`` as a non-contiguous slice of a larger tensor of the given layout."""
    B, C, h, w = t.shape
    big = _to_layout(torch.zeros(B, C + 3, h + 2, w + 5), layout)
    view = big[:, 2:2 + C, 1:1 + h, 3:3 + w]
    view.copy_(t)
    assert not view.is_contiguous() and not view.is_contiguous(memory_format=torch.channels_last)
    return view


def _margin(up, exempt=None):
    """min |pre| / max |pre| of an fp64 upsampled tensor (channels ``exempt`` left out)."""
    a = up.detach().abs()
    if exempt is not None:
        keep = [c for c in range(a.shape[1]) if c != exempt]
        a = a[:, keep]
    return (a.min() / a.max()).item()


def _reference(gs, w, size, grs=None, exempt=None, check_margin=True):
    """fp64 CPU autograd from the fp32 values: (outs, grad_gs, grad_w); grs[v] None: view v is not in the loss."""
    gd = [g.double().requires_grad_() for g in gs]
    wd = w.double().requires_grad_()
    ups = [F.interpolate(g, size, mode="bilinear") for g in gd]
    if check_margin:
        for v, u in enumerate(ups):
            m = _margin(u, exempt)
            assert m > 1e-5, f"view {v}: a pre-activation within 1e-5 of zero (min/max = {m:.2e}): pick another seed"
    outs = [F.conv2d(F.relu(u), wd.view(*wd.shape, 1, 1)) for u in ups]
    if grs is None:
        return [o.detach() for o in outs], None, None
    sum((o * gr.double()).sum() for o, gr in zip(outs, grs) if gr is not None).backward()
    return [o.detach() for o in outs], [g.grad for g in gd], wd.grad


def _run(gs_dev, w, size, grs, g_grad=True, w_grad=True):
    from mvdet_amd import upsample_relu_conv1x1
    leaves = [g.detach().requires_grad_(g_grad) for g in gs_dev]
    wl = w.to(DEV).requires_grad_(w_grad)
    outs = upsample_relu_conv1x1(leaves, wl, size)
    assert len(outs) == len(leaves)
    for o in outs:
        assert type(o.grad_fn).__name__.startswith("UpsampleReluConv1x1")
        assert o.shape == (leaves[0].shape[0], w.shape[0]) + tuple(size) and o.is_contiguous()
    sum((o * gr.to(DEV)).sum() for o, gr in zip(outs, grs) if gr is not None).backward()
    torch.cuda.synchronize()
    return outs, leaves, wl


def _check(gs, w, size, layout, sliced=(), exempt=None, seed=0):
    co = w.shape[0]
    grs = [_randn((g.shape[0], co) + tuple(size), 2000 + seed + v) for v, g in enumerate(gs)]
    ref_o, ref_g, ref_w = _reference(gs, w, size, grs, exempt)
    gs_dev = [_sliced(g, layout) if v in sliced else _to_layout(g, layout) for v, g in enumerate(gs)]
    outs, leaves, wl = _run(gs_dev, w, size, grs)
    for v in range(len(gs)):
        assert_parity(outs[v], ref_o[v], f"out {v}", normwise_tol=GATE)
        assert_parity(leaves[v].grad, ref_g[v], f"grad_g {v}", normwise_tol=GATE)
    assert_parity(wl.grad, ref_w, "grad_W", normwise_tol=GATE)
    return outs, leaves, wl


@pytest.mark.parametrize("layout", LAYOUTS)
def test_non_integer_ratio_three_views_strided(layout):
    """Case 1: 7x9 -> 20x31, 5 channels (no multiple of 4), batch 2, three views with different data, view 1 a
    non-contiguous slice of a larger tensor."""
    gs = [_randn((2, 5, 7, 9), s) for s in CASE1_SEEDS]
    _check(gs, _weight(2, 5, 1), (20, 31), layout, sliced=(1,), seed=1)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_product_channels_exact_3x(layout):
    """Case 2: the product's 64 channels at exact 3x (upsampled index 3k + 1 sits on a source pixel: zero-weight
    taps)."""
    _check([_randn((1, 64, 6, 8), 0)], _weight(2, 64, 2), (18, 24), layout, seed=2)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_source_row_clamped_taps(layout):
    """Case 3: one source row: i1 == i0 along y, both taps count in the adjoint."""
    _check([_randn((1, 8, 1, 5), 0)], _weight(2, 8, 3), (3, 15), layout, seed=3)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_scale_one(layout):
    """Case 4: scale 1, Co = 1."""
    _check([_randn((2, 3, 4, 6), 0)], _weight(1, 3, 4), (4, 6), layout, seed=4)


def _case5():
    gs = [_offset_randn((1, 64, 23, 37), s) for s in CASE5_SEEDS]
    return gs, _weight(2, 64, 5), (69, 111)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_many_tiles_ragged_edges(layout):
    """Case 5: 23x37 -> 69x111, 2 views: several tiles in each direction, forward and backward, ragged edges."""
    gs, w, size = _case5()
    for g in gs:  # the data keeps both ReLU branches inside channels
        up = F.interpolate(g.double(), size, mode="bilinear")
        mixed = ((up > 0).flatten(2).any(2) & (up < 0).flatten(2).any(2)).sum().item()
        assert mixed == 64, mixed
    _check(gs, w, size, layout, seed=5)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_exact_zero_channel(layout):
    """Case 6: case 2 with channel 7 of g exactly 0: pre is exactly 0 there, so its contribution, its grad_g and
    its grad_W column are exactly 0 on both sides (that channel is exempt from the margin condition)."""
    g = _randn((1, 64, 6, 8), 0)
    g[:, 7] = 0
    w = _weight(2, 64, 2)
    w0 = w.clone()
    w0[:, 7] = 0
    outs, leaves, wl = _check([g], w, (18, 24), layout, exempt=7, seed=2)
    assert (leaves[0].grad[:, 7] == 0).all() and (wl.grad[:, 7] == 0).all()
    from mvdet_amd import upsample_relu_conv1x1
    with torch.no_grad():  # the channel adds exactly nothing: the same bits without its weights
        o0 = upsample_relu_conv1x1([leaves[0].detach()], w0.to(DEV), (18, 24))[0]
    assert torch.equal(o0, outs[0].detach())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_nonfinite_forward_pattern(layout):
    """Case 7: +inf, -inf and NaN at three interior pixels of g (case 2's shape) and one NaN in W: the NaN / inf
    pattern equals the reference's exactly (zero-weight taps multiply: 0 * inf = NaN; ReLU keeps NaN)."""
    from mvdet_amd import upsample_relu_conv1x1
    g = _randn((1, 64, 6, 8), 0)
    g[0, 3, 2, 3] = float("inf")
    g[0, 9, 3, 5] = float("-inf")
    g[0, 20, 4, 2] = float("nan")
    w = _weight(2, 64, 2)
    for poison_w in (False, True):
        if poison_w:
            w[1, 11] = float("nan")
        ref, _, _ = _reference([g], w, (18, 24), check_margin=False)
        nf = ~torch.isfinite(ref[0])
        assert 0 < int(nf.sum()) and int(torch.isnan(ref[0]).sum()) > 0
        if not poison_w:
            assert int(torch.isinf(ref[0]).sum()) > 0 and int(nf.sum()) < ref[0].numel()
        with torch.no_grad():
            out = upsample_relu_conv1x1([_to_layout(g, layout)], w.to(DEV), (18, 24))[0]
        s = parity_stats(out, ref[0])  # asserts the NaN and the non-finite patterns are equal
        assert s["n_bad"] == 0 and s["normwise"] <= GATE, s


@pytest.mark.parametrize("val", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_nonfinite_weight_meets_an_exact_zero_channel(layout, val):
    """A non-finite 1x1 weight (a diverging ``optimizer.step()``) on ``test_exact_zero_channel``'s all-zero channel 7
    of finite features: the reference multiplies 0 * NaN and 0 * inf = NaN at every pixel of that output channel
    (a kernel that skipped a zero activation would stay finite); on a general channel 12 of output 0, +-inf where
    the ReLU passes and NaN where it gives 0.  NaN, +inf and -inf patterns equal the fp64 reference's, the finite
    entries pass the gate."""
    from mvdet_amd import upsample_relu_conv1x1
    g = _randn((1, 64, 6, 8), 0)
    g[:, 7] = 0
    w = _weight(2, 64, 2)
    w[1, 7] = val
    w[0, 12] = val
    ref = _reference([g], w, (18, 24), check_margin=False)[0][0]
    assert torch.isnan(ref[0, 1]).all()
    if val == val:
        assert 0 < int(torch.isinf(ref[0, 0]).sum()) and 0 < int(torch.isnan(ref[0, 0]).sum()) < ref[0, 0].numel()
    with torch.no_grad():
        out = upsample_relu_conv1x1([_to_layout(g, layout)], w.to(DEV), (18, 24))[0].cpu()
    assert torch.equal(torch.isposinf(out), torch.isposinf(ref)) and torch.equal(torch.isneginf(out), torch.isneginf(ref))
    s = parity_stats(out, ref)  # asserts the NaN and the non-finite patterns are equal
    assert s["n_bad"] == 0 and s["normwise"] <= GATE, s


@pytest.mark.parametrize("layout", LAYOUTS)
def test_selective_gradients(layout):
    """Case 8: W without grad; g without grad; a loss over views 0 and 2 only.  Wanted gradients match, the
    others are None."""
    gs = [_randn((2, 5, 7, 9), s) for s in CASE1_SEEDS]
    w, size = _weight(2, 5, 1), (20, 31)
    grs = [_randn((2, 2) + size, 2100 + v) for v in range(3)]
    ref_o, ref_g, ref_w = _reference(gs, w, size, grs)
    gs_dev = [_to_layout(g, layout) for g in gs]
    _, leaves, wl = _run(gs_dev, w, size, grs, w_grad=False)
    assert wl.grad is None
    for v in range(3):
        assert_parity(leaves[v].grad, ref_g[v], f"W frozen: grad_g {v}", normwise_tol=GATE)
    _, leaves, wl = _run(gs_dev, w, size, grs, g_grad=False)
    assert all(l.grad is None for l in leaves)
    assert_parity(wl.grad, ref_w, "g frozen: grad_W", normwise_tol=GATE)
    grs[1] = None
    _, ref_g, ref_w = _reference(gs, w, size, grs)
    assert ref_g[1] is None
    _, leaves, wl = _run(gs_dev, w, size, grs)
    assert leaves[1].grad is None
    for v in (0, 2):
        assert_parity(leaves[v].grad, ref_g[v], f"views 0 and 2: grad_g {v}", normwise_tol=GATE)
    assert_parity(wl.grad, ref_w, "views 0 and 2: grad_W", normwise_tol=GATE)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_backward_is_bitwise_repeatable(layout):
    """Case 9: case 5's backward twice: every gradient has the same bits."""
    gs, w, size = _case5()
    grs = [_randn((1, 2) + size, 2200 + v) for v in range(2)]
    gs_dev = [_to_layout(g, layout) for g in gs]
    _, l1, w1 = _run(gs_dev, w, size, grs)
    _, l2, w2 = _run(gs_dev, w, size, grs)
    assert torch.equal(w1.grad, w2.grad)
    for a, b in zip(l1, l2):
        assert torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_no_upsampled_intermediate_is_kept(layout):
    """Case 10: with grad enabled the forward keeps less than half of one upsampled intermediate
    (0.5 * 64 * 90 * 120 * 4 B = 1.38 MB; the outputs are 86 kB; the torch sequence keeps two intermediates)."""
    from mvdet_amd import upsample_relu_conv1x1
    g = _to_layout(_randn((1, 64, 30, 40), 0), layout).requires_grad_()
    w = _weight(2, 64, 2).to(DEV).requires_grad_()
    upsample_relu_conv1x1([g], w, (90, 120))  # warm-up: the library and its code objects are loaded
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    outs = upsample_relu_conv1x1([g], w, (90, 120))
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    assert outs[0].requires_grad
    assert grown < 0.5 * 64 * 90 * 120 * 4, grown


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape,size", [((1, 64, 90, 160), (270, 480)), ((2, 16, 7, 9), (20, 31)),
                                        ((1, 8, 9, 11), (27, 33))])
def test_pre_activation_has_the_bits_of_gpu_interpolate(layout, shape, size):
    """The kernel's pre-activation is F.interpolate's on this GPU bit for bit, so its ReLU pattern is the one
    the torch ops had (and the one mask tests replay from ``F.interpolate(g) > 0``): with identity weights the
    output is relu(pre) exactly.  Config 2's head shape, a non-integer ratio and a channel count below 16
    (where torch's channels-last upsample falls back to its NCHW arithmetic), plain N(0,1) data, both layouts."""
    from mvdet_amd import upsample_relu_conv1x1
    g = _to_layout(_randn(shape, 7), layout)
    eye = torch.eye(shape[1], device=DEV)
    with torch.no_grad():
        ref = F.interpolate(g, size, mode="bilinear")
        mine = torch.cat([upsample_relu_conv1x1([g], eye[c:c + 4].contiguous(), size)[0]
                          for c in range(0, shape[1], 4)], 1)
    assert torch.equal((mine > 0), (ref > 0).contiguous())
    assert torch.equal(mine.view(torch.int32), F.relu(ref).contiguous().view(torch.int32))


# ---- through the detector -----------------------------------------------------------------------------------

def _detector(native, seed):
    """tests/test_gpu_nonfinite.py's recipe: a 2-view synthetic rig, C = 64, identity backbone, heads rebuilt
    for C, train mode.  The head's first conv gets biases of +-1.5 by channel parity (see ``_offset_randn``)."""
    from mvdet_amd import PerspTransDetector, ProjectFuse, synthetic
    from oracle import fixtures
    C, N = 64, 2
    ds = synthetic.wildtrack_like(N, 4, seed=0, img_shape=(216, 384), worldgrid_shape=(96, 288))
    params = fixtures.head_params(N, seed=11, C=C)
    up, grid = tuple(ds.upsample_shape), tuple(ds.reducedgrid_shape)
    model = PerspTransDetector(ds, native_img_head=native)
    mc = nn.Sequential(nn.Conv2d(C * N + 2, 512, 3, padding=1), nn.ReLU(),
                       nn.Conv2d(512, 512, 3, padding=2, dilation=2), nn.ReLU(),
                       nn.Conv2d(512, 1, 3, padding=4, dilation=4, bias=False))
    mc.load_state_dict({k.replace("map_classifier.", ""): torch.from_numpy(v) for k, v in params.items()
                        if k.startswith("map_classifier.")})
    model.map_classifier = mc.to(DEV)
    model.img_classifier = _img_head(C, seed).to(DEV)
    model.engine = ProjectFuse(model.proj_mats, up, grid, C)
    model.base_pt1, model.base_pt2 = nn.Identity(), nn.Identity()
    model.train()
    hb = [u // 3 for u in up]
    low = torch.stack([_randn((1, C, *hb), seed + 10 + v) for v in range(N)], 1)
    return model, low, up


def _img_head(C, seed):
    gen = torch.Generator().manual_seed(seed)
    head = nn.Sequential(nn.Conv2d(C, 64, 1), nn.ReLU(), nn.Conv2d(64, 2, 1, bias=False))
    with torch.no_grad():
        head[0].weight.copy_(torch.randn(head[0].weight.shape, generator=gen) / 16)
        head[0].bias.copy_(torch.tensor([1.5, -1.5]).repeat(32))
        head[2].weight.copy_(torch.randn(head[2].weight.shape, generator=gen) / 8)
    return head


def test_detector_uses_the_native_head_and_matches_the_torch_path():
    outs = {}
    for native in (True, False):
        model, low, up = _detector(native, DETECTOR_SEED)
        x = low.to(DEV).requires_grad_()
        pre = []
        hook = model.img_classifier[0].register_forward_hook(
            lambda m, i, o: pre.append(F.interpolate(o.detach(), up, mode="bilinear")))
        _, imgs = model(x)
        hook.remove()
        assert len(pre) == 2 and len(imgs) == 2
        for r in imgs:
            name = type(r.grad_fn).__name__
            if native:
                assert name.startswith("UpsampleReluConv1x1"), name
            else:
                assert "onvolution" in name and "UpsampleRelu" not in name, name  # torch's own conv
            assert r.shape == (1, 2) + up
        if not native:
            for v, p in enumerate(pre):
                m = _margin(p.double())
                assert m > 1e-5, f"view {v}: a pre-activation within 1e-5 of zero (min/max = {m:.2e})"
                assert 0 < (p > 0).float().mean().item() < 1
        grs = [_randn(r.shape, 2300 + v).to(DEV) for v, r in enumerate(imgs)]
        sum((r * gr).sum() for r, gr in zip(imgs, grs)).backward()
        torch.cuda.synchronize()
        head = model.img_classifier
        outs[native] = ([r.detach().cpu() for r in imgs], x.grad.cpu(),
                        {k: p.grad.cpu() for k, p in head.named_parameters()})
    (imgs_n, dx_n, par_n), (imgs_t, dx_t, par_t) = outs[True], outs[False]
    for v in range(2):
        assert_parity(imgs_n[v], imgs_t[v], f"imgs_result {v}", normwise_tol=GATE)
        assert_parity(dx_n[:, v], dx_t[:, v], f"d input features view {v}", normwise_tol=GATE)
    assert sorted(par_n) == ["0.bias", "0.weight", "2.weight"]
    for k in par_n:
        assert_parity(par_n[k], par_t[k], f"d img_classifier.{k}", normwise_tol=GATE)


# seeds that meet the margin condition (asserted in every case): found on the CPU from the fp64 reference
CASE1_SEEDS = (0, 1, 4)
CASE5_SEEDS = (3, 13)
DETECTOR_SEED = 11
