"""NaN / inf in a PARAMETER of ``map_classifier`` (a diverging ``optimizer.step()``): the map's NaN / inf pattern
must be the reference's (``persp_trans_detector.py:51-54`` over ``:65-82`` on the CPU oracle), as it is for non-finite
geometry and non-finite features (``test_gpu_nonfinite.py``).

The fast path cannot keep that pattern: its frustum mask never multiplies a masked view's w1 columns (the reference
computes 0 * NaN = NaN at every pixel), the hi/lo bf16 split of +-inf is (inf, NaN) and the Winograd weight
transform G w takes differences of weights, where the reference keeps ``x * -inf = -inf``, which ReLU turns into 0 —
a finite map value.  So the parameters raise the non-finite guard's flag (``ProjectFuse.param_word``: a device word
per weight version, no host sync) and the gated exact path rewrites the map.  Every poison sits at a centre tap
(``nonfinite_weight_cases``: what a non-finite weight does against zero padding is the conv back end's business).
The cases' oracle maps are pinned on the CPU by ``test_oracle.py::test_nonfinite_weight_cases_discriminate``."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import nonfinite_weight_cases as nw
from helpers import assert_parity_t, masked_relu
from oracle import cpu_path
from test_gpu_nonfinite import _mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, PINF, NINF = nw.NAN, nw.PINF, nw.NINF


def assert_pattern(got, ref, what, normwise_tol=1e-3):
    """The parity gate with the NaN, +inf and -inf patterns equal."""
    g, r = got.detach().cpu(), ref.detach().cpu()
    assert torch.equal(torch.isposinf(g), torch.isposinf(r)), f"{what}: +inf pattern differs"
    assert torch.equal(torch.isneginf(g), torch.isneginf(r)), f"{what}: -inf pattern differs"
    return assert_parity_t(g, r, what, normwise_tol=normwise_tol)


def _poke(param, idx, val):
    """Write ``val`` in place (bumps ``_version``: packs, coord term and the parameter word follow); the old value."""
    with torch.no_grad():
        old = param[idx].item()
        param[idx] = val
    return old


@functools.lru_cache(maxsize=None)
def _rig():
    """The shared rig of the inference cases: dataset, head parameters, matrices, CPU features, the finite oracle
    map and per case the poisoned oracle map (computed once, never modified)."""
    from mvdet_amd.geometry import projection_matrices
    ds, params = nw.rig()
    pm = projection_matrices(ds)
    mats = [M.numpy() for M in pm]
    feats = nw.features(ds)
    grid = tuple(ds.reducedgrid_shape)
    with torch.no_grad():
        fine = cpu_path.project_fuse(feats, mats, grid, {k: torch.from_numpy(v) for k, v in params.items()})
        refs = {name: cpu_path.project_fuse(feats, mats, grid, nw.poisoned(params, name)) for name in nw.CASES}
    return ds, params, pm, feats, fine, refs


# -- (a) the engine, inference from upsampled maps -------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(nw.CASES))
def test_engine_inference_nonfinite_parameter(case):
    """``ProjectFuse.project_fuse`` (fused warp + B^T, Winograd convs) with one parameter poisoned in place on the
    GPU module: the flag fires, the map has the oracle's pattern; the finite value restored in place, the next
    frame does not fire the flag, is finite and is bitwise the map computed before the poisoning (packs, coord
    term and the parameter word follow the weights in both directions)."""
    from mvdet_amd import ProjectFuse
    ds, params, pm, cpu_feats, ref_fine, refs = _rig()
    key, idx, val, kind = nw.CASES[case]
    C, N = nw.RIG_C, ds.num_cam
    up, grid = tuple(ds.upsample_shape), tuple(ds.reducedgrid_shape)
    mc = _mc(C, N, params)
    eng = ProjectFuse(pm, up, grid, C)
    feats = [f.to(DEV) for f in cpu_feats]
    param = dict(mc.named_parameters())[key]
    ref = refs[case]
    nw.check_kind(ref, kind)
    if kind == "partial":
        assert 0 < int(torch.isfinite(ref).sum()) < ref.numel()
    with torch.no_grad():
        before = eng.project_fuse(feats, mc).clone()
        ws = eng.workspace(1, DEV)
        assert int(ws.nf.item()) != ws.nf_tag and torch.isfinite(before).all()
        # a fresh engine packs everything on its first frame: the parameter scan rode on those launches
        st = eng._param_words[str(param.device)]
        assert st.done and st.covered == {"w1_views", "w1_coord", "b1", "w2", "b2", "w3"}
        old = _poke(param, idx, val)
        got = eng.project_fuse(feats, mc).clone()
        assert int(ws.nf.item()) == ws.nf_tag, "the non-finite parameter did not raise the guard's flag"
        again = eng.project_fuse(feats, mc).clone()  # the same weight version: the word is not recomputed
        assert int(ws.nf.item()) == ws.nf_tag
        _poke(param, idx, old)
        after = eng.project_fuse(feats, mc).clone()
        assert int(ws.nf.item()) != ws.nf_tag, "the flag fired on finite weights"
    assert_pattern(got, ref, f"engine, {case} (NaN / inf pattern included)")
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    assert torch.isfinite(after).all()
    assert_parity_t(after, ref_fine, "engine, finite weights restored", normwise_tol=5e-5)
    assert torch.equal(after, before), "the map after restoring the weights is not bitwise the map before"


@pytest.mark.parametrize("case", ["w1_view_nan", "w1_view_ninf", "w2_ninf"])
def test_engine_cases_discriminate_without_the_guard(case):
    """Without the guard the fast path's NaN pattern is not the oracle's — the cases the parameter flag exists
    for: ``w1 = NaN`` on a view-1 channel (the last tile column lies outside view 1's frustum, so the mask never
    multiplies the weight there and the map's last columns stay finite; the oracle is all NaN), ``w1 = -inf`` and
    ``w2 = -inf`` (the hi/lo split and G w turn inf into NaN; the oracle is partly finite)."""
    from mvdet_amd import ProjectFuse
    ds, params, pm, cpu_feats, _, refs = _rig()
    key, idx, val, _ = nw.CASES[case]
    C, N = nw.RIG_C, ds.num_cam
    up, grid = tuple(ds.upsample_shape), tuple(ds.reducedgrid_shape)
    mc = _mc(C, N, params)
    eng = ProjectFuse(pm, up, grid, C)
    assert eng.conv1_active_fraction(DEV, 0, grid[0], grid=True) < 1.0  # some (tile, view) pair is masked
    feats = [f.to(DEV) for f in cpu_feats]
    _poke(dict(mc.named_parameters())[key], idx, val)
    eng.nonfinite_guard = False
    with torch.no_grad():
        fast = eng.project_fuse(feats, mc).clone()
    torch.cuda.synchronize()
    assert not torch.equal(torch.isnan(fast.cpu()), torch.isnan(refs[case]))


# -- (b) the drop-in module ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["w1_view_nan", "w2_ninf"])
def test_detector_nonfinite_parameter(case):
    """``PerspTransDetector``'s default inference path (backbone-resolution maps -> channels-last copy -> fused
    upsample + warp + B^T -> Winograd convs) with a poisoned ``map_classifier`` parameter: map_result with the
    oracle's pattern and the flag raised; imgs_result is unaffected.  The value restored in place, the next frame
    does not fire the flag, is finite and is bitwise the frame before the poisoning."""
    from mvdet_amd import PerspTransDetector, ProjectFuse, synthetic
    from mvdet_amd.geometry import projection_matrices
    ds, params = nw.rig()
    C, N, B = nw.RIG_C, ds.num_cam, 1
    up, grid = tuple(ds.upsample_shape), tuple(ds.reducedgrid_shape)
    hb = [u // 3 for u in up]
    key, idx, val, kind = nw.CASES[case]
    model = PerspTransDetector(ds)
    model.map_classifier = _mc(C, N, params)
    model.img_classifier = nn.Sequential(nn.Conv2d(C, 64, 1), nn.ReLU(), nn.Conv2d(64, 2, 1, bias=False)).to(DEV)
    model.engine = ProjectFuse(model.proj_mats, up, grid, C)
    model.base_pt1, model.base_pt2 = nn.Identity(), nn.Identity()
    model.eval()
    low = [synthetic.backbone_features(B, C, hb, seed=300 + v, device=DEV) for v in range(N)]
    param = dict(model.map_classifier.named_parameters())[key]
    eng = model.engine
    with torch.no_grad():
        before = model(torch.stack(low, 1))[0].clone()
        old = _poke(param, idx, val)
        map_res, imgs_res = model(torch.stack(low, 1))
        map_res = map_res.clone()
        ws = eng.workspace(B, DEV)
        assert ws.t_from_warp and eng.wino_active(DEV)
        assert int(ws.nf.item()) == ws.nf_tag, "the non-finite parameter did not raise the guard's flag"
        _poke(param, idx, old)
        after = model(torch.stack(low, 1))[0].clone()
        assert int(ws.nf.item()) != ws.nf_tag, "the flag fired on finite weights"
        assert torch.isfinite(after).all() and torch.equal(after, before)
        torch.cuda.synchronize()
        ups = [cpu_path.upsample(f.cpu(), up) for f in low]
        ref = cpu_path.project_fuse(ups, [M.numpy() for M in projection_matrices(ds)], grid,
                                    nw.poisoned(params, case))
        head = model.img_classifier.cpu()
        ref_imgs = [head(u) for u in ups]
    assert int(torch.isnan(ref).sum()) > 0
    if kind == "partial":
        assert 0 < int(torch.isfinite(ref).sum()) < ref.numel()
    assert_pattern(map_res, ref, f"detector, {case}: map_result (NaN / inf pattern included)")
    for v in range(N):
        assert torch.isfinite(imgs_res[v]).all()
        assert_parity_t(imgs_res[v], ref_imgs[v], f"detector, {case}: imgs_result {v}")


# -- (d) the training step -------------------------------------------------------------------------------------------

TRAIN_CASES = {"w2_nan": ("2.weight", (9, 17, 1, 1), NAN), "b1_ninf": ("0.bias", (7,), NINF)}


def _train_rig():
    from mvdet_amd import synthetic
    from mvdet_amd.geometry import projection_matrices
    C = 128
    ds, params = nw.rig(C=C, seed=5)
    up = tuple(ds.upsample_shape)
    low = [synthetic.backbone_features(1, C, [u // 3 for u in up], seed=700 + v) for v in range(ds.num_cam)]
    ups = [F.interpolate(f, list(up), mode="bilinear") for f in low]  # generic sample coordinates
    return C, ds, params, projection_matrices(ds), ups


@functools.lru_cache(maxsize=None)
def _train_step(case):
    """One training step on the GPU with ``case``'s parameter poisoned, and CPU autograd through the
    ``masked_relu`` reference with the GPU's activation masks: a dict of CPU tensors (computed once per case)."""
    from mvdet_amd import ProjectFuse
    from mvdet_amd.autograd import project_fuse
    C, ds, params, pm, ups = _train_rig()
    N, B = ds.num_cam, 1
    up, grid = tuple(ds.upsample_shape), tuple(ds.reducedgrid_shape)
    key, idx, val = TRAIN_CASES[case]
    mc = _mc(C, N, params)
    _poke(dict(mc.named_parameters())[key], idx, val)
    eng = ProjectFuse(pm, up, grid, C)
    feats = [f.to(DEV).requires_grad_() for f in ups]
    out = project_fuse(eng, feats, mc)
    ws = out.grad_fn.ws
    assert ws.train_t_only and ws.t_from_warp and ws.guard_src is None  # the guard ran and closed the frame
    fired = int(ws.nf.item()) == ws.nf_tag
    m1, m2 = (eng.y1_fp32(ws) > 0).float().cpu(), (ws.y2 > 0).float().cpu()
    gmap = torch.randn(out.shape, generator=torch.Generator().manual_seed(1))
    out.backward(gmap.to(DEV))
    # the reference: torch-CPU autograd through the kornia restatement, cat, the convs
    fr = [f.clone().requires_grad_() for f in ups]
    pr = {k: v.requires_grad_() for k, v in nw.poisoned(params, (key, idx, val, None)).items()
          if k.startswith("map_classifier.")}
    warped = cpu_path.warp_views(fr, [M.numpy() for M in pm], grid)
    x = torch.cat(warped + [cpu_path.coord_map(*grid).repeat([B, 1, 1, 1])], 1)
    pre1 = F.conv2d(x, pr["map_classifier.0.weight"], pr["map_classifier.0.bias"], padding=1)
    pre2 = F.conv2d(masked_relu(pre1, m1), pr["map_classifier.2.weight"], pr["map_classifier.2.bias"], padding=2,
                    dilation=2)
    ref = F.conv2d(masked_relu(pre2, m2), pr["map_classifier.4.weight"], None, padding=4, dilation=4)
    ref.backward(gmap)
    got = dict(mc.named_parameters())
    keys = ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight")
    return dict(fired=fired, out=out.detach().cpu(), ref=ref.detach(), m1=m1, m2=m2, pre1=pre1.detach(),
                pre2=pre2.detach(), y1=masked_relu(pre1, m1).detach(),
                feat=[(feats[v].grad.cpu(), fr[v].grad) for v in range(N)],
                param={k: (got[k].grad.cpu(), pr["map_classifier." + k].grad) for k in keys})


def _check_gradients(case, pairs):
    """``~isfinite`` equal to the reference's and the finite entries within the gate, for every pair; the figures
    of every pair are printed before the first assertion."""
    bad, n_ref = [], 0
    for what, g, r in pairs:
        diff = int((torch.isfinite(g) != torch.isfinite(r)).sum())
        n_ref += int((~torch.isfinite(r)).sum())
        print(f"{case}: {what}: non-finite {int((~torch.isfinite(g)).sum())} (reference "
              f"{int((~torch.isfinite(r)).sum())}) of {r.numel()}, differing {diff}")
        if diff:
            bad.append((what, diff))
    assert not bad, f"{case}: non-finite entries differ: {bad}"
    for what, g, r in pairs:
        fin = torch.isfinite(r)
        if fin.any():
            assert_parity_t(g[fin], r[fin], f"{case}: {what}, finite entries")
    return n_ref


@pytest.mark.parametrize("case", sorted(TRAIN_CASES))
def test_training_forward_nonfinite_parameter_vs_cpu(case):
    """A training step (``autograd.project_fuse`` from upsampled features, C = 128) with a poisoned parameter: the
    flag fires, the forward map has the oracle's pattern, and the exact activations are the ones the backward
    reads (the ``ws`` masks against torch's).  ``w2 = NaN`` makes y2's channel 9 and the map NaN; ``b1[7] = -inf``
    is a dead channel, everything finite."""
    t = _train_step(case)
    assert t["fired"], "the non-finite parameter did not raise the guard's flag"
    for m, pre in ((t["m1"], t["pre1"]), (t["m2"], t["pre2"])):  # the GPU's pattern is torch's up to fp32 rounding near 0
        fin = torch.isfinite(pre)
        flip = (m != (pre > 0).float()) & fin
        assert flip.sum().item() <= max(2, pre.numel() // 20000)
        assert (pre[flip].abs() <= 1e-4 * pre[fin].abs().max()).all()
        assert torch.equal(m[~fin].bool(), (pre[~fin] > 0))
    ref = t["ref"]
    assert not torch.isinf(ref).any()
    if case == "w2_nan":
        assert torch.isnan(ref).all() and torch.isnan(t["pre2"][:, 9]).all()
    else:
        assert torch.isfinite(ref).all() and torch.count_nonzero(t["y1"][:, 7]) == 0
    assert_pattern(t["out"], ref, f"training forward, {case} (NaN / inf pattern)")


@pytest.mark.parametrize("case", sorted(TRAIN_CASES))
def test_training_parameter_gradients_nonfinite_parameter_vs_cpu_autograd(case):
    """The same step's gradients of w1, b1, w2, b2 and w3: non-finite exactly where CPU autograd through the
    ``masked_relu`` reference is, the finite entries within the gate.  ``w2 = NaN``: dy1's channel 17 is NaN where
    y1's is positive, so conv1's row 17 of dW and db are NaN, and conv3's dW is NaN in channel 9."""
    t = _train_step(case)
    n_ref = _check_gradients(case, [(f"d {k}", g, r) for k, (g, r) in t["param"].items()])
    assert (n_ref > 0) == (case == "w2_nan")


@pytest.mark.parametrize("case", sorted(TRAIN_CASES))
def test_training_feature_gradients_nonfinite_parameter_vs_cpu_autograd(case):
    """The same step's feature gradients: non-finite exactly where CPU autograd is, the finite entries within the
    gate.  ``w2 = NaN``: the reference's feature gradient is NaN at the source pixels sampled by a grid pixel with a
    positive y1[17] in its 3 x 3 neighbourhood.

    conv1's row-Winograd data gradient alone cannot do that: B^T mixes the five dy1 rows under a 3-row tile, so a NaN
    of dy1 reaches every output row of its tile (144128 / 169600 / 151936 non-finite entries per view against the
    reference's 128512 / 155008 / 136192 of 663552, none missing).  The direct data gradient behind it, gated on
    the forward's flag (``autograd._dgrad1_exact``), rewrites the tiles and gives the reference's entries."""
    t = _train_step(case)
    n_ref = _check_gradients(case, [(f"d features view {v}", g, r) for v, (g, r) in enumerate(t["feat"])])
    assert (n_ref > 0) == (case == "w2_nan")


def test_training_steps_finite_poisoned_finite_on_one_engine():
    """Three consecutive training steps on one engine, the weights updated in place between them (as an optimizer
    does): finite -> ``w2 = NaN`` -> finite again.  The flag fires only on the middle step; the outer steps are
    finite, equal bitwise (map and conv3's weight gradient) and within the gate of the oracle."""
    from mvdet_amd import ProjectFuse
    from mvdet_amd.autograd import project_fuse
    C, ds, params, pm, ups = _train_rig()
    N = ds.num_cam
    up, grid = tuple(ds.upsample_shape), tuple(ds.reducedgrid_shape)
    key, idx, val = TRAIN_CASES["w2_nan"]
    mc = _mc(C, N, params)
    eng = ProjectFuse(pm, up, grid, C)
    feats = [f.to(DEV) for f in ups]
    gmap = torch.randn((1, 1) + grid, generator=torch.Generator().manual_seed(2)).to(DEV)
    param = dict(mc.named_parameters())[key]
    steps = []
    for poison in (False, True, False):
        if poison:
            old = _poke(param, idx, val)
        mc.zero_grad(set_to_none=True)
        out = project_fuse(eng, [f.clone().requires_grad_() for f in feats], mc)
        ws = out.grad_fn.ws
        fired = int(ws.nf.item()) == ws.nf_tag
        out.backward(gmap)
        steps.append((fired, out.detach().clone(), mc[4].weight.grad.clone()))
        if poison:
            _poke(param, idx, old)
    assert [s[0] for s in steps] == [False, True, False]
    assert torch.isnan(steps[1][1]).all()
    for s in (steps[0], steps[2]):
        assert torch.isfinite(s[1]).all() and torch.isfinite(s[2]).all()
    assert torch.equal(steps[0][1], steps[2][1]) and torch.equal(steps[0][2], steps[2][2])
    with torch.no_grad():
        ref = cpu_path.project_fuse(ups, [M.numpy() for M in pm], grid,
                                    {k: torch.from_numpy(v) for k, v in params.items()})
    assert_parity_t(steps[2][1], ref, "training forward, finite step after a poisoned one", normwise_tol=5e-5)


# -- (e) the exact path's building blocks ----------------------------------------------------------------------------

def _conv_ref(x, w, b, d):
    """``conv2d(x, w, b, padding=d, dilation=d)`` as plain fp64 products and sums (one tap at a time: every product
    is formed, 0 * inf = NaN, whatever a conv library does), as fp32."""
    B, cin, H, W = x.shape
    xp = F.pad(x.double(), (d, d, d, d))
    out = torch.zeros(B, w.shape[0], H, W, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, :, ky * d:ky * d + H, kx * d:kx * d + W]
            out += (xs[:, None] * w.double()[None, :, :, ky, kx, None, None]).sum(2)
    if b is not None:
        out += b.double().view(1, -1, 1, 1)
    return out.float()


def _signed(x, g):
    """Features with exact zeros (0 * inf = NaN) and negatives."""
    x = torch.randn(x, generator=g)
    x[torch.rand(x.shape, generator=g) < 0.2] = 0.0
    return x


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("H,W,d", [(9, 70, 1), (9, 70, 2), (4, 32, 1), (4, 32, 2)])
def test_conv3x3_fp32_nonfinite_centre_weights(H, W, d, relu):
    """``ops.conv3x3`` at fp32 precision (the exact path's conv1 / conv2) with NaN, +inf and -inf at centre taps,
    cin = 19 (K padded to the pack's multiple, the padding channels 1e30 against zero weights), an input with
    exact zeros and negatives: NaN, +inf and -inf patterns and the finite values are the plain fp64 sum's."""
    from mvdet_amd import ops
    g = torch.Generator().manual_seed(H * 100 + W + d)
    B, cin, cout = 1, 19, 128
    x = _signed((B, cin, H, W), g)
    w = (torch.rand(cout, cin, 3, 3, generator=g) - 0.5) / (cin * 9) ** 0.5
    b = torch.rand(cout, generator=g) - 0.5
    w[3, 5, 1, 1] = NAN
    w[10, 2, 1, 1] = PINF
    w[20, 7, 1, 1] = NINF
    w[30, 1, 1, 1], w[30, 4, 1, 1] = PINF, NINF  # both signs into one output channel
    w[127, 18, 1, 1] = NINF  # the last real channel, next to the padding
    ref = _conv_ref(x, w, b, d)
    if relu:
        ref = F.relu(ref)
    assert torch.isnan(ref[:, 3]).all() and 0 < int(torch.isnan(ref[:, 10]).sum()) < ref[:, 10].numel()
    assert int(torch.isposinf(ref[:, 10]).sum()) > 0 and (relu or int(torch.isneginf(ref[:, 10]).sum()) > 0)
    K = ops.padded_channels(cin)
    xp = torch.full((B, K, H, W), 1e30)
    xp[:, :cin] = x
    pk = ops.PackedConv3x3(list(range(cin)) + [-1] * (K - cin), "fp32").get(w.to(DEV))
    got = ops.conv3x3(xp.to(DEV), pk, cout, b.to(DEV), d, relu).cpu()
    assert_pattern(got, ref, f"conv3x3 fp32, non-finite centre weights, dilation {d}", normwise_tol=2e-5)


@pytest.mark.parametrize("W", [70, 72])  # the scalar kernel, and the 4-pixel one (W % 4 == 0)
def test_conv3x3_cout1_nonfinite_centre_weights(W):
    """``ops.conv3x3_cout1`` (the exact path's conv3, dilation 4) with +inf and -inf centre weights, C = 24, 9 rows:
    +inf / -inf by the input's sign and NaN at its exact zeros, as the plain fp64 sum; with ``same_size_interp``
    (``persp_trans_detector.py:82`` behind it) every inf is NaN, the rest unchanged bitwise, as
    ``F.interpolate`` of the reference to its own size makes it."""
    from mvdet_amd import ops
    g = torch.Generator().manual_seed(W)
    C, H = 24, 9
    x = _signed((1, C, H, W), g)
    w = (torch.rand(1, C, 3, 3, generator=g) - 0.5) / (C * 9) ** 0.5
    w[0, 5, 1, 1] = NINF
    w[0, 11, 1, 1] = PINF
    ref = _conv_ref(x, w, None, 4)
    assert min(int(torch.isnan(ref).sum()), int(torch.isposinf(ref).sum()), int(torch.isneginf(ref).sum())) > 0
    got = ops.conv3x3_cout1(x.to(DEV), w.to(DEV), 4).cpu()
    assert_pattern(got, ref, "conv3x3_cout1, +-inf centre weights", normwise_tol=2e-5)
    ref10 = F.interpolate(ref, [H, W], mode="bilinear")
    assert not torch.isinf(ref10).any() and torch.equal(torch.isnan(ref10), ~torch.isfinite(ref))
    got10 = ops.conv3x3_cout1(x.to(DEV), w.to(DEV), 4, same_size_interp=True).cpu()
    assert torch.equal(torch.isnan(got10), torch.isnan(ref10)) and not torch.isinf(got10).any()
    fin = torch.isfinite(got)
    assert torch.equal(got10[fin], got[fin])


@pytest.mark.parametrize("which,val", [("x", PINF), ("y", NINF), ("x", NAN), ("bias", PINF), ("bias", NINF),
                                       ("bias", NAN)])
def test_coord_term_nonfinite_parameters(which, val):
    """``ops.coord_term`` with a NaN / inf centre weight of a coord channel or in the bias, on a 9 x 71 grid: odd
    sides, so the coord value is exactly 0 on the middle row and column, where 0 * inf must be NaN as in
    ``F.conv2d`` of the coord map."""
    from mvdet_amd import ops
    H, W, cout, cin, c0 = 9, 71, 64, 10, 8
    g = torch.Generator().manual_seed(5)
    w = (torch.rand(cout, cin, 3, 3, generator=g) - 0.5) / 3
    b = torch.rand(cout, generator=g) - 0.5
    if which == "bias":
        b[13] = val
    else:
        w[13, c0 + (which == "y"), 1, 1] = val
    coord = cpu_path.coord_map(H, W)
    assert (coord[0, 0, :, W // 2] == 0).all() and (coord[0, 1, H // 2] == 0).all()
    ref = _conv_ref(coord, w[:, c0:c0 + 2], b, 1)[0]
    nan = torch.isnan(ref[13])
    if which != "bias" and val == val:
        line = nan[:, W // 2] if which == "x" else nan[H // 2]
        assert line.all() and int(nan.sum()) == line.numel()
    got = ops.coord_term(w.to(DEV), b.to(DEV), c0, (H, W)).cpu()
    # 18 fp32 fmas and one add per value, each within 2^-24 of a running sum of at most ~4 max|ref|
    assert_pattern(got, ref, f"coord term, {which} = {val}", normwise_tol=19 * 4 * 2.0 ** -24)
