"""GPU tests of ``mvdet_amd.ProjectViews`` (``mvdet_amd/csrc/project_views.hip`` and the NCHW glue) against the CPU
reference ``project_views_ref.project_views`` — ``persp_trans_detector.py:65, :69, :77`` in stock torch-CPU ops.

Forward gates: ``helpers.assert_parity`` and normwise < 1e-4, the project's bound for the fused upsample warp
(``test_gpu_parity.py``).  Backward gates: 4 x the CPU fp32 reference's own coordinate-rounding floor
(``test_gpu_backward._adjoint_gate``); ``FLOORS`` pins the measured floors, which ``test_project_views_host.py``
re-measures on the CPU.  Where the arithmetic is the same the comparison is bitwise: the two store widths, 16-bit
maps against their fp32 casts, the channels-last adjoint against the fp32 NCHW gather."""
import ctypes

import pytest
import torch

import backward_cases as bc
import project_views_ref as pr
from helpers import assert_parity, load_golden, parity_stats
from test_gpu_backward import _adjoint_gate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last

# the CPU fp32 reference's distance from float64 on each case's own inputs (worst view), rounded up <= 15 %
FLOORS = {
    pr.CASES[0]: 1.72e-6,   # gate 6.9e-6
    pr.CASES[1]: 2.97e-6,   # gate 1.2e-5
    pr.CASES[2]: 3.82e-6,   # gate 1.5e-5
    pr.CASES[3]: 1.39e-6,   # gate 5.6e-6
    pr.CASES[4]: 2.94e-6,   # gate 1.2e-5
}
cases = pytest.mark.parametrize("case", pr.CASES, ids=pr.case_id)


def _op(case, **kw):
    import mvdet_amd
    Ms, _, _, up_hw = pr.inputs(case)
    return mvdet_amd.ProjectViews([M[0] for M in Ms], up_hw, case[5], **kw)


def _dev(ts, cl, dtype=torch.float32):
    return [t.to(DEV, dtype).contiguous(memory_format=CL) if cl else t.to(DEV, dtype).contiguous() for t in ts]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---------------------------------------------------------------------------------- 1. forward

@cases
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("coord", [True, False], ids=["coord", "nocoord"])
def test_forward_vs_cpu_reference(case, cl, coord):
    _, _, feats, _ = pr.inputs(case)
    ref, _ = pr.reference(case)
    n, C = len(feats), case[2]
    with torch.no_grad():
        got = _op(case, coord_channels=coord)(_dev(feats, cl))
    assert got.dtype == torch.float32 and got.is_contiguous(memory_format=CL if cl else torch.contiguous_format)
    want = ref if coord else ref[:, :n * C]
    assert tuple(got.shape) == tuple(want.shape)
    s = assert_parity(got.cpu(), want, f"ProjectViews {pr.case_id(case)}")
    print(f"[forward] {pr.case_id(case)} cl={cl} coord={coord}: normwise {s['normwise']:.3g} < 1e-4")
    assert s["normwise"] < 1e-4, s
    if coord:
        assert torch.equal(got[:, n * C:].cpu(), ref[:, n * C:])  # mvbev_fill_coord_map_f32's values


@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "channels_last"])
def test_forward_reproduces_the_reference_module_golden(cl):
    """module_wt2 (2 views, C = 512): the fixture's own ``warp_out`` and ``coord_map``."""
    import mvdet_amd
    g = load_golden("module_wt2")
    m = g["meta"]
    x = torch.from_numpy(g["feat_in"])
    pv = mvdet_amd.ProjectViews([torch.from_numpy(M) for M in g["proj_mats"]], m["upsample_shape"],
                                m["reducedgrid_shape"])
    with torch.no_grad():
        got = pv(_dev([x[:, v] for v in range(x.shape[1])], cl)).cpu()
    N, C = x.shape[1], x.shape[2]
    want = torch.from_numpy(g["warp_out"]).flatten(1, 2)
    s = assert_parity(got[:, :N * C], want, "module_wt2 warp_out")
    assert s["normwise"] < 1e-4, s
    assert torch.equal(got[:, N * C:], torch.from_numpy(g["coord_map"]).repeat(x.shape[0], 1, 1, 1))


# ---------------------------------------------------------------------------------- 2. store widths

def _c_forward(feats_cl, pv, ctot, coord, out):
    from mvdet_amd import _native, ops
    B, C, h, w = feats_cl[0].shape
    arr = ops._view_table(feats_cl, pv.m_norm_cpu)
    for v in arr:
        v.src_strides = (ctypes.c_int64 * 4)(h * w * C, 1, w * C, C)
    kinds = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    st = _native.load().mvbev_project_views_cl_forward(
        arr, len(feats_cl), kinds[feats_cl[0].dtype], B, C, h, w, pv.up_hw[0], pv.up_hw[1], pv.grid_hw[0],
        pv.grid_hw[1], out.data_ptr(), kinds[out.dtype], ctot, int(coord), _native.stream_ptr(out.device))
    _native.check(st, "mvbev_project_views_cl_forward")


@cases
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_both_store_widths_and_untouched_channels(case, dtype):
    """With the coord channels a pixel is 8-B (fp32) / 4-B (16-bit) aligned: narrow stores; without them and with
    C a multiple of the 16-B unit: 16-B stores.  The same values either way, and through the C entry point nothing
    outside the op's channels of a wider pixel is written."""
    _, _, feats, _ = pr.inputs(case)
    n, C = len(feats), case[2]
    x = _dev(feats, True, dtype)
    with torch.no_grad():
        a = _op(case, coord_channels=True)(x)
        b = _op(case, coord_channels=False)(x)
    assert a.dtype == b.dtype == dtype
    assert torch.equal(_bits(a[:, :n * C]), _bits(b))
    pv = _op(case)
    B, (Ho, Wo) = case[1], case[5]
    for coord, extra in ((True, 3), (False, 5), (False, 8)):
        own = n * C + (2 if coord else 0)
        buf = torch.full((B, Ho, Wo, own + extra), -7.0, dtype=dtype, device=DEV)  # [B][Ho][Wo][Ctot]
        _c_forward(x, pv, own + extra, coord, buf)
        torch.cuda.synchronize()
        assert (buf[..., own:] == -7.0).all(), "channels past the op's were written"
        assert torch.equal(_bits(buf[..., :own]), _bits((a if coord else b).permute(0, 2, 3, 1)))


# ---------------------------------------------------------------------------------- 3. 16-bit maps

@cases
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_half_maps_are_exact_where_they_must_be(case, dtype):
    """fp32 math throughout: 16-bit maps with an fp32 result are bitwise their fp32 casts' result, and the 16-bit
    result is bitwise that one rounded once."""
    _, _, feats, _ = pr.inputs(case)
    x16 = _dev(feats, True, dtype)
    with torch.no_grad():
        from16 = _op(case, out_dtype=torch.float32)(x16)
        from32 = _op(case)([t.float().contiguous(memory_format=CL) for t in x16])
        out16 = _op(case)(x16)
    assert from16.dtype == torch.float32 and out16.dtype == dtype and out16.is_contiguous(memory_format=CL)
    assert torch.equal(_bits(from16), _bits(from32))
    assert torch.equal(_bits(out16), _bits(from16.to(dtype)))


# ---------------------------------------------------------------------------------- 4. backward

@cases
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "channels_last"])
def test_backward_vs_cpu_autograd(case, cl):
    _, gouts, feats, _ = pr.inputs(case)
    _, ref_grads = pr.reference(case)
    n, C = len(feats), case[2]
    x = _dev(feats, cl)
    for i in (0, 2):
        x[i].requires_grad_()
    world = _op(case)(x)
    assert world.grad_fn is not None
    up = torch.cat(gouts + [torch.ones_like(gouts[0][:, :2])], 1).to(DEV)
    world.backward(up.contiguous(memory_format=CL) if cl else up)
    assert x[1].grad is None  # a view that does not require grad gets none (and is not gathered)
    gate = _adjoint_gate(FLOORS[case])
    for i in (0, 2):
        g = x[i].grad
        assert g.dtype == torch.float32 and g.is_contiguous(memory_format=CL if cl else torch.contiguous_format)
        bc.assert_gated(g.cpu(), ref_grads[i], f"ProjectViews backward {pr.case_id(case)} view {i}", gate)


# ---------------------------------------------------------------------------------- 5. adjoint, bitwise

@cases
def test_adjoint_is_bitwise_the_nchw_gather_and_repeatable(case):
    from mvdet_amd import ops
    _, gouts, feats, _ = pr.inputs(case)
    n, C, src = len(feats), case[2], case[3]
    B = case[1]
    pv = _op(case)
    up = torch.cat(gouts + [torch.ones_like(gouts[0][:, :2])], 1).to(DEV)

    def run(dtype, gdtype):
        x = [t.requires_grad_() for t in _dev(feats, True, dtype)]
        world = _op(case, out_dtype=gdtype if gdtype != dtype else None)(x)
        world.backward(up.to(gdtype).contiguous(memory_format=CL))
        return [t.grad for t in x]

    g32 = run(torch.float32, torch.float32)
    plans = pv.plans(DEV, src)
    nchw = [torch.full((B, C, *src), float("nan"), device=DEV) for _ in range(n)]
    ops.warp_views_adjoint([up[:, i * C:(i + 1) * C] for i in range(n)], plans, nchw)
    for i in range(n):
        assert torch.equal(_bits(g32[i]), _bits(nchw[i])), f"view {i}: not the fp32 NCHW gather's sums"
    again = run(torch.float32, torch.float32)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, g32))
    for dtype in (torch.bfloat16, torch.float16):
        g16 = run(dtype, dtype)
        x = [t.requires_grad_() for t in _dev(feats, True)]  # the fp32 run fed that grad_out cast to fp32
        _op(case)(x).backward(up.to(dtype).float().contiguous(memory_format=CL))
        for i in range(n):
            assert g16[i].dtype == dtype and g16[i].is_contiguous(memory_format=CL)
            assert torch.equal(_bits(g16[i]), _bits(x[i].grad.to(dtype))), (dtype, i)


# ---------------------------------------------------------------------------------- 6. dot-product identity

@pytest.mark.parametrize("up", [False, True], ids=["plain", "upsampled"])
@pytest.mark.parametrize("name", ["magnify", "minify"])
def test_dot_product_identity(name, up):
    """<pv(x), y> = <x, pv^T(y)> in float64 from the GPU's fp32 outputs, within (n_max + 8) 2^-24 sum |x| |S|^T |y|
    (``test_gpu_warp_adjoint_identity.py``), |S| and n_max from the CPU restatement of the plan; the third view's
    samples fall outside the source and into the one-corner-pair bands."""
    import mvdet_amd
    import test_gpu_warp_adjoint_identity as ti
    mns, mats = ti._geometry(name)
    (H, W), grid = ti.GEOMETRIES[name]
    C = 8
    xs, ys = ti._inputs("gather", name, C, seed=1)
    pv = mvdet_amd.ProjectViews([torch.eye(3)] * 3, (3 * H, 3 * W) if up else (H, W), grid, coord_channels=False)
    pv.m_norm_cpu = torch.stack(mns)  # the geometry's matrices are given normalised
    x = [t.requires_grad_() for t in _dev(xs, True)]
    world = pv(x)
    world.backward(torch.cat(ys, 1).to(DEV).contiguous(memory_format=CL))
    for v in range(3):
        absS, cnt = mats[up][v]
        lhs = (world[:, v * C:(v + 1) * C].detach().cpu().double() * ys[v].double()).sum().item()
        rhs = (xs[v].double() * x[v].grad.cpu().double()).sum().item()
        spread = torch.einsum("op,bco->bcp", absS, ys[v].abs().double().flatten(2))
        bound = (int(cnt.max()) + 8) * ti.U * (xs[v].abs().double().flatten(2) * spread).sum().item()
        print(f"[identity] {name} up={up} view {v}: |lhs - rhs| {abs(lhs - rhs):.3g} <= {bound:.3g}")
        assert abs(lhs - rhs) <= bound, (name, up, v, lhs, rhs, bound)


# ---------------------------------------------------------------------------------- 7. a torch head

def _bf16(t, mode):
    """``t`` (fp32) as a bf16 value, rounded to nearest even or truncated; None: unchanged."""
    if mode is None:
        return t
    if mode == "nearest":
        return t.bfloat16().float()
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


class _Bf16(torch.autograd.Function):
    """A bf16 tensor between two ops: its value stored with one rounding mode, its gradient with another."""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return _bf16(x, fwd)

    @staticmethod
    def backward(ctx, g):
        return _bf16(g, ctx.bwd), None, None


def _conv_bf16_arithmetic(head, world):
    """How this GPU's torch conv under bf16 autocast rounds, found on the CPU reference's own ``world`` (no
    ``ProjectViews`` in it) by comparing bits: "nearest" — y = rne(conv + bias), what torch's own kernels give — or
    "truncating" — y = rne(trunc(conv) + bias): MIOpen's bf16 conv truncates its fp32 accumulators, in the forward
    and in the input gradient alike, and torch adds the bias to that bf16 result as an op of its own.  fp32
    summation order moves a few values across a rounding boundary: 1 % of mismatches are allowed, the wrong model
    has 30-50 %."""
    import torch.nn.functional as F
    wq, wt, b = world.bfloat16(), head.weight.detach().bfloat16(), head.bias.detach().bfloat16()
    conv = F.conv2d(wq.float(), wt.float(), None, padding=1)
    bias = b.float().view(1, -1, 1, 1)
    cands = {"nearest": _bf16(conv + bias, "nearest"), "truncating": _bf16(_bf16(conv, "truncate") + bias, "nearest")}
    dhead = torch.nn.Conv2d(head.in_channels, head.out_channels, 3, padding=1)
    dhead.load_state_dict(head.state_dict())
    dhead = dhead.to(DEV, memory_format=CL)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = dhead(wq.to(DEV).contiguous(memory_format=CL)).float().cpu()
    miss = {k: (y != c).float().mean().item() for k, c in cands.items()}
    model = min(miss, key=miss.get)
    print(f"[head] the GPU conv's bf16 arithmetic: {model} (values that differ: " +
          ", ".join(f"{k} {v:.2%}" for k, v in miss.items()) + ")")
    assert miss[model] <= 0.01, f"the conv under bf16 autocast rounds in neither way this test knows: {miss}"
    return model


def test_training_step_through_a_torch_head_under_bf16_autocast():
    """bf16 channels-last maps -> ProjectViews -> nn.Conv2d in channels-last under bf16 autocast: the formats meet
    (no copy, no cast between the maps and the head) and the step matches the same head on the CPU reference at the
    1e-3 gate, loosened only by what the bf16 arithmetic of that torch conv costs — measured here as the CPU
    reference with and without the bf16 roundings of the autocast step: the world and the conv's weight and bias
    rounded to nearest, the conv's result and input gradient stored as that conv stores them
    (``_conv_bf16_arithmetic``), the loss's gradient and the views' gradients rounded to nearest.

    On an MI355X the conv is MIOpen's, which truncates: with every rounding taken as to-nearest the cost came out at
    2.6e-4 (loss) and 3.6e-3 (gradients) and the step missed it with 6.0e-3 and 7.8e-3 ... 1.03e-2, the loss low by
    0.6 %; the same conv fed the CPU reference's world, without ``ProjectViews``, showed the same distance, and its
    bits are rne(trunc(conv) + bias) exactly (0 of 6256 values differ; input gradient: 6 of 95404 from trunc)."""
    import torch.nn.functional as F
    case = pr.CASES[0]
    Ms, _, feats, up_hw = pr.inputs(case)
    n, C = len(feats), case[2]
    ctot = n * C + 2
    feats = [f.bfloat16().float() for f in feats]  # the backbone's bf16 maps
    g = torch.Generator().manual_seed(7)
    head = torch.nn.Conv2d(ctot, 8, 3, padding=1)
    with torch.no_grad():
        head.weight.copy_(torch.randn(head.weight.shape, generator=g) * 0.05)
        head.bias.copy_(torch.randn(8, generator=g) * 0.1)

    def cpu_step(model):
        """``model``: None (fp32), "nearest" or "truncating" (the conv's stores)."""
        rq = (lambda t, fwd="nearest", bwd="nearest": t) if model is None else _Bf16.apply
        store = "truncate" if model == "truncating" else "nearest"
        leaves = [f.clone().requires_grad_() for f in feats]
        world = pr.project_views([rq(l, None, "nearest") for l in leaves], [M[0] for M in Ms], up_hw, case[5])
        world = rq(world, "nearest", store)  # ProjectViews' store; the conv's input-gradient store
        wt, b = rq(head.weight.detach(), "nearest", None), rq(head.bias.detach(), "nearest", None)
        if model == "truncating":  # the bias added to the conv's bf16 result by an op of its own
            y = rq(rq(F.conv2d(world, wt, None, padding=1), store, None) + b.view(1, -1, 1, 1), "nearest", "nearest")
        else:
            y = rq(F.conv2d(world, wt, b, padding=1), "nearest", "nearest")
        loss = y.square().mean()
        loss.backward()
        return loss.item(), [l.grad for l in leaves], world.detach()

    loss_ref, grads_ref, world_ref = cpu_step(None)
    loss_q, grads_q, _ = cpu_step(_conv_bf16_arithmetic(head, world_ref))
    cost_loss = abs(loss_q - loss_ref) / abs(loss_ref)
    cost_grad = max(parity_stats(a, b)["normwise"] for a, b in zip(grads_q, grads_ref))

    x = [f.to(DEV, torch.bfloat16).contiguous(memory_format=CL).requires_grad_() for f in feats]
    dhead = torch.nn.Conv2d(ctot, 8, 3, padding=1)
    dhead.load_state_dict(head.state_dict())
    dhead = dhead.to(DEV, memory_format=CL)
    pv = _op(case)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        world = pv(x)
        assert world.dtype == torch.bfloat16 and world.is_contiguous(memory_format=CL)
        y = dhead(world)
    loss = y.float().square().mean()
    loss.backward()
    err_loss = abs(loss.item() - loss_ref) / abs(loss_ref)
    errs = []
    for i in range(n):
        gi = x[i].grad
        assert gi.dtype == torch.bfloat16 and gi.is_contiguous(memory_format=CL)
        errs.append(parity_stats(gi.float().cpu(), grads_ref[i])["normwise"])
    print(f"[head] loss {loss.item():.6g} vs {loss_ref:.6g}: {err_loss:.3g} <= 1e-3 + {cost_loss:.3g}")
    print("[head] view gradients: normwise " + ", ".join(f"{e:.3g}" for e in errs) + f" <= 1e-3 + {cost_grad:.3g}")
    assert err_loss <= 1e-3 + cost_loss, f"loss {loss.item()} vs {loss_ref}: bf16 autocast itself costs {cost_loss:.3g}"
    for i, e in enumerate(errs):
        assert e <= 1e-3 + cost_grad, f"view {i}: {e:.3g}; bf16 autocast of the conv itself costs {cost_grad:.3g}"
