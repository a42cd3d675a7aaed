"""GPU tests of ``mvdet_amd.ProjectPlanes`` (``mvdet_amd/csrc/project_planes.hip``) against the CPU reference
``project_planes_ref.project_planes`` — the op's formula in stock torch-CPU ops, plane by plane.

Forward gate: ``helpers.assert_parity`` and normwise < 1e-4, the project's bound for the fused upsample warp.
Backward gates: 4 x the CPU fp32 reference's own distance from its float64 evaluation (``FLOORS``, re-measured on
the CPU by ``test_project_planes_host.py``).  Where the arithmetic is the same the comparison is bitwise: D = 1 with
unit weights against ``ProjectViews``, an added all-zero plane, 16-bit maps against their fp32 casts, two backwards,
one gradient alone against both."""
import ctypes

import pytest
import torch

import backward_cases as bc
import project_planes_ref as pr
from helpers import assert_parity
from test_gpu_backward import _adjoint_gate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last

# the CPU fp32 reference's normwise distance from float64 on each case's own inputs (softmax weights), rounded up
# <= 15 %: (forward, grad_feats, grad_weights); the gradients' gates are 4 x theirs
FLOORS = {
    pr.CASES[0]: (3.45e-6, 2.28e-6, 1.51e-6),   # gates 9.1e-6, 6.0e-6
    pr.CASES[1]: (1.70e-6, 2.12e-6, 1.47e-6),   # gates 8.5e-6, 5.9e-6
    pr.CASES[2]: (3.70e-6, 3.89e-6, 3.06e-6),   # gates 1.6e-5, 1.2e-5
    pr.CASES[3]: (1.46e-6, 1.06e-6, 7.2e-7),    # gates 4.2e-6, 2.9e-6
    pr.CASES[4]: (3.00e-6, 2.61e-6, 2.38e-6),   # gates 1.0e-5, 9.5e-6
}
cases = pytest.mark.parametrize("case", pr.CASES, ids=pr.case_id)


def _op(case, mats=None, **kw):
    import mvdet_amd
    Ms, _, _, _, up_hw = pr.inputs(case)
    return mvdet_amd.ProjectPlanes(Ms if mats is None else mats, up_hw, case[6], **kw)


def _maps(ts, dtype=torch.float32):
    return [t.to(DEV, dtype).contiguous(memory_format=CL) for t in ts]


def _wts(ts):
    return [t.to(DEV).contiguous() for t in ts]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _upstream(case, dtype=torch.float32):
    gouts = pr.inputs(case)[1]
    return torch.cat(gouts + [torch.ones_like(gouts[0][:, :2])], 1).to(DEV, dtype).contiguous(memory_format=CL)


# ---------------------------------------------------------------------------------- 1. forward

@cases
@pytest.mark.parametrize("kind", ["softmax", "raw"])
@pytest.mark.parametrize("coord", [True, False], ids=["coord", "nocoord"])
def test_forward_vs_cpu_reference(case, kind, coord):
    _, _, feats, weights, _ = pr.inputs(case)
    ref = pr.reference(case, kind)[0]
    n, C = len(feats), case[2]
    with torch.no_grad():
        got = _op(case, coord_channels=coord)(_maps(feats), _wts(weights[kind]))
    assert got.dtype == torch.float32 and got.is_contiguous(memory_format=CL)
    want = ref if coord else ref[:, :n * C]
    assert tuple(got.shape) == tuple(want.shape)
    s = assert_parity(got.cpu(), want, f"ProjectPlanes {pr.case_id(case)} {kind}")
    print(f"[forward] {pr.case_id(case)} {kind} coord={coord}: normwise {s['normwise']:.3g} < 1e-4")
    assert s["normwise"] < 1e-4, s
    if coord:
        assert torch.equal(got[:, n * C:].cpu(), ref[:, n * C:])  # mvbev_fill_coord_map_f32's values


# ---------------------------------------------------------------------------------- 2. backward

def _backward(case, dtype=torch.float32, feats_grad=True, weights_grad=True, gdtype=None, **kw):
    _, _, feats, weights, _ = pr.inputs(case)
    x = [t.requires_grad_(feats_grad) for t in _maps(feats, dtype)]
    w = [t.requires_grad_(weights_grad) for t in _wts(weights["softmax"])]
    world = _op(case, **kw)(x, w)
    world.backward(_upstream(case, gdtype or world.dtype))
    return world.detach(), [t.grad for t in x], [t.grad for t in w]


@cases
def test_backward_vs_cpu_autograd(case):
    _, ref_gf, ref_gw = pr.reference(case)
    _, gf, gw = _backward(case)
    _, floor_f, floor_w = FLOORS[case]
    for i in range(pr.N_VIEWS):
        assert gf[i].dtype == torch.float32 and gf[i].is_contiguous(memory_format=CL)
        assert gw[i].dtype == torch.float32 and gw[i].is_contiguous()
        bc.assert_gated(gf[i].cpu(), ref_gf[i], f"ProjectPlanes grad_feats {pr.case_id(case)} view {i}",
                        _adjoint_gate(floor_f))
        bc.assert_gated(gw[i].cpu(), ref_gw[i], f"ProjectPlanes grad_weights {pr.case_id(case)} view {i}",
                        _adjoint_gate(floor_w))


# ---------------------------------------------------------------------------------- 3. bitwise pins

@cases
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("coord", [True, False], ids=["coord", "nocoord"])
def test_one_plane_of_unit_weights_is_project_views_bitwise(case, dtype, coord):
    import mvdet_amd
    Ms, _, feats, _, up_hw = pr.inputs(case)
    B, src = case[1], case[4]
    mats = [planes[0] for planes in Ms]
    n, C = len(feats), case[2]
    up = _upstream(case, dtype)
    up = up if coord else up[:, :n * C].contiguous(memory_format=CL)
    x = [t.requires_grad_() for t in _maps(feats, dtype)]
    one = [torch.ones((B, 1, *src), device=DEV) for _ in range(n)]
    a = mvdet_amd.ProjectPlanes([[M] for M in mats], up_hw, case[6], coord_channels=coord)(x, one)
    a.backward(up)
    ga = [t.grad for t in x]
    y = [t.requires_grad_() for t in _maps(feats, dtype)]
    b = mvdet_amd.ProjectViews(mats, up_hw, case[6], coord_channels=coord)(y)
    b.backward(up)
    assert a.dtype == b.dtype == dtype
    assert torch.equal(_bits(a), _bits(b))
    for i in range(n):
        assert ga[i].dtype == dtype and torch.equal(_bits(ga[i]), _bits(y[i].grad)), i


@cases
def test_an_all_zero_plane_changes_nothing(case):
    Ms, _, feats, weights, _ = pr.inputs(case)
    x, w = _maps(feats), _wts(weights["raw"])
    extra = [planes + [planes[0] * 1.0] for planes in Ms]  # the added plane samples inside the source somewhere
    wz = [torch.cat([t, torch.zeros_like(t[:, :1])], 1).contiguous() for t in w]
    with torch.no_grad():
        a = _op(case)(x, w)
        b = _op(case, mats=extra)(x, wz)
    assert torch.equal(a, b)


@cases
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_half_maps_are_exact_where_they_must_be(case, dtype):
    """fp32 math throughout: 16-bit maps with an fp32 result are bitwise their fp32 casts' result, and the 16-bit
    result is bitwise that one rounded once."""
    _, _, feats, weights, _ = pr.inputs(case)
    x16, w = _maps(feats, dtype), _wts(weights["softmax"])
    with torch.no_grad():
        from16 = _op(case, out_dtype=torch.float32)(x16, w)
        from32 = _op(case)([t.float().contiguous(memory_format=CL) for t in x16], w)
        out16 = _op(case)(x16, w)
    assert from16.dtype == torch.float32 and out16.dtype == dtype and out16.is_contiguous(memory_format=CL)
    assert torch.equal(_bits(from16), _bits(from32))
    assert torch.equal(_bits(out16), _bits(from16.to(dtype)))


@cases
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_backward_is_repeatable_and_needs_input_grad_is_honoured(case, dtype):
    """Two backwards give the same bits; when only the maps or only the weights require grad the other gradient is
    None and the one returned has the bits of the run that computes both."""
    _, gf, gw = _backward(case, dtype)
    _, gf2, gw2 = _backward(case, dtype)
    assert all(g.dtype == dtype and g.is_contiguous(memory_format=CL) for g in gf)
    assert all(g.dtype == torch.float32 for g in gw)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(gf + gw, gf2 + gw2))
    _, gf_only, none_w = _backward(case, dtype, weights_grad=False)
    assert all(g is None for g in none_w)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(gf_only, gf))
    _, none_f, gw_only = _backward(case, dtype, feats_grad=False)
    assert all(g is None for g in none_f)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(gw_only, gw))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_half_map_gradients_are_the_fp32_sums_rounded_once(dtype):
    """16-bit maps under an fp32 upstream gradient (``out_dtype=float32``): grad_feats is bitwise the fp32 op's on the
    maps cast to fp32, rounded once.  grad_weights holds the same fp32 terms summed in another fixed order (a lane's
    16-B unit is 8 channels of a 16-bit map, 4 of an fp32 one): it meets that op's at the case's grad_weights gate."""
    case = pr.CASES[0]
    _, _, feats, _, _ = pr.inputs(case)
    _, gf16, gw16 = _backward(case, dtype, out_dtype=torch.float32)
    cast = [t.to(dtype).float() for t in feats]
    x = [t.requires_grad_() for t in _maps(cast)]
    w = [t.requires_grad_() for t in _wts(pr.inputs(case)[3]["softmax"])]
    _op(case)(x, w).backward(_upstream(case))
    for i in range(pr.N_VIEWS):
        assert gf16[i].dtype == dtype and torch.equal(_bits(gf16[i]), _bits(x[i].grad.to(dtype)))
        bc.assert_gated(gw16[i].cpu(), w[i].grad.cpu(), f"grad_weights from {dtype} maps, view {i}",
                        _adjoint_gate(FLOORS[case][2]))


# ---------------------------------------------------------------------------------- 4. adjoint identities

@pytest.mark.parametrize("up", [False, True], ids=["plain", "upsampled"])
@pytest.mark.parametrize("name", ["magnify", "minify"])
def test_dot_product_identities(name, up):
    """<g, out> = <grad_feats, feats> = <grad_weights, weights> (the op is bilinear), sums in float64 on the host from
    the GPU's fp32 results, within ``test_gpu_project_views.test_dot_product_identity``'s bound (n_max + 8) 2^-24
    sum |x| |S|^T |y| for the op's own linear map: |S| = sum_d |S_d| diag(|w_d|) and n_max = sum_d n_max,d, the
    entries of a source pixel over the D = 3 planes (each term's extra rounding, a_t w, is one of the 8).  The
    geometry's three matrices are one view's three planes; the third reaches outside the source."""
    import mvdet_amd
    import test_gpu_warp_adjoint_identity as ti
    mns, mats = ti._geometry(name)
    (H, W), grid = ti.GEOMETRIES[name]
    C, D = 8, 3
    xs, ys = ti._inputs("gather", name, C, seed=1)
    x0, y0 = xs[0], ys[0]
    w0 = torch.randn((x0.shape[0], D, H, W), generator=torch.Generator().manual_seed(5))
    pp = mvdet_amd.ProjectPlanes([[torch.eye(3)] * D], (3 * H, 3 * W) if up else (H, W), grid, coord_channels=False)
    pp.m_norm_cpu = torch.stack(mns)[None]  # the geometry's matrices are given normalised
    x = _maps([x0])[0].requires_grad_()
    w = w0.to(DEV).requires_grad_()
    world = pp([x], [w])
    world.backward(y0.to(DEV).contiguous(memory_format=CL))
    lhs = (world.detach().cpu().double() * y0.double()).sum().item()
    via_f = (x0.double() * x.grad.cpu().double()).sum().item()
    via_w = (w0.double() * w.grad.cpu().double()).sum().item()
    n_max, mag = 0, 0.0
    for d in range(D):
        absS, cnt = mats[up][d]
        n_max += int(cnt.max())
        spread = torch.einsum("op,bco->bcp", absS, y0.abs().double().flatten(2))  # |S_d|^T |y|
        mag += ((x0 * w0[:, d:d + 1]).abs().double().flatten(2) * spread).sum().item()
    bound = (n_max + 8) * ti.U * mag
    print(f"[identity] {name} up={up}: |lhs - <gf, f>| {abs(lhs - via_f):.3g}, |lhs - <gw, w>| "
          f"{abs(lhs - via_w):.3g} <= {bound:.3g} (n_max {n_max}, lhs {lhs:.6g})")
    assert abs(lhs - via_f) <= bound and abs(lhs - via_w) <= bound, (name, up, lhs, via_f, via_w, bound)


# ---------------------------------------------------------------------------------- 5. through a head

def test_training_step_through_a_plane_head():
    """maps -> Conv2d(C, D, 1) -> softmax over D -> ProjectPlanes(maps, .) -> square().mean(): the maps feed both
    inputs; the conv's and the maps' gradients match the CPU composition at the case's grad_feats gate."""
    case = pr.CASES[1]
    Ms, _, feats, _, up_hw = pr.inputs(case)
    n, C, D = len(feats), case[2], case[3]
    g = torch.Generator().manual_seed(11)
    head = torch.nn.Conv2d(C, D, 1)
    with torch.no_grad():
        head.weight.copy_(torch.randn(head.weight.shape, generator=g) * 0.2)
        head.bias.copy_(torch.randn(D, generator=g) * 0.1)
    leaves = [f.clone().requires_grad_() for f in feats]
    cpu_weights = [torch.softmax(head(l), 1) for l in leaves]
    pr.project_planes(leaves, cpu_weights, Ms, up_hw, case[6]).square().mean().backward()
    ref = [l.grad for l in leaves] + [head.weight.grad, head.bias.grad]

    dhead = torch.nn.Conv2d(C, D, 1)
    dhead.load_state_dict(head.state_dict())
    dhead = dhead.to(DEV)
    x = [t.requires_grad_() for t in _maps(feats)]
    world = _op(case)(x, [torch.softmax(dhead(t), 1).contiguous() for t in x])
    world.square().mean().backward()
    got = [t.grad for t in x] + [dhead.weight.grad, dhead.bias.grad]
    gate = _adjoint_gate(FLOORS[case][1])
    for name, a, b in zip(["feats[0]", "feats[1]", "conv weight", "conv bias"], got, ref):
        bc.assert_gated(a.cpu(), b, f"plane head {name}", gate)


# ---------------------------------------------------------------------------------- 6. ABI

def test_entry_points_return_their_error_codes():
    from mvdet_amd import _native
    lib = _native.load()
    NULL, RANK, SHAPE, STRIDE = -5, -1, -2, -3  # MVBEV_ERR_*
    B, C, D, h, w, H, W, Ho, Wo = 1, 8, 2, 4, 6, 12, 18, 5, 7
    f = torch.zeros((B, C, h, w), device=DEV).contiguous(memory_format=CL)
    wt = torch.zeros((B, D, h, w), device=DEV)
    mats = torch.eye(3, device=DEV).reshape(1, 1, 9).repeat(1, D, 1).contiguous()
    out = torch.zeros((B, Ho, Wo, C), device=DEV)
    cl = (h * w * C, 1, w * C, C)

    def fwd(feat=f.data_ptr(), weight=wt.data_ptr(), strides=cl, m=mats.data_ptr(), o=out.data_ptr(), nplanes=D,
            Bv=B, Hv=H, kind=0, okind=0, views=True):
        arr = (_native.ProjectPlanesView * 1)()
        arr[0] = _native.ProjectPlanesView(feat, (ctypes.c_int64 * 4)(*strides), weight)
        return lib.mvbev_project_planes_cl_forward(arr if views else None, 1, nplanes, m, kind, Bv, C, h, w, Hv, W, Ho,
                                                   Wo, o, okind, C, 0, None)

    assert fwd(views=False) == NULL and fwd(o=None) == NULL and fwd(m=None) == NULL
    assert fwd(feat=None) == NULL and fwd(weight=None) == NULL
    assert fwd(Bv=0) == RANK and fwd(nplanes=0) == RANK
    assert fwd(nplanes=9) == SHAPE and fwd(Hv=h - 1) == SHAPE and fwd(kind=3) == SHAPE and fwd(okind=1) == SHAPE
    assert fwd(strides=(h * w * C, 2, w * C, C)) == STRIDE and fwd(strides=(h * w * C, 1, w * C, C - 1)) == STRIDE

    rp = torch.zeros(D * (h * w + 1), dtype=torch.int32, device=DEV)
    col = torch.zeros(8, dtype=torch.int32, device=DEV)
    val = torch.zeros(8, device=DEV)
    go = torch.zeros((B, Ho, Wo, C), device=DEV)
    gf, gw = torch.zeros_like(f), torch.zeros_like(wt)

    def bwd(g=go.data_ptr(), rowp=rp.data_ptr(), feat=f.data_ptr(), weight=wt.data_ptr(), gfp=gf.data_ptr(),
            gwp=gw.data_ptr(), fs=cl, gs=cl, nplanes=D, Cv=C, kind=0, gkind=0, views=True):
        arr = (_native.ProjectPlanesGrad * 1)()
        arr[0] = _native.ProjectPlanesGrad(rowp, col.data_ptr(), val.data_ptr(), feat, (ctypes.c_int64 * 4)(*fs),
                                           weight, gfp, (ctypes.c_int64 * 4)(*gs), gwp)
        return lib.mvbev_project_planes_cl_backward(g, gkind, C, arr if views else None, 1, nplanes, kind, B, Cv, h, w,
                                                    Ho, Wo, None)

    assert bwd(g=None) == NULL and bwd(views=False) == NULL and bwd(rowp=None) == NULL
    assert bwd(feat=None) == NULL and bwd(weight=None) == NULL
    assert bwd(Cv=0) == RANK and bwd(nplanes=0) == RANK
    assert bwd(nplanes=9) == SHAPE and bwd(kind=3) == SHAPE and bwd(kind=0, gkind=2) == SHAPE
    assert bwd(gs=(h * w * C, 2, w * C, C)) == STRIDE and bwd(gs=(h * w * C, 1, w * C + 1, C)) == STRIDE
    assert bwd(fs=(h * w * C, 1, w * C, C - 1)) == STRIDE
    assert bwd(gfp=None, gwp=None) == 0  # nothing asked: no launch
    torch.cuda.synchronize()
