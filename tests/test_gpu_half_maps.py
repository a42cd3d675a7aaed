"""16-bit (bf16 / fp16) backbone maps on the fused upsample warp and ``PerspTransDetector(backbone_dtype=...)``.

A 16-bit value converts to fp32 exactly and the channels-last fused 3x upsample + warp + B^T does all its
arithmetic in fp32, so from 16-bit maps it must write, bit for bit, what it writes from the same maps cast to
fp32 — the transform T (both forms), the non-finite report, the exact path's slab.  Against the CPU oracle the
gate is therefore the fp32 path's own (``normwise_tol=5e-5`` on this rig): the rounding to 16 bits is in the
oracle's input too.

Default size: the small rig of ``test_gpu_nonfinite.py`` (backbone maps 18 x 32, upsampled 54 x 96, grid
24 x 72); config 1's rig at C = 32 where F(4,3) is wanted."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from helpers import assert_parity_t
from oracle import cpu_path, fixtures

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
UPCL_STAGE = 128  # MVBEV_UPCL_STAGE: a block stages its box of backbone pixels when it holds at most this many


def _small(C, N=3, seed=0):
    from mvdet_amd import synthetic
    ds = synthetic.wildtrack_like(N, 4, seed=seed, img_shape=(216, 384), worldgrid_shape=(96, 288))
    return ds, fixtures.head_params(N, seed=11, C=C)


def _geometry(ds):
    from mvdet_amd.geometry import kornia_src_norm_from_dst_norm, projection_matrices
    up, grid = tuple(ds.upsample_shape), tuple(ds.reducedgrid_shape)
    hb = tuple(u // 3 for u in up)
    ms = [kornia_src_norm_from_dst_norm(M.float().reshape(1, 3, 3), up, grid)[0] for M in projection_matrices(ds)]
    return up, grid, hb, ms


def _maps(B, C, hb, N, dtype, seed=700):
    from mvdet_amd import synthetic
    return [synthetic.backbone_features(B, C, hb, seed=seed + v, device=DEV).to(dtype) for v in range(N)]


def _mc(C, N, params):
    mc = nn.Sequential(nn.Conv2d(C * N + 2, 512, 3, padding=1), nn.ReLU(),
                       nn.Conv2d(512, 512, 3, padding=2, dilation=2), nn.ReLU(),
                       nn.Conv2d(512, 1, 3, padding=4, dilation=4, bias=False))
    mc.load_state_dict({k.replace("map_classifier.", ""): torch.from_numpy(v) for k, v in params.items()
                        if k.startswith("map_classifier.")})
    return mc.to(DEV)


def _t_numel(B, K, Ho, Wo, form):
    from mvdet_amd import ops
    return B * (K // 8) * (form + 2) * ops.wino_tile_rows(Ho, form) * Wo * 16


def _run_t(src, ms, C, grid, up, form, zeroed, boxes, tag, fill=None):
    from mvdet_amd import ops
    N, B = len(src), src[0].shape[0]
    Ho, Wo = grid
    t = torch.zeros(_t_numel(B, N * C, Ho, Wo, form), dtype=torch.bfloat16, device=DEV)
    if fill is not None:
        t.view(torch.int16).fill_(fill)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.warp_views_wino_rows_into(src, ms, t, list(range(N)), C, N * C, Ho, Wo, dst_zeroed=zeroed, up_hw=up,
                                  nonfinite=(flag, tag), boxes=boxes, form=form)
    return t.view(torch.int16).cpu(), int(flag.item())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("rig,form", [("small", 3), ("cfg1", 3), ("cfg1", 4)])
def test_fused_upsample_warp_from_16_bit_maps_is_bitwise_the_fp32_one(rig, form, dtype):
    """``ops.warp_views_wino_rows_into`` from channels-last 16-bit maps writes the T (as int16) and the non-finite
    tag it writes from ``maps.float()``: B = 2, ``dst_zeroed`` on and off, with and without the box table, a view
    with a non-finite matrix entry, an inf feature; staged, unstaged (near-field) and empty blocks all present
    (read from the box table; both rigs hold all three kinds).  F(4,3) on config 1's rig at C = 32."""
    from mvdet_amd import ops, synthetic
    if rig == "small":
        ds, C = _small(64)[0], 64
    else:
        ds, C = synthetic.CONFIGS[1]["make"](), 32
    B, N = 2, ds.num_cam
    up, grid, hb, ms = _geometry(ds)
    ms[-1] = ms[-1].clone()
    ms[-1][0, 2] = float("inf")
    low = _maps(B, C, hb, N, dtype)
    low[0][B - 1, C - 1, hb[0] // 2, hb[1] // 2] = float("inf")
    low = [f.contiguous(memory_format=torch.channels_last) for f in low]
    assert all(ops.is_channels_last_source(f) and f.dtype == dtype for f in low)
    low32 = [f.float() for f in low]
    assert all(ops.is_channels_last_source(f) for f in low32)
    boxes = ops.warp_wino_boxes(ms, up, grid, DEV, backbone_hw=hb, form=form)
    bc = boxes.cpu()[:-1].reshape(-1, 4).long()  # (the last view: non-finite geometry, no box)
    area = (bc[:, 1] - bc[:, 0] + 1) * ((bc[:, 3] & 0x3FFFFFFF) - bc[:, 2] + 1)
    inside = bc[:, 1] >= 0
    kinds = dict(empty=int((~inside).sum()), staged=int((inside & (area <= UPCL_STAGE)).sum()),
                 unstaged=int((inside & (area > UPCL_STAGE)).sum()))
    print(f"{rig} form {form}: blocks {kinds}")
    assert kinds["empty"] > 0 and kinds["staged"] > 0 and kinds["unstaged"] > 0, kinds
    assert ((boxes.cpu()[-1, :, 3] >> 30) == 1).all()
    for zeroed in (False, True):
        for bx in (None, boxes):
            ref, ref_tag = _run_t(low32, ms, C, grid, up, form, zeroed, bx, 7)
            got, got_tag = _run_t(low, ms, C, grid, up, form, zeroed, bx, 7)
            assert ref_tag == 7 and got_tag == ref_tag
            assert torch.equal(got, ref), f"dst_zeroed={zeroed}, boxes={bx is not None}: T differs from the fp32 maps'"
    assert (ref != 0).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_16_bit_copy_to_channels_last(dtype):
    """``to_channels_last_into`` on 16-bit NCHW maps is torch's channels_last copy exactly (the vector form and,
    from a strided window, the scalar one), and the fused warp from the copy is the fused warp from native
    channels-last maps, bitwise."""
    from mvdet_amd import ops
    ds, C = _small(64)[0], 64
    B, N = 2, ds.num_cam
    up, grid, hb, ms = _geometry(ds)
    low = _maps(B, C, hb, N, dtype)
    low[1][0, 5, hb[0] // 2, hb[1] // 2] = float("inf")  # (near the image centre: sampled by the warp)
    cl = [f.contiguous(memory_format=torch.channels_last) for f in low]
    bufs = [torch.empty(B, hb[0], hb[1], C, dtype=dtype, device=DEV) for _ in range(N)]
    copied = ops.to_channels_last_into(low, bufs)
    for a_, b_ in zip(copied, cl):
        assert a_.dtype == dtype and ops.is_channels_last_source(a_)
        assert torch.equal(a_.view(torch.int16), b_.view(torch.int16))
        assert a_.stride() == b_.stride()
    # a window of the maps (row pitch != width, odd width, 40 of the channels): the scalar form
    win = [f[:, 3:43, 1:, 1:] for f in low]
    wb = [torch.empty(B, hb[0] - 1, hb[1] - 1, 40, dtype=dtype, device=DEV) for _ in range(N)]
    for a_, b_ in zip(ops.to_channels_last_into(win, wb), win):
        assert torch.equal(a_.view(torch.int16), b_.contiguous(memory_format=torch.channels_last).view(torch.int16))
    with pytest.raises(ValueError):  # one dtype for source and destination
        ops.to_channels_last_into(low, [b_.float() for b_ in bufs])
    a, ta = _run_t(cl, ms, C, grid, up, 3, True, None, 4)
    b, tb = _run_t(copied, ms, C, grid, up, 3, True, None, 4)
    assert ta == tb == 4 and torch.equal(a, b)


def test_refusals_write_nothing():
    """What the fused warps do not take raises the documented error and leaves ``t`` as it was."""
    from mvdet_amd import _native, ops
    ds, C = _small(64)[0], 64
    B, N = 1, ds.num_cam
    up, grid, hb, ms = _geometry(ds)
    Ho, Wo = grid
    PAT = 0x1234

    def pattern(K, form=3):
        t = torch.zeros(_t_numel(B, K, Ho, Wo, form), dtype=torch.bfloat16, device=DEV)
        t.view(torch.int16).fill_(PAT)
        return t

    def untouched(t):
        torch.cuda.synchronize()
        return bool((t.view(torch.int16) == PAT).all())

    for dtype in DTYPES:
        low = _maps(B, C, hb, N, dtype)
        # 16-bit NCHW straight to the fused upsample warp
        t = pattern(N * C)
        with pytest.raises(TypeError, match="channels-last"):
            ops.warp_views_wino_rows_into(low, ms, t, list(range(N)), C, N * C, Ho, Wo, up_hw=up)
        assert untouched(t)
        # C = 40 channels-last: no whole 32-channel groups
        low40 = [f.contiguous(memory_format=torch.channels_last) for f in _maps(B, 40, hb, N, dtype)]
        t = pattern(N * 40)
        with pytest.raises(TypeError, match="channels-last"):
            ops.warp_views_wino_rows_into(low40, ms, t, list(range(N)), 40, N * 40, Ho, Wo, up_hw=up)
        assert untouched(t)
    # both source bits set, through the raw entry point (valid bf16 channels-last maps otherwise)
    cl = [f.contiguous(memory_format=torch.channels_last) for f in _maps(B, C, hb, N, torch.bfloat16)]
    t = pattern(N * C)
    r3 = ops.wino_tile_rows(Ho)
    K8 = N * C // 8
    arr = ops._view_table(cl, ms, [t.data_ptr() + 32 * (v * (C // 8)) * 5 * r3 * Wo for v in range(N)],
                          [(K8 * 5 * r3 * Wo, 5 * r3 * Wo, Wo, 1)] * N)
    lib = _native.load()
    for flags in (_native.WARP_SRC_F16 | _native.WARP_SRC_BF16,
                  _native.WARP_SRC_F16 | _native.WARP_SRC_BF16 | _native.WARP_DST_ZEROED):
        st = lib.mvbev_warp_views_upsampled_wino_rows_ex(arr, N, B, C, hb[0], hb[1], up[0], up[1], Ho, Wo, r3, flags,
                                                         None, 0, None, _native.stream_ptr(t.device))
        assert st == _native.ERR_SHAPE
    assert untouched(t)
    # (the same call with the one right bit runs: the table above is a valid one)
    st = lib.mvbev_warp_views_upsampled_wino_rows_ex(arr, N, B, C, hb[0], hb[1], up[0], up[1], Ho, Wo, r3,
                                                     _native.WARP_SRC_BF16, None, 0, None, _native.stream_ptr(t.device))
    assert st == 0 and not untouched(t)
    # bf16 to the plain fused warp (already-upsampled features): the wrapper and the entry point
    feats = [torch.zeros(B, C, up[0], up[1], dtype=torch.bfloat16, device=DEV) for _ in range(N)]
    t = pattern(N * C)
    with pytest.raises(TypeError, match="bf16"):
        ops.warp_views_wino_rows_into(feats, ms, t, list(range(N)), C, N * C, Ho, Wo)
    arr = ops._view_table(feats, ms, [t.data_ptr() + 32 * (v * (C // 8)) * 5 * r3 * Wo for v in range(N)],
                          [(K8 * 5 * r3 * Wo, 5 * r3 * Wo, Wo, 1)] * N)
    st = lib.mvbev_warp_views_wino_rows_ex(arr, N, B, C, up[0], up[1], Ho, Wo, r3, _native.WARP_SRC_BF16, None, 0,
                                           None, _native.stream_ptr(t.device))
    assert st == _native.ERR_SHAPE
    assert untouched(t)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_exact_path_from_16_bit_maps_is_bitwise_the_fp32_one(dtype):
    """``warp_views_exact_into`` (the non-finite guard's reference-order upsample + warp) from bf16 / fp16 maps
    equals the same call on ``.float()`` maps bit for bit: the whole grid and a row window, NCHW and
    channels-last strides, inf / NaN features included."""
    from mvdet_amd import ops
    ds, C = _small(64)[0], 64
    B, N = 2, ds.num_cam
    up, grid, hb, ms = _geometry(ds)
    Ho, Wo = grid
    low = _maps(B, C, hb, N, dtype)
    low[0][1, 3, hb[0] // 2, hb[1] // 2] = float("inf")
    low[1][0, 7, hb[0] // 2 + 3, hb[1] // 2 - 5] = float("nan")
    low[2] = low[2].contiguous(memory_format=torch.channels_last)

    def run(src, row0s, rows):
        dsts = [torch.full((B, C, rows, Wo), -7.0, device=DEV) for _ in range(N)]
        ops.warp_views_exact_into(src, ms, dsts, up_hw=up, row0s=row0s, grid_rows=None if row0s is None else Ho)
        return torch.stack(dsts).view(torch.int32).cpu()

    low32 = [f.float() for f in low]
    for row0s, rows in ((None, Ho), ([5, 0, Ho - 9], 9)):
        ref = run(low32, row0s, rows)
        got = run(low, row0s, rows)
        assert torch.equal(got, ref), f"row0s={row0s}"
    full = run(low32, None, Ho).view(torch.float32)
    assert torch.isnan(full).any() and torch.isfinite(full).any() and (full != -7.0).all()


@pytest.mark.parametrize("layout", ["channels_last", "nchw"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_engine_from_16_bit_maps_vs_oracle(dtype, layout):
    """``ProjectFuse.warp_views_upsampled`` + ``fuse`` from 16-bit maps at C = 64 stays on the fused path
    (``ws.t_from_warp``; NCHW maps through the 16-bit copy) and passes the suite's own gate for that path on this
    rig against the CPU oracle on the same 16-bit values."""
    from mvdet_amd import ProjectFuse
    from mvdet_amd.geometry import projection_matrices
    C = 64
    ds, params = _small(C)
    B, N = 1, ds.num_cam
    up, grid, hb, _ = _geometry(ds)
    pm = projection_matrices(ds)
    mc = _mc(C, N, params)
    low = _maps(B, C, hb, N, dtype)
    if layout == "channels_last":
        low = [f.contiguous(memory_format=torch.channels_last) for f in low]
    eng = ProjectFuse(pm, up, grid, C)
    with torch.no_grad():
        ws = eng.workspace(B, DEV)
        eng.warp_views_upsampled(ws, list(range(N)), low)
        assert ws.t_from_warp
        assert all(f.dtype == dtype for _, f, _ in ws.guard_src.values())  # the exact path would read them as they are
        got = eng.fuse(ws, mc).clone()
        ref = cpu_path.project_fuse([cpu_path.upsample(f.float().cpu(), up) for f in low], [M.numpy() for M in pm],
                                    grid, {k: torch.from_numpy(v) for k, v in params.items()})
    assert torch.isfinite(got).all()
    assert_parity_t(got, ref, f"engine from {dtype} {layout} maps", normwise_tol=5e-5)


def test_engine_casts_16_bit_maps_without_whole_channel_groups():
    """C % 32 != 0: 16-bit maps are cast once with ``.float()`` and take the fp32 path — the map of the fp32
    engine call on ``f.float()``, bitwise."""
    from mvdet_amd import ProjectFuse
    from mvdet_amd.geometry import projection_matrices
    C = 40
    ds, params = _small(C)
    B, N = 1, ds.num_cam
    up, grid, hb, _ = _geometry(ds)
    pm = projection_matrices(ds)
    mc = _mc(C, N, params)
    low = _maps(B, C, hb, N, torch.bfloat16)
    eng = ProjectFuse(pm, up, grid, C)
    with torch.no_grad():
        ws = eng.workspace(B, DEV)
        eng.warp_views_upsampled(ws, list(range(N)), low)
        got = eng.fuse(ws, mc).clone()
        eng.warp_views_upsampled(ws, list(range(N)), [f.float() for f in low])
        ref = eng.fuse(ws, mc).clone()
    assert torch.isfinite(got).all() and torch.equal(got, ref)


def _poison(low, hb):
    """+inf, NaN and -inf near each view's image centre, as ``test_nonfinite_features_through_the_detector``."""
    h, w = hb
    low[0][0, 3, h // 2, w // 2] = float("inf")
    low[1][0, 7, h // 2 + 3, w // 2 - 5] = float("nan")
    low[2][0, 1, h // 2 - 4, w // 2 + 6] = float("-inf")
    return low


def test_nonfinite_bf16_features_through_the_engine():
    """+inf / NaN / -inf in bf16 maps: the fused warp reports, the exact path (reading the bf16 maps) writes the
    oracle's NaN / inf pattern inside the gate; the finite frame right after is the fast path's map."""
    from mvdet_amd import ProjectFuse
    from mvdet_amd.geometry import projection_matrices
    C = 64
    ds, params = _small(C)
    B, N = 1, ds.num_cam
    up, grid, hb, _ = _geometry(ds)
    pm = projection_matrices(ds)
    mc = _mc(C, N, params)
    tp = {k: torch.from_numpy(v) for k, v in params.items()}
    good = [f.contiguous(memory_format=torch.channels_last) for f in _maps(B, C, hb, N, torch.bfloat16, seed=300)]
    bad = _poison([f.clone() for f in good], hb)
    eng, fresh = ProjectFuse(pm, up, grid, C), ProjectFuse(pm, up, grid, C)
    cams = list(range(N))
    with torch.no_grad():
        ws = eng.workspace(B, DEV)
        eng.warp_views_upsampled(ws, cams, bad)
        assert ws.t_from_warp
        got = eng.fuse(ws, mc).clone()
        assert int(ws.nf.item()) == ws.nf_tag, "the fused warp did not report the non-finite bf16 features"
        ref = cpu_path.project_fuse([cpu_path.upsample(f.float().cpu(), up) for f in bad], [M.numpy() for M in pm],
                                    grid, tp)
        nf = ~torch.isfinite(ref)
        assert 0 < int(nf.sum()) < ref.numel() and int(torch.isnan(ref).sum()) > 0  # the case discriminates
        assert_parity_t(got, ref, "bf16 maps, non-finite features (NaN / inf pattern included)")
        eng.warp_views_upsampled(ws, cams, good)
        got2 = eng.fuse(ws, mc).clone()
        assert int(ws.nf.item()) != ws.nf_tag
        wf = fresh.workspace(B, DEV)
        fresh.warp_views_upsampled(wf, cams, good)
        fast = fresh.fuse(wf, mc).clone()
        ref2 = cpu_path.project_fuse([cpu_path.upsample(f.float().cpu(), up) for f in good], [M.numpy() for M in pm],
                                     grid, tp)
    assert torch.isfinite(got2).all() and torch.equal(got2, fast)
    assert_parity_t(got2, ref2, "bf16 maps, the finite frame after a non-finite one", normwise_tol=5e-5)


def _module(ds, C, params, head_sd=None, **kw):
    """``PerspTransDetector`` with the backbone halves replaced by identities and heads for C channels (as the
    non-finite test builds it): ``imgs`` are then the backbone maps."""
    from mvdet_amd import PerspTransDetector, ProjectFuse
    model = PerspTransDetector(ds, **kw)
    N = ds.num_cam
    model.map_classifier = _mc(C, N, params)
    model.img_classifier = nn.Sequential(nn.Conv2d(C, 64, 1), nn.ReLU(), nn.Conv2d(64, 2, 1, bias=False)).to(DEV)
    if head_sd is not None:
        model.img_classifier.load_state_dict(head_sd)
    model.engine = ProjectFuse(model.proj_mats, tuple(ds.upsample_shape), tuple(ds.reducedgrid_shape), C)
    model.base_pt1, model.base_pt2 = nn.Identity(), nn.Identity()
    return model


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_module_with_backbone_dtype(dtype, monkeypatch):
    """``PerspTransDetector(ds, backbone_dtype=dtype)`` fed 16-bit maps (identity backbone) in eval / no_grad:
    ``map_result`` against the oracle on the same 16-bit values at the fused path's gate; ``imgs_result`` against
    the reference ops on the CPU from the captured output of the head's first conv (torch's own 16-bit GEMM stays
    out of the comparison), the native head running on fp32 input.  With ``backbone_dtype=None`` and fp32 maps
    the module gives bitwise what a module built without the option gives."""
    from mvdet_amd import detector
    from mvdet_amd.geometry import projection_matrices
    C = 64
    ds, params = _small(C)
    B, N = 1, ds.num_cam
    up, grid, hb, _ = _geometry(ds)
    torch.manual_seed(5)
    model = _module(ds, C, params, backbone_dtype=dtype).eval()
    assert all(p.dtype == torch.float32 for p in model.parameters())
    low = _maps(B, C, hb, N, dtype, seed=300)
    captured, head_in = [], []
    hook = model.img_classifier[0].register_forward_hook(lambda m, i, o: captured.append(o.detach()))
    native = detector.img_head.upsample_relu_conv1x1

    def spy(gs, *a, **k):
        head_in.extend(g.dtype for g in gs)
        return native(gs, *a, **k)
    monkeypatch.setattr(detector.img_head, "upsample_relu_conv1x1", spy)
    with torch.no_grad():
        map_res, imgs_res = model(torch.stack(low, 1))
        hook.remove()
        ws = model.engine.workspace(B, DEV)
        ref =cpu_path.project_fuse([cpu_path.upsample(f.float().cpu(), up) for f in low],
                                    [M.numpy() for M in projection_matrices(ds)], grid,
                                    {k: torch.from_numpy(v) for k, v in params.items()})
        assert len(captured) == N and all(g.dtype == dtype for g in captured)  # the first conv ran under autocast
        assert head_in == [torch.float32] * N, "the fused image head did not run (or not on fp32 input)"
        last = nn.Conv2d(64, 2, 1, bias=False)
        last.load_state_dict(model.img_classifier[2].state_dict())
        ref_imgs = [last(F.relu(F.interpolate(g.float().cpu(), up, mode="bilinear"))) for g in captured]
    assert ws.t_from_warp
    assert_parity_t(map_res, ref, f"module, backbone_dtype={dtype}: map_result", normwise_tol=5e-5)
    assert len(imgs_res) == N
    for v in range(N):
        assert imgs_res[v].dtype == torch.float32
        assert_parity_t(imgs_res[v], ref_imgs[v], f"module, backbone_dtype={dtype}: imgs_result {v}")
    # backbone_dtype=None: the code path of a module built without the option, bitwise
    monkeypatch.undo()
    low32 = [f.float() for f in low]
    head_sd = model.img_classifier.state_dict()
    none = _module(ds, C, params, head_sd=head_sd, backbone_dtype=None).eval()
    plain = _module(ds, C, params, head_sd=head_sd).eval()
    with torch.no_grad():
        a_map, a_imgs = none(torch.stack(low32, 1))
        a_map = a_map.clone()
        b_map, b_imgs = plain(torch.stack(low32, 1))
    assert torch.equal(a_map, b_map)
    assert all(torch.equal(x, y) for x, y in zip(a_imgs, b_imgs))


def test_module_training_from_bf16_maps():
    """``train()``: bf16 maps as leaves, one ``map_result.sum().backward()``: each map's gradient is bf16 and equals
    the fp32 path's gradient (the same module on ``maps.float()`` leaves) cast to bf16 — the maps enter the native
    forward and backward through a differentiable ``.float()``."""
    C = 64
    ds, params = _small(C)
    B, N = 1, ds.num_cam
    _, _, hb, _ = _geometry(ds)
    torch.manual_seed(5)
    model = _module(ds, C, params, backbone_dtype=torch.bfloat16).train()
    low = _maps(B, C, hb, N, torch.bfloat16, seed=300)

    def grads(maps):
        leaves = [m.clone().requires_grad_() for m in maps]
        map_res, _ = model(torch.stack(leaves, 1))
        assert map_res.dtype == torch.float32 and map_res.requires_grad
        map_res.sum().backward()
        model.zero_grad(set_to_none=True)
        return [leaf.grad for leaf in leaves]

    g16 = grads(low)
    g32 = grads([m.float() for m in low])
    for a_, b_ in zip(g16, g32):
        assert a_.dtype == torch.bfloat16 and b_.dtype == torch.float32
        assert torch.isfinite(b_).all() and (b_ != 0).any()
        assert torch.equal(a_, b_.to(torch.bfloat16))
