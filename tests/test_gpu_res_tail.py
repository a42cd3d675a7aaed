"""The inference residual tail on the GPU: ``mvdet_amd.res_tail.ResidualTail``, the kernels of ``res_tail.hip`` and
``PerspTransDetector(native_tail=True)``.

The layout and epilogue kernels are checked bitwise against torch constructions of their layouts; the convs and
the whole tail against the same torch modules in float64 on the CPU at the project's forward 3xbf16 gate, 5e-5
normwise, which ``test_res_tail_host.py`` proves discriminating on these very inputs (``res_tail_cases``).
"""
import copy

import pytest
import torch

import res_tail_cases as rc
from helpers import RTOL, assert_parity_t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(5, 7), (13, 22)]
NAN = float("nan")


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _views(M, C, h, w, dtype, seed):
    """Two channels-last views [1,C,h,w] (M = 2) on the GPU and the same as one CPU [M,C,h,w] fp32 tensor."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, C, h, w, generator=g) * 3).to(dtype)
    return [_cl(x[m:m + 1].to(DEV)) for m in range(M)], x


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------ 1. the conversion kernel

@pytest.mark.parametrize("poly", [False, True], ids=["plain", "polyphase"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("C", [16, 40])
def test_channels_last_to_split_bitwise(C, h, w, dtype, poly):
    from mvdet_amd import ops
    M = 2
    xs, x = _views(M, C, h, w, dtype, seed=C + h)
    shape = ops.split_polyphase_shape(M, C, h, w) if poly else ops.split_shape(M, C, h, w)
    out = torch.full(shape, NAN, dtype=torch.bfloat16, device=DEV)  # a pad left unwritten would stay NaN
    got = ops.channels_last_to_split(xs, polyphase=poly, out=out)
    assert got is out
    ref = rc.blocked_split(rc.polyphase(x.float()) if poly else x.float())
    assert tuple(got.shape) == tuple(ref.shape)
    assert torch.equal(_bits(got.cpu()), _bits(ref))
    # hi + lo restores a 16-bit input exactly and an fp32 input to 2^-16 relative
    dec = rc.split_decode(got.cpu())
    want = rc.polyphase(x.float()) if poly else x.float()
    if dtype != torch.float32:
        assert torch.equal(dec, want)
    else:
        assert ((dec - want).abs() <= want.abs() * 2.0 ** -16).all()


def test_channels_last_to_split_refuses_what_it_cannot_read():
    from mvdet_amd import ops
    x = torch.randn(1, 16, 5, 7, device=DEV)
    with pytest.raises(ValueError):
        ops.channels_last_to_split([x])                       # NCHW: no unit channel stride
    with pytest.raises(ValueError):
        ops.channels_last_to_split([_cl(torch.randn(1, 12, 5, 7, device=DEV))])  # C % 8
    with pytest.raises(RuntimeError):
        ops.channels_last_to_split([_cl(torch.randn(1, 16, 5, 7))])              # a CPU tensor


# ------------------------------------------------------------------ 2. the block close

@pytest.mark.parametrize("nxt", [None, False, True], ids=["nonext", "next-plain", "next-polyphase"])
@pytest.mark.parametrize("ypoly", [False, True], ids=["y-plain", "y-polyphase"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_residual_close_bitwise(h, w, ypoly, nxt):
    from mvdet_amd import ops
    M, C = 2, 128
    g = torch.Generator().manual_seed(h + 31 * w)
    y32 = torch.randn(M, C, h, w, generator=g)
    ident = torch.randn(M, C, h, w, generator=g)
    y32[0, 3, 1, 2] = NAN
    y32[1, 77, h - 1, w - 1] = -0.0
    ident[1, 77, h - 1, w - 1] = -0.0
    ident[0, 9, 0, 0] = NAN
    y_split = rc.blocked_split(rc.polyphase(y32) if ypoly else y32)   # what a conv would have written
    # -0.0 splits into hi = -0.0, lo = +0.0, which sum to +0.0: give that element lo = -0.0 too, so that
    # (-0.0) + (-0.0) = -0.0 reaches the ReLU
    r, c = h - 1, w - 1
    at = (4 * 1 + 2 * (r & 1) + (c & 1), 77 // 8, r >> 1, c >> 1) if ypoly else (1, 77 // 8, r, c)
    assert _bits(y_split[at][0, 77 % 8]).item() == -32768 and _bits(y_split[at][1, 77 % 8]).item() == 0
    y_split[at][1, 77 % 8] = -0.0
    y_dec = rc.split_decode(y_split)
    y_dec = rc.unpolyphase(y_dec, h, w) if ypoly else y_dec
    # the identity as two per-view tensors, as block 0 gets it
    ids = [_cl(ident[m:m + 1].to(DEV)) for m in range(M)]
    nbuf = None
    if nxt is not None:
        nshape = ops.split_polyphase_shape(M, C, h, w) if nxt else ops.split_shape(M, C, h, w)
        nbuf = torch.full(nshape, NAN, dtype=torch.bfloat16, device=DEV)
    out, nx = ops.residual_close(y_split.to(DEV), ids, (h, w), y_polyphase=ypoly, next_polyphase=nxt, next_out=nbuf)
    assert _bits(y_dec[1, 77, r, c].to(torch.bfloat16)).item() == -32768   # the planted -0.0 survives the decode
    ref = torch.relu(y_dec.to(DEV) + ident.to(DEV))           # torch's own ReLU on the same device
    assert tuple(out.shape) == (M, C, h, w) and out.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(out.contiguous().view(torch.int32), ref.contiguous().view(torch.int32))
    assert torch.isnan(out[0, 3, 1, 2]) and torch.isnan(out[0, 9, 0, 0])
    if nxt is None:
        assert nx is None
    else:  # the dual store is the conversion kernel's result on out, pads included
        assert nx is nbuf
        want = ops.channels_last_to_split([out], polyphase=nxt)
        assert torch.equal(_bits(nx), _bits(want))
    # one [M,...] identity tensor gives the same result
    out1, _ = ops.residual_close(y_split.to(DEV), _cl(ident.to(DEV)), (h, w), y_polyphase=ypoly)
    assert torch.equal(out1.contiguous().view(torch.int32), out.contiguous().view(torch.int32))


@pytest.mark.parametrize("h,w", SHAPES)
def test_polyphase_to_plain_bitwise(h, w):
    from mvdet_amd import ops
    M, C = 2, 40
    g = torch.Generator().manual_seed(w)
    y = torch.randn(M, C, h, w, generator=g)
    yp = rc.blocked_split(rc.polyphase(y)).to(DEV)
    out = torch.full(ops.split_shape(M, C, h, w), NAN, dtype=torch.bfloat16, device=DEV)
    got = ops.split_polyphase_to_plain(yp, (h, w), out=out)
    assert torch.equal(_bits(got.cpu()), _bits(rc.blocked_split(y)))


# ------------------------------------------------------------------ 3. one folded dilation-4 conv, polyphase route

@pytest.mark.parametrize("M,cin,cout,h,w", rc.D4_CASES)
def test_folded_dilation4_conv_through_polyphase(M, cin, cout, h, w):
    from mvdet_amd import ops, res_tail
    x, conv, bn = rc.d4_inputs(M, cin, cout, h, w)
    ref = rc.d4_ref64(x, conv, bn)
    blk = torch.nn.Sequential(res_tail.BasicBlock(cin, cout, 1, 4, True))
    assert res_tail.supported(blk, (M, cin, h, w))
    wf, bf = res_tail.fold_bn(conv.weight.to(DEV), bn.to(DEV))
    wf, bf = wf.float().contiguous(), bf.float().contiguous()
    packed = ops.PackedConv3x3(precision="bf16x3").get(wf)
    xp = ops.channels_last_to_split([x.to(DEV)], polyphase=True)
    h2, w2 = ops.polyphase_hw(h, w)
    d = ops.conv_desc(4 * M, cin, h2, w2, group=cin, group_stride=0, batch_stride=cin * h2 * w2)
    yp = torch.full(ops.split_polyphase_shape(M, cout, h, w), NAN, dtype=torch.bfloat16, device=DEV)
    ops.conv3x3_desc(xp, d, packed, cout, bias=bf, dilation=2, relu=False, out=yp)
    y = ops.split_decode(ops.split_polyphase_to_plain(yp, (h, w)))
    s = assert_parity_t(y, ref, f"d4 conv {M}-{cin}-{cout}-{h}-{w}", normwise_tol=rc.GATE)
    print(f"\n[d4 {M}-{cin}-{cout}-{h}-{w}] normwise {s['normwise']:.3g}")


# ------------------------------------------------------------------ 4. the whole tail

@pytest.fixture(scope="module", params=rc.TAIL_CASES, ids=lambda c: "-".join(map(str, c)))
def tail_case(request):
    """(case, blocks on the GPU, inputs on the GPU, fp64 reference): computed once per case."""
    n, B, cin, cout, h, w = request.param
    blocks, xs = rc.make_tail(cin, cout, seed=h), rc.tail_inputs(n, B, cin, h, w)
    ref = rc.ref64(blocks, xs)
    return request.param, blocks.to(DEV), [_cl(x.to(DEV)) for x in xs], ref


def _run(tail, xs):
    with torch.no_grad():
        return tail(xs)


def test_whole_tail_against_fp64_modules(tail_case):
    from mvdet_amd import res_tail
    (n, B, cin, cout, h, w), blocks, xs, ref = tail_case
    tail = res_tail.ResidualTail(blocks)
    assert tail.supported(tuple(xs[0].shape), n)
    with torch.no_grad():
        assert tail.native_applies(xs)
    outs = _run(tail, xs)
    assert len(outs) == n
    base = outs[0]._base if outs[0]._base is not None else outs[0]
    for v, o in enumerate(outs):
        assert tuple(o.shape) == (B, cout, h, w) and o.dtype == torch.float32
        assert o.is_contiguous(memory_format=torch.channels_last)
        # each view is a slice of one [n * B, ...] tensor
        assert o.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
        assert o.storage_offset() == v * B * cout * h * w
    s = assert_parity_t(torch.cat(outs), ref, f"tail {tail_case[0]}", normwise_tol=rc.GATE)
    print(f"\n[tail {tail_case[0]}] normwise {s['normwise']:.3g}")
    # NCHW-contiguous inputs are converted by torch: the same result, bitwise
    outs2 = _run(tail, [x.contiguous() for x in xs])
    assert all(torch.equal(a, b) for a, b in zip(outs, outs2))
    # and a second call reuses the folds and buffers: bitwise repeatable
    outs3 = _run(tail, xs)
    assert all(torch.equal(a, b) for a, b in zip(outs, outs3))


# ------------------------------------------------------------------ 5. weight versions

def test_weight_versions_rebuild_the_folds():
    from mvdet_amd import res_tail
    n, B, cin, cout, h, w = rc.TAIL_CASES[0]
    blocks, xs = rc.make_tail(cin, cout, seed=5).to(DEV), [_cl(x.to(DEV)) for x in rc.tail_inputs(n, B, cin, h, w)]
    tail = res_tail.ResidualTail(blocks)

    def check(what, must_differ_from=None):
        got = torch.cat(_run(tail, xs))
        assert_parity_t(got, rc.ref64(blocks, xs), what, normwise_tol=rc.GATE)
        if must_differ_from is not None:
            assert not torch.equal(got, must_differ_from), f"{what}: the result did not move"
        return got

    r0 = check("fresh")
    with torch.no_grad():
        blocks[1].conv2.weight.mul_(1.5)
    r1 = check("conv2.weight edited in place", r0)
    with torch.no_grad():
        blocks[0].bn1.running_var.mul_(3.0).add_(0.1)
    r2 = check("bn1.running_var edited in place", r1)
    donor = rc.make_tail(cin, cout, seed=6)
    blocks.load_state_dict(donor.state_dict())
    r3 = check("load_state_dict", r2)
    assert_parity_t(r3, rc.ref64(donor, xs), "load_state_dict vs the donor", normwise_tol=rc.GATE)


# ------------------------------------------------------------------ 6. fallbacks

def _record_block_calls(blocks):
    """A forward hook on ``blocks`` that keeps every call's (input, output) tensors; returns (records, handle)."""
    records = []
    handle = blocks.register_forward_hook(lambda mod, args, out: records.append((args[0], out)))
    return records, handle


def test_fallbacks_are_the_torch_modules_bitwise():
    """In train mode and under autograd the tail's output IS the torch blocks' output: the very tensors the blocks'
    own ``forward`` returned for the very inputs, one call per view, in order (which is bitwise by construction and
    does not lean on two separate torch evaluations agreeing bit for bit: on an MI355X two copies of these blocks
    differed by up to 2e-6 on the same input unless ``torch.backends.cudnn.deterministic`` was set), and gradients
    reach the parameters and the inputs."""
    from mvdet_amd import res_tail
    n, B, cin, cout, h, w = rc.TAIL_CASES[0]
    blocks, xs = rc.make_tail(cin, cout, seed=8).to(DEV), [_cl(x.to(DEV)) for x in rc.tail_inputs(n, B, cin, h, w)]
    tail = res_tail.ResidualTail(blocks)
    native = []
    inner = tail._native_forward
    tail._native_forward = lambda v: (native.append(len(v)), inner(v))[1]
    records, handle = _record_block_calls(blocks)
    try:
        # train mode: batch statistics, the torch modules
        blocks.train()
        stats0 = blocks[0].bn1.running_mean.clone()
        with torch.no_grad():
            assert not tail.native_applies(xs)
            got = tail(xs)
        assert len(got) == len(records) == n and not native
        assert all(a is x and o is b for o, x, (a, b) in zip(got, xs, records))
        assert not torch.equal(blocks[0].bn1.running_mean, stats0)      # train-mode BatchNorm did run
        assert_parity_t(torch.cat(got), rc.ref64(blocks, xs), "train-mode fallback vs fp64 train-mode modules")
        # eval mode under autograd: the torch modules, and gradients reach the parameters and the inputs
        blocks.eval()
        records.clear()
        xg = [x.clone().requires_grad_() for x in xs]
        assert not tail.native_applies(xg)
        got = tail(xg)
        assert len(got) == len(records) == n and not native
        assert all(a is x and o is b for o, x, (a, b) in zip(got, xg, records))
        assert all(o.grad_fn is not None for o in got)
        assert_parity_t(torch.cat(got).detach(), rc.ref64(blocks, xs), "autograd fallback vs fp64 modules")
        sum(o.square().sum() for o in got).backward()
        twin = copy.deepcopy(blocks).cpu().double()
        for p in twin.parameters():
            p.grad = None
        sum(twin(x.detach().cpu().double()).square().sum() for x in xs).backward()
        for (name, p), q in zip(blocks.named_parameters(), twin.parameters()):
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
            assert_parity_t(p.grad, q.grad, f"grad of {name}")
        assert all(x.grad is not None and x.grad.abs().sum() > 0 for x in xg)
        # parameters that require grad, grad mode on, plain inputs: still autograd
        records.clear()
        assert not tail.native_applies(xs)
        got = tail(xs)
        assert len(records) == n and not native and all(o is b for o, (_, b) in zip(got, records))
        for p in blocks.parameters():
            p.requires_grad_(False)
        records.clear()
        assert tail.native_applies(xs)
        tail(xs)
        assert native == [n] and not records
    finally:
        handle.remove()


# ------------------------------------------------------------------ 7. the detector

def test_detector_native_tail_against_the_torch_tail():
    """``native_tail=True`` against ``False`` in eval / no_grad on a small synthetic rig, at the project's end-to-end
    1e-3 normwise, for ``map_result`` and every ``imgs_result``; the flag leaves the ``state_dict`` alone."""
    from mvdet_amd import PerspTransDetector, synthetic
    ds = synthetic.wildtrack_like(2, 4, seed=0, img_shape=(216, 384), worldgrid_shape=(96, 288))
    torch.manual_seed(0)
    ref_model = PerspTransDetector(ds, device=DEV).eval()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():  # running statistics, gamma and beta a trained layer4 would have
        for m in ref_model.base_pt2.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_((torch.randn(m.num_features, generator=g) * 0.2).to(DEV))
                m.running_var.copy_((0.5 + torch.rand(m.num_features, generator=g)).to(DEV))
                m.weight.copy_((0.5 + torch.rand(m.num_features, generator=g)).to(DEV))
                m.bias.copy_((torch.randn(m.num_features, generator=g) * 0.2).to(DEV))
    model = PerspTransDetector(ds, device=DEV, native_tail=True).eval()
    model.load_state_dict(ref_model.state_dict())
    assert list(model.state_dict().keys()) == list(ref_model.state_dict().keys())
    imgs = torch.randn(1, ds.num_cam, 3, *ds.img_shape, generator=g)
    calls = []
    with torch.no_grad():
        want_map, want_imgs = ref_model(imgs)
        tail = model._native_tail()
        inner = tail._native_forward
        tail._native_forward = lambda xs: (calls.append(len(xs)), inner(xs))[1]
        got_map, got_imgs = model(imgs)
    assert calls == [ds.num_cam], "the native tail did not run once over all views"
    s = assert_parity_t(got_map, want_map, "map_result", normwise_tol=RTOL)
    print(f"\n[detector] map_result normwise {s['normwise']:.3g}")
    assert len(got_imgs) == len(want_imgs) == ds.num_cam
    for v, (a, b) in enumerate(zip(got_imgs, want_imgs)):
        s = assert_parity_t(a, b, f"imgs_result[{v}]", normwise_tol=RTOL)
        print(f"[detector] imgs_result[{v}] normwise {s['normwise']:.3g}")
    # training mode falls back to the torch modules: base_pt2's own forward per view, the native tail not called
    # (two torch evaluations need not agree bit for bit, so the two models are held to the end-to-end gate)
    model.train(), ref_model.train()
    model.base_pt1.eval(), ref_model.base_pt1.eval()  # (keep base_pt1's statistics alike in both)
    records, handle = _record_block_calls(model.base_pt2[0])
    try:
        with torch.no_grad():
            a, _ = model(imgs)
            b, _ = ref_model(imgs)
    finally:
        handle.remove()
    assert calls == [ds.num_cam] and len(records) == ds.num_cam
    assert_parity_t(a, b, "train-mode map_result", normwise_tol=RTOL)
