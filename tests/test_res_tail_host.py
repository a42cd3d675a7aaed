"""Host side of the inference residual tail (``mvdet_amd.res_tail``): no GPU.

The fold, the polyphase identity, ``supported``, the placement of the GPU tests' gate on their own inputs, the
kernels' resource report and the detector's unchanged default.
"""
import re
from pathlib import Path

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import res_tail_cases as rc
from helpers import parity_stats
from mvdet_amd import res_tail, synthetic
from mvdet_amd.backbone import BasicBlock, build_backbone
from mvdet_amd.detector import PerspTransDetector

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------ 1. the fold

def test_fold_equals_bn_of_conv_in_fp64():
    """conv(x, w') + b' == bn(conv(x, w)) in fp64 to 1e-12, for conv1, conv2 and the downsample of a block with
    non-trivial running statistics, gamma, beta and eps."""
    blocks = rc.make_tail(32, 128, seed=3).double()
    blk = blocks[0]
    g = torch.Generator().manual_seed(7)
    for conv, bn, cin in ((blk.conv1, blk.bn1, 32), (blk.conv2, blk.bn2, 128),
                          (blk.downsample[0], blk.downsample[1], 32)):
        assert bn.eps != 1e-5 and not torch.allclose(bn.running_var, torch.ones_like(bn.running_var))
        x = torch.randn(2, cin, 9, 11, generator=g, dtype=torch.float64)
        w, b = res_tail.fold_bn(conv.weight, bn)
        assert w.dtype == torch.float64 and b.dtype == torch.float64
        with torch.no_grad():
            ref = bn(conv(x))
        got = F.conv2d(x, w, b, padding=conv.padding, dilation=conv.dilation)
        assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


def test_fold_reads_fp32_parameters_in_fp64():
    """The fold of fp32 modules is computed in fp64 (not an fp32 rsqrt): it equals the independent fp64 fold."""
    blk = rc.make_tail(32, 128, seed=4)[0]
    w, b = res_tail.fold_bn(blk.conv1.weight, blk.bn1)
    w_ref, b_ref = rc.fold64(blk.conv1, blk.bn1)
    assert torch.equal(w, w_ref) and torch.equal(b, b_ref)


# ------------------------------------------------------------------ 2. the polyphase identity

@pytest.mark.parametrize("h,w", [(13, 21), (10, 24), (5, 7)])
def test_polyphase_dilation4_is_dilation2_exactly(h, w):
    """F.conv2d(dilation=4, padding=4) == the dilation-2 conv of the four zero-padded 2 x 2 sub-grids put back on
    the grid, with a maximum difference of 0.0 (small integers: every sum is exact, whatever its order)."""
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randint(-4, 5, (2, 3, h, w), generator=g).double()
    wt = torch.randint(-3, 4, (5, 3, 3, 3), generator=g).double()
    ref = F.conv2d(x, wt, padding=4, dilation=4)
    for split, join in ((res_tail.polyphase_split, res_tail.polyphase_join),
                        (rc.polyphase, lambda y, hw: rc.unpolyphase(y, *hw))):
        xp = split(x)
        h2, w2 = (h + 1) // 2, (w + 1) // 2
        assert tuple(xp.shape) == (8, 3, h2, w2)
        if h % 2:  # the added row of the odd-row sub-grids is an exact zero
            assert not xp.view(2, 2, 2, 3, h2, w2)[:, 1, :, :, h2 - 1].any()
        if w % 2:
            assert not xp.view(2, 2, 2, 3, h2, w2)[:, :, 1, :, :, w2 - 1].any()
        got = join(F.conv2d(xp, wt, padding=2, dilation=2), (h, w))
        assert tuple(got.shape) == tuple(ref.shape)
        assert (got - ref).abs().max().item() == 0.0
    assert torch.equal(res_tail.polyphase_split(x), rc.polyphase(x))


# ------------------------------------------------------------------ 3. supported()

def test_supported_and_its_reasons():
    pt1, pt2, _ = build_backbone("resnet18")
    layer4 = pt2[0]
    assert res_tail.supported(layer4) and res_tail.why_not(layer4) is None
    assert res_tail.supported(layer4, (1, 256, 90, 160), n_views=7)
    tail = res_tail.ResidualTail(layer4)
    assert tail.supported((2, 256, 13, 22), 3) and not list(tail.__dict__.get("_parameters", []))
    assert "256" in res_tail.why_not(layer4, (1, 128, 9, 16))          # the wrong channel count
    assert not res_tail.supported(layer4, (1, 256, 9, 16), n_views=17)
    # a strided block: ResNet-18's layer2 (base_pt1[5]) keeps its stride 2
    why = res_tail.why_not(pt1[5])
    assert why is not None and "stride" in why and not res_tail.supported(pt1[5])
    strided = nn.Sequential(BasicBlock(128, 128, 2, 1, True))
    assert "stride" in res_tail.why_not(strided)
    # a VGG sequence
    vgg = build_backbone("vgg11")[1]
    why = res_tail.why_not(vgg)
    assert why is not None and "BasicBlock" in why
    # Cout = 64 (layer1)
    why = res_tail.why_not(pt1[4])
    assert why is not None and "Cout=64" in why
    # and what else the docstring names
    assert "Cin=24" in res_tail.why_not(nn.Sequential(BasicBlock(24, 128, 1, 1, True)))
    assert "dilation" in res_tail.why_not(nn.Sequential(BasicBlock(128, 128, 1, 3, False)))
    odd = BasicBlock(128, 128, 1, 1, False)
    odd.conv2 = nn.Conv2d(128, 128, 3, padding=2, dilation=2, bias=False)
    assert "conv2" in res_tail.why_not(nn.Sequential(odd))


def test_tail_is_no_module_and_falls_back_on_the_cpu():
    """The tail holds no parameters (it is not an nn.Module), and where the native path does not apply (here: CPU
    tensors) it returns the torch blocks' output, bitwise."""
    blocks = rc.make_tail(32, 128, seed=1)
    tail = res_tail.ResidualTail(blocks)
    assert not isinstance(tail, nn.Module)
    xs = rc.tail_inputs(2, 1, 32, 5, 7)
    assert not tail.native_applies(xs)
    with torch.no_grad():
        got, ref = tail(xs), [blocks(x) for x in xs]
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    with pytest.raises(ValueError):
        res_tail.ResidualTail(blocks, precision="fp32")


# ------------------------------------------------------------------ 4. gate placement

def _window(key, e_int, e_lapse):
    worst = min(e_lapse, key=e_lapse.get)
    print(f"\n[window] {key}: e_int {e_int:.3g}  3*e_int {3 * e_int:.3g} <= GATE {rc.GATE:.3g} <= "
          f"min(e_lapse)/3 {e_lapse[worst] / 3:.3g}  (min e_lapse {e_lapse[worst]:.3g}: {worst}; " +
          ", ".join(f"{l} {e:.3g}" for l, e in e_lapse.items()) + ")")
    assert 3 * e_int <= rc.GATE, (key, e_int)
    assert all(e >= 3 * rc.GATE for e in e_lapse.values()), (key, e_lapse)


@pytest.mark.parametrize("n,B,cin,cout,h,w", rc.TAIL_CASES)
def test_tail_gate_window(n, B, cin, cout, h, w):
    """On the GPU test's own inputs: the intended arithmetic <= gate / 3, every single lost ``lo`` pass (the
    activations' or the weights', in any one of the four convs) >= 3 * gate."""
    blocks, xs = rc.make_tail(cin, cout, seed=h), rc.tail_inputs(n, B, cin, h, w)
    ref = rc.ref64(blocks, xs)
    e_int = parity_stats(rc.emulate_tail(blocks, xs), ref)["normwise"]
    e_lapse = {f"{op}{k}": parity_stats(rc.emulate_tail(blocks, xs, (op, k)), ref)["normwise"]
               for op, k in rc.TAIL_LAPSES}
    _window(f"tail/{n}-{B}-{cin}-{cout}-{h}-{w}", e_int, e_lapse)


@pytest.mark.parametrize("M,cin,cout,h,w", rc.D4_CASES)
def test_d4_gate_window(M, cin, cout, h, w):
    x, conv, bn = rc.d4_inputs(M, cin, cout, h, w)
    ref = rc.d4_ref64(x, conv, bn)
    e_int = parity_stats(rc.emulate_d4(x, conv, bn), ref)["normwise"]
    e_lapse = {op: parity_stats(rc.emulate_d4(x, conv, bn, op), ref)["normwise"] for op in ("x", "w")}
    _window(f"d4/{M}-{cin}-{cout}-{h}-{w}", e_int, e_lapse)


# ------------------------------------------------------------------ 5. no scratch

def test_res_tail_kernels_use_no_scratch():
    """Every kernel of res_tail.hip is element-wise and keeps its 8 values in registers: 0 bytes of scratch per
    lane in the build's resource report (``build/obj/res_tail.o.res``, written by the Makefile)."""
    res = ROOT / "build" / "obj" / "res_tail.o.res"
    if not res.exists():
        pytest.skip("no build tree (build/obj/res_tail.o.res)")
    names, scratch = [], []
    for line in res.read_text().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            names.append(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            scratch.append(int(m.group(1)))
    assert len(names) == len(scratch) >= 13, (names, scratch)  # 6 conversions, 6 closes, the permutation copy
    for kind in ("cl_to_split_kernel", "res_close_kernel", "poly_to_plain_kernel"):
        assert any(kind in n for n in names), kind
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))


# ------------------------------------------------------------------ 6. the detector's default

def test_detector_default_is_unchanged_and_bad_combinations_raise():
    ds = synthetic.wildtrack_like(2, 4, seed=0, img_shape=(72, 128), worldgrid_shape=(32, 96))
    torch.manual_seed(0)
    plain = PerspTransDetector(ds, device="cpu")
    torch.manual_seed(0)
    flagged = PerspTransDetector(ds, device="cpu", native_tail=True)
    assert plain.native_tail is False and flagged.native_tail is True
    assert list(plain.state_dict().keys()) == list(flagged.state_dict().keys())
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), flagged.state_dict().values()))
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in flagged.named_modules()]
    assert not any("tail" in k for k in flagged.state_dict())
    # the tail object, once made, still adds nothing
    tail = res_tail.ResidualTail(flagged.base_pt2[0])
    flagged._tail = tail
    assert list(plain.state_dict().keys()) == list(flagged.state_dict().keys())
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in flagged.named_modules()]
    assert tail.supported()
    with pytest.raises(ValueError, match="vgg11"):
        PerspTransDetector(ds, arch="vgg11", device="cpu", native_tail=True)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(ValueError, match="backbone_dtype"):
            PerspTransDetector(ds, device="cpu", native_tail=True, backbone_dtype=dt)
    PerspTransDetector(ds, arch="vgg11", device="cpu")  # the default still takes vgg11
