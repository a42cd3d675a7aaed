"""Inputs, references and the CPU emulation shared by ``test_res_tail_host.py`` and ``test_gpu_res_tail.py``.

Nothing here touches the GPU or the library under test.  ``make_tail`` builds layer4's real structure at a small
width (block 0: ``cin -> cout``, dilation 2, 1x1 downsample; block 1: ``cout -> cout``, dilation 4; conv2 of both
dilation 1) with BatchNorm statistics, gamma and beta randomised; ``ref64`` evaluates the same modules in float64;
``emulate_tail`` / ``emulate_conv`` restate the native path's arithmetic (fp64 fold rounded once to fp32, operands
split hi + lo as ``bf16x3_ref.split``, the three bf16 passes in fp32, split-bf16 conv outputs) with one optional
lapse: the ``lo`` part of the activations (``("x", k)``) or of the weights (``("w", k)``) of conv ``k`` zeroed, which
is one lost ``lo`` pass of that conv.
"""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16x3_ref as br
from mvdet_amd.backbone import BasicBlock

GATE = br.DIRECT  # 5e-5 normwise: the project's forward 3xbf16 gate

# (views, B, cin, cout, h, w): the whole-tail cases of the GPU test
TAIL_CASES = [(3, 1, 32, 128, 13, 22),   # odd h: 7 x 11 sub-grids with a zero row
              (2, 2, 64, 128, 24, 40)]   # two ring row tiles, w no multiple of 32
# (M, cin, cout, h, w): one folded dilation-4 conv through the polyphase route
D4_CASES = [(2, 32, 128, 13, 22),        # odd h, sub-grids 7 x 11
            (1, 16, 128, 9, 33)]         # both odd, w spanning two 32-column tiles


def _randomise_bn(bn: nn.BatchNorm2d, g: torch.Generator, var_scale: float) -> None:
    c = bn.num_features
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.3 * var_scale ** 0.5)
        bn.running_var.copy_((0.5 + 1.5 * torch.rand(c, generator=g)) * var_scale)
        bn.weight.copy_(0.5 + torch.rand(c, generator=g))
        bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
    bn.eps = 1e-3 if c % 256 else 1e-5  # a non-default eps where the width allows both


def make_tail(cin: int, cout: int, seed: int = 0, dilations=(2, 4)) -> nn.Sequential:
    """Layer4-shaped blocks in eval mode, fp32, on the CPU; every conv and BatchNorm tensor randomised."""
    g = torch.Generator().manual_seed(seed)
    blocks, c = [], cin
    for i, d in enumerate(dilations):
        blk = BasicBlock(c, cout, 1, d, downsample=(c != cout))
        convs = [blk.conv1, blk.conv2] + ([blk.downsample[0]] if blk.downsample is not None else [])
        for conv in convs:
            fan = conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1]
            with torch.no_grad():
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (1.0 / fan) ** 0.5)
        bns = [blk.bn1, blk.bn2] + ([blk.downsample[1]] if blk.downsample is not None else [])
        for bn in bns:
            _randomise_bn(bn, g, 1.0)
        blocks.append(blk)
        c = cout
    return nn.Sequential(*blocks).eval()


def tail_inputs(n: int, B: int, cin: int, h: int, w: int, seed: int = 0):
    """n maps [B,cin,h,w] like ``base_pt1``'s output: post-ReLU, fp32, channels-last."""
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.relu(torch.randn(B, cin, h, w, generator=g) + 0.3).contiguous(memory_format=torch.channels_last)
            for _ in range(n)]


def ref64(blocks: nn.Sequential, xs):
    """The same modules in float64 on the CPU (eval mode as given), one [n * B, cout, h, w] tensor."""
    b64 = copy.deepcopy(blocks).cpu().double()
    with torch.no_grad():
        return torch.cat([b64(x.detach().cpu().double()) for x in xs])


def d4_inputs(M: int, cin: int, cout: int, h: int, w: int, seed: int = 0):
    """(x [M,cin,h,w] channels-last, conv, bn): one dilation-4 conv with its BatchNorm, randomised."""
    g = torch.Generator().manual_seed(2000 + seed)
    x = torch.relu(torch.randn(M, cin, h, w, generator=g) + 0.3).contiguous(memory_format=torch.channels_last)
    conv = nn.Conv2d(cin, cout, 3, padding=4, dilation=4, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (1.0 / (9 * cin)) ** 0.5)
    bn = nn.BatchNorm2d(cout).eval()
    _randomise_bn(bn, g, 1.0)
    return x, conv, bn


def d4_ref64(x, conv, bn):
    with torch.no_grad():
        return copy.deepcopy(bn).double()(copy.deepcopy(conv).double()(x.double()))


# ------------------------------------------------------------------ the fold (independent of mvdet_amd.res_tail)

def fold64(conv: nn.Conv2d, bn: nn.BatchNorm2d):
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return (conv.weight.detach().double() * s.view(-1, 1, 1, 1),
            bn.bias.detach().double() - bn.running_mean.detach().double() * s)


# ------------------------------------------------------------------ layouts as torch statements

def blocked_split(x: torch.Tensor) -> torch.Tensor:
    """fp32 (or 16-bit) [M,C,h,w] -> the split-bf16 blocked layout [M, C/8, h, w, 2, 8] (bf16): hi = bf16(x),
    lo = bf16(x - hi), both rounded to nearest even."""
    M, C, h, w = x.shape
    x = x.float()
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    t = torch.stack([hi, lo], dim=1)                                  # [M, 2, C, h, w]
    return t.view(M, 2, C // 8, 8, h, w).permute(0, 2, 4, 5, 1, 3).contiguous()


def polyphase(x: torch.Tensor) -> torch.Tensor:
    """[M,C,h,w] -> [4M,C,ceil(h/2),ceil(w/2)]: item 4m + 2p + q = x[m, :, p::2, q::2], zero rows / columns added
    where h / w is odd."""
    M, C, h, w = x.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    out = torch.zeros(M, 4, C, h2, w2, dtype=x.dtype, device=x.device)
    for p in range(2):
        for q in range(2):
            s = x[:, :, p::2, q::2]
            out[:, 2 * p + q, :, :s.shape[2], :s.shape[3]] = s
    return out.view(4 * M, C, h2, w2)


def unpolyphase(y: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """The inverse: [4M,C,h2,w2] -> [M,C,h,w], pads dropped."""
    M4, C, h2, w2 = y.shape
    y = y.view(M4 // 4, 4, C, h2, w2)
    out = torch.empty(M4 // 4, C, h, w, dtype=y.dtype, device=y.device)
    for p in range(2):
        for q in range(2):
            t = out[:, :, p::2, q::2]
            t.copy_(y[:, 2 * p + q, :, :t.shape[2], :t.shape[3]])
    return out


def split_decode(t: torch.Tensor) -> torch.Tensor:
    """[M, G, h, w, 2, 8] bf16 -> fp32 [M, 8G, h, w]: hi + lo in fp32."""
    M, G, h, w, _, _ = t.shape
    v = t[..., 0, :].float() + t[..., 1, :].float()
    return v.permute(0, 1, 4, 2, 3).reshape(M, 8 * G, h, w)


# ------------------------------------------------------------------ the emulation

def emulate_conv(x: torch.Tensor, w32: torch.Tensor, b32: torch.Tensor, dil: int, relu: bool, lapse=None):
    """One native 3x3 conv: x (fp32 values that are hi + lo already, or any fp32: split here) with the folded fp32
    weight, the three passes in fp32, bias, ReLU, the result rounded to the split-bf16 encoding.  ``lapse``:
    "x" / "w" zeroes that operand's ``lo``."""
    (xh, xl), (wh, wl) = br.split(x), br.split(w32)
    if lapse == "x":
        xl = torch.zeros_like(xl)
    elif lapse == "w":
        wl = torch.zeros_like(wl)
    elif lapse is not None:
        raise ValueError(lapse)
    y = br._three(lambda a, b: F.conv2d(a, b, padding=dil, dilation=dil), (xh, xl), (wh, wl))
    y = y + b32.view(1, -1, 1, 1)
    if relu:
        y = torch.relu(y)
    return sum(br.split(y))


def emulate_d4(x, conv, bn, lapse=None):
    """The folded dilation-4 conv as the native path runs it (no ReLU)."""
    w, b = fold64(conv, bn)
    return emulate_conv(x.float(), w.float(), b.float(), 4, False, lapse)


TAIL_LAPSES = [(op, k) for k in range(4) for op in ("x", "w")]


def emulate_tail(blocks: nn.Sequential, xs, lapse=None) -> torch.Tensor:
    """The native tail on the CPU: [n * B, cout, h, w] fp32.  ``lapse`` = (operand, k): conv k (0: block 0 conv1,
    1: block 0 conv2, 2: block 1 conv1, 3: block 1 conv2) loses that operand's ``lo`` pass."""
    x = torch.cat([t.detach().cpu().float() for t in xs])
    k = 0
    with torch.no_grad():
        for blk in blocks:
            ident = x
            if blk.downsample is not None:
                wd, bd = fold64(blk.downsample[0], blk.downsample[1])
                ident = F.conv2d(x, wd.float(), bd.float())
            w1, b1 = fold64(blk.conv1, blk.bn1)
            w2, b2 = fold64(blk.conv2, blk.bn2)
            y = emulate_conv(x, w1.float(), b1.float(), blk.conv1.dilation[0], True,
                             lapse[0] if lapse is not None and lapse[1] == k else None)
            y = emulate_conv(y, w2.float(), b2.float(), 1, False,
                             lapse[0] if lapse is not None and lapse[1] == k + 1 else None)
            k += 2
            x = torch.relu(y + ident)
    return x
