"""ResNet-18's layer4 for inference on the 3xbf16 convs, eval-mode BatchNorm folded in.

``base_pt2`` of the ResNet-18 detector is layer4 and nothing else (``backbone.py``: the trunk split at 7): two
``BasicBlock``s, four dense 3x3 convs and one 1x1 downsample conv on the 1/8-resolution map, about 72 % of the
backbone's arithmetic.  Those 3x3 convs have the shapes of ``map_classifier``'s conv2, so in inference they can run
on the kernel that runs it: ``ops.conv3x3_desc`` on the split-bf16 blocked layout (the LDS-DMA ring kernel, fp32-class
accuracy), with every view's every batch item as the conv's batch.

``ResidualTail(blocks)`` wraps the ``nn.Sequential`` of blocks (``base_pt2[0]``).  It is not a module: it holds no
parameters and adds nothing to any ``state_dict``.  ``tail(xs)`` takes the N per-view maps ``[B,Cin,h,w]`` and returns
N fp32 channels-last maps ``[B,Cout,h,w]``, slices of one ``[N*B,...]`` tensor.

The native path runs when no autograd is needed, every BatchNorm of the blocks is in eval mode and ``supported``
holds; otherwise the torch modules run, unchanged.  ``why_not`` names what ``supported`` excludes:

* a strided block (ResNet-18's layer2-4 without ``replace_stride_with_dilation``), anything but 3x3 convs with
  padding = dilation, groups 1 and no bias, a conv1 dilation outside {1, 2, 4} or a conv2 dilation other than 1;
* ``Cin % 16 != 0`` (the convs walk K in chunks of 16) or ``Cout % 128 != 0`` (their output-channel tile): layer1
  (64 channels) is out, layer2-4 of ResNet-18 are in by channel count;
* a downsample that is not Conv2d(1x1, stride 1, no bias) + BatchNorm2d, BatchNorm without affine parameters or
  running statistics, anything that is not fp32, a module that is not a ``BasicBlock``;
* more than 16 views, or a map too large for the kernels' 32-bit pixel indices.

Per block, on the GPU:

* conv1 with the folded weights and bias and ReLU in the epilogue, split-bf16 in and out.  Dilation 4 does not fit
  the ring kernel (``RingGeo<4>``: 3 * 1536 + 2 * 3328 entries of 16 B = 176 KiB of LDS against 160 KiB), so it
  runs as dilation 2 on the four 2 x 2 polyphase sub-grids ``x_pq[r, c] = x[2r + p, 2c + q]``: four times the
  items at ceil(h/2) x ceil(w/2), the rows / columns added for odd sizes exact zeros.  The taps of output
  (2r + p, 2c + q) are ``x[2(r + 2i) + p, 2(c + 2j) + q]``, all in sub-grid (p, q) at dilation 2, and a tap
  outside the sub-grid is a tap outside the map: the identity is exact, zero padding included.
* conv2 (dilation 1) with the folded bias and no ReLU;
* the 1x1 downsample as a torch GEMM on the channels-last input with the folded weight and bias (the README's
  policy for plain GEMMs);
* ``relu(conv2 + identity)`` as one HIP pass (``ops.residual_close``) that also writes the next block's conv1
  input, plain or polyphase, so block 1 reads block 0's result without a conversion launch.

BN folding, per conv and once per weight version: ``w' = w * gamma / sqrt(var + eps)``,
``b' = beta - mean * gamma / sqrt(var + eps)``, computed in fp64 and rounded once to fp32.  The folds and their
packed forms are rebuilt when the ``_version`` (or storage) of any conv or BatchNorm tensor changes, which covers
in-place edits, ``running_mean`` / ``running_var`` and ``load_state_dict``.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native
from . import ops
from .backbone import BasicBlock

MAX_VIEWS = 16
CIN_GRANULE = 16     # the convs' K chunk
COUT_GRANULE = 128   # MVBEV_CONV_BN
CONV1_DILATIONS = (1, 2, 4)


def fold_bn(weight: torch.Tensor, bn: nn.BatchNorm2d) -> Tuple[torch.Tensor, torch.Tensor]:
    """Eval-mode ``bn(conv(x, weight))`` as ``conv(x, w') + b'``: (w', b') in fp64 on ``weight``'s device."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    w = weight.detach().double() * s.view(-1, 1, 1, 1)
    b = bn.bias.detach().double() - bn.running_mean.detach().double() * s
    return w, b


def polyphase_split(x: torch.Tensor) -> torch.Tensor:
    """[M,C,h,w] -> [4M,C,ceil(h/2),ceil(w/2)], item 4m + 2p + q = x[m, :, p::2, q::2] zero-padded (the torch
    statement of the polyphase layout; the GPU path never calls it)."""
    M, C, h, w = x.shape
    h2, w2 = ops.polyphase_hw(h, w)
    xp = F.pad(x, (0, 2 * w2 - w, 0, 2 * h2 - h))
    return xp.view(M, C, h2, 2, w2, 2).permute(0, 3, 5, 1, 2, 4).reshape(4 * M, C, h2, w2)


def polyphase_join(y: torch.Tensor, hw) -> torch.Tensor:
    """The inverse of ``polyphase_split`` for an (h, w) grid: [4M,C,h2,w2] -> [M,C,h,w] (pads dropped)."""
    h, w = hw
    M4, C, h2, w2 = y.shape
    full = y.view(M4 // 4, 2, 2, C, h2, w2).permute(0, 3, 4, 1, 5, 2).reshape(M4 // 4, C, 2 * h2, 2 * w2)
    return full[:, :, :h, :w]


def _bn_problem(bn, what: str) -> Optional[str]:
    if not isinstance(bn, nn.BatchNorm2d):
        return f"{what} is not a BatchNorm2d"
    if not bn.affine or bn.weight is None or bn.bias is None:
        return f"{what} has no affine parameters"
    if not bn.track_running_stats or bn.running_mean is None or bn.running_var is None:
        return f"{what} has no running statistics"
    if any(t.dtype != torch.float32 for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)):
        return f"{what} is not fp32"
    return None


def _conv_problem(conv, what: str, k: int, dilations) -> Optional[str]:
    if not isinstance(conv, nn.Conv2d):
        return f"{what} is not a Conv2d"
    if conv.kernel_size != (k, k):
        return f"{what} is not a {k}x{k} conv"
    if conv.stride != (1, 1):
        return f"{what} has stride {conv.stride[0]} (the native convs are stride 1)"
    if conv.groups != 1 or conv.bias is not None or conv.padding_mode != "zeros":
        return f"{what} must be a bias-free, ungrouped, zero-padded conv"
    d = conv.dilation[0]
    if conv.dilation != (d, d) or d not in dilations:
        return f"{what} has dilation {conv.dilation} (supported: {tuple(dilations)})"
    if conv.padding != ((k // 2) * d, (k // 2) * d):
        return f"{what} has padding {conv.padding}, not its dilation"
    if conv.weight.dtype != torch.float32:
        return f"{what} is not fp32"
    return None


def why_not(blocks, shape=None, n_views: int = 1) -> Optional[str]:
    """None when the native path takes these blocks (and, when given, ``n_views`` maps of ``shape`` [B,Cin,h,w]);
    else the reason, one line."""
    try:
        mods = list(blocks)
    except TypeError:
        return "blocks is not a sequence of BasicBlocks"
    if not mods:
        return "no blocks"
    cin = None
    for i, blk in enumerate(mods):
        if not isinstance(blk, BasicBlock):
            return f"block {i} is a {type(blk).__name__}, not a BasicBlock"
        p = (_conv_problem(blk.conv1, f"block {i} conv1", 3, CONV1_DILATIONS) or _bn_problem(blk.bn1, f"block {i} bn1")
             or _conv_problem(blk.conv2, f"block {i} conv2", 3, (1,)) or _bn_problem(blk.bn2, f"block {i} bn2"))
        if p:
            return p
        ci, co = blk.conv1.in_channels, blk.conv1.out_channels
        if cin is not None and ci != cin:
            return f"block {i} takes {ci} channels, the block before it gives {cin}"
        if blk.conv2.in_channels != co or blk.conv2.out_channels != co:
            return f"block {i} conv2 is not {co} -> {co}"
        if ci % CIN_GRANULE:
            return f"block {i} has Cin={ci}, not a multiple of {CIN_GRANULE}"
        if co % COUT_GRANULE:
            return f"block {i} has Cout={co}, not a multiple of {COUT_GRANULE}"
        ds = blk.downsample
        if ds is None:
            if ci != co:
                return f"block {i} changes {ci} -> {co} channels without a downsample"
        else:
            if not isinstance(ds, nn.Sequential) or len(ds) != 2:
                return f"block {i} downsample is not Conv2d + BatchNorm2d"
            p = _conv_problem(ds[0], f"block {i} downsample conv", 1, (1,)) or \
                _bn_problem(ds[1], f"block {i} downsample bn")
            if p:
                return p
            if ds[0].in_channels != ci or ds[0].out_channels != co:
                return f"block {i} downsample is not {ci} -> {co}"
        cin = co
    if shape is not None:
        if len(shape) != 4:
            return f"maps must be [B,Cin,h,w], got {tuple(shape)}"
        B, C, h, w = (int(v) for v in shape)
        if C != mods[0].conv1.in_channels:
            return f"maps have {C} channels, block 0 takes {mods[0].conv1.in_channels}"
        if not 0 < n_views <= MAX_VIEWS:
            return f"{n_views} views (1..{MAX_VIEWS})"
        if B <= 0 or h <= 0 or w <= 0:
            return "empty maps"
        cmax = max(max(b.conv1.in_channels, b.conv1.out_channels) for b in mods)
        if (h + 1) * (w + 1) >= 2 ** 29 or 4 * n_views * B * cmax * (h + 1) * (w + 1) >= 2 ** 40:
            return "maps too large for the kernels' indices"
    return None


def supported(blocks, shape=None, n_views: int = 1) -> bool:
    """Whether the native path takes these blocks (and shape): see ``why_not`` and the module docstring."""
    return why_not(blocks, shape, n_views) is None


class _Fold:
    """One block's folded fp32 weights and biases and the 3x3 weights' 3xbf16 packs."""
    __slots__ = ("key", "w1", "b1", "p1", "w2", "b2", "p2", "wd", "bd")


def _block_tensors(blk: BasicBlock) -> List[torch.Tensor]:
    ts = [blk.conv1.weight, blk.bn1.weight, blk.bn1.bias, blk.bn1.running_mean, blk.bn1.running_var,
          blk.conv2.weight, blk.bn2.weight, blk.bn2.bias, blk.bn2.running_mean, blk.bn2.running_var]
    if blk.downsample is not None:
        c, bn = blk.downsample[0], blk.downsample[1]
        ts += [c.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var]
    return ts


class ResidualTail:
    """See the module docstring.  ``precision``: "bf16x3" (the only one; fp32-class accuracy)."""

    def __init__(self, blocks: nn.Sequential, precision: str = "bf16x3"):
        if precision != "bf16x3":
            raise ValueError('precision must be "bf16x3"')
        self.blocks = blocks
        self.precision = precision
        self._folds: List[Optional[_Fold]] = []
        self._packs: List[Tuple[ops.PackedConv3x3, ops.PackedConv3x3]] = []
        self._bufs = {}
        self.mark = None  # a callable(name) run before every launch group (tools/res_tail_bench.py's timing marks)

    # -- applicability ---------------------------------------------------------------------------
    def why_not(self, shape=None, n_views: int = 1) -> Optional[str]:
        return why_not(self.blocks, shape, n_views)

    def supported(self, shape=None, n_views: int = 1) -> bool:
        return self.why_not(shape, n_views) is None

    def _bn_eval(self) -> bool:
        return not any(m.training for m in self.blocks.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm))

    def _needs_autograd(self, xs) -> bool:
        return torch.is_grad_enabled() and (any(x.requires_grad for x in xs)
                                            or any(p.requires_grad for p in self.blocks.parameters()))

    def native_applies(self, xs: Sequence[torch.Tensor]) -> bool:
        """Whether ``tail(xs)`` runs the HIP path: GPU fp32 maps of one shape, no autograd, eval BN, ``supported``."""
        if not xs or not all(isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
                             and x.shape == xs[0].shape and x.device == xs[0].device for x in xs):
            return False
        return (not self._needs_autograd(xs) and self._bn_eval()
                and self.supported(tuple(xs[0].shape), len(xs)))

    # -- folds -----------------------------------------------------------------------------------
    def _fold(self, i: int, blk: BasicBlock) -> _Fold:
        key = tuple((t.data_ptr(), t._version, t.device) for t in _block_tensors(blk)) + \
            (blk.bn1.eps, blk.bn2.eps, None if blk.downsample is None else blk.downsample[1].eps, id(_native.load()))
        while len(self._folds) <= i:
            self._folds.append(None)
            self._packs.append((ops.PackedConv3x3(precision="bf16x3"), ops.PackedConv3x3(precision="bf16x3")))
        f = self._folds[i]
        if f is not None and f.key == key:
            return f
        f = _Fold()
        w1, b1 = fold_bn(blk.conv1.weight, blk.bn1)
        w2, b2 = fold_bn(blk.conv2.weight, blk.bn2)
        f.w1, f.b1 = w1.float().contiguous(), b1.float().contiguous()
        f.w2, f.b2 = w2.float().contiguous(), b2.float().contiguous()
        # fresh pack objects per fold: PackedConv3x3 keys on (data_ptr, _version), which a new tensor at a freed
        # tensor's address would repeat
        self._packs[i] = (ops.PackedConv3x3(precision="bf16x3"), ops.PackedConv3x3(precision="bf16x3"))
        f.p1 = self._packs[i][0].get(f.w1)
        f.p2 = self._packs[i][1].get(f.w2)
        f.wd = f.bd = None
        if blk.downsample is not None:
            wd, bd = fold_bn(blk.downsample[0].weight, blk.downsample[1])
            f.wd = wd.float().reshape(wd.shape[0], wd.shape[1]).t().contiguous()  # [Cin, Cout]: x @ wd
            f.bd = bd.float().contiguous()
        f.key = key
        self._folds[i] = f
        return f

    # -- forward ---------------------------------------------------------------------------------
    def _buf(self, name: str, shape, device) -> torch.Tensor:
        b = self._bufs.get(name)
        if b is None or tuple(b.shape) != tuple(shape) or b.device != device:
            b = self._bufs[name] = torch.empty(shape, dtype=torch.bfloat16, device=device)
        return b

    def _mark(self, name: str) -> None:
        if self.mark is not None:
            self.mark(name)

    def __call__(self, xs: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        xs = list(xs)
        if not self.native_applies(xs):
            return [self.blocks(x) for x in xs]
        return self._native_forward(xs)

    @staticmethod
    def _conv(x, M, K, h, w, packed, cout, bias, dilation, relu, out):
        d = ops.conv_desc(M, K, h, w, group=K, group_stride=0, batch_stride=K * h * w)
        return ops.conv3x3_desc(x, d, packed, cout, bias=bias, dilation=dilation, relu=relu, out=out)

    def _native_forward(self, xs: List[torch.Tensor]) -> List[torch.Tensor]:
        n = len(xs)
        B, _, h, w = xs[0].shape
        M, dev = n * B, xs[0].device
        h2, w2 = ops.polyphase_hw(h, w)
        cl = torch.channels_last
        xs = [x if x.is_contiguous(memory_format=cl) else x.contiguous(memory_format=cl) for x in xs]
        blocks = list(self.blocks)
        with torch.no_grad():
            poly = blocks[0].conv1.dilation[0] == 4
            self._mark("to_split")
            cin = xs[0].shape[1]
            xsplit = ops.channels_last_to_split(
                xs, polyphase=poly, out=self._buf("x0", ops.split_polyphase_shape(M, cin, h, w) if poly
                                                  else ops.split_shape(M, cin, h, w), dev))
            ident = xs  # block 0's identity: the per-view inputs; later blocks': one [M,...] tensor
            out = None
            for i, blk in enumerate(blocks):
                f = self._fold(i, blk)
                cin, cout, d1 = blk.conv1.in_channels, blk.conv1.out_channels, blk.conv1.dilation[0]
                if f.wd is not None:  # the 1x1 downsample: a GEMM per view on its channels-last pixels
                    self._mark(f"b{i}.downsample")
                    idt = torch.empty((M, h, w, cout), dtype=torch.float32, device=dev)
                    srcs = ident if isinstance(ident, list) else [ident]
                    rows = idt.view(len(srcs), -1, cout)
                    for v, x in enumerate(srcs):
                        torch.addmm(f.bd, x.permute(0, 2, 3, 1).reshape(-1, cin), f.wd, out=rows[v])
                    ident = idt.permute(0, 3, 1, 2)
                self._mark(f"b{i}.conv1")
                if d1 == 4:  # dilation 2 on the polyphase sub-grids, then back onto the full grid for conv2
                    y1p = self._conv(xsplit, 4 * M, cin, h2, w2, f.p1, cout, f.b1, 2, True,
                                     self._buf(f"y1p{i}", ops.split_polyphase_shape(M, cout, h, w), dev))
                    self._mark(f"b{i}.to_plain")
                    y1 = ops.split_polyphase_to_plain(y1p, (h, w), out=self._buf("y1", ops.split_shape(M, cout, h, w),
                                                                                 dev))
                else:
                    y1 = self._conv(xsplit, M, cin, h, w, f.p1, cout, f.b1, d1, True,
                                    self._buf("y1", ops.split_shape(M, cout, h, w), dev))
                self._mark(f"b{i}.conv2")
                y2 = self._conv(y1, M, cout, h, w, f.p2, cout, f.b2, 1, False,
                                self._buf("y2", ops.split_shape(M, cout, h, w), dev))
                self._mark(f"b{i}.close")
                nxt_poly, nxt_buf = None, None
                if i + 1 < len(blocks):
                    nxt_poly = blocks[i + 1].conv1.dilation[0] == 4
                    nxt_buf = self._buf(f"x{i + 1}", ops.split_polyphase_shape(M, cout, h, w) if nxt_poly
                                        else ops.split_shape(M, cout, h, w), dev)
                out, xsplit = ops.residual_close(y2, ident, (h, w), next_polyphase=nxt_poly, next_out=nxt_buf)
                ident = out
            self._mark("end")
        return [out[v * B:(v + 1) * B] for v in range(n)]
