"""Drop-in ``NoJointConvVariant`` (``multiview_detector/models/no_joint_conv_variant.py:13-86``), the paper's
"no joint spatial reasoning" ablation: every view's 512-channel map is upsampled, warped and concatenated, and
``map_classifier`` is two 1x1 convs, ``Conv2d(512 N + 2, 512, 1) -> ReLU -> Conv2d(512, 1, 1, bias=False)``.

Same constructor (``dataset`` duck-type, ``arch``), attributes, sub-modules and ``state_dict`` keys as the
reference class, same ``forward(imgs, visualize=False) -> (map_result [B,1,Ho,Wo], imgs_result)``.  The
backbone and the image head run exactly as in ``PerspTransDetector`` (shared code, ``detector._ViewsDetector``).
The ground-plane head runs in the commuted order of ``mvdet_amd.sum_head``: the view blocks of
``map_classifier[0].weight`` are applied at backbone resolution by ONE batched fp32 GEMM on the channels-last
maps (torch's, like ``img_classifier[0]``; its gradients are torch's own), and upsample + warp + sum over views +
bias + coord term + ReLU + the second conv are one HIP launch (``ProjectSumHead``), in inference and under
autograd.  The 265 MB upsampled maps and the 620 MB concatenated slab of config 2 are never written.  The
same-size final interpolate (``:81``, an exact identity) is elided.  There is no CPU fallback.

Non-finite features or weights are outside the contract of the commuted order (see ``mvdet_amd.sum_head``).

``ResProjVariant`` (``multiview_detector/models/res_proj_variant.py:15-84``) is the "late fusion" ablation: the
ground plane sees only the warped FOOT channel of every view's image result (``img_res[:, 1]``, ``:72``) and the
coord map, and ``map_classifier`` is ``PerspTransDetector``'s three 3x3 convs over ``num_cam + 2`` input channels
(``:53-56``).  Same drop-in contract.  The planes are channel slices of ``imgs_result`` (views, not copies):
warp + coord channels + conv1 + bias + ReLU are one HIP launch and conv2 / conv3 the engine's
(``mvdet_amd.thin_fuse.ProjectThinFuse``), in inference and under autograd, where the planes' gradient joins the
loss's own gradient of ``imgs_result`` on its way into the image head's backward.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .detector import _ViewsDetector
from .sum_head import ProjectSumHead
from .thin_fuse import ProjectThinFuse


def view_gemm(feats, weight: torch.Tensor, n_views: int):
    """``z_v = W_v feat_v`` for every view in one batched GEMM: ``feats`` a list of N ``[B,C,h,w]`` maps,
    ``weight`` ``map_classifier[0].weight`` ``[Cm, C N + 2, 1, 1]``.  Returns N ``[B,Cm,h,w]`` views with channel
    stride 1 (channels-last lines, no copy of the result)."""
    B, C, h, w = feats[0].shape
    cm = weight.shape[0]
    # [N, B h w, C]: a channels-last map is already pixel-major, so the permute + reshape is a view of it
    x = torch.stack([f.permute(0, 2, 3, 1).reshape(B * h * w, C) for f in feats], 0)
    wv = weight.reshape(cm, -1)[:, :C * n_views].reshape(cm, n_views, C).permute(1, 2, 0)  # [N, C, Cm]
    z = torch.bmm(x, wv).view(n_views, B, h, w, cm).permute(0, 1, 4, 2, 3)  # [N, B, Cm, h, w], Cm innermost
    return list(z.unbind(0))


class NoJointConvVariant(_ViewsDetector):
    def __init__(self, dataset, arch: str = "resnet18", device=None, channels_last: bool = True,
                 native_img_head: bool = True):
        super().__init__()
        out_channel = self._init_views(dataset, arch, device, channels_last, native_img_head)
        self.map_classifier = nn.Sequential(nn.Conv2d(out_channel * self.num_cam + 2, 512, 1), nn.ReLU(),
                                            nn.Conv2d(512, 1, 1, bias=False))          # :51-53
        self._place()
        self._out_channel = out_channel
        self.head = ProjectSumHead(self.proj_mats, tuple(self.upsample_shape), tuple(self.reducedgrid_shape))

    def forward(self, imgs: torch.Tensor, visualize: bool = False):
        B, N, C, H, W = imgs.shape
        assert N == self.num_cam
        if self._device.type != "cuda":
            raise RuntimeError("NoJointConvVariant.forward needs a ROCm GPU (the hot path has no CPU fallback)")
        low, imgs_result = self._views_forward(imgs, visualize)
        first, last = self.map_classifier[0], self.map_classifier[2]
        zs = view_gemm(low, first.weight, self.num_cam)
        w_coord = first.weight[:, self._out_channel * self.num_cam:, 0, 0]  # the coord channels' columns (:76)
        map_result = self.head(zs, first.bias, w_coord, last.weight)
        if visualize:
            self._show(torch.norm(map_result[0].detach(), dim=0))
        return map_result, imgs_result


class ResProjVariant(_ViewsDetector):
    def __init__(self, dataset, arch: str = "resnet18", device=None, channels_last: bool = True,
                 native_img_head: bool = True):
        super().__init__()
        self._init_views(dataset, arch, device, channels_last, native_img_head)
        self.map_classifier = nn.Sequential(nn.Conv2d(self.num_cam + 2, 512, 3, padding=1), nn.ReLU(),
                                            nn.Conv2d(512, 512, 3, padding=2, dilation=2), nn.ReLU(),
                                            nn.Conv2d(512, 1, 3, padding=4, dilation=4, bias=False))  # :53-56
        self._place()
        self.head = ProjectThinFuse(self.proj_mats, tuple(self.upsample_shape), tuple(self.reducedgrid_shape))

    def forward(self, imgs: torch.Tensor, visualize: bool = False):
        B, N, C, H, W = imgs.shape
        assert N == self.num_cam
        if self._device.type != "cuda":
            raise RuntimeError("ResProjVariant.forward needs a ROCm GPU (the hot path has no CPU fallback)")
        _, imgs_result = self._views_forward(imgs, False)
        planes = [r[:, 1:2] for r in imgs_result]  # head, *foot* (:72): views of the image results
        c1, c2, c3 = self.map_classifier[0], self.map_classifier[2], self.map_classifier[4]
        map_result = self.head(planes, c1.weight, c1.bias, c2.weight, c2.bias, c3.weight)
        if visualize:
            for r in imgs_result:
                self._show(r[0, 0].detach())
            self._show(torch.norm(map_result[0].detach(), dim=0))
        return map_result, imgs_result
