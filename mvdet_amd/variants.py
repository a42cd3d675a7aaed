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

``ImageProjVariant`` (``multiview_detector/models/image_proj_variant.py:16-118``) is the "early fusion" ablation: the
3-channel IMAGES are resized (``:67``), warped (``:69``) and concatenated with the coord map (``:88``), ONE ResNet-18
with ``3 * num_cam + 2`` input channels runs on the ground plane (``:44-48,89-90``), and ``map_classifier`` is three
3x3 convs without coord channels on the dense ``[B,512,h',w']`` world feature at 1/8 of the grid (``:53-56,91``),
followed by a real ~8x bilinear interpolate (``:92``).  Same drop-in contract (no ``img_classifier``: the
``state_dict`` holds ``base_pt1.*``, ``base_pt2.*``, ``map_classifier.{0,2,4}.*``; ``imgs_result`` is N all-zero
``[B,2,H,W]`` tensors at the input image size, ``:65-66``).  The backbone is torch; everything in front of it is one
HIP launch (``mvdet_amd.img_proj``: resize + warp + concat + coord channels, born in the backbone's memory format)
and everything behind it the native dense head (``mvdet_amd.dense_head``: the MFMA convs and the closing upsample,
in inference and under autograd); ``native_map_head=False`` keeps ``map_classifier`` + ``F.interpolate`` as torch
ops, the front stays native.  Nothing in front of the backbone has parameters, so the front has no backward.

Every variant takes ``frame_transform=`` as ``PerspTransDetector`` does (``detector._ViewsDetector._frames``): with it,
``forward`` also accepts the decoded uint8 ``[B,N,H,W,3]`` frames and runs ``mvdet_amd.frames`` on them first.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native
from .backbone import build_backbone
from .dense_head import DenseFuseHead
from .detector import _ViewsDetector
from .geometry import coord_map as make_coord_map
from .geometry import projection_matrices, upsample_shape
from .img_proj import ImageProjection
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
                 native_img_head: bool = True, frame_transform=None):
        super().__init__()
        self.frame_transform = frame_transform
        out_channel = self._init_views(dataset, arch, device, channels_last, native_img_head)
        self.map_classifier = nn.Sequential(nn.Conv2d(out_channel * self.num_cam + 2, 512, 1), nn.ReLU(),
                                            nn.Conv2d(512, 1, 1, bias=False))          # :51-53
        self._place()
        self._out_channel = out_channel
        self.head = ProjectSumHead(self.proj_mats, tuple(self.upsample_shape), tuple(self.reducedgrid_shape))

    def forward(self, imgs: torch.Tensor, visualize: bool = False):
        imgs = self._frames(imgs)
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
                 native_img_head: bool = True, frame_transform=None):
        super().__init__()
        self.frame_transform = frame_transform
        self._init_views(dataset, arch, device, channels_last, native_img_head)
        self.map_classifier = nn.Sequential(nn.Conv2d(self.num_cam + 2, 512, 3, padding=1), nn.ReLU(),
                                            nn.Conv2d(512, 512, 3, padding=2, dilation=2), nn.ReLU(),
                                            nn.Conv2d(512, 1, 3, padding=4, dilation=4, bias=False))  # :53-56
        self._place()
        self.head = ProjectThinFuse(self.proj_mats, tuple(self.upsample_shape), tuple(self.reducedgrid_shape))

    def forward(self, imgs: torch.Tensor, visualize: bool = False):
        imgs = self._frames(imgs)
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


class ImageProjVariant(_ViewsDetector):
    def __init__(self, dataset, arch: str = "resnet18", device=None, channels_last: bool = True,
                 native_map_head: bool = True, frame_transform=None):
        super().__init__()
        self.frame_transform = frame_transform
        self.num_cam = dataset.num_cam
        self.img_shape, self.reducedgrid_shape = list(dataset.img_shape), list(dataset.reducedgrid_shape)
        self.coord_map = make_coord_map(*self.reducedgrid_shape)                    # :24 (not a buffer)
        self.upsample_shape = upsample_shape(self.img_shape, dataset.img_reduce)   # :26
        self.proj_mats = projection_matrices(dataset)                               # :21-33 (fp64 list)
        if device is None:
            device = "cuda:0" if torch.cuda.is_available() else "cpu"
        self._device = torch.device(device)
        if self._device.type == "cuda":
            _native.load()  # no fallback: fail at construction if the HIP library is missing
        self.base_pt1, self.base_pt2, out_channel = build_backbone(arch, in_channels=3 * self.num_cam + 2)  # :35-49
        self.map_classifier = nn.Sequential(nn.Conv2d(out_channel, 512, 3, padding=1), nn.ReLU(),
                                            nn.Conv2d(512, 512, 3, padding=2, dilation=2), nn.ReLU(),
                                            nn.Conv2d(512, 1, 3, padding=4, dilation=4, bias=False))  # :53-56
        self.channels_last = bool(channels_last)
        # on: map_classifier and the closing interpolate on the HIP kernels (dense_head.py), inference and training;
        # off: the torch ops (the front is native either way)
        self.native_map_head = bool(native_map_head)
        self._place()
        self.front = ImageProjection(self.proj_mats, tuple(self.upsample_shape), tuple(self.reducedgrid_shape))
        self.head = DenseFuseHead(tuple(self.reducedgrid_shape))

    def forward(self, imgs: torch.Tensor, visualize: bool = False):
        imgs = self._frames(imgs)
        B, N, C, H, W = imgs.shape
        assert N == self.num_cam
        dev = self._device
        if dev.type != "cuda":
            raise RuntimeError("ImageProjVariant.forward needs a ROCm GPU (the hot path has no CPU fallback)")
        imgs = imgs.to(dev)  # once, not per camera (:67)
        # one memset where the reference has N (:65-66)
        imgs_result = list(torch.zeros([N, B, 2, H, W], device=dev).unbind(0))
        projected_imgs = self.front(imgs, channels_last=self.channels_last)          # :67-69, :88
        if visualize:
            for cam in range(N):
                self._show(projected_imgs[0, 3 * cam:3 * cam + 3].detach().permute(1, 2, 0))
        world_feature = self.base_pt2(self.base_pt1(projected_imgs))                  # :89-90
        if self.native_map_head:
            c1, c2, c3 = self.map_classifier[0], self.map_classifier[2], self.map_classifier[4]
            map_result = self.head(world_feature, c1.weight, c1.bias, c2.weight, c2.bias, c3.weight)  # :91-92
        else:
            map_result = F.interpolate(self.map_classifier(world_feature), self.reducedgrid_shape, mode="bilinear")
        return map_result, imgs_result
