"""Drop-in ``PerspTransDetector`` (``multiview_detector/models/persp_trans_detector.py:13-112``).

Same constructor (``dataset`` duck-type, ``arch``), same attributes
(``num_cam``, ``img_shape``, ``reducedgrid_shape``, ``coord_map``,
``upsample_shape``, ``proj_mats``), same sub-modules and therefore the same
``state_dict`` keys (``base_pt1.*``, ``base_pt2.*``, ``img_classifier.*``,
``map_classifier.*``), same ``forward(imgs, visualize=False) ->
(map_result [B,1,Ho,Wo], imgs_result: list[N] of [B,2,h,w])``.

What changes is the hot path (upsample + warp + concat + fusion), which runs on the
HIP kernels of ``libmvbev.so`` through ``ProjectFuse``:
* the 3x upsample of ``:65`` is fused into the warp (the 265 MB/view upsampled map is
  never written) and all views warp in one launch, straight into the fused tensor;
* the image head's first 1x1 conv runs before the upsample (64 instead of 512 channels
  upsampled; it commutes with bilinear interpolation), and the rest of the head (upsample, ReLU,
  second 1x1 conv) runs as one fused HIP launch over all views, forward and backward
  (``img_head.upsample_relu_conv1x1``; ``native_img_head=False`` keeps the torch ops);
* the coord channels are written once, not copied every forward;
* conv1/conv2 are MFMA implicit GEMMs (default 3xbf16 split precision, fp32
  accumulation — same parity as exact fp32; ``precision="fp32"`` selects the
  fp32-input MFMA), conv3 a dot-product kernel;
* the same-size final interpolate (an exact identity) is elided.

Training (autograd through the hot path, ``trainer.py:38-49``):
when grad is required upsample + warp + concat + fusion run as
``autograd.ProjectFuseFunction`` from the backbone-resolution maps — HIP forward (the fused
upsample + warp), HIP backward (the fused upsample + warp adjoint, conv data/weight/bias
gradients).  There is no stock-torch fallback for the hot path.
The library is loaded at construction on a GPU, so a missing build fails there.

``frame_transform=`` (a ``mvdet_amd.frames.FrameTransform``, default None) lets ``forward`` take the decoded frames, a
uint8 ``[B,N,H,W,3]`` tensor: the reference's ``train_trans`` (``main.py:38-40``) then runs first as one HIP launch and
its result is what ``forward`` would have been given.  Any other input takes the path above unchanged; the
``state_dict`` does not hold the transform.

``backbone_dtype=`` (``PerspTransDetector`` only; None, ``torch.bfloat16`` or ``torch.float16``; default None: nothing
changes) runs the backbone halves and the image head's first conv under ``torch.autocast`` in that dtype.  Parameters
and the ``state_dict`` stay fp32 (the reference's checkpoints load as before).  In inference the 16-bit maps go to the
fused upsample warp as they come out: it converts each value to fp32 exactly, so the hot path computes what it
computes from those maps cast to fp32, bit for bit; the rounding to 16 bits is the backbone's.  In training the maps
are cast to fp32 before the native forward and backward.  There is no loss scaling: fp16 training (a
``torch.amp.GradScaler``) is the caller's business.

``native_tail=`` (``PerspTransDetector`` with ``arch="resnet18"`` only; default False: nothing changes) runs
``base_pt2`` — ResNet-18's layer4, about 72 % of the backbone's arithmetic — in inference as
``res_tail.ResidualTail``: eval-mode BatchNorm folded into the convs, the four 3x3 convs on the 3xbf16 kernels over
all views at once, fp32-class accuracy (unlike ``backbone_dtype``, with which it cannot be combined).  ``base_pt1``
still runs per camera.  With autograd, BatchNorm in train mode or blocks the kernels do not take, the torch modules
run as without the flag.  The ``state_dict`` is unchanged.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native
from . import autograd as native_autograd
from . import img_head
from . import ops
from . import res_tail
from .backbone import build_backbone
from .geometry import coord_map as make_coord_map
from .geometry import projection_matrices, upsample_shape
from .pipeline import ProjectFuse


class _ViewsDetector(nn.Module):
    """What the reference's detector variants share (``persp_trans_detector.py`` and
    ``no_joint_conv_variant.py`` repeat it verbatim): the dataset attributes, the backbone halves, the image
    head, the per-view part of ``forward`` and the reference's helper methods.  A subclass adds its
    ``map_classifier`` between ``_init_views`` and ``_place``, which keeps the reference's ``state_dict`` order."""

    # a ``mvdet_amd.frames.FrameTransform`` (or None): when set, ``forward`` also takes the decoded frames, a uint8
    # ``[B,N,H,W,3]`` tensor, and runs the transform first.  A plain attribute: the ``state_dict`` does not hold it.
    frame_transform = None
    # None, torch.bfloat16 or torch.float16: the autocast dtype of the backbone halves and the image head's first
    # conv in ``_views_forward`` (``PerspTransDetector(backbone_dtype=...)`` sets it; the variants leave it None).
    # A plain attribute: parameters and the ``state_dict`` stay fp32.
    backbone_dtype = None
    # True: in inference ``base_pt2`` (ResNet-18's layer4) runs as ``res_tail.ResidualTail`` over all views at once,
    # eval-mode BatchNorm folded into the 3xbf16 convs (``PerspTransDetector(native_tail=True)`` sets it; the
    # variants leave it False).  A plain attribute; where the native path does not apply the torch modules run.
    native_tail = False
    _tail = None  # the ResidualTail of base_pt2[0], made on first use (not a module: nothing joins the state_dict)

    def _native_tail(self):
        """The ``ResidualTail`` when this forward runs ``base_pt2`` natively, else None: the flag is on, the
        module is on a GPU, ``base_pt2`` is one ``Sequential`` of blocks, no autograd is needed and every
        BatchNorm of the blocks is in eval mode (the shape is checked by the tail itself)."""
        if not self.native_tail or self._device.type != "cuda" or self.backbone_dtype is not None or \
                len(self.base_pt2) != 1 or not isinstance(self.base_pt2[0], nn.Sequential):
            return None
        if self._tail is None or self._tail.blocks is not self.base_pt2[0]:
            self._tail = res_tail.ResidualTail(self.base_pt2[0])
        return self._tail

    def _frames(self, imgs):
        """``imgs`` as ``forward`` takes them: decoded uint8 frames go through ``frame_transform`` (on the module's
        device), anything else (the reference's fp32 ``[B,N,3,H,W]``) is returned as it is."""
        ft = self.frame_transform
        if ft is not None and ft.takes(imgs):
            return ft(imgs.to(self._device))
        return imgs

    def _init_views(self, dataset, arch: str, device, channels_last: bool, native_img_head: bool) -> int:
        self.num_cam = dataset.num_cam
        self.img_shape, self.reducedgrid_shape = list(dataset.img_shape), list(dataset.reducedgrid_shape)
        self.coord_map = make_coord_map(*self.reducedgrid_shape)          # :21 (not a buffer)
        self.upsample_shape = upsample_shape(self.img_shape, dataset.img_reduce)  # :23
        self.proj_mats = projection_matrices(dataset)                       # :18-30 (fp64 list)
        if device is None:
            device = "cuda:0" if torch.cuda.is_available() else "cpu"
        self._device = torch.device(device)
        if self._device.type == "cuda":
            _native.load()  # no fallback: fail at construction if the HIP library is missing
        self.base_pt1, self.base_pt2, out_channel = build_backbone(arch)
        self.img_classifier = nn.Sequential(nn.Conv2d(out_channel, 64, 1), nn.ReLU(),
                                            nn.Conv2d(64, 2, 1, bias=False))
        self.channels_last = bool(channels_last)
        # on: the image head after its first conv as one fused launch over the views (img_head.py), inference and
        # training; off: the torch ops per view inside the camera loop (F.interpolate, F.relu, the second conv)
        self.native_img_head = bool(native_img_head)
        return out_channel

    def _place(self) -> None:
        self.to(self._device)
        # the backbone in torch's channels_last memory format (the same weights and state_dict): its maps then
        # reach the fused upsample warp's line-per-pixel kernel without a transposing copy (cfg2: 0.29-0.32 vs
        # 0.39 ms), and the MIOpen backbone itself ran no slower (7 x 720 x 1280: 21.4 vs 22.8 ms,
        # profiles/r05ah_backbone_layout.json)
        if self.channels_last:
            self.base_pt1.to(memory_format=torch.channels_last)
            self.base_pt2.to(memory_format=torch.channels_last)

    def _needs_autograd(self) -> bool:
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def _views_forward(self, imgs: torch.Tensor, visualize: bool = False):
        """The camera loop up to the warp: every view's backbone map (channels-last when the backbone is) and
        the image head's results (``:62-66``).  With ``backbone_dtype`` the backbone halves and the image head's
        first conv run under ``torch.autocast`` in that dtype: the maps come out 16-bit (and go on as they come
        out — whatever dtype arrives is what the engine dispatches on), the head's 64-channel ``g`` is cast to
        fp32 so that the fused image head still runs."""
        dev = self._device
        imgs_result, low, head_low = [], [], []
        split_head, native_head = self._img_head_splits(), None
        bdt = self.backbone_dtype

        def cast():  # a fresh context per use: the backbone's autocast, or nothing
            return torch.autocast("cuda", dtype=bdt) if bdt is not None else contextlib.nullcontext()
        def front(cam):  # one camera's frames through the first backbone half
            x = imgs[:, cam].to(dev)
            return self.base_pt1(x.contiguous(memory_format=torch.channels_last) if self.channels_last else x)
        feats, tail = None, self._native_tail()
        if tail is not None:  # base_pt1 per camera as below, then the tail once over all views
            mids = [front(cam) for cam in range(self.num_cam)]
            feats = tail(mids)  # (the torch blocks per view where the native path does not apply)
        for cam in range(self.num_cam):
            if feats is not None:
                feat = feats[cam]
            else:
                with cast():
                    feat = self.base_pt2(front(cam))
            # the image head runs its first 1x1 conv before upsampling (it commutes with the
            # bilinear upsample: per-pixel affine, weights summing to 1) on 64 instead of 512
            # channels
            if split_head:
                with cast():
                    g = self.img_classifier[0](feat)
                if g.dtype in ops.HALF_MAP_DTYPES:
                    g = g.float()
                if native_head is None:
                    native_head = self._img_head_native(g)
                if native_head:
                    head_low.append(g)  # all views go through one fused launch after the loop
                else:
                    imgs_result.append(self.img_classifier[2](
                        F.relu(F.interpolate(g, self.upsample_shape, mode="bilinear"))))
            else:
                imgs_result.append(self.img_classifier(F.interpolate(
                    feat.float() if feat.dtype in ops.HALF_MAP_DTYPES else feat, self.upsample_shape, mode="bilinear")))
            # the 3x upsample (:65) happens inside the fused warp below (and, training, its
            # adjoint inside the warp adjoint)
            # (a channels-last backbone's maps stay channels-last: the fused warp's line-per-pixel kernel)
            cl = feat.dim() == 4 and feat.is_contiguous(memory_format=torch.channels_last)
            low.append(feat if cl else feat.contiguous())
            if visualize:
                up = F.interpolate(feat, self.upsample_shape, mode="bilinear")
                self._show(torch.norm(up[0].detach(), dim=0))
        if head_low:
            imgs_result = img_head.upsample_relu_conv1x1(head_low, self.img_classifier[2].weight,
                                                         tuple(self.upsample_shape))
        return low, imgs_result

    def _img_head_splits(self) -> bool:
        """Whether ``img_classifier`` is Conv2d(1x1) -> ReLU -> module, so that its first conv can run
        before the upsample: ``img_classifier(F.interpolate(feat, upsample_shape))`` (:65-66) evaluated
        as head[2](relu(upsample(head[0](feat)))), identical in exact arithmetic."""
        head = self.img_classifier
        return (len(head) == 3 and isinstance(head[0], nn.Conv2d) and head[0].kernel_size == (1, 1)
                and isinstance(head[1], nn.ReLU))

    def _img_head_native(self, g: torch.Tensor) -> bool:
        """Whether relu(upsample(g)) -> head[2] runs as the fused HIP op: the flag is on, the second conv is a
        plain bias-free 1x1 conv, everything is fp32 and the shape is inside the kernels' range."""
        last = self.img_classifier[2]
        return (self.native_img_head and isinstance(last, nn.Conv2d) and last.kernel_size == (1, 1)
                and last.stride == (1, 1) and last.padding == (0, 0) and last.groups == 1 and last.bias is None
                and last.weight.dtype == torch.float32 and g.dtype == torch.float32 and g.is_cuda
                and img_head.supported(self.num_cam, g.shape, last.out_channels, tuple(self.upsample_shape)))

    @staticmethod
    def _show(img):
        import matplotlib.pyplot as plt
        plt.imshow(img.cpu().numpy())
        plt.show()

    # -- reference helpers (same names) ----------------------------------------------------
    def get_imgcoord2worldgrid_matrices(self, intrinsic_matrices, extrinsic_matrices, worldgrid2worldcoord_mat):
        from .geometry import imgcoord2worldgrid_matrices
        mats = imgcoord2worldgrid_matrices(intrinsic_matrices, extrinsic_matrices, worldgrid2worldcoord_mat,
                                           self.num_cam)
        return {cam: m for cam, m in enumerate(mats)}

    def create_coord_map(self, img_size, with_r=False):
        H, W, _ = img_size
        ret = make_coord_map(H, W)
        if with_r:
            rr = torch.sqrt(ret[:, 0] ** 2 + ret[:, 1] ** 2).view([1, 1, H, W])
            ret = torch.cat([ret, rr], dim=1)
        return ret


class PerspTransDetector(_ViewsDetector):
    def __init__(self, dataset, arch: str = "resnet18", device=None, precision: str = "bf16x3",
                 wino_conv1: bool = True, wino_conv2: bool = True, channels_last: bool = True,
                 native_img_head: bool = True, frame_transform=None, backbone_dtype=None, native_tail: bool = False):
        super().__init__()
        if backbone_dtype not in (None, torch.bfloat16, torch.float16):
            raise ValueError(f"backbone_dtype must be None, torch.bfloat16 or torch.float16, not {backbone_dtype!r}")
        if native_tail and arch != "resnet18":
            raise ValueError(f"native_tail runs ResNet-18's layer4; arch={arch!r} has no residual tail")
        if native_tail and backbone_dtype is not None:
            raise ValueError("native_tail takes the fp32 backbone: it cannot be combined with backbone_dtype")
        self.frame_transform = frame_transform
        self.backbone_dtype = backbone_dtype
        self.native_tail = bool(native_tail)
        out_channel = self._init_views(dataset, arch, device, channels_last, native_img_head)
        self.map_classifier = nn.Sequential(nn.Conv2d(out_channel * self.num_cam + 2, 512, 3, padding=1), nn.ReLU(),
                                            nn.Conv2d(512, 512, 3, padding=2, dilation=2), nn.ReLU(),
                                            nn.Conv2d(512, 1, 3, padding=4, dilation=4, bias=False))
        self._place()
        # conv1 and conv2 as row-Winograd F(3,3) (ProjectFuse.conv1_wino, conv2_partials), inference and
        # training (forward, data and weight gradients: autograd.py)
        self.engine = ProjectFuse(self.proj_mats, tuple(self.upsample_shape), tuple(self.reducedgrid_shape),
                                  out_channel, precision=precision, wino_conv1=wino_conv1, wino_conv2=wino_conv2)

    # -- hot path --------------------------------------------------------------------------
    def forward(self, imgs: torch.Tensor, visualize: bool = False):
        imgs = self._frames(imgs)
        B, N, C, H, W = imgs.shape
        assert N == self.num_cam
        dev = self._device
        if dev.type != "cuda":
            raise RuntimeError("PerspTransDetector.forward needs a ROCm GPU (the hot path has no CPU fallback)")
        training = self._needs_autograd()
        ws = None if training else self.engine.workspace(B, dev)
        low, imgs_result = self._views_forward(imgs, visualize)
        if training:  # a4-a9 forward and backward on the HIP kernels (autograd.py)
            # 16-bit maps (backbone_dtype) enter the native forward + backward as fp32: a differentiable cast,
            # the gradient returns to the backbone in the maps' dtype
            low = [f.float() if f.dtype in ops.HALF_MAP_DTYPES else f for f in low]
            map_result = native_autograd.project_fuse_backbone(self.engine, low, self.map_classifier)
        else:
            self.engine.warp_views_upsampled(ws, list(range(self.num_cam)), low)  # a4 + a5 + a6
            map_result = self.engine.fuse(ws, self.map_classifier)
        if visualize:
            self._show(torch.norm(map_result[0].detach(), dim=0))
        return map_result, imgs_result
