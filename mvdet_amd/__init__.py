"""mvdet_amd — MI355X-native MVDet perspective-transform hot path.

Public surface (mirrors the reference's):
* ``PerspTransDetector`` — drop-in for
  ``multiview_detector.models.persp_trans_detector.PerspTransDetector``.
* ``warp_perspective`` — drop-in for kornia 0.6.11
  ``kornia.geometry.transform.warp_perspective`` (default-argument path).
* ``ProjectFuse`` — the hot path (warp + zero-copy concat + fusion) as an engine.
* ``ProjectViews`` — the projection alone (upsample, warp, concat, coord channels) as a differentiable op for a
  head of your own: contiguous fp32 or channels-last fp32 / bf16 / fp16 maps in, the same format out
  (``mvdet_amd.project_views``).
* ``ProjectPlanes`` — the weighted multi-plane projection: every view through D ground-parallel planes, mixed by a
  per-pixel weight, summed inside the gather (one launch forward, one backward; ``mvdet_amd.project_planes``).
* ``postprocess.nms`` / ``threshold_rows`` / ``frame_results`` — drop-ins for
  ``multiview_detector.utils.nms.nms`` and the evaluation rows of ``trainer.py:97-157``.
* ``GaussianMSE`` / ``detection_loss`` / ``gaussian_kernels`` — drop-ins for
  ``multiview_detector.loss.gaussian_mse.GaussianMSE`` and the loss / precision-recall lines of
  ``trainer.py:43-56`` (``mvdet_amd.loss``).
* ``PointTargets`` / ``pack_step`` — the ground truth as point lists from the dataset's ``coo_matrix``
  objects to the criterion's kernel, one upload of a few kB per step (``mvdet_amd.targets``); the
  criterion takes one wherever it takes a dense target, with bitwise the dense result.
* ``upsample_relu_conv1x1`` — the image head after its first conv (bilinear upsample, ReLU, 1x1
  conv) for all views in one launch, with a native backward (``mvdet_amd.img_head``).
* ``NoJointConvVariant`` — drop-in for ``multiview_detector.models.no_joint_conv_variant.NoJointConvVariant``
  (``mvdet_amd.variants``); ``ProjectSumHead`` — its ground-plane head after the first 1x1 conv (upsample,
  warp, sum over views, ReLU, second conv) as one launch with a native backward (``mvdet_amd.sum_head``).
* ``ResProjVariant`` — drop-in for ``multiview_detector.models.res_proj_variant.ResProjVariant``
  (``mvdet_amd.variants``); ``ProjectThinFuse`` — its ground-plane head: warp of the views' foot planes, coord
  channels, the thin first conv, bias and ReLU as one launch, then the engine's conv2 / conv3, with a native
  backward (``mvdet_amd.thin_fuse``).
* ``ImageProjVariant`` — drop-in for ``multiview_detector.models.image_proj_variant.ImageProjVariant``
  (``mvdet_amd.variants``); ``ImageProjection`` — its front: image resize, warp, concat and coord channels as one
  launch (``mvdet_amd.img_proj``); ``DenseFuseHead`` — its ground-plane head on the dense world feature: the three
  convs and the closing bilinear upsample, with a native backward (``mvdet_amd.dense_head``).
* ``FrameTransform`` / ``resize_normalize`` — the reference's ``train_trans`` (``main.py:38-40``: Pillow's bilinear
  ``T.Resize``, ``T.ToTensor``, ``T.Normalize``) on the decoded uint8 frames of every view in one launch, bit for bit
  (``mvdet_amd.frames``); every detector takes one as ``frame_transform=`` and then accepts the uint8 frames.
* ``evaluation`` — drop-ins for ``multiview_detector.evaluation.evaluate.evaluate`` and ``evaluation/pyeval``
  (``CLEAR_MOD_HUN``, ``evaluateDetection_py``): MODA, MODP, precision and recall with the Hungarian matching of
  all frames in one launch; ``DetectionEvaluator`` — a test epoch from output maps to the four numbers with
  no host sync per frame (``mvdet_amd.evaluation``).
* ``ResidualTail`` — ResNet-18's layer4 (``base_pt2``) for inference: eval-mode BatchNorm folded into the convs, the
  3x3 convs on the 3xbf16 kernels over all views at once, fp32-class accuracy (``mvdet_amd.res_tail``;
  ``PerspTransDetector(native_tail=True)``, off by default).

The compute runs in ``mvdet_amd/lib/libmvbev.so`` (HIP, gfx950; C ABI in
``include/mvbev.h``); there is no CPU fallback.
"""
from .detector import PerspTransDetector  # noqa: F401
from .ops import warp_perspective  # noqa: F401
from .pipeline import ProjectFuse  # noqa: F401
from . import postprocess  # noqa: F401
from . import loss  # noqa: F401
from .loss import GaussianMSE, detection_loss, gaussian_kernels  # noqa: F401
from . import targets  # noqa: F401
from .targets import PointTargets, pack_step  # noqa: F401
from . import img_head  # noqa: F401
from .img_head import upsample_relu_conv1x1  # noqa: F401
from . import sum_head  # noqa: F401
from .sum_head import ProjectSumHead  # noqa: F401
from . import thin_fuse  # noqa: F401
from .thin_fuse import ProjectThinFuse  # noqa: F401
from . import img_proj  # noqa: F401
from .img_proj import ImageProjection  # noqa: F401
from . import dense_head  # noqa: F401
from .dense_head import DenseFuseHead  # noqa: F401
from . import frames  # noqa: F401
from .frames import FrameTransform, resize_normalize  # noqa: F401
from . import evaluation  # noqa: F401
from .evaluation import DetectionEvaluator, evaluate  # noqa: F401
from . import project_views  # noqa: F401
from .project_views import ProjectViews  # noqa: F401
from . import project_planes  # noqa: F401
from .project_planes import ProjectPlanes  # noqa: F401
from . import res_tail  # noqa: F401
from .res_tail import ResidualTail  # noqa: F401
from .variants import ImageProjVariant, NoJointConvVariant, ResProjVariant  # noqa: F401

__all__ = ["PerspTransDetector", "warp_perspective", "ProjectFuse", "postprocess", "loss", "GaussianMSE",
           "detection_loss", "gaussian_kernels", "targets", "PointTargets", "pack_step", "img_head", "upsample_relu_conv1x1",
           "sum_head", "ProjectSumHead", "NoJointConvVariant", "thin_fuse", "ProjectThinFuse", "ResProjVariant",
           "img_proj", "ImageProjection", "dense_head", "DenseFuseHead", "ImageProjVariant", "frames",
           "FrameTransform", "resize_normalize", "evaluation", "DetectionEvaluator", "evaluate", "project_views",
           "ProjectViews", "project_planes", "ProjectPlanes", "res_tail", "ResidualTail"]
