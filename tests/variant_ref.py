"""Test-side reference of ``NoJointConvVariant`` (``no_joint_conv_variant.py``): the seeded recipes of the
``variant_njc`` fixture's parameters and features, the CPU restatement of the reference's ``forward`` in the
REFERENCE'S ORDER, and the commuted order the native path evaluates.  Test infrastructure only.

Geometry is fp32 whatever the value dtype: the reference hands kornia the fp32 ``proj_mat`` (``:67``) and
kornia's sample coordinates are fp32 numbers, including where they overflow (a degenerate camera).  In fp64
the same fp32 coordinates are cast up for ``grid_sample``, so only the values gain precision.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from helpers import masked_relu
from oracle import kornia_warp
from oracle.fixtures import feature_input, params_sha256  # noqa: F401  (re-exported for the tests)


def njc_param_shapes(num_cam: int, C: int = 512, Cm: int = 512):
    """``img_classifier`` / ``map_classifier`` of ``no_joint_conv_variant.py:49-53`` in ``state_dict`` order."""
    return OrderedDict([
        ("img_classifier.0.weight", (64, C, 1, 1)),
        ("img_classifier.0.bias", (64,)),
        ("img_classifier.2.weight", (2, 64, 1, 1)),
        ("map_classifier.0.weight", (Cm, C * num_cam + 2, 1, 1)),
        ("map_classifier.0.bias", (Cm,)),
        ("map_classifier.2.weight", (1, Cm, 1, 1)),
    ])


def njc_params(num_cam: int, seed: int, C: int = 512, Cm: int = 512):
    """uniform(+-1/sqrt(fan_in)) per parameter (PyTorch's Conv2d bound) in ``state_dict`` order from PCG64(seed)."""
    shapes = njc_param_shapes(num_cam, C, Cm)
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for name, shp in shapes.items():
        fan_in = int(np.prod(shapes[name.replace(".bias", ".weight")][1:]))
        b = 1.0 / np.sqrt(fan_in)
        out[name] = rng.uniform(-b, b, size=shp).astype(np.float32)
    return out


def coord_map(ho: int, wo: int) -> torch.Tensor:
    """``create_coord_map`` (``:102-107``): [1, 2, ho, wo] fp32."""
    gx, gy = np.meshgrid(np.arange(wo), np.arange(ho))
    return torch.stack([torch.from_numpy(gx / (wo - 1) * 2 - 1).float(),
                        torch.from_numpy(gy / (ho - 1) * 2 - 1).float()], 0).unsqueeze(0)


def warp(src: torch.Tensor, M, dsize) -> torch.Tensor:
    """``kornia.warp_perspective(src, proj_mat.repeat([B,1,1]).float(), dsize)`` (``:67-68``).  fp32: the
    oracle's restatement itself.  Other dtypes: its own lines with the fp32 matrix, fp32 sample grid and fp32
    pixel coordinates; only the bilinear weights and sums run in the values' dtype (``test_variant_host`` pins
    the two to each other)."""
    B, _, H, W = src.shape
    pm = torch.as_tensor(np.asarray(M)).reshape(1, 3, 3).repeat([B, 1, 1]).float()
    if src.dtype == torch.float32:
        return kornia_warp.warp_perspective(src, pm, list(dsize))
    # grid_sample's own first step, the pixel coordinate ((x + 1) / 2) (size - 1), belongs to the fp32 geometry
    # too (it is where a degenerate camera's coordinates overflow): formed in fp32, then handed over as the
    # normalised fp64 coordinate that gives the same pixel
    g = sample_grid(pm, (H, W), dsize)
    size = torch.tensor([W - 1, H - 1], dtype=torch.float32)
    pix = ((g + 1) / 2) * size
    g64 = pix.to(src.dtype) / size.to(src.dtype) * 2 - 1
    return F.grid_sample(src, g64, align_corners=True, mode="bilinear", padding_mode="zeros")


def sample_grid(pm: torch.Tensor, src_hw, dsize) -> torch.Tensor:
    """The fp32 sample grid of ``kornia_warp.warp_perspective`` ([B, ho, wo, 2])."""
    ho, wo = dsize
    m = kornia_warp._torch_inverse_cast(kornia_warp.normalize_homography(pm, tuple(src_hw), (ho, wo)))
    grid = kornia_warp.create_meshgrid(ho, wo, True).to(torch.float32).repeat(pm.shape[0], 1, 1, 1)
    return kornia_warp.transform_points(m[:, None, None], grid)


def reference_order(feats, proj_mats, upsample_shape, grid_shape, w1, b1, w2, dtype=torch.float32, pattern=None):
    """``NoJointConvVariant.forward`` after the backbone, line by line (``:64-81``): interpolate, warp, cat with
    the coord map, conv 1x1, ReLU, conv 1x1, the same-size interpolate.  ``feats``: N tensors [B,C,h,w];
    ``w1`` [Cm, C N + 2, 1, 1], ``b1`` [Cm], ``w2`` [1, Cm, 1, 1] (autograd flows to all of them).
    ``pattern``: the ReLU decides by this 0/1 pattern (``helpers.masked_relu``).  Returns (map, pre)."""
    B = feats[0].shape[0]
    world = []
    for f, M in zip(feats, proj_mats):
        up = F.interpolate(f.to(dtype), list(upsample_shape), mode="bilinear")                # :64
        world.append(warp(up, M, grid_shape))                                                    # :67-68
    x = torch.cat(world + [coord_map(*grid_shape).to(dtype).repeat([B, 1, 1, 1])], dim=1)        # :76
    pre = F.conv2d(x, w1.to(dtype), b1.to(dtype))                                                # :80
    hid = F.relu(pre) if pattern is None else masked_relu(pre, pattern.to(pre.device))
    out = F.conv2d(hid, w2.to(dtype))
    return F.interpolate(out, list(grid_shape), mode="bilinear"), pre                            # :81


def img_head(feats, upsample_shape, params, dtype=torch.float32):
    """``img_classifier(F.interpolate(feat, upsample_shape))`` per view (``:64-65``)."""
    p = {k: torch.as_tensor(v).to(dtype) for k, v in params.items()}
    out = []
    for f in feats:
        up = F.interpolate(f.to(dtype), list(upsample_shape), mode="bilinear")
        h = F.relu(F.conv2d(up, p["img_classifier.0.weight"], p["img_classifier.0.bias"]))
        out.append(F.conv2d(h, p["img_classifier.2.weight"]))
    return out


def commuted_order(feats, proj_mats, upsample_shape, grid_shape, w1, b1, w2, dtype=torch.float32):
    """The order the native path evaluates: z_v = W_v feat_v at backbone resolution, then upsample, warp, the
    sum over views, bias and coord term, ReLU, the dot with w2.  Returns (map, pre)."""
    B, C = feats[0].shape[:2]
    N = len(feats)
    w1 = w1.to(dtype)
    acc = None
    for v, (f, M) in enumerate(zip(feats, proj_mats)):
        z = F.conv2d(f.to(dtype), w1[:, v * C:(v + 1) * C])
        t = warp(F.interpolate(z, list(upsample_shape), mode="bilinear"), M, grid_shape)
        acc = t if acc is None else acc + t
    coord = coord_map(*grid_shape).to(dtype).repeat([B, 1, 1, 1])
    pre = acc + F.conv2d(coord, w1[:, N * C:], b1.to(dtype))
    return F.conv2d(F.relu(pre), w2.to(dtype)), pre


def head_weight(cm: int, n: int, w_coord: torch.Tensor) -> torch.Tensor:
    """The first conv's weight under which ``reference_order`` on the ``z_v`` themselves is the op
    ``ProjectSumHead`` evaluates: N identity blocks and the coord columns, [Cm, Cm N + 2, 1, 1]."""
    eye = torch.eye(cm, dtype=w_coord.dtype)
    return torch.cat([eye] * n + [w_coord.reshape(cm, 2)], dim=1).reshape(cm, cm * n + 2, 1, 1)


def relu_flips(pattern: torch.Tensor, pre: torch.Tensor) -> None:
    """``test_gpu_backward.py``'s rule for an activation pattern taken from the GPU: it differs from ``pre > 0``
    in at most max(2, numel // 20000) places, each with |pre| <= 1e-4 max|pre|."""
    fin = torch.isfinite(pre)
    flip = (pattern.to(pre.device) > 0) != (pre > 0)
    flip &= fin
    assert int(flip.sum()) <= max(2, pre.numel() // 20000), int(flip.sum())
    assert (pre[flip].abs() <= 1e-4 * pre[fin].abs().max()).all(), pre[flip]


def ds_from_golden(g):
    """The dataset duck-type of the fixture's rig (its K, E, G and sizes)."""
    from mvdet_amd.synthetic import SyntheticBase, SyntheticFrameDataset
    m = g["meta"]
    base = SyntheticBase("fixture", m["img_shape"], m["worldgrid_shape"], m["num_cam"], g["G"], tuple(g["K"]),
                         tuple(g["E"]))
    return SyntheticFrameDataset(base, grid_reduce=m["grid_reduce"], img_reduce=m["img_reduce"])


_FIXTURE = {}


def fixture():
    """``variant_njc`` with its recipe's parameters and features regenerated (and checked against the stored
    sha256), once per session: dict(g, params, feats [B,N,512,h,w] fp32 tensor)."""
    if not _FIXTURE:
        from helpers import load_golden
        g = load_golden("variant_njc")
        m = g["meta"]
        params = njc_params(m["num_cam"], m["weight_seed"])
        assert params_sha256(params) == m["weights_sha256"], "the parameter recipe no longer gives the fixture's weights"
        feats = torch.from_numpy(feature_input((m["B"], m["num_cam"], 512, *m["backbone_hw"]), m["feature_seed"]))
        _FIXTURE.update(g=g, params={k: torch.from_numpy(v) for k, v in params.items()}, feats=feats)
    return _FIXTURE
