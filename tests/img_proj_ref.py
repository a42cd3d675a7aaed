"""Test-side reference of ``ImageProjVariant`` (``image_proj_variant.py``): the seeded recipe of the
``variant_img_proj`` fixture's parameters and BatchNorm statistics (15.9 M values: only the seeds and a sha256 are
stored), and the CPU restatement of the reference's ``forward`` in the REFERENCE'S ORDER, in two halves around the
backbone: the front (interpolate, warp, cat with the coord map: ``:64-88``) and the head (``map_classifier`` and the
closing interpolate: ``:91-92``).  Test infrastructure only.

Geometry is fp32 whatever the value dtype, as in ``variant_ref`` (whose ``warp``, ``coord_map``, ``relu_flips`` and
``ds_from_golden`` are used here)."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from helpers import masked_relu
from oracle.fixtures import feature_input, params_sha256  # noqa: F401  (re-exported for the tests)
from variant_ref import coord_map, ds_from_golden, relu_flips, warp  # noqa: F401

HEAD_KEYS = ("map_classifier.0.weight", "map_classifier.0.bias", "map_classifier.2.weight", "map_classifier.2.bias",
             "map_classifier.4.weight")


def _bn(prefix: str, c: int):
    return [(f"{prefix}.weight", (c,)), (f"{prefix}.bias", (c,)), (f"{prefix}.running_mean", (c,)),
            (f"{prefix}.running_var", (c,)), (f"{prefix}.num_batches_tracked", ())]


def _block(prefix: str, cin: int, cout: int, downsample: bool):
    out = [(f"{prefix}.conv1.weight", (cout, cin, 3, 3))] + _bn(f"{prefix}.bn1", cout)
    out += [(f"{prefix}.conv2.weight", (cout, cout, 3, 3))] + _bn(f"{prefix}.bn2", cout)
    if downsample:
        out += [(f"{prefix}.downsample.0.weight", (cout, cin, 1, 1))] + _bn(f"{prefix}.downsample.1", cout)
    return out


def param_shapes(num_cam: int, Cm: int = 512):
    """The ``state_dict`` of ``ImageProjVariant(arch='resnet18')`` in order (``image_proj_variant.py:44-56``,
    ``resnet.py``): the ResNet-18 trunk with ``3 * num_cam + 2`` input channels split at child 7 (a slice of an
    ``nn.Sequential`` keeps its children's indices), then ``map_classifier``.  125 entries."""
    out = [("base_pt1.0.weight", (64, 3 * num_cam + 2, 7, 7))] + _bn("base_pt1.1", 64)
    cin = 64
    for prefix, planes in (("base_pt1.4", 64), ("base_pt1.5", 128), ("base_pt1.6", 256), ("base_pt2.7", 512)):
        out += _block(f"{prefix}.0", cin, planes, cin != planes) + _block(f"{prefix}.1", planes, planes, False)
        cin = planes
    out += [("map_classifier.0.weight", (Cm, 512, 3, 3)), ("map_classifier.0.bias", (Cm,)),
            ("map_classifier.2.weight", (Cm, Cm, 3, 3)), ("map_classifier.2.bias", (Cm,)),
            ("map_classifier.4.weight", (1, Cm, 3, 3))]
    return OrderedDict(out)


def params(num_cam: int, seed: int, Cm: int = 512):
    """Every ``state_dict`` entry in order from PCG64(seed).  ``map_classifier``: uniform(+-1/sqrt(fan_in)), the
    existing recipes' scale.  The backbone's convs: uniform(+-sqrt(6/fan_in)) (He's bound: with 1/sqrt(fan_in)
    seventeen conv + ReLU layers without batch statistics shrink the world feature by orders of magnitude).
    BatchNorm: weight uniform [0.5, 1.5], bias and running mean uniform +-0.1, running variance uniform
    [0.5, 1.5], ``num_batches_tracked`` 0 (int64)."""
    shapes = param_shapes(num_cam, Cm)
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for name, shp in shapes.items():
        leaf = name.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            out[name] = np.zeros(shp, dtype=np.int64)
        elif len(shp) == 4 or name in HEAD_KEYS:  # a conv's weight or bias
            fan_in = int(np.prod(shapes[name.replace(".bias", ".weight")][1:]))
            b = 1.0 / np.sqrt(fan_in) if name in HEAD_KEYS else np.sqrt(6.0 / fan_in)
            out[name] = rng.uniform(-b, b, size=shp).astype(np.float32)
        elif leaf in ("weight", "running_var"):
            out[name] = rng.uniform(0.5, 1.5, size=shp).astype(np.float32)
        else:  # a BatchNorm bias or running mean
            out[name] = rng.uniform(-0.1, 0.1, size=shp).astype(np.float32)
    return out


def front(imgs, proj_mats, upsample_shape, grid_shape, dtype=torch.float32):
    """``forward`` up to the backbone, line by line (``:64-88``): per camera the bilinear interpolate of the image
    to ``upsample_shape`` and its warp, then the cat with the coord map.  ``imgs`` [B,N,3,H,W]."""
    B = imgs.shape[0]
    projected = []
    for cam, M in enumerate(proj_mats):
        img_res = F.interpolate(imgs[:, cam].to(dtype), list(upsample_shape), mode="bilinear")      # :67
        projected.append(warp(img_res, M, grid_shape))                                               # :68-69
    return torch.cat(projected + [coord_map(*grid_shape).to(dtype).repeat([B, 1, 1, 1])], dim=1)    # :88


def head(world_feature, p, grid_shape, dtype=torch.float32, patterns=(None, None)):
    """``forward`` after the backbone (``:91-92``): the three convs of ``map_classifier`` (``:53-56``) and the
    bilinear interpolate to the grid.  ``p``: the parameters by ``state_dict`` name (autograd flows to them and to
    ``world_feature``).  ``patterns``: the two ReLUs decide by these 0/1 patterns (``helpers.masked_relu``; None:
    ``F.relu``).  Returns (map_result, (pre1, pre2))."""
    q = {k: p[k].to(dtype) for k in HEAD_KEYS}

    def relu(pre, pattern):
        return F.relu(pre) if pattern is None else masked_relu(pre, pattern.to(pre.device))

    pre1 = F.conv2d(world_feature.to(dtype), q["map_classifier.0.weight"], q["map_classifier.0.bias"], padding=1)
    y1 = relu(pre1, patterns[0])
    pre2 = F.conv2d(y1, q["map_classifier.2.weight"], q["map_classifier.2.bias"], padding=2, dilation=2)
    y2 = relu(pre2, patterns[1])
    out = F.conv2d(y2, q["map_classifier.4.weight"], padding=4, dilation=4)
    return F.interpolate(out, list(grid_shape), mode="bilinear"), (pre1, pre2)                      # :92


_FIXTURE = {}


def fixture():
    """``variant_img_proj`` with its recipe's parameters and images regenerated (and checked against the stored
    sha256), once per session: dict(g, params (torch tensors by ``state_dict`` name), imgs [B,N,3,H,W] fp32)."""
    if not _FIXTURE:
        from helpers import load_golden
        g = load_golden("variant_img_proj")
        m = g["meta"]
        ps = params(m["num_cam"], m["weight_seed"])
        assert params_sha256(ps) == m["weights_sha256"], "the parameter recipe no longer gives the fixture's weights"
        imgs = torch.from_numpy(feature_input((m["B"], m["num_cam"], 3, *m["input_hw"]), m["image_seed"]))
        _FIXTURE.update(g=g, params={k: torch.from_numpy(v) for k, v in ps.items()}, imgs=imgs)
    return _FIXTURE
