"""Test-side reference of ``ResProjVariant`` (``res_proj_variant.py``): the seeded recipe of the
``variant_res_proj`` fixture's parameters and features, and the CPU restatement of the reference's ``forward``
after the backbone in the REFERENCE'S ORDER.  Test infrastructure only.

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


def param_shapes(num_cam: int, C: int = 512, Cm: int = 512):
    """``img_classifier`` / ``map_classifier`` of ``res_proj_variant.py:51-56`` in ``state_dict`` order."""
    return OrderedDict([
        ("img_classifier.0.weight", (64, C, 1, 1)),
        ("img_classifier.0.bias", (64,)),
        ("img_classifier.2.weight", (2, 64, 1, 1)),
        ("map_classifier.0.weight", (Cm, num_cam + 2, 3, 3)),
        ("map_classifier.0.bias", (Cm,)),
        ("map_classifier.2.weight", (Cm, Cm, 3, 3)),
        ("map_classifier.2.bias", (Cm,)),
        ("map_classifier.4.weight", (1, Cm, 3, 3)),
    ])


def params(num_cam: int, seed: int, C: int = 512, Cm: int = 512):
    """uniform(+-1/sqrt(fan_in)) per parameter (PyTorch's Conv2d bound) in ``state_dict`` order from PCG64(seed)."""
    shapes = param_shapes(num_cam, C, Cm)
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for name, shp in shapes.items():
        fan_in = int(np.prod(shapes[name.replace(".bias", ".weight")][1:]))
        b = 1.0 / np.sqrt(fan_in)
        out[name] = rng.uniform(-b, b, size=shp).astype(np.float32)
    return out


def reference_order(feats, proj_mats, upsample_shape, grid_shape, p, dtype=torch.float32, patterns=(None, None)):
    """``ResProjVariant.forward`` after the backbone, line by line (``:67-83``): interpolate, ``img_classifier``,
    the warp of the foot channel, cat with the coord map, the three convs of ``map_classifier``, the same-size
    interpolate.  ``feats``: N tensors [B,C,h,w]; ``p``: the parameters by ``state_dict`` name (autograd flows to
    them and to ``feats``).  ``patterns``: the two ReLUs of ``map_classifier`` decide by these 0/1 patterns
    (``helpers.masked_relu``; None: ``F.relu``).  Returns (map_result, imgs_result, (pre1, pre2))."""
    q = {k: v.to(dtype) for k, v in p.items()}
    B = feats[0].shape[0]
    world, imgs_result = [], []
    for f, M in zip(feats, proj_mats):
        up = F.interpolate(f.to(dtype), list(upsample_shape), mode="bilinear")                    # :67
        h = F.relu(F.conv2d(up, q["img_classifier.0.weight"], q["img_classifier.0.bias"]))         # :68
        res = F.conv2d(h, q["img_classifier.2.weight"])
        imgs_result.append(res)                                                                      # :69
        world.append(warp(res[:, 1].unsqueeze(1), M, grid_shape))                                    # :70-73
    x = torch.cat(world + [coord_map(*grid_shape).to(dtype).repeat([B, 1, 1, 1])], dim=1)           # :81

    def relu(pre, pattern):
        return F.relu(pre) if pattern is None else masked_relu(pre, pattern.to(pre.device))

    pre1 = F.conv2d(x, q["map_classifier.0.weight"], q["map_classifier.0.bias"], padding=1)         # :82 (:53-56)
    y1 = relu(pre1, patterns[0])
    pre2 = F.conv2d(y1, q["map_classifier.2.weight"], q["map_classifier.2.bias"], padding=2, dilation=2)
    y2 = relu(pre2, patterns[1])
    out = F.conv2d(y2, q["map_classifier.4.weight"], padding=4, dilation=4)
    return F.interpolate(out, list(grid_shape), mode="bilinear"), imgs_result, (pre1, pre2)       # :83


_FIXTURE = {}


def fixture():
    """``variant_res_proj`` with its recipe's parameters and features regenerated (and checked against the stored
    sha256), once per session: dict(g, params, feats [B,N,512,h,w] fp32 tensor)."""
    if not _FIXTURE:
        from helpers import load_golden
        g = load_golden("variant_res_proj")
        m = g["meta"]
        ps = params(m["num_cam"], m["weight_seed"])
        assert params_sha256(ps) == m["weights_sha256"], "the parameter recipe no longer gives the fixture's weights"
        feats = torch.from_numpy(feature_input((m["B"], m["num_cam"], 512, *m["backbone_hw"]), m["feature_seed"]))
        _FIXTURE.update(g=g, params={k: torch.from_numpy(v) for k, v in ps.items()}, feats=feats)
    return _FIXTURE
