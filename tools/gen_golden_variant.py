"""Generate ``tests/golden/variant_njc.npz`` from the reference's own ``NoJointConvVariant``.

Runs ONLY in the build container (needs ``/root/reference``).  The reference class is imported through
``tools/ref_harness.py`` (kornia stubbed with the oracle restatement, ``cuda:0`` redirected to CPU), its
backbone halves are replaced by ``nn.Identity`` so that ``forward`` receives backbone-resolution features, and
its classifier weights come from the seeded recipe in ``tests/variant_ref.py`` (they are about 3 MB: the
fixture stores the recipe's seeds and a sha256 instead).  Everything downstream — the matrix chain, the coord
map, the upsample (``no_joint_conv_variant.py:64``), the warp (``:68``), the concat (``:76``), the two 1x1 convs
(``:51-53,80``) and the final interpolate (``:81``) — is the reference's own code.

The rig is small (3 cameras, image 96 x 128 -> upsampled 24 x 32, backbone maps 8 x 11, grid 10 x 14, B = 2)
and must discriminate: every view's share of grid pixels sampled inside its source lies in [5 %, 95 %].

Usage:  python tools/gen_golden_variant.py
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

from ref_harness import load_reference_no_joint_conv_variant  # noqa: E402
import variant_ref  # noqa: E402
from mvdet_amd import synthetic  # noqa: E402

OUT = ROOT / "tests" / "golden"
# 20 cm cells: a 8 m x 11.2 m ground area seen from 2.5 m (Wildtrack's 2.5 cm cells would put the whole 40 x 56
# grid inside every view)
RIG = dict(num_cam=3, grid_reduce=4, seed=21, img_shape=(96, 128), worldgrid_shape=(40, 56), cell=20.0, height=250.0)
B, BACKBONE_HW, WSEED, FSEED = 2, (8, 11), 301, 302


def make_dataset():
    rows, cols = RIG["worldgrid_shape"]
    cell = RIG["cell"]
    G = np.array([[cell, 0, -cell * rows / 2], [0, cell, -cell * cols / 2], [0, 0, 1]], dtype=np.float64)
    base = synthetic.make_rig("Variant-synthetic", RIG["img_shape"], RIG["worldgrid_shape"], RIG["num_cam"], G,
                              height=RIG["height"], seed=RIG["seed"])
    return synthetic.SyntheticFrameDataset(base, grid_reduce=RIG["grid_reduce"], img_reduce=4)


def inside_share(proj_mats, up_hw, grid_hw):
    """Per view, the share of grid pixels whose kornia sample lands inside the source (fp32 coordinates)."""
    out = []
    for M in proj_mats:
        g = variant_ref.sample_grid(torch.as_tensor(np.asarray(M)).reshape(1, 3, 3).float(), up_hw, grid_hw)[0]
        ix, iy = (g[..., 0] + 1) / 2 * (up_hw[1] - 1), (g[..., 1] + 1) / 2 * (up_hw[0] - 1)
        inside = (ix > -1) & (ix < up_hw[1]) & (iy > -1) & (iy < up_hw[0])
        out.append(float(inside.float().mean()))
    return out


def main():
    ds = make_dataset()
    Ref = load_reference_no_joint_conv_variant()
    torch.manual_seed(0)
    model = Ref(ds)
    sd_shapes = {k: list(v.shape) for k, v in model.state_dict().items()}
    model.base_pt1, model.base_pt2 = nn.Identity(), nn.Identity()
    params = variant_ref.njc_params(ds.num_cam, WSEED)
    sd = model.state_dict()
    for k, v in params.items():
        assert tuple(sd[k].shape) == v.shape, (k, tuple(sd[k].shape), v.shape)
        sd[k] = torch.from_numpy(v)
    model.load_state_dict(sd)
    model.eval()
    share = inside_share(model.proj_mats, tuple(model.upsample_shape), tuple(model.reducedgrid_shape))
    assert all(0.05 <= s <= 0.95 for s in share), f"the rig does not discriminate: inside shares {share}"
    feats = variant_ref.feature_input((B, ds.num_cam, 512, *BACKBONE_HW), FSEED)
    with torch.no_grad():
        map_res, imgs_res = model(torch.from_numpy(feats))
    b = ds.base
    meta = dict(num_cam=ds.num_cam, img_shape=list(ds.img_shape), worldgrid_shape=list(ds.worldgrid_shape),
                grid_reduce=ds.grid_reduce, img_reduce=ds.img_reduce, reducedgrid_shape=ds.reducedgrid_shape,
                upsample_shape=ds.upsample_shape, rig=b.name, B=B, backbone_hw=list(BACKBONE_HW), weight_seed=WSEED,
                feature_seed=FSEED, weights_sha256=variant_ref.params_sha256(params), state_dict_shapes=sd_shapes,
                inside_share=share)
    OUT.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT / "variant_njc.npz", meta=np.array(json.dumps(meta)),
                        proj_mats=np.stack([m.numpy() for m in model.proj_mats]), coord_map=model.coord_map.numpy(),
                        map_result=map_res.numpy(), imgs_result=torch.stack(imgs_res, 0).numpy(),
                        K=np.stack(b.intrinsic_matrices), E=np.stack(b.extrinsic_matrices),
                        G=np.asarray(b.worldgrid2worldcoord_mat, np.float64))
    print("variant_njc", tuple(map_res.shape), "inside shares", [round(s, 3) for s in share], "map max",
          float(map_res.abs().max()))


if __name__ == "__main__":
    main()
