"""Generate ``tests/golden/variant_res_proj.npz`` from the reference's own ``ResProjVariant``.

Runs ONLY where the reference checkout is present (``ref_harness.REF_ROOT``).  The reference class is imported
through ``tools/ref_harness.py`` (kornia stubbed with the oracle restatement, ``cuda:0`` redirected to CPU), its backbone
halves are replaced by ``nn.Identity`` so that ``forward`` receives backbone-resolution features, and its
classifier weights come from the seeded recipe in ``tests/res_proj_ref.py`` (they are about 9 MB: the fixture
stores the recipe's seeds and a sha256 instead).  Everything downstream — the matrix chain, the coord map, the
upsample (``res_proj_variant.py:67``), the image head (``:68``), the warp of its foot channel (``:72``), the concat
(``:81``), the three convs (``:53-56,82``) and the final interpolate (``:83``) — is the reference's own code.

The rig is ``tools/gen_golden_variant.py``'s (3 cameras, image 96 x 128 -> upsampled 24 x 32, backbone maps 8 x 11,
grid 10 x 14, B = 2) and must discriminate: every view's share of grid pixels sampled inside its source lies in
[5 %, 95 %], and no view's warped foot plane is constant.

Usage:  python tools/gen_golden_res_proj.py
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

from ref_harness import load_reference_res_proj_variant  # noqa: E402
import res_proj_ref  # noqa: E402
from gen_golden_variant import BACKBONE_HW, B, OUT, inside_share, make_dataset  # noqa: E402

WSEED, FSEED = 311, 312


def main():
    ds = make_dataset()
    Ref = load_reference_res_proj_variant()
    torch.manual_seed(0)
    model = Ref(ds)
    sd_shapes = {k: list(v.shape) for k, v in model.state_dict().items()}
    model.base_pt1, model.base_pt2 = nn.Identity(), nn.Identity()
    params = res_proj_ref.params(ds.num_cam, WSEED)
    sd = model.state_dict()
    for k, v in params.items():
        assert tuple(sd[k].shape) == v.shape, (k, tuple(sd[k].shape), v.shape)
        sd[k] = torch.from_numpy(v)
    model.load_state_dict(sd)
    model.eval()
    up_hw, grid_hw = tuple(model.upsample_shape), tuple(model.reducedgrid_shape)
    share = inside_share(model.proj_mats, up_hw, grid_hw)
    assert all(0.05 <= s <= 0.95 for s in share), f"the rig does not discriminate: inside shares {share}"
    feats = res_proj_ref.feature_input((B, ds.num_cam, 512, *BACKBONE_HW), FSEED)
    with torch.no_grad():
        map_res, imgs_res = model(torch.from_numpy(feats))
    spread = []
    for r, M in zip(imgs_res, model.proj_mats):
        wf = res_proj_ref.warp(r[:, 1].unsqueeze(1), M, grid_hw)
        spread.append(float(wf.max() - wf.min()))
    assert all(s > 0 for s in spread), f"a warped foot plane is constant: {spread}"
    b = ds.base
    meta = dict(num_cam=ds.num_cam, img_shape=list(ds.img_shape), worldgrid_shape=list(ds.worldgrid_shape),
                grid_reduce=ds.grid_reduce, img_reduce=ds.img_reduce, reducedgrid_shape=ds.reducedgrid_shape,
                upsample_shape=ds.upsample_shape, rig=b.name, B=B, backbone_hw=list(BACKBONE_HW), weight_seed=WSEED,
                feature_seed=FSEED, weights_sha256=res_proj_ref.params_sha256(params), state_dict_shapes=sd_shapes,
                inside_share=share, foot_spread=spread)
    OUT.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT / "variant_res_proj.npz", meta=np.array(json.dumps(meta)),
                        proj_mats=np.stack([m.numpy() for m in model.proj_mats]), coord_map=model.coord_map.numpy(),
                        map_result=map_res.numpy(), imgs_result=torch.stack(imgs_res, 0).numpy(),
                        K=np.stack(b.intrinsic_matrices), E=np.stack(b.extrinsic_matrices),
                        G=np.asarray(b.worldgrid2worldcoord_mat, np.float64))
    print("variant_res_proj", tuple(map_res.shape), "inside shares", [round(s, 3) for s in share], "foot spread",
          [round(s, 4) for s in spread], "map max", float(map_res.abs().max()))


if __name__ == "__main__":
    main()
