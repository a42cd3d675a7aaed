"""Generate ``tests/golden/variant_img_proj.npz`` from the reference's own ``ImageProjVariant``.

Runs ONLY where the reference checkout is present (``ref_harness.REF_ROOT``).  The reference class is imported
through ``tools/ref_harness.py`` (kornia stubbed with the oracle restatement, ``cuda:0`` redirected to CPU, ``cv2``
stubbed) and runs WHOLE, its ground-plane ResNet-18 included, in ``eval()``: all 15.9 M parameters and the BatchNorm
running statistics come from the seeded recipe in ``tests/img_proj_ref.py`` (the fixture stores the recipe's seeds
and a sha256 instead).  The matrix chain, the coord map, the image resize (``image_proj_variant.py:67``), the warp
(``:69``), the concat (``:88``), the backbone (``:89-90``), the three convs (``:53-56,91``) and the final
interpolate (``:92``) are the reference's own code.

The rig is ``tools/gen_golden_variant.py``'s with ``grid_reduce=1``, as the reference's own ``test()`` uses: 3
cameras, grid 40 x 56, ``upsample_shape`` 24 x 32, world feature 5 x 7 (dilation 4 exceeds its height, W % 4 != 0),
B = 2; the input images are 64 x 86, so the resize ratios (2.667 and 2.6875) are no integers.  It must discriminate:
every view's share of grid pixels sampled inside its resized image lies in [5 %, 95 %], and no warped plane is
constant.

Stored: ``projected_imgs`` (the input of ``base_pt1``, captured by a forward pre-hook), ``world_feature`` (the output
of ``base_pt2``), ``map_result``, the geometry and ``meta``.

Usage:  python tools/gen_golden_img_proj.py
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

from ref_harness import load_reference_image_proj_variant  # noqa: E402
import img_proj_ref  # noqa: E402
import gen_golden_variant as gv  # noqa: E402
from mvdet_amd import synthetic  # noqa: E402

WSEED, ISEED, B, INPUT_HW = 321, 322, 2, (64, 86)


def make_dataset():
    ds = gv.make_dataset()
    return synthetic.SyntheticFrameDataset(ds.base, grid_reduce=1, img_reduce=ds.img_reduce)


def main():
    ds = make_dataset()
    Ref = load_reference_image_proj_variant()
    torch.manual_seed(0)
    model = Ref(ds)
    sd_shapes = {k: list(v.shape) for k, v in model.state_dict().items()}
    params = img_proj_ref.params(ds.num_cam, WSEED)
    sd = model.state_dict()
    assert list(sd) == list(params), "the recipe's names are not the reference's state_dict"
    for k, v in params.items():
        assert tuple(sd[k].shape) == v.shape, (k, tuple(sd[k].shape), v.shape)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    model.eval()
    up_hw, grid_hw = tuple(model.upsample_shape), tuple(model.reducedgrid_shape)
    share = gv.inside_share(model.proj_mats, up_hw, grid_hw)
    assert all(0.05 <= s <= 0.95 for s in share), f"the rig does not discriminate: inside shares {share}"
    imgs = torch.from_numpy(img_proj_ref.feature_input((B, ds.num_cam, 3, *INPUT_HW), ISEED))
    seen = {}
    h1 = model.base_pt1.register_forward_pre_hook(lambda mod, args: seen.__setitem__("projected_imgs", args[0].clone()))
    h2 = model.base_pt2.register_forward_hook(lambda mod, args, out: seen.__setitem__("world_feature", out.clone()))
    with torch.no_grad():
        map_res, imgs_res = model(imgs)
    h1.remove()
    h2.remove()
    proj, world = seen["projected_imgs"], seen["world_feature"]
    planes = proj[:, :3 * ds.num_cam]
    spread = [float(planes[:, c].max() - planes[:, c].min()) for c in range(3 * ds.num_cam)]
    assert all(s > 0 for s in spread), f"a warped plane is constant: {spread}"
    assert all(float(r.abs().max()) == 0 for r in imgs_res)
    # the restatement is the reference, bit for bit
    assert torch.equal(img_proj_ref.front(imgs, model.proj_mats, up_hw, grid_hw), proj)
    tp = {k: torch.from_numpy(v) for k, v in params.items()}
    with torch.no_grad():
        assert torch.equal(img_proj_ref.head(world, tp, grid_hw)[0], map_res)
    b = ds.base
    meta = dict(num_cam=ds.num_cam, img_shape=list(ds.img_shape), worldgrid_shape=list(ds.worldgrid_shape),
                grid_reduce=ds.grid_reduce, img_reduce=ds.img_reduce, reducedgrid_shape=ds.reducedgrid_shape,
                upsample_shape=ds.upsample_shape, rig=b.name, B=B, input_hw=list(INPUT_HW),
                world_feature_hw=list(world.shape[2:]), weight_seed=WSEED, image_seed=ISEED,
                weights_sha256=img_proj_ref.params_sha256(params), state_dict_shapes=sd_shapes,
                imgs_result_shape=[len(imgs_res)] + list(imgs_res[0].shape), inside_share=share, plane_spread=spread)
    gv.OUT.mkdir(parents=True, exist_ok=True)
    out = gv.OUT / "variant_img_proj.npz"
    np.savez_compressed(out, meta=np.array(json.dumps(meta)),
                        proj_mats=np.stack([m.numpy() for m in model.proj_mats]), coord_map=model.coord_map.numpy(),
                        projected_imgs=proj.numpy(), world_feature=world.numpy(), map_result=map_res.numpy(),
                        K=np.stack(b.intrinsic_matrices), E=np.stack(b.extrinsic_matrices),
                        G=np.asarray(b.worldgrid2worldcoord_mat, np.float64))
    assert out.stat().st_size < (1 << 20), out.stat().st_size
    print("variant_img_proj", tuple(map_res.shape), "bytes", out.stat().st_size, "inside shares",
          [round(s, 3) for s in share], "spread", [round(s, 2) for s in spread], "world max",
          float(world.abs().max()), "world zero share", float((world == 0).float().mean()), "map max",
          float(map_res.abs().max()))


if __name__ == "__main__":
    main()
