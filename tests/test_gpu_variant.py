"""``NoJointConvVariant`` on the GPU on the ``variant_njc`` fixture's rig (identity backbone halves, the
recipe's parameters): inference against what the reference class itself produced, and one training step
against fp64 CPU autograd of the reference-order restatement (``variant_ref``), gate 5e-5 normwise with
``test_gpu_backward.py``'s ReLU flip rule."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import variant_ref as vr
from helpers import assert_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5


def _model():
    from mvdet_amd import NoJointConvVariant
    fx = vr.fixture()
    model = NoJointConvVariant(vr.ds_from_golden(fx["g"]), device=DEV)
    sd = model.state_dict()
    sd.update(fx["params"])
    model.load_state_dict(sd)
    model.base_pt1, model.base_pt2 = nn.Identity(), nn.Identity()
    return fx, model


def test_inference_matches_the_reference_golden():
    fx, model = _model()
    model.eval()
    with torch.no_grad():
        map_res, imgs_res = model(fx["feats"].to(DEV))
    g = fx["g"]
    assert map_res.grad_fn is None and tuple(map_res.shape) == g["map_result"].shape
    assert_parity(map_res.cpu(), g["map_result"], "map_result vs the reference's", normwise_tol=TOL)
    assert len(imgs_res) == g["meta"]["num_cam"]
    for v, r in enumerate(imgs_res):
        assert_parity(r.cpu(), g["imgs_result"][v], f"imgs_result {v} vs the reference's", normwise_tol=TOL)


def test_training_step_matches_fp64_autograd():
    fx, model = _model()
    model.train()
    g, m = fx["g"], fx["g"]["meta"]
    N = m["num_cam"]
    x = fx["feats"].to(DEV).requires_grad_()
    # the activation pattern the GPU used: the head's own hidden output, from the same z as the forward
    seen = {}
    real = model.head

    def spy(zs, bias, w_coord, w2):
        out, hidden = real(zs, bias, w_coord, w2, return_hidden=True)
        seen["hidden"] = hidden.detach().cpu()
        return out

    model.head = spy
    map_res, imgs_res = model(x)
    assert type(map_res.grad_fn).__name__.startswith("WarpSumHead")
    assert_parity(map_res.detach().cpu(), g["map_result"], "training-mode forward vs golden", normwise_tol=TOL)
    rng = np.random.default_rng(0)
    gmap = torch.from_numpy(rng.standard_normal(map_res.shape).astype(np.float32))
    (map_res * gmap.to(DEV)).sum().backward()
    torch.cuda.synchronize()

    p = fx["params"]
    feats = [fx["feats"][:, v] for v in range(N)]
    args = (list(g["proj_mats"]), m["upsample_shape"], m["reducedgrid_shape"])

    def ref(pattern):
        fr = [f.double().requires_grad_() for f in feats]
        w1, b1, w2 = (p[k].double().requires_grad_() for k in
                      ("map_classifier.0.weight", "map_classifier.0.bias", "map_classifier.2.weight"))
        out, pre = vr.reference_order(fr, *args, w1, b1, w2, dtype=torch.float64, pattern=pattern)
        out.backward(gmap.double())
        return pre.detach(), [f.grad for f in fr], {"0.weight": w1.grad, "0.bias": b1.grad, "2.weight": w2.grad}

    pre, _, _ = ref(None)
    pattern = (seen["hidden"] > 0).double()
    vr.relu_flips(pattern, pre)
    _, gfeat, gpar = ref(pattern)
    for v in range(N):
        assert_parity(x.grad[:, v].cpu(), gfeat[v], f"d features view {v}", normwise_tol=TOL)
    for k, r in gpar.items():
        assert_parity(model.map_classifier.get_parameter(k).grad.cpu(), r, f"d map_classifier.{k}", normwise_tol=TOL)
