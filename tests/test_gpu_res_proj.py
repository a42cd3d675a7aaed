"""``ResProjVariant`` on the GPU on the ``variant_res_proj`` fixture's rig (identity backbone halves, the recipe's
parameters): inference against what the reference class itself produced, and one training step against fp64 CPU
autograd of the reference-order restatement (``res_proj_ref``), gate 5e-5 normwise with ``test_gpu_backward.py``'s
ReLU flip rule on the GPU's own y1 / y2 activation patterns."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import res_proj_ref as rr
from helpers import assert_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5


def _model():
    from mvdet_amd import ResProjVariant
    fx = rr.fixture()
    model = ResProjVariant(rr.ds_from_golden(fx["g"]), device=DEV)
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
    """The loss uses ``map_result`` and every ``imgs_result``: autograd adds the foot plane's gradient from the
    ground-plane head to the loss's own gradient of ``imgs_result`` before the image head's backward."""
    from mvdet_amd import ops
    fx, model = _model()
    model.train()
    g, m = fx["g"], fx["g"]["meta"]
    N = m["num_cam"]
    x = fx["feats"].to(DEV).requires_grad_()
    map_res, imgs_res = model(x)
    fn = map_res.grad_fn
    assert type(fn).__name__.startswith("ThinFuseFunction")
    assert_parity(map_res.detach().cpu(), g["map_result"], "training-mode forward vs golden", normwise_tol=TOL)
    for v, r in enumerate(imgs_res):
        assert_parity(r.detach().cpu(), g["imgs_result"][v], f"training-mode imgs_result {v}", normwise_tol=TOL)
    # the activation patterns the GPU used: the saved y1 (split-bf16) and y2 of this very forward
    y1 = ops.split_decode(fn.ws.y1, 512) if fn.ws.y1.dtype == torch.bfloat16 else fn.ws.y1
    patterns = ((y1 > 0).double().cpu(), (fn.ws.y2 > 0).double().cpu())
    rng = np.random.default_rng(0)
    gmap = torch.from_numpy(rng.standard_normal(map_res.shape).astype(np.float32))
    gimgs = [torch.from_numpy(rng.standard_normal(r.shape).astype(np.float32)) * 0.05 for r in imgs_res]
    loss = (map_res * gmap.to(DEV)).sum() + sum((r * gi.to(DEV)).sum() for r, gi in zip(imgs_res, gimgs))
    loss.backward()
    torch.cuda.synchronize()
    # a second backward through a released graph raises, as ProjectFuseFunction's does
    c1, c2, c3 = model.map_classifier[0], model.map_classifier[2], model.map_classifier[4]
    again = model.head([r.detach()[:, 1:2] for r in imgs_res], c1.weight, c1.bias, c2.weight, c2.bias, c3.weight)
    grads = torch.autograd.grad(again.sum(), [c3.weight], retain_graph=True)
    assert torch.isfinite(grads[0]).all()
    with pytest.raises(RuntimeError, match="second time"):
        torch.autograd.grad(again.sum(), [c3.weight])

    feats = [fx["feats"][:, v] for v in range(N)]
    args = (list(g["proj_mats"]), m["upsample_shape"], m["reducedgrid_shape"])

    def ref(pats):
        fr = [f.double().requires_grad_() for f in feats]
        p = {k: v.double().requires_grad_() for k, v in fx["params"].items()}
        out, imgs, pre = rr.reference_order(fr, *args, p, dtype=torch.float64, patterns=pats)
        (out * gmap.double()).sum().add(sum((r * gi.double()).sum() for r, gi in zip(imgs, gimgs))).backward()
        return [t.detach() for t in pre], [f.grad for f in fr], {k: v.grad for k, v in p.items()}

    pre, _, _ = ref((None, None))
    for pat, pr in zip(patterns, pre):
        rr.relu_flips(pat, pr)
    _, gfeat, gpar = ref(patterns)
    for v in range(N):
        assert_parity(x.grad[:, v].cpu(), gfeat[v], f"d features view {v}", normwise_tol=TOL)
    for k, r in gpar.items():
        assert_parity(model.get_parameter(k).grad.cpu(), r, f"d {k}", normwise_tol=TOL)


def test_inference_allocates_nothing_of_y1_size_on_the_second_call():
    """The first call builds the engine's cached workspace (y1, conv3's partials, conv2's transform); the second
    allocates nothing of [B,512,Ho,Wo] size beyond it."""
    fx, model = _model()
    model.eval()
    x = fx["feats"].to(DEV)
    B, (Ho, Wo) = x.shape[0], fx["g"]["meta"]["reducedgrid_shape"]
    with torch.no_grad():
        first, imgs = model(x)
        planes = [r[:, 1:2] for r in imgs]
        c1, c2, c3 = model.map_classifier[0], model.map_classifier[2], model.map_classifier[4]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = model.head(planes, c1.weight, c1.bias, c2.weight, c2.bias, c3.weight)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    assert peak < B * 512 * Ho * Wo * 4 // 4, (peak, B * 512 * Ho * Wo * 4)
    assert torch.equal(out, first)
