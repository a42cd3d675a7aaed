"""``mvdet_amd.warp_perspective`` under autograd: the kornia call-site swap of INTEGRATION.md §2 trains.

The forward is the kernel of the no-grad call, bit for bit; the gradient of ``src`` is the deterministic plan gather,
gated as ``test_gpu_backward.py`` gates the warp adjoints: 4 x the CPU fp32 reference's own floor, on the cases and
inputs of its ``_ATOMIC_FLOOR``, against ``oracle.kornia_warp.warp_perspective``'s CPU autograd.  What has no
gradient raises instead of dropping it."""
import sys
import types

import pytest
import torch

import backward_cases as bc
from oracle import kornia_warp
from test_gpu_backward import _ATOMIC_FLOOR, _adjoint_gate, _adjoint_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("B,C,H,W,ho,wo", list(_ATOMIC_FLOOR))
def test_gradient_vs_grid_sample_autograd(B, C, H, W, ho, wo):
    from mvdet_amd import ops, warp_perspective
    gate = _adjoint_gate(_ATOMIC_FLOOR[B, C, H, W, ho, wo])
    Ms, gouts, _ = _adjoint_inputs(100 * B + C, 3, B, C, H, W, ho, wo)
    g = torch.Generator().manual_seed(B + C)
    srcs = [torch.randn((B, C, H, W), generator=g) for _ in Ms]
    grads = []
    for i, (M, go, s) in enumerate(zip(Ms, gouts, srcs)):
        ref = s.clone().requires_grad_()
        kornia_warp.warp_perspective(ref, M.repeat(B, 1, 1), (ho, wo)).backward(go)
        x = s.to(DEV).requires_grad_()
        Md = M.repeat(B, 1, 1).to(DEV)
        out = warp_perspective(x, Md, (ho, wo))
        assert out.grad_fn is not None
        with torch.no_grad():
            assert torch.equal(out.detach(), warp_perspective(x, Md, (ho, wo)))  # the same kernel, the same bits
        out.backward(go.to(DEV))
        bc.assert_gated(x.grad.cpu(), ref.grad, f"warp_perspective gradient, view {i}", gate)
        grads.append(x.grad)
    if B == 2:
        # two different matrices in one batch: each item's gradient is its own matrix's, bit for bit, and a second
        # backward with the same matrices builds no new plan
        ops._WARP_PLAN_CACHE.clear()
        M2 = torch.cat([Ms[0], Ms[1]]).to(DEV)
        go2 = torch.stack([gouts[0][0], gouts[1][1]]).to(DEV)
        for _ in range(2):
            x = torch.stack([srcs[0][0], srcs[1][1]]).to(DEV).requires_grad_()
            warp_perspective(x, M2, (ho, wo)).backward(go2)
            assert torch.equal(x.grad[0], grads[0][0]) and torch.equal(x.grad[1], grads[1][1])
            assert len(ops._WARP_PLAN_CACHE) == 2


def test_what_has_no_gradient_raises():
    from mvdet_amd import warp_perspective
    src = torch.zeros((1, 2, 9, 11), device=DEV)
    M = torch.eye(3, device=DEV)[None]
    with pytest.raises(NotImplementedError, match="no gradient with respect to the homography"):
        warp_perspective(src, M.clone().requires_grad_(), (5, 6))
    with pytest.raises(NotImplementedError, match="float32 src"):
        warp_perspective(src.half().requires_grad_(), M, (5, 6))
    with pytest.raises(RuntimeError, match="out=... arguments don't support automatic differentiation"):
        warp_perspective(src.clone().requires_grad_(), M, (5, 6), out=torch.empty((1, 2, 5, 6), device=DEV))
    with torch.no_grad():  # without grad mode nothing changes: these calls run
        assert warp_perspective(src.clone().requires_grad_(), M.clone().requires_grad_(), (5, 6)).grad_fn is None
        out = torch.empty((1, 2, 5, 6), device=DEV)
        assert warp_perspective(src.clone().requires_grad_(), M, (5, 6), out=out) is out
    for kw in (dict(mode="nearest"), dict(padding_mode="border"), dict(align_corners=False)):
        with pytest.raises(NotImplementedError, match="only mode='bilinear'"):
            warp_perspective(src.clone().requires_grad_(), M, (5, 6), **kw)


def test_the_kornia_swap_trains(monkeypatch):
    """INTEGRATION.md §2's two-line swap on a stub that calls kornia as ``persp_trans_detector.py:69`` does: the
    map loss reaches the source maps."""
    import mvdet_amd
    kornia = types.ModuleType("kornia")
    kornia.geometry = types.ModuleType("kornia.geometry")
    kornia.geometry.transform = types.ModuleType("kornia.geometry.transform")
    for name, mod in (("kornia", kornia), ("kornia.geometry", kornia.geometry),
                      ("kornia.geometry.transform", kornia.geometry.transform)):
        monkeypatch.setitem(sys.modules, name, mod)
    kornia.geometry.transform.warp_perspective = mvdet_amd.warp_perspective
    kornia.warp_perspective = mvdet_amd.warp_perspective

    class Stub(torch.nn.Module):
        def __init__(self, proj_mats, reducedgrid_shape):
            super().__init__()
            self.proj_mats, self.reducedgrid_shape = proj_mats, reducedgrid_shape
            self.map_classifier = torch.nn.Conv2d(4 * len(proj_mats), 1, 3, padding=1)

        def forward(self, feats):
            import kornia
            B = feats[0].shape[0]
            world = []
            for cam, img_feature in enumerate(feats):
                proj_mat = self.proj_mats[cam].repeat([B, 1, 1]).float().to(DEV)
                world.append(kornia.geometry.transform.warp_perspective(img_feature.to(DEV), proj_mat,
                                                                        self.reducedgrid_shape))
            return self.map_classifier(torch.cat(world, dim=1))

    Ms, _, _ = _adjoint_inputs(5, 2, 2, 4, 27, 48, 12, 36)
    model = Stub([M[0].double() for M in Ms], [12, 36]).to(DEV)
    g = torch.Generator().manual_seed(0)
    feats = [torch.randn((2, 4, 27, 48), generator=g).to(DEV).requires_grad_() for _ in Ms]
    loss = model(feats).square().mean()
    loss.backward()
    for f in feats:
        assert f.grad is not None and torch.isfinite(f.grad).all() and f.grad.abs().max() > 0
    assert model.map_classifier.weight.grad is not None
