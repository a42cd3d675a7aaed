"""CPU tests of the fused image head's host side: the new entry points refuse bad arguments with the
documented codes before any launch (the pointers are never dereferenced), the ctypes item matches the
header's struct, and ``mvdet_amd.upsample_relu_conv1x1`` raises on arguments it cannot run."""
import ctypes
import subprocess
from pathlib import Path

import pytest
import torch

from mvdet_amd import _native

ROOT = Path(__file__).resolve().parents[1]
P = 16  # a pointer value that is never dereferenced: validation fails first


def _items(n=1, g=P, out=P, grad_out=P, grad_g=P, stride=1):
    arr = (_native.ImgHeadItem * n)()
    s4 = _native._i64x4(stride, stride, stride, stride)
    for i in range(n):
        arr[i] = _native.ImgHeadItem(g, s4, out, s4, grad_out, s4, grad_g, s4)
    return arr


# (n, B, Cm, h, w, Co, Hu, Wu) -> status
GOOD = (1, 1, 64, 6, 8, 2, 18, 24)
BAD_DIMS = [
    ((1, 1, 64, 6, 8, 5, 18, 24), -2),    # Co = 5
    ((1, 1, 257, 6, 8, 2, 18, 24), -2),   # Cm = 257
    ((1, 1, 64, 6, 8, 2, 5, 24), -2),     # Hu < h
    ((1, 1, 64, 6, 8, 2, 18, 7), -2),     # Wu < w
    ((17, 1, 64, 6, 8, 2, 18, 24), -2),   # 17 views
    ((1, 0, 64, 6, 8, 2, 18, 24), -1),    # empty batch
    ((0, 1, 64, 6, 8, 2, 18, 24), -1),    # no view
    ((1, 1, 64, 6, 8, 0, 18, 24), -1),    # Co = 0
]


def test_item_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "mvbev.h"\n'
                   'int main(){printf("%zu %zu %zu %zu\\n", sizeof(mvbev_img_head_item),'
                   ' offsetof(mvbev_img_head_item, out), offsetof(mvbev_img_head_item, grad_out),'
                   ' offsetof(mvbev_img_head_item, grad_g_strides));}\n')
    exe = tmp_path / "sz"
    subprocess.run(["g++", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = _native.ImgHeadItem
    assert got == [ctypes.sizeof(T), T.out.offset, T.grad_out.offset, T.grad_g_strides.offset]


def test_forward_validation_codes():
    lib = _native.load()
    n, *dims = GOOD
    assert lib.mvbev_img_head_forward_f32(None, n, *dims, P, None) == -5
    assert lib.mvbev_img_head_forward_f32(_items(), n, *dims, None, None) == -5
    assert lib.mvbev_img_head_forward_f32(_items(g=None), n, *dims, P, None) == -5
    assert lib.mvbev_img_head_forward_f32(_items(out=None), n, *dims, P, None) == -5
    assert lib.mvbev_img_head_forward_f32(_items(stride=-1), n, *dims, P, None) == -3
    for (n, *dims), status in BAD_DIMS:
        assert lib.mvbev_img_head_forward_f32(_items(max(n, 1)), n, *dims, P, None) == status, (n, dims)
    assert lib.mvbev_img_head_forward_f32(_items(), 1, 1 << 20, 64, 6, 8, 2, 18, 24, P, None) == -2  # >= 2^31 elements


def test_backward_validation_codes():
    lib = _native.load()
    n, *dims = GOOD
    assert lib.mvbev_img_head_backward_f32(None, n, *dims, P, P, 1 << 30, None) == -5
    assert lib.mvbev_img_head_backward_f32(_items(), n, *dims, None, P, 1 << 30, None) == -5
    assert lib.mvbev_img_head_backward_f32(_items(g=None), n, *dims, P, P, 1 << 30, None) == -5
    assert lib.mvbev_img_head_backward_f32(_items(stride=-1), n, *dims, P, P, 1 << 30, None) == -3
    for (n, *dims), status in BAD_DIMS:
        assert lib.mvbev_img_head_backward_f32(_items(max(n, 1)), n, *dims, P, P, 1 << 30, None) == status, (n, dims)
        assert lib.mvbev_img_head_backward_blocks(_items(max(n, 1)), n, *dims) == 0
    n, *dims = GOOD
    # one workgroup per (view with a grad_out, b, 4 x 16 tile of g): 2 x 1 tiles of the 6 x 8 map
    assert lib.mvbev_img_head_backward_blocks(_items(), n, *dims) == 2
    assert lib.mvbev_img_head_backward_blocks(_items(3), 3, 2, *dims[1:]) == 3 * 2 * 2
    assert lib.mvbev_img_head_backward_blocks(None, n, *dims) == 0
    assert lib.mvbev_img_head_backward_blocks(_items(grad_out=None), n, *dims) == 0
    # partials too small for Co * Cm * blocks values
    assert lib.mvbev_img_head_backward_f32(_items(), n, *dims, P, P, 2 * 64 * 2 - 1, None) == -2
    # no view with a grad_out, or nothing wanted: nothing to do, nothing launched
    assert lib.mvbev_img_head_backward_f32(_items(grad_out=None), n, *dims, P, P, 1 << 30, None) == 0
    assert lib.mvbev_img_head_backward_f32(_items(grad_g=None), n, *dims, P, None, 0, None) == 0


def test_grad_weight_validation_codes():
    lib = _native.load()
    assert lib.mvbev_img_head_grad_weight_f32(None, 4, 64, 2, P, None) == -5
    assert lib.mvbev_img_head_grad_weight_f32(P, 4, 64, 2, None, None) == -5
    assert lib.mvbev_img_head_grad_weight_f32(P, 0, 64, 2, P, None) == -1
    assert lib.mvbev_img_head_grad_weight_f32(P, 4, 257, 2, P, None) == -2
    assert lib.mvbev_img_head_grad_weight_f32(P, 4, 64, 5, P, None) == -2


def test_wrapper_refuses_arguments_it_cannot_run():
    from mvdet_amd import upsample_relu_conv1x1
    from mvdet_amd.img_head import supported
    w = torch.zeros(2, 8)
    g = torch.zeros(1, 8, 4, 6)
    with pytest.raises(ValueError, match="cpu"):  # a CPU tensor: there is no CPU fallback
        upsample_relu_conv1x1([g], w, (12, 18))
    with pytest.raises(TypeError, match="float16"):
        upsample_relu_conv1x1([g.half()], w, (12, 18))
    with pytest.raises(TypeError, match="float64"):
        upsample_relu_conv1x1([g], w.double(), (12, 18))
    with pytest.raises(ValueError, match=r"\(1, 8, 4, 7\)"):  # mismatched view shapes
        upsample_relu_conv1x1([g, torch.zeros(1, 8, 4, 7)], w, (12, 18))
    with pytest.raises(ValueError, match="4-D"):
        upsample_relu_conv1x1([g[0]], w, (12, 18))
    with pytest.raises(ValueError, match="views per call"):
        upsample_relu_conv1x1([], w, (12, 18))
    with pytest.raises(ValueError, match="views per call"):
        upsample_relu_conv1x1([g] * 17, w, (12, 18))
    with pytest.raises(TypeError, match="sequence"):
        upsample_relu_conv1x1(g, w, (12, 18))
    with pytest.raises(TypeError, match="tensor"):
        upsample_relu_conv1x1([None], w, (12, 18))
    meta = torch.zeros(1, 8, 4, 6, device="meta")  # shape checks that come after the device check
    assert supported(1, meta.shape, 2, (12, 18))
    assert not supported(1, meta.shape, 5, (12, 18))      # Co = 5
    assert not supported(1, meta.shape, 2, (3, 18))       # Hu < h
    assert not supported(17, meta.shape, 2, (12, 18))
    assert not supported(1, (1, 257, 4, 6), 2, (12, 18))  # Cm = 257


def test_detector_flag_keeps_the_state_dict():
    """``native_img_head`` is a constructor flag; it adds no parameter or buffer."""
    from mvdet_amd import PerspTransDetector, synthetic
    ds = synthetic.wildtrack_like(2, 4, seed=0, img_shape=(216, 384), worldgrid_shape=(96, 288))
    on = PerspTransDetector(ds, device="cpu", native_img_head=True)
    off = PerspTransDetector(ds, device="cpu", native_img_head=False)
    assert on.native_img_head is True and off.native_img_head is False
    assert list(on.state_dict()) == list(off.state_dict())
    assert all(k.split(".")[0] in ("base_pt1", "base_pt2", "img_classifier", "map_classifier") for k in on.state_dict())
