"""The camera-frame front on the host: the restatement (``frames_ref``) pinned to Pillow's own output (the golden file,
and live Pillow where it is installed), ``mvdet_amd.frames``' coefficient and value tables against the restatement,
the range predicate, the argument checks and the library's new symbol — no GPU compute."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import frames_ref as fr
from mvdet_amd import _native

ROOT = Path(__file__).resolve().parents[1]
SYMBOL = "mvbev_frames_resize_normalize_u8"


def test_the_front_is_exported():
    import mvdet_amd
    from mvdet_amd import FrameTransform, frames, resize_normalize  # noqa: F401
    for name in ("frames", "FrameTransform", "resize_normalize"):
        assert name in mvdet_amd.__all__, name
    assert frames.resize_normalize is resize_normalize


def test_restatement_is_the_golden_pillow_output():
    g = fr.golden()
    assert re.match(r"\d+\.\d+", str(g["pillow_version"]))
    assert g["random_in"].shape == (54, 96, 3) and g["random_out"].shape == (36, 64, 3)
    assert g["rows_in"].shape == (23, 41, 3) and g["rows_out"].shape == (23, 17, 3)
    assert np.array_equal(fr.resize(g["random_in"], (36, 64)), g["random_out"])
    assert np.array_equal(fr.resize(g["rows_in"], (23, 17)), g["rows_out"])
    assert np.array_equal(g["rows_in"], fr.alternating(23, 41))
    # the skipped axis really is skipped: rows of 0 and 255 stay rows of 0 and 255
    assert set(np.unique(g["rows_out"])) == {0, 255}


@pytest.mark.parametrize("in_hw,out_hw", fr.SHAPE_PAIRS, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in fr.SHAPE_PAIRS])
def test_restatement_is_live_pillow(in_hw, out_hw):
    Image = pytest.importorskip("PIL.Image")
    if in_hw == (37, 53):
        img = np.full((*in_hw, 3), 255, dtype=np.uint8)
    elif in_hw == (23, 41):
        img = fr.alternating(*in_hw)
    else:
        img = fr.random_frames((*in_hw, 3), seed=in_hw[0] + out_hw[1])
    want = np.asarray(Image.fromarray(img).resize((out_hw[1], out_hw[0]), Image.BILINEAR))
    assert np.array_equal(fr.resize(img, out_hw), want)


@pytest.mark.parametrize("in_hw,out_hw", fr.SHAPE_PAIRS, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in fr.SHAPE_PAIRS])
def test_resample_table_is_the_restatement_s(in_hw, out_hw):
    from mvdet_amd import frames
    for n_in, n_out in zip(in_hw, out_hw):
        bounds, coef = frames.resample_table(n_in, n_out)
        rb, rk = fr.coeffs(n_in, n_out)
        assert bounds.dtype == np.int32 and coef.dtype == np.int32
        assert coef.shape == (n_out, frames.ksize(n_in, n_out))
        assert np.array_equal(bounds, rb), "bounds (first index, tap count)"
        assert np.array_equal(coef, rk), "coefficients"
        assert bounds[:, 0].min() >= 0 and (bounds[:, 0] + bounds[:, 1]).max() <= n_in
    assert frames.resample_table(1080, 720)[0][:, 1].max() == 3   # at most 3 taps per axis at config 2
    assert frames.resample_table(1920, 480)[0][:, 1].max() == 8


def test_equal_sizes_give_the_copy_table():
    """Pillow skips a pass whose sizes are equal; the kernel runs it with the formula's own table for that case,
    which is an exact copy: one tap of weight 1 << 22 on the same index (a second tap of weight 0 inside the image)."""
    from mvdet_amd import frames
    bounds, coef = frames.resample_table(23, 23)
    assert np.array_equal(bounds[:, 0], np.arange(23))
    assert np.array_equal(coef[:, 0], np.full(23, 1 << 22)) and not coef[:, 1:].any()


def test_value_table_is_the_op_chain():
    from mvdet_amd import frames
    ramp = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (1, 256, 3))  # [H=1, W=256, C=3]
    for mean, std in ((fr.MEAN, fr.STD), ((0.1, 0.5, 0.9), (0.3, 1.0, 2.5))):
        lut = frames.value_table(mean, std)
        assert lut.shape == (3, 256) and lut.dtype == torch.float32
        assert torch.equal(lut, fr.to_tensor_normalize(ramp, mean, std)[:, 0, :])
    with pytest.raises(ValueError, match="three values"):
        frames.value_table((0.5,), (0.5,))
    with pytest.raises(ValueError, match="zero"):
        frames.value_table(fr.MEAN, (0.2, 0.0, 0.2))


def test_supported_range():
    from mvdet_amd import frames
    for in_hw, out_hw in fr.SHAPE_PAIRS + [((70, 131), (33, 70)), ((120, 480), (20, 80))]:
        assert frames.supported(in_hw, out_hw), (in_hw, out_hw)
    assert frames.pick_tile((1080, 1920), (720, 1280)) == (16, 64)
    assert frames.pick_tile((1080, 1920), (270, 480)) == (8, 64)   # 4x down
    assert frames.pick_tile((2160, 3840), (720, 1280)) == (16, 64)  # 4K -> 720
    assert frames.pick_tile((120, 480), (20, 80)) == (8, 32)       # 6x down
    assert not frames.supported((1080, 1920), (120, 213))           # 9x down: the staged box does not fit
    assert not frames.supported((1080, 1920), (720, 1280), n_views=17)
    assert not frames.supported((0, 1920), (720, 1280))
    frames_u8 = torch.zeros(1, 1, 1080, 1920, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="outside the kernel's range"):
        frames.resize_normalize(frames_u8, (120, 213))


def test_argument_errors():
    from mvdet_amd import FrameTransform, frames
    ok = torch.zeros(2, 3, 12, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"\[B,N,H,W,3\]"):
        frames.resize_normalize(ok[0], (6, 8))  # wrong rank
    with pytest.raises(ValueError, match=r"\[B,H,W,3\]"):
        frames.resize_normalize([ok[0, 0]], (6, 8))  # wrong rank in a sequence
    with pytest.raises(ValueError, match=r"\[B,H,W,3\]"):
        frames.resize_normalize(torch.zeros(2, 3, 12, 16, 4, dtype=torch.uint8), (6, 8))  # last dimension
    with pytest.raises(TypeError, match="uint8"):
        frames.resize_normalize(ok.float(), (6, 8))
    with pytest.raises(ValueError, match="differs"):
        frames.resize_normalize([ok[:, 0], ok[:, 1, :, :8]], (6, 8))
    with pytest.raises(ValueError, match="1 .. 16"):
        frames.resize_normalize([ok[:, 0]] * 17, (6, 8))
    with pytest.raises(ValueError, match="positive"):
        frames.resize_normalize(ok, (0, 8))
    with pytest.raises(ValueError, match="out must be"):
        frames.resize_normalize(ok, (6, 8), out=torch.zeros(2, 3, 3, 6, 9))
    with pytest.raises(ValueError, match="out must be"):
        frames.resize_normalize(ok, (6, 8), out=torch.zeros(2, 3, 3, 6, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="ROCm GPU"):
        frames.resize_normalize(ok, (6, 8))  # CPU tensors: no fallback
    with pytest.raises(ValueError, match="ROCm GPU"):
        FrameTransform((6, 8))(ok)
    with pytest.raises(ValueError, match="positive"):
        FrameTransform((6,))
    ft = FrameTransform()
    assert ft.size == (720, 1280) and ft.mean == fr.MEAN and ft.std == fr.STD
    assert ft.takes(ok) and not ft.takes(ok.float()) and not ft.takes(torch.zeros(2, 3, 3, 12, 16))


def test_pack_frames():
    from mvdet_amd.frames import pack_frames
    imgs = [fr.random_frames((12, 16, 3), seed=v) for v in range(3)]
    buf = pack_frames(imgs)
    assert buf.shape == (1, 3, 12, 16, 3) and buf.dtype == torch.uint8 and buf.is_contiguous()
    assert np.array_equal(buf.numpy()[0], np.stack(imgs))

    class Decoded:  # what np.asarray makes of a PIL.Image, without PIL
        def __array__(self, dtype=None, copy=None):
            return imgs[1]
    assert np.array_equal(pack_frames([Decoded()]).numpy()[0, 0], imgs[1])
    with pytest.raises(ValueError, match="uint8"):
        pack_frames([imgs[0].astype(np.float32)])
    with pytest.raises(ValueError, match="differs"):
        pack_frames([imgs[0], imgs[1][:8]])
    with pytest.raises(ValueError, match="H x W x 3"):
        pack_frames([imgs[0][..., 0]])


def test_modules_keep_their_state_dict():
    from mvdet_amd import FrameTransform, NoJointConvVariant, PerspTransDetector, synthetic
    ds = synthetic.wildtrack_like(2, 4, seed=0, img_shape=(72, 128), worldgrid_shape=(48, 96))
    ft = FrameTransform((72, 128))
    for cls in (PerspTransDetector, NoJointConvVariant):
        torch.manual_seed(0)
        plain = cls(ds, device="cpu")
        torch.manual_seed(0)
        with_ft = cls(ds, device="cpu", frame_transform=ft)
        assert with_ft.frame_transform is ft and plain.frame_transform is None
        assert list(plain.state_dict()) == list(with_ft.state_dict())
        assert not any("frame" in k for k in with_ft.state_dict())


def test_symbol_is_declared_and_validates_before_launch():
    header = (ROOT / "include" / "mvbev.h").read_text()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", header), "not declared in include/mvbev.h"
    assert SYMBOL in _native.EXPORTS
    lib = _native.load()
    assert hasattr(lib, SYMBOL) and lib.mvbev_version() == 12500
    fn = getattr(lib, SYMBOL)
    p = ctypes.c_void_p(16)  # never dereferenced: every call below is refused before the launch
    s5 = (_native._i64 * 5)(1, 1, 1, 1, 1)
    view = (_native.FrameView * 1)()
    view[0].src, view[0].batch_stride, view[0].row_stride = 16, 12 * 16 * 3, 16 * 3

    def call(views=view, n=1, B=1, H=12, W=16, h=6, w=8, ksx=5, ksy=5, lut=p, strides=s5):
        return fn(views, n, B, H, W, h, w, p, p, ksx, p, p, ksy, lut, p, strides, None)

    assert call(views=None) == -5 and call(lut=None) == -5
    assert call(n=0) == -1 and call(h=0) == -1 and call(ksx=0) == -1
    assert call(n=17) == -2 and call(ksy=65) == -2
    assert call(H=1080, W=1920, h=120, w=213, ksx=19, ksy=19) == -2  # 9x down: the staged box does not fit LDS
    assert call(strides=(_native._i64 * 5)(1, 1, 1, -1, 1)) == -3
    view[0].row_stride = -48
    assert call() == -3
    view[0].row_stride, view[0].src = 48, None
    assert call() == -5
