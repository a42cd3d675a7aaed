"""16-bit (bf16 / fp16) backbone maps on the fused upsample warp, the parts that need no GPU: the
``backbone_dtype`` option of ``PerspTransDetector`` (validation, an unchanged ``state_dict``), the
channels-last source rule for 2-byte elements, and the C ABI (the new flag, symbol and source kind as the
built library exports and refuses them — every call below returns before a launch)."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from mvdet_amd import _native, ops

ROOT = Path(__file__).resolve().parents[1]


def _ds():
    from mvdet_amd import synthetic
    return synthetic.wildtrack_like(2, 4, seed=0, img_shape=(72, 128), worldgrid_shape=(48, 96))


def test_backbone_dtype_is_validated():
    from mvdet_amd import PerspTransDetector
    ds = _ds()
    for bad in (torch.float32, torch.float64, "bf16", 16, torch.int8):
        with pytest.raises(ValueError, match="backbone_dtype"):
            PerspTransDetector(ds, device="cpu", backbone_dtype=bad)
    assert PerspTransDetector(ds, device="cpu").backbone_dtype is None
    for ok in (None, torch.bfloat16, torch.float16):
        assert PerspTransDetector(ds, device="cpu", backbone_dtype=ok).backbone_dtype is ok


def test_state_dict_is_the_same_with_the_option():
    from mvdet_amd import PerspTransDetector
    ds = _ds()
    torch.manual_seed(0)
    plain = PerspTransDetector(ds, device="cpu").state_dict()
    for dt in (torch.bfloat16, torch.float16):
        torch.manual_seed(0)
        sd = PerspTransDetector(ds, device="cpu", backbone_dtype=dt).state_dict()
        assert list(sd) == list(plain)
        for k in plain:
            assert sd[k].dtype == plain[k].dtype and sd[k].shape == plain[k].shape, k
            assert torch.equal(sd[k], plain[k]), k
        assert all(v.dtype == torch.float32 for v in sd.values() if v.is_floating_point())
        # the reference's fp32 checkpoint loads as before
        PerspTransDetector(ds, device="cpu", backbone_dtype=dt).load_state_dict(plain)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_channels_last_source_rule_for_16_bit_views(dtype):
    B, C, h, w = 2, 64, 6, 10
    # a buffer whose storage is 16-B aligned with room to shift a view by single elements
    buf = torch.zeros(B * h * w * C + 64, dtype=dtype)
    off = (-buf.data_ptr() % 16) // 2
    base = buf[off:off + B * h * w * C]
    assert base.data_ptr() % 16 == 0
    cl = base.view(B, h, w, C).permute(0, 3, 1, 2)
    assert ops.is_channels_last_source(cl)                                 # aligned, whole groups
    assert ops.is_channels_last_source(cl[:, :32])                         # one 32-channel group of a wider pixel
    assert ops.is_channels_last_source(cl[:, :, 1:, 2:])                   # a window: strides unchanged, base + 64 B k
    shifted = buf[off + 1:off + 1 + B * h * w * C].view(B, h, w, C).permute(0, 3, 1, 2)
    assert not ops.is_channels_last_source(shifted)                        # misaligned by one element
    assert not ops.is_channels_last_source(cl[:, 4:36])                    # a group starting 8 B into a line
    assert not ops.is_channels_last_source(cl[:, :40])                     # C % 32 != 0
    assert not ops.is_channels_last_source(cl.contiguous())                # NCHW
    # strides that are multiples of 4 elements but not of 8 keep fp32 groups aligned, not 16-bit ones
    odd = torch.zeros(B * h * w * 36 + 64, dtype=dtype)
    o2 = (-odd.data_ptr() % 16) // 2
    v = odd[o2:o2 + B * h * w * 36].view(B, h, w, 36).permute(0, 3, 1, 2)[:, :32]
    assert v.stride(3) == 36 and not ops.is_channels_last_source(v)
    f32 = torch.zeros(B * h * w * 36 + 64)
    o3 = (-f32.data_ptr() % 16) // 4
    assert ops.is_channels_last_source(f32[o3:o3 + B * h * w * 36].view(B, h, w, 36).permute(0, 3, 1, 2)[:, :32])
    assert not ops.is_channels_last_source(cl.to(torch.float64))


def test_abi_flag_symbol_and_source_kind():
    header = (ROOT / "include" / "mvbev.h").read_text()
    for name, val in (("MVBEV_WARP_DST_ZEROED", _native.WARP_DST_ZEROED), ("MVBEV_WARP_SRC_F16", _native.WARP_SRC_F16),
                      ("MVBEV_WARP_WINO43", _native.WARP_WINO43), ("MVBEV_WARP_SRC_BF16", _native.WARP_SRC_BF16)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", header)
        assert m and int(m.group(1)) == val, name
    assert _native.WARP_SRC_BF16 == 8
    assert (_native.EXACT_SRC_F32, _native.EXACT_SRC_F16, _native.EXACT_SRC_BF16) == (0, 1, 2)
    assert re.search(r"\bint\s+mvbev_nchw_to_nhwc_ex\s*\(", header)
    assert re.search(r"mvbev_warp_views_exact_rows\([^)]*int src_kind,", header)
    assert "mvbev_nchw_to_nhwc_ex" in _native.EXPORTS and "mvbev_nchw_to_nhwc_f32" in _native.EXPORTS
    lib = _native.load()
    assert hasattr(lib, "mvbev_nchw_to_nhwc_ex") and hasattr(lib, "mvbev_nchw_to_nhwc_f32")
    assert lib.mvbev_version() == 12500


def test_bad_flags_and_kinds_are_refused_before_any_launch():
    lib = _native.load()
    view = (_native.WarpView * 1)()
    view[0].src, view[0].dst = 64, 64  # never dereferenced: every call below is refused before the launch
    view[0].src_strides = _native._i64x4(18 * 32 * 64, 1, 32 * 64, 64)
    view[0].dst_strides = _native._i64x4(1, 1, 1, 1)
    both = _native.WARP_SRC_F16 | _native.WARP_SRC_BF16

    def up(flags, strides=None):
        if strides is not None:
            view[0].src_strides = _native._i64x4(*strides)
        return lib.mvbev_warp_views_upsampled_wino_rows_ex(view, 1, 1, 64, 18, 32, 54, 96, 24, 72, 8, flags, None, 0,
                                                           None, None)

    assert up(both) == _native.ERR_SHAPE and up(both | _native.WARP_DST_ZEROED) == _native.ERR_SHAPE
    assert up(16) == _native.ERR_SHAPE  # an unknown bit
    nchw = (64 * 18 * 32, 18 * 32, 32, 1)
    assert up(_native.WARP_SRC_F16, nchw) == _native.ERR_SHAPE and up(_native.WARP_SRC_BF16, nchw) == _native.ERR_SHAPE
    # channels-last strides that keep fp32 groups aligned but not 16-bit ones (pixel pitch 68 elements)
    assert up(_native.WARP_SRC_BF16, (18 * 32 * 68, 1, 32 * 68, 68)) == _native.ERR_SHAPE
    # the plain fused warp (already-upsampled features) refuses the bf16 bit
    view[0].src_strides = _native._i64x4(64 * 54 * 96, 54 * 96, 96, 1)
    assert lib.mvbev_warp_views_wino_rows_ex(view, 1, 1, 64, 54, 96, 24, 72, 8, _native.WARP_SRC_BF16, None, 0, None,
                                             None) == _native.ERR_SHAPE
    # the exact path's source kind: 0 / 1 / 2 only
    r0 = (ctypes.c_int32 * 1)(0)
    for kind in (-1, 3):
        assert lib.mvbev_warp_views_exact_rows(view, r0, 1, kind, 1, 64, 18, 32, 54, 96, 24, 72, 24, None, 0,
                                               None) == _native.ERR_SHAPE
    # the copy's element size: 4 or 2 only
    for es in (0, 1, 3, 8):
        assert lib.mvbev_nchw_to_nhwc_ex(view, 1, es, 1, 64, 18, 32, None) == _native.ERR_SHAPE


def test_ops_refuse_what_the_kernels_do_not_take():
    """The Python wrappers' own refusals need no device call either (a CPU tensor is refused first, so the dtype
    rules are exercised through ``is_channels_last_source`` above and on the GPU in test_gpu_half_maps.py)."""
    x = torch.zeros(1, 64, 6, 10, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.to_channels_last_into([x], [torch.zeros(1, 6, 10, 64, dtype=torch.bfloat16)])
