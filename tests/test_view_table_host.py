"""CPU tests of the warp bindings' shared plumbing: the ``mvbev_warp_view`` table builder (``ops._view_table``,
``ops._m9``, ``ops._split_dst_strides``), the rig base (``rig.Rig``), and the null / stride refusals of every
``mvbev_warp_views_*`` entry point (returned before anything is launched, so they need no GPU)."""
import ctypes

import pytest
import torch

from mvdet_amd import _native, ops
from mvdet_amd.geometry import kornia_src_norm_from_dst_norm
from mvdet_amd.rig import Rig

EMPTY = [0.0, 0.0, 1e6, 0.0, 0.0, 1e6, 0.0, 0.0, 1.0]


def _entry(v):
    return (v.src, list(v.src_strides), v.dst, list(v.dst_strides), list(v.m))


def test_view_table_fields_of_strided_tensors():
    base = torch.zeros(2, 3, 4, 5)
    a = base[:, 1:3]                                              # [2,2,4,5], strides (60,20,5,1), offset 20 floats
    b = torch.zeros(2, 2, 4, 5).contiguous(memory_format=torch.channels_last)  # strides (40,1,10,2)
    assert a.stride() == (60, 20, 5, 1) and b.stride() == (40, 1, 10, 2)
    da, db = torch.zeros(2, 2, 3, 4), torch.zeros(2, 7, 3, 4)[:, 2:4]  # strides (24,12,4,1) and (84,12,4,1)
    m0 = torch.arange(9, dtype=torch.float64).reshape(3, 3) / 4   # exact in fp32
    arr = ops._view_table([a, b], [m0, None], [da, db])
    assert len(arr) == 2
    assert _entry(arr[0]) == (base.data_ptr() + 80, [60, 20, 5, 1], da.data_ptr(), [24, 12, 4, 1],
                              [0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0])
    assert _entry(arr[1]) == (b.data_ptr(), [40, 1, 10, 2], db.data_ptr(), [84, 12, 4, 1], EMPTY)
    # ABI strides of the caller's, a raw address as the destination, a unit stride for a size-1 dimension
    one = torch.zeros(2, 4, 4, 5)[:, 1:2]                         # [2,1,4,5], strides (80,20,5,1)
    arr = ops._view_table([one], [m0], [4096], [(7, 5, 3, 1)], unit_dim=1)
    assert _entry(arr[0]) == (one.data_ptr(), [80, 1, 5, 1], 4096, [7, 5, 3, 1], list((m0.reshape(9)).tolist()))
    # matrices alone; no matrices at all
    arr = ops._view_table(None, [None, m0])
    assert _entry(arr[0]) == (None, [0] * 4, None, [0] * 4, EMPTY)
    assert _entry(arr[1]) == (None, [0] * 4, None, [0] * 4, m0.reshape(9).tolist())
    arr = ops._view_table([a], None, [da], [(0, 0, 0, 1)])
    assert _entry(arr[0]) == (a.data_ptr(), [60, 20, 5, 1], da.data_ptr(), [0, 0, 0, 1], [0.0] * 9)


def test_m9_converts_to_fp32_and_maps_none_to_the_empty_slot():
    assert list(ops._m9(None)) == EMPTY
    m = torch.tensor([[1 / 3, 0, 0], [0, 1e-20, 0], [0, 0, 1]], dtype=torch.float64)
    assert list(ops._m9(m)) == m.float().reshape(9).tolist()       # rounded to fp32 once, as torch rounds
    assert list(ops._m9(m.numpy())) == list(ops._m9(m))


def test_split_dst_strides():
    shape = ops.split_shape(2, 9, 4, 5)
    assert shape == (2, 2, 4, 5, 2, 8)
    d = torch.zeros(shape, dtype=torch.bfloat16)
    assert d.stride() == (640, 320, 80, 16, 8, 1)
    assert ops._split_dst_strides(d, shape) == (40, 20, 5, 1)
    # a group slice of a wider slab keeps contiguous pixels: the slab's strides in 32-byte units
    slab = torch.zeros(ops.split_shape(2, 24, 4, 5), dtype=torch.bfloat16)
    assert ops._split_dst_strides(slab[:, 1:3], shape) == (slab.stride(0) // 16, 20, 5, 1) == (60, 20, 5, 1)
    wide = torch.zeros((2, 2, 4, 5, 2, 16), dtype=torch.bfloat16)[..., :8]   # hi and lo 16 apart
    cols = torch.zeros((2, 2, 4, 10, 2, 8), dtype=torch.bfloat16)[:, :, :, ::2]  # every other pixel
    for bad in (wide, cols, d.float(), d[:, :1]):
        with pytest.raises(ValueError, match="contiguous pixels"):
            ops._split_dst_strides(bad, shape)


def test_rig_matrices_are_bitwise_the_kornia_recipe():
    mats = [torch.tensor([[1.1, 0.02, 3.0], [-0.01, 0.9, -2.0], [1e-4, 2e-4, 1.0]], dtype=torch.float64),
            torch.tensor([[0.7, -0.2, 10.0], [0.3, 1.2, 5.0], [-3e-4, 1e-4, 1.0]], dtype=torch.float64),
            torch.eye(3, dtype=torch.float64)]
    up, grid = (18, 24), (10, 14)
    want = torch.stack([kornia_src_norm_from_dst_norm(M.float().reshape(1, 3, 3), up, grid)[0] for M in mats])
    rig = Rig(mats, up, grid)
    assert rig.up_hw == up and rig.grid_hw == grid and rig.num_views == 3
    assert rig.m_norm_cpu.dtype == torch.float32 and torch.equal(rig.m_norm_cpu, want)
    from mvdet_amd import ProjectFuse, ProjectSumHead, ProjectThinFuse
    thin = ProjectThinFuse(mats, up, grid)
    assert thin.m_norm_cpu is thin.engine.m_norm_cpu
    for head in (ProjectSumHead(mats, up, grid), thin, ProjectFuse(mats, up, grid, 8)):
        assert torch.equal(head.m_norm_cpu, want)
    calls = []
    assert rig.cached(("k", 1), lambda: calls.append(1) or "made") == "made"
    assert rig.cached(("k", 1), lambda: calls.append(1) or "again") == "made" and calls == [1]


# One view, B = 1, C = 8, a 4 x 5 source and a 3 x 4 grid (the upsampling entry points: a 4 x 5 backbone map
# upsampled to 12 x 15); T rows of r3 = 4 three-row tiles.  Every call is valid but for the one field under test.
P = ctypes.c_void_p(4096)  # never dereferenced: validation fails first
ROW0 = (ctypes.c_int32 * 1)(0)
DIMS, UP = (1, 8, 4, 5, 3, 4), (1, 8, 4, 5, 12, 15, 3, 4)
ENTRY_POINTS = {
    "mvbev_warp_views_f32": lambda a: (a, 1, *DIMS, None),
    "mvbev_warp_views_f16": lambda a: (a, 1, *DIMS, None),
    "mvbev_warp_views_split_bf16_ex": lambda a: (a, 1, 0, *DIMS, 0, None),
    "mvbev_warp_views_split_bf16_rows": lambda a: (a, ROW0, 1, 0, *DIMS, 3, 0, None, 0, None),
    "mvbev_warp_views_wino_rows": lambda a: (a, 1, *DIMS, 4, 0, None, 0, None),
    "mvbev_warp_views_wino_rows_ex": lambda a: (a, 1, *DIMS, 4, 0, None, 0, None, None),
    "mvbev_warp_views_exact_f32": lambda a: (a, 1, 1, 8, 4, 5, 4, 5, 3, 4, None, 0, None),
    "mvbev_warp_views_exact_rows": lambda a: (a, ROW0, 1, 0, 1, 8, 4, 5, 4, 5, 3, 4, 3, None, 0, None),
    "mvbev_warp_views_upsampled": lambda a: (a, 1, 0, *UP, 0, None),
    "mvbev_warp_views_upsampled_ex": lambda a: (a, 1, 0, *UP, 0, 0, None),
    "mvbev_warp_views_upsampled_wino_rows": lambda a: (a, 1, *UP, 4, 0, None, 0, None),
    "mvbev_warp_views_upsampled_wino_rows_ex": lambda a: (a, 1, *UP, 4, 0, None, 0, None, None),
    "mvbev_warp_views_backward_f32": lambda a: (a, 1, *DIMS, None),
}


def _one_view(src=P, dst=P, dst_col_stride=1):
    arr = (_native.WarpView * 1)()
    arr[0].src, arr[0].src_strides = src, _native._i64x4(160, 20, 5, 1)
    arr[0].dst, arr[0].dst_strides = dst, _native._i64x4(96, 12, 4, dst_col_stride)
    arr[0].m = (1, 0, 0, 0, 1, 0, 0, 0, 1)
    return arr


def test_every_warp_views_entry_point_is_covered():
    declared = {n for n in _native.EXPORTS if n.startswith("mvbev_warp_views_")}
    assert declared - set(ENTRY_POINTS) == {"mvbev_warp_views_adjoint"}  # (its own view struct: test_host.py)


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_warp_views_entry_points_refuse_null_and_strided_views(name):
    fn, args = getattr(_native.load(), name), ENTRY_POINTS[name]
    assert fn(*args(None)) == -5                                 # MVBEV_ERR_NULL: no table
    assert fn(*args(_one_view(src=None))) == -5
    assert fn(*args(_one_view(dst=None))) == -5
    assert fn(*args(_one_view(dst_col_stride=2))) == -3          # MVBEV_ERR_STRIDE: dst_strides[3] != 1
