"""CPU tests of the point-list ground truth (``mvdet_amd.targets``): the constructors against a numpy
restatement of the reference's ``toarray()`` block (``frameDataset.py:134-148``), the contract's
refusals, the packing of a step into one buffer, the window-range rule the kernel scatters by against
``loss.pool_windows``, and the new C entry's refusals before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import loss_ref
from mvdet_amd import _native, loss, targets
from mvdet_amd.targets import PointTargets, pack_step


class Coo:
    """What the code reads of a ``scipy.sparse.coo_matrix``: row, col, data, shape."""

    def __init__(self, rows, cols, data, shape):
        self.row, self.col = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
        self.data, self.shape = np.asarray(data), tuple(shape)

    def toarray(self):  # as scipy: duplicates are summed
        out = np.zeros(self.shape, dtype=self.data.dtype if len(self.data) else np.int64)
        np.add.at(out, (self.row, self.col), self.data)
        return out


def reference_getitem(map_coo, views, reid=False):
    """frameDataset.py:134-148 with ``target_transform = ToTensor()``: ([1,Hg,Wg], N x [2,H,W]), fp32."""
    map_gt = map_coo.toarray()
    if reid:
        map_gt = (map_gt > 0).astype(np.int32)
    map_gt = torch.from_numpy(map_gt[:, :, None].transpose(2, 0, 1).copy()).float()
    imgs_gt = []
    for head, foot in views:
        img_gt = np.stack([head.toarray(), foot.toarray()], axis=2)
        if reid:
            img_gt = (img_gt > 0).astype(np.int32)
        imgs_gt.append(torch.from_numpy(img_gt.transpose(2, 0, 1).copy()).float())
    return map_gt, imgs_gt


def frame(seed, n, map_shape=(12, 36), img_shape=(27, 48), views=3, ids=False):
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 9, size=n) if ids else np.ones(n, np.int64)
    m = Coo(rng.integers(0, map_shape[0], n), rng.integers(0, map_shape[1], n), v, map_shape)
    vs = []
    for _ in range(views):
        col = rng.integers(0, img_shape[1], n)
        vs.append((Coo(rng.integers(0, img_shape[0], n), col, v, img_shape),
                   Coo(rng.integers(0, img_shape[0], n), col, v, img_shape)))
    return m, vs


def test_from_coo_sums_duplicates_and_binarizes_after_the_sum():
    m = Coo([1, 1, 2, 3], [3, 3, 0, 5], [1, 1, 1, 4], (4, 6))
    p = PointTargets.from_coo([m], (4, 6))
    assert p.shape == (1, 1, 4, 6) and len(p) == 3 and p.device == torch.device("cpu")
    d = p.dense()
    assert d.dtype == torch.float32 and d[0, 0, 1, 3] == 2 and d[0, 0, 2, 0] == 1 and d[0, 0, 3, 5] == 4
    assert torch.equal(d[0, 0], torch.from_numpy(m.toarray()).float())
    b = PointTargets.from_coo([m], (4, 6), binarize=True).dense()
    assert torch.equal(b, (d > 0).float()) and b.sum() == 3
    # a sum that cancels leaves no cell, before and after binarize
    z = Coo([1, 1], [2, 2], [1.0, -1.0], (4, 6))
    assert len(PointTargets.from_coo([z], (4, 6))) == 0 and len(PointTargets.from_coo([z], (4, 6), True)) == 0


def test_from_coo_nestings():
    a, b = Coo([0], [1], [1], (3, 4)), Coo([2, 2], [3, 0], [1, 1], (3, 4))
    flat = PointTargets.from_coo([a, b], (3, 4))            # [C], B = 1
    assert flat.shape == (1, 2, 3, 4)
    nested = PointTargets.from_coo([[a, b], [b, a]], (3, 4))  # [B][C]
    assert nested.shape == (2, 2, 3, 4) and nested.offsets.tolist() == [0, 3, 6]
    da, db = torch.from_numpy(a.toarray()).float(), torch.from_numpy(b.toarray()).float()
    assert torch.equal(flat.dense()[0], torch.stack([da, db]))
    assert torch.equal(nested.dense(), torch.stack([torch.stack([da, db]), torch.stack([db, da])]))
    with pytest.raises(ValueError):
        PointTargets.from_coo([[a, b], [a]], (3, 4))


def test_duck_typed_lists_without_scipy():
    class Plain:
        row, col, data = [0, 2], [1, 1], [1, 3.0]
    p = PointTargets.from_coo([Plain()], (3, 2))
    assert p.dense().tolist() == [[[[0, 1], [0, 0], [0, 3]]]]
    assert not any(getattr(v, "__name__", "").startswith("scipy") for v in vars(targets).values())


@pytest.mark.parametrize("reid", [False, True])
def test_from_frame_equals_the_reference_getitem(reid):
    m, vs = frame(1, 9, ids=reid)
    m.row[1], m.col[1] = m.row[0], m.col[0]  # two pedestrians in one map cell
    map_t, view_ts = PointTargets.from_frame(m, vs, binarize=reid)
    map_ref, views_ref = reference_getitem(m, vs, reid)
    assert map_t.shape == (1, 1, 12, 36) and torch.equal(map_t.dense()[0], map_ref)
    assert map_ref.max() == (1 if reid else 2)
    assert len(view_ts) == 3
    for t, ref, (head, foot) in zip(view_ts, views_ref, vs):
        assert t.shape == (1, 2, 27, 48) and torch.equal(t.dense()[0], ref)
        d = t.dense()[0]
        assert d[0, head.row[0], head.col[0]] > 0 and d[1, foot.row[0], foot.col[0]] > 0  # head = 0, foot = 1
    by_cam = PointTargets.from_frame(m, dict(enumerate(vs)), binarize=reid)[1]  # imgs_head_foot_gt[frame]
    assert all(torch.equal(a.dense(), b.dense()) for a, b in zip(by_cam, view_ts))


def test_from_dense_round_trip():
    for t in (loss_ref.points((2, 2, 5, 7), [(0, 0, 1, 1), (1, 1, 4, 6), (1, 0, 0, 0)]),
              loss_ref.dense((1, 1, 4, 4), [(0, 0, 3, 3), (0, 0, 0, 2)], [2.0, 0.5]),
              loss_ref.points((3, 1, 2, 2), []),
              torch.from_numpy(np.random.default_rng(3).uniform(0, 1, size=(2, 3, 4, 5)).astype(np.float32))):
        p = PointTargets.from_dense(t)
        assert p.shape == tuple(t.shape) and len(p) == int((t != 0).sum())
        assert torch.equal(p.dense(), t)
        assert p.offsets.dtype == torch.int32 and p.cells.dtype == torch.int32 and p.values.dtype == torch.float32
        assert p.offsets.tolist() == [int((t[:b] != 0).sum()) for b in range(t.shape[0] + 1)]


def test_cat_of_frames_with_different_cell_counts():
    shapes = (1, 2, 6, 9)
    ds = [loss_ref.points(shapes, [(0, 0, 1, 1), (0, 1, 5, 8), (0, 0, 0, 0)]), torch.zeros(shapes),
          loss_ref.dense(shapes, [(0, 1, 2, 3)], [2.0])]
    ps = [PointTargets.from_dense(d) for d in ds]
    c = PointTargets.cat(ps)
    assert c.shape == (3, 2, 6, 9) and len(c) == 4 and c.offsets.tolist() == [0, 3, 3, 4]
    assert torch.equal(c.dense(), torch.cat(ds))
    two = PointTargets.cat([c, ps[2]])  # B > 1 inputs
    assert torch.equal(two.dense(), torch.cat(ds + [ds[2]]))
    with pytest.raises(ValueError):
        PointTargets.cat([ps[0], PointTargets.from_dense(torch.zeros(1, 1, 6, 9))])
    with pytest.raises(ValueError):
        PointTargets.cat([ps[0], PointTargets.from_dense(torch.zeros(1, 2, 6, 8))])
    with pytest.raises(ValueError):
        PointTargets.cat([ps[0], PointTargets.from_dense(torch.zeros(1, 2, 7, 9))])
    with pytest.raises(ValueError):
        PointTargets.cat([])


def test_pack_step_items_view_one_buffer():
    frames = [frame(s, n) for s, n in ((5, 6), (6, 0), (7, 11))]
    per = [PointTargets.from_frame(m, vs) for m, vs in frames]
    map_t = PointTargets.cat([p[0] for p in per])
    view_ts = [PointTargets.cat([p[1][v] for p in per]) for v in range(3)]
    pm, pvs = pack_step(map_t, view_ts)
    items, src = [pm] + pvs, [map_t] + view_ts
    buf = pm.buffer
    assert buf.dtype == torch.int32 and buf.dim() == 1 and buf.is_contiguous()
    assert buf.numel() == sum(t.words for t in src) and buf.numel() * 4 < 4096  # a few kB
    lo, hi = buf.data_ptr(), buf.data_ptr() + 4 * buf.numel()
    for got, ref in zip(items, src):
        assert got.buffer is buf and got.shape == ref.shape and len(got) == len(ref)
        for part in (got.offsets, got.cells, got.values):
            assert lo <= part.data_ptr() and part.data_ptr() + 4 * part.numel() <= hi
        assert torch.equal(got.dense(), ref.dense())
        cells, values, offsets = got.pointers()  # non-NULL for the empty frame's items too
        assert offsets == got.offsets.data_ptr() and cells == offsets + 4 * 4 and values == cells + 12 * len(got)
        assert len(got) == 0 or (cells == got.cells.data_ptr() and values == got.values.data_ptr())
    empty = PointTargets.from_dense(torch.zeros(1, 1, 3, 3))
    assert len(empty) == 0 and all(empty.pointers())
    assert pm.to("cpu") is pm and not pm.is_pinned()
    with pytest.raises(TypeError):
        pack_step(map_t, [torch.zeros(1, 2, 3, 3)])


@pytest.mark.parametrize("val", [-1.0, float("nan"), float("inf")])
def test_bad_values_raise_naming_the_cell(val):
    with pytest.raises(ValueError, match=r"row=2, col=3"):
        PointTargets.from_coo([Coo([0, 2], [0, 3], [1.0, val], (4, 6))], (4, 6))
    t = torch.zeros(1, 1, 4, 6)
    t[0, 0, 2, 3] = val
    with pytest.raises(ValueError, match=r"row=2, col=3"):
        PointTargets.from_dense(t)
    if val != val:
        with pytest.raises(ValueError, match=r"row=2, col=3"):
            PointTargets.from_coo([Coo([0, 2], [0, 3], [1.0, val], (4, 6))], (4, 6), binarize=True)


def test_coordinates_out_of_range_raise():
    for rows, cols in (([4], [0]), ([0], [6]), ([-1], [0]), ([0], [-1])):
        with pytest.raises(ValueError, match=rf"row={rows[0]}, col={cols[0]}"):
            PointTargets.from_coo([Coo(rows, cols, [1], (9, 9))], (4, 6))
    for c in (2, -1):  # the channel, through the array constructor every other one ends in
        with pytest.raises(ValueError, match=rf"c={c}"):
            PointTargets._from_arrays([0], [c], [0], [0], [1.0], (1, 2, 4, 6))
    with pytest.raises(ValueError, match="b=1"):
        PointTargets._from_arrays([1], [0], [0], [0], [1.0], (1, 2, 4, 6))
    with pytest.raises(ValueError, match="twice"):
        PointTargets._from_arrays([0, 0], [1, 1], [2, 2], [3, 3], [1.0, 1.0], (1, 2, 4, 6))
    with pytest.raises(ValueError):
        PointTargets.from_coo([], (4, 6))


def test_pooled_range_is_pool_window_membership():
    """Source position p lies in the windows of exactly the pooled positions first[p] .. last[p]."""
    for n_in in range(1, 41):
        for n_out in range(1, 41):
            first, last = targets.pooled_range(n_in, n_out)
            starts, ends = loss.pool_windows(n_in, n_out)
            member = (starts[None, :] <= np.arange(n_in)[:, None]) & (np.arange(n_in)[:, None] < ends[None, :])
            i = np.arange(n_out)[None, :]
            assert np.array_equal(member, (first[:, None] <= i) & (i <= last[:, None])), (n_in, n_out)
            width = last - first + 1
            if n_in % n_out == 0:
                assert (width == 1).all()
            elif n_in > n_out:
                assert width.max() <= 2
            else:
                assert width.max() <= -(-n_out // n_in) + 1


def test_criterion_argument_errors_follow_the_dense_rules():
    crit = loss.GaussianMSE()
    mk, ik = loss.gaussian_kernels()
    x = torch.zeros(1, 1, 8, 8)
    pt = lambda *shape: PointTargets.from_dense(torch.zeros(*shape))  # noqa: E731
    for args in ((x, pt(2, 1, 16, 16), mk),            # batch mismatch
                 (x, pt(1, 2, 16, 16), mk),            # channel mismatch
                 (x, pt(1, 1, 16, 16), ik),            # kernel channels != x's
                 (x.double(), pt(1, 1, 16, 16), mk),
                 (torch.zeros(1, 1, 8, 8, device="meta"), pt(1, 1, 16, 16), mk)):  # other device than x
        with pytest.raises((ValueError, TypeError)):
            crit(*args)
        with pytest.raises((ValueError, TypeError)):
            crit._traget_transform(*args)
    with pytest.raises(RuntimeError):  # valid arguments on the host: there is no CPU fallback
        crit(x, pt(1, 1, 16, 16), mk)
    with pytest.raises(ValueError):    # the stats item's logical shape must be map_res's
        loss.detection_loss(x, [], pt(1, 1, 16, 16), [], mk, ik)


def test_public_surface_and_version():
    import mvdet_amd
    assert mvdet_amd.PointTargets is PointTargets and mvdet_amd.pack_step is pack_step
    assert mvdet_amd.targets is targets
    assert "mvbev_gaussian_mse_points_f32" in _native.EXPORTS
    lib = _native.load()
    assert hasattr(lib, "mvbev_gaussian_mse_points_f32")
    assert lib.mvbev_version() == 12500


def _item(fake, C=1, h=8, w=8, Ht=8, Wt=8, target=True):
    s = _native._i64x4(C * h * w, h * w, w, 1)
    st = _native._i64x4(C * Ht * Wt, Ht * Wt, Wt, 1)
    return _native.LossItem(fake, s, fake if target else None, st, C, h, w, Ht, Wt, None, fake, fake, 0, 1.0)


def test_points_entry_refuses_before_any_launch():
    lib = _native.load()
    fake = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    kern = lambda k, C=1: (_native.LossKernel * 1)(_native.LossKernel(fake, C, k, 1, 1))  # noqa: E731
    rec = lambda cells=fake, values=fake, offsets=fake, Ht=8, Wt=8: (_native.LossPoints * 1)(  # noqa: E731
        _native.LossPoints(cells, values, offsets, Ht, Wt))
    items = (_native.LossItem * 1)(_item(fake, target=False))
    call = lambda it, pts, n=1, kn=None, stats=-1, np_=1 << 20: lib.mvbev_gaussian_mse_points_f32(  # noqa: E731
        it, pts, n, 1, kn if kn is not None else kern(3), 1, 0.4, stats, fake, np_, None)
    assert call(items, None) == -5                        # no records
    assert call(None, rec()) == -5
    assert call(items, rec(cells=None)) == -5             # a record with some of its pointers
    assert call(items, rec(values=None)) == -5
    assert call(items, rec(offsets=None)) == -5
    assert call(items, rec(Ht=16)) == -2                  # not the item's Ht x Wt
    assert call(items, rec(Wt=4)) == -2
    assert call(items, rec(None, None, None)) == -5       # a dense record: the item's target is required
    # the checks of mvbev_gaussian_mse_f32 hold for point items too
    assert call(items, rec(), kn=kern(4)) == -2           # even k
    assert call(items, rec(), n=0) == -1
    assert call(items, rec(), n=17) == -2
    assert call(items, rec(), kn=kern(3, C=2)) == -2
    assert call(items, rec(), kn=kern(129)) == -2         # the tile does not fit the LDS
    assert call(items, rec(), np_=3) == -2                # partials too small
    assert call(items, rec(), stats=1) == -2
    pooled = (_native.LossItem * 1)(_item(fake, Ht=16, Wt=16, target=False))
    assert call(pooled, rec(Ht=16, Wt=16), stats=0) == -2  # the stats item's target must have x's size
    assert call(pooled, rec(Ht=16, Wt=16), np_=3) == -2    # accepted without target or pooled up to the last check
    # a point item needs no pooling launch and counts its workgroups as a dense one
    assert lib.mvbev_gaussian_mse_blocks(pooled, 1, 3) == 3
