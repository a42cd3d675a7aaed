"""Ground truth as point lists, from the dataset to the criterion's LDS tile.

The reference keeps a frame's ground truth as ``scipy.sparse.coo_matrix`` objects
(``frameDataset.py:114-122``) and expands them per item into dense fp32 maps (``:134-148``) that are
moved to the GPU every step (``trainer.py:45-46``): 116 MB per frame at 7 views for a few dozen
non-zero cells.  ``PointTargets`` keeps the cells: ``mvdet_amd.loss`` takes one wherever it takes a
dense target and gives bitwise the result it gives on ``dense()`` of the same cells.

* ``PointTargets.from_coo(mats, shape)`` / ``from_frame(map_coo, views)`` — from the reference's
  ``coo_matrix`` objects (anything with ``.row``, ``.col``, ``.data``), on the host in numpy.
* ``PointTargets.from_dense(t)`` / ``.dense()`` — to and from a dense ``[B,C,Ht,Wt]`` tensor.
* ``PointTargets.cat(list)`` — frames joined along B (a ``DataLoader`` ``collate_fn``).
* ``pack_step(map_targets, view_targets)`` — every item of a step in one host buffer, so that the
  move to the GPU is one copy of a few kB.
* ``pooled_range(in_size, out_size)`` — the pooled positions whose ``adaptive_max_pool2d`` window
  holds each source position (the rule the kernel scatters by).

Layout.  A holder is a run of int32 words in a buffer: ``B + 1`` offsets, then ``n`` cells of three
words (channel, row, column), then the ``n`` fp32 values.  The cells are sorted by batch item (then
channel, row, column) and item ``b`` owns the cells ``offsets[b] .. offsets[b + 1] - 1``, so a
workgroup finds its item's cells without a search.
"""
from __future__ import annotations

import numpy as np
import torch

__all__ = ["PointTargets", "pack_step", "pooled_range"]


def pooled_range(in_size: int, out_size: int):
    """``(first, last)``, two int64 arrays of ``in_size``: source position ``p`` lies in the
    ``adaptive_max_pool2d`` windows (``mvdet_amd.loss.pool_windows``) of exactly the pooled positions
    ``first[p] .. last[p]`` = ``floor(p out / in) .. ceil((p + 1) out / in) - 1``.  One position when
    ``in`` is a multiple of ``out``, up to two for uneven windows, a run of at most
    ``ceil(out / in) + 1`` when ``in < out``."""
    n_in, n_out = int(in_size), int(out_size)
    p = np.arange(n_in, dtype=np.int64)
    return (p * n_out) // n_in, ((p + 1) * n_out + n_in - 1) // n_in - 1


class _Store:
    """An int32 buffer that one or more holders view.  ``to`` moves the whole buffer, once per
    device: every holder of a packed step that is moved to a device views the same copy."""

    def __init__(self, buf: torch.Tensor):
        self.buf = buf
        self.moved = {}

    def to(self, device, non_blocking=False) -> "_Store":
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.buf.device:
            return self
        store = self.moved.get(device)
        if store is None:
            out = torch.empty(self.buf.shape, dtype=torch.int32, device=device)
            out.copy_(self.buf, non_blocking=non_blocking)
            store = self.moved[device] = _Store(out)
        return store


def _check_shape(B, C, Ht, Wt):
    if min(B, C, Ht, Wt) <= 0:
        raise ValueError(f"empty target shape {(B, C, Ht, Wt)}")
    if max(B, C, Ht, Wt) > np.iinfo(np.int32).max:
        raise ValueError(f"target shape {(B, C, Ht, Wt)} does not fit int32 coordinates")


class PointTargets:
    """The non-zero cells of a logical ``[B,C,Ht,Wt]`` fp32 target: every ``(b, c, row, col)`` at
    most once, with its value.  Values are finite and > 0 (ground truth is counts; absent cells are
    0), coordinates lie inside the shape: checked wherever the data is on the host (``ValueError``
    naming the cell).  A holder built on the GPU by ``from_dense`` is trusted.

    ``offsets`` [B + 1] int32, ``cells`` [n, 3] int32 (channel, row, column) and ``values`` [n] fp32
    are views of one int32 buffer (see the module docstring)."""

    def __init__(self, store: _Store, start: int, shape, n: int):
        self._store, self._start, self._n = store, int(start), int(n)
        self._shape = tuple(int(s) for s in shape)

    # ---- the views ----
    @property
    def shape(self):
        return self._shape

    @property
    def device(self):
        return self._store.buf.device

    def __len__(self):
        return self._n

    @property
    def words(self) -> int:
        """int32 words this holder occupies in its buffer."""
        return self._shape[0] + 1 + 4 * self._n

    @property
    def buffer(self) -> torch.Tensor:
        """The int32 buffer this holder views (shared by the holders of one ``pack_step``)."""
        return self._store.buf

    @property
    def offsets(self) -> torch.Tensor:
        return self._store.buf[self._start:self._start + self._shape[0] + 1]

    @property
    def cells(self) -> torch.Tensor:
        s = self._start + self._shape[0] + 1
        return self._store.buf[s:s + 3 * self._n].view(self._n, 3)

    @property
    def values(self) -> torch.Tensor:
        s = self._start + self._shape[0] + 1 + 3 * self._n
        return self._store.buf[s:s + self._n].view(torch.float32)

    def pointers(self):
        """The addresses ``(cells, values, offsets)`` for ``mvbev_loss_points``, from the buffer's base:
        an empty list has addresses too (an empty tensor's ``data_ptr()`` is 0, which would read as a
        dense item)."""
        base = self._store.buf.data_ptr() + 4 * self._start
        cells = base + 4 * (self._shape[0] + 1)
        return cells, cells + 12 * self._n, base

    def __repr__(self):
        return f"PointTargets(shape={self._shape}, cells={self._n}, device={self.device})"

    # ---- constructors ----
    @classmethod
    def _from_arrays(cls, b, c, row, col, val, shape) -> "PointTargets":
        """From host arrays of unique cells: checks the contract, drops zeros, sorts, packs."""
        B, C, Ht, Wt = (int(s) for s in shape)
        _check_shape(B, C, Ht, Wt)
        b, c, row, col = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (b, c, row, col))
        val = np.asarray(val, dtype=np.float32).reshape(-1)
        bad = ~np.isfinite(val) | (val < 0)
        for a, hi in ((b, B), (c, C), (row, Ht), (col, Wt)):
            bad |= (a < 0) | (a >= hi)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError(f"cell (b={b[i]}, c={c[i]}, row={row[i]}, col={col[i]}) with value {val[i]} does not "
                             f"fit a target of shape {(B, C, Ht, Wt)}: coordinates must lie inside the shape, "
                             "values must be finite and >= 0")
        keep = val != 0
        b, c, row, col, val = b[keep], c[keep], row[keep], col[keep], val[keep]
        key = ((b * C + c) * Ht + row) * Wt + col
        order = np.argsort(key, kind="stable")
        key = key[order]
        if len(key) > 1 and (key[1:] == key[:-1]).any():
            i = int(order[1:][key[1:] == key[:-1]][0])
            raise ValueError(f"cell (b={b[i]}, c={c[i]}, row={row[i]}, col={col[i]}) is listed twice")
        n = len(key)
        words = np.empty(B + 1 + 4 * n, dtype=np.int32)
        words[:B + 1] = np.searchsorted(b[order], np.arange(B + 1))
        words[B + 1:B + 1 + 3 * n] = np.stack([c[order], row[order], col[order]], axis=1).reshape(-1)
        words[B + 1 + 3 * n:] = val[order].view(np.int32)
        return cls(_Store(torch.from_numpy(words)), 0, (B, C, Ht, Wt), n)

    @classmethod
    def from_coo(cls, mats, shape, binarize=False) -> "PointTargets":
        """From ``mats``, a ``[B][C]`` nesting (or ``[C]`` for B = 1) of objects with ``.row``,
        ``.col`` and ``.data`` (the reference's ``coo_matrix`` objects fit), and the target's
        ``(Ht, Wt)``.  Duplicate ``(row, col)`` entries are summed, as ``coo_matrix.toarray()`` sums
        them (two pedestrians in one cell give 2); ``binarize`` then applies the reference's re-ID
        rule ``(t > 0)`` (``frameDataset.py:136,145``).  Runs on the host in numpy."""
        mats = list(mats)
        if mats and hasattr(mats[0], "row"):
            mats = [mats]
        mats = [list(m) for m in mats]
        B, C = len(mats), len(mats[0]) if mats else 0
        if any(len(m) != C for m in mats):
            raise ValueError("every batch item must list the same number of channels")
        Ht, Wt = (int(s) for s in shape)
        _check_shape(B, C, Ht, Wt)
        bs, cs, rows, cols, vals = [], [], [], [], []
        for b, per_channel in enumerate(mats):
            for c, m in enumerate(per_channel):
                row = np.asarray(m.row, dtype=np.int64).reshape(-1)
                col = np.asarray(m.col, dtype=np.int64).reshape(-1)
                data = np.asarray(m.data, dtype=np.float64).reshape(-1)
                if not len(row) == len(col) == len(data):
                    raise ValueError(f"item (b={b}, c={c}): row, col and data differ in length")
                out = (row < 0) | (row >= Ht) | (col < 0) | (col >= Wt)
                if out.any():
                    i = int(np.flatnonzero(out)[0])
                    raise ValueError(f"cell (b={b}, c={c}, row={row[i]}, col={col[i]}) lies outside the "
                                     f"{Ht} x {Wt} target")
                key, inverse = np.unique(row * Wt + col, return_inverse=True)
                total = np.zeros(len(key), dtype=np.float64)
                np.add.at(total, inverse.reshape(-1), data)
                if binarize:
                    if np.isnan(total).any():
                        i = int(np.flatnonzero(np.isnan(total))[0])
                        raise ValueError(f"cell (b={b}, c={c}, row={key[i] // Wt}, col={key[i] % Wt}) holds NaN")
                    total = (total > 0).astype(np.float64)
                bs.append(np.full(len(key), b)), cs.append(np.full(len(key), c))
                rows.append(key // Wt), cols.append(key % Wt), vals.append(total)
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)  # noqa: E731
        return cls._from_arrays(cat(bs), cat(cs), cat(rows), cat(cols), cat(vals), (B, C, Ht, Wt))

    @classmethod
    def from_frame(cls, map_coo, views, binarize=False):
        """One frame as ``frameDataset.__getitem__`` returns it (``:134-149``), as points:
        ``(map_targets [1,1,Hg,Wg], [view_targets [1,2,H,W]] * N)`` from the map's ``coo_matrix`` and
        ``views``, a list (or a dict by camera) of N ``(head_coo, foot_coo)`` pairs; channel 0 is the
        head, channel 1 the foot.  The sizes are the matrices' ``.shape``."""
        if hasattr(views, "keys"):
            views = [views[k] for k in sorted(views.keys())]
        map_t = cls.from_coo([map_coo], map_coo.shape, binarize)
        view_ts = [cls.from_coo([head, foot], head.shape, binarize) for head, foot in views]
        return map_t, view_ts

    @classmethod
    def from_dense(cls, t: torch.Tensor) -> "PointTargets":
        """The non-zero cells of a dense ``[B,C,Ht,Wt]`` tensor, on ``t``'s device.  On the host the
        values are checked; on the GPU they are trusted (no sync is added to look at them)."""
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError("from_dense takes a 4-D [B,C,Ht,Wt] tensor")
        t = t.detach()
        if t.device.type == "cpu":
            # NaN != 0, so non-finite cells are among these and are refused by the check
            idx = t.nonzero().numpy()
            vals = t[t != 0].float().numpy()
            return cls._from_arrays(idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3], vals, t.shape)
        B = int(t.shape[0])
        _check_shape(*t.shape)
        idx = t.nonzero()  # lexicographic order: sorted by batch item
        n = int(idx.shape[0])
        b = idx[:, 0].contiguous()
        offsets = torch.searchsorted(b, torch.arange(B + 1, device=t.device)).to(torch.int32)
        vals = t[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]].float().contiguous()
        buf = torch.cat([offsets, idx[:, 1:].to(torch.int32).reshape(-1), vals.view(torch.int32)])
        return cls(_Store(buf), 0, t.shape, n)

    @classmethod
    def cat(cls, items) -> "PointTargets":
        """Frames joined along B (for a ``DataLoader`` ``collate_fn``); ``C``, ``Ht`` and ``Wt`` must
        agree.  The result owns a new buffer on the items' device."""
        items = list(items)
        if not items:
            raise ValueError("cat of an empty list")
        tail = items[0].shape[1:]
        for it in items:
            if not isinstance(it, PointTargets):
                raise TypeError(f"cat takes PointTargets, got {type(it).__name__}")
            if it.shape[1:] != tail:
                raise ValueError(f"cat: shapes {items[0].shape} and {it.shape} differ beyond the batch size")
            if it.device != items[0].device:
                raise ValueError(f"cat: holders on {items[0].device} and {it.device}")
        offsets, base = [items[0].offsets[:1] * 0], 0
        for it in items:
            offsets.append(it.offsets[1:] + base)
            base += len(it)
        buf = torch.cat(offsets + [it.cells.reshape(-1) for it in items] +
                        [it.values.view(torch.int32) for it in items])
        return cls(_Store(buf), 0, (sum(it.shape[0] for it in items),) + tail, base)

    # ---- moving and expanding ----
    def to(self, device, non_blocking=False) -> "PointTargets":
        """This holder on ``device``.  The whole buffer is moved, once per device: the holders of
        one ``pack_step`` that are moved to the GPU view one device buffer, filled by one copy."""
        store = self._store.to(device, non_blocking)
        return self if store is self._store else PointTargets(store, self._start, self._shape, self._n)

    def pin_memory(self) -> "PointTargets":
        if self._store.buf.is_pinned():
            return self
        return PointTargets(_Store(self._store.buf.pin_memory()), self._start, self._shape, self._n)

    def is_pinned(self) -> bool:
        return self._store.buf.is_pinned()

    def dense(self) -> torch.Tensor:
        """The dense fp32 ``[B,C,Ht,Wt]`` tensor on the holder's device (for tests and for
        ``visualize``); torch ops only."""
        out = torch.zeros(self._shape, dtype=torch.float32, device=self.device)
        if self._n:
            counts = (self.offsets[1:] - self.offsets[:-1]).long()
            b = torch.repeat_interleave(torch.arange(self._shape[0], device=self.device), counts, output_size=self._n)
            cells = self.cells.long()
            out[b, cells[:, 0], cells[:, 1], cells[:, 2]] = self.values
        return out


def pack_step(map_targets: PointTargets, view_targets):
    """Every item of a step — the map and the N views, each holding the step's B frames — in one
    contiguous host buffer: ``(map_targets, [view_targets] * N)`` as views of it.  The buffer is
    pinned when every input is.  ``.to(device, non_blocking=True)`` of the first returned holder moves
    the whole buffer in one copy of a few kB and every other holder's ``.to(device)`` views that copy:

        map_gt, imgs_gt = pack_step(map_gt, imgs_gt)
        map_gt, imgs_gt = map_gt.to(dev, non_blocking=True), [g.to(dev) for g in imgs_gt]
    """
    items = [map_targets] + list(view_targets)
    for it in items:
        if not isinstance(it, PointTargets):
            raise TypeError(f"pack_step takes PointTargets, got {type(it).__name__}")
        if it.device.type != "cpu":
            raise ValueError(f"pack_step packs host holders for one upload, got one on {it.device}")
    buf = torch.empty(sum(it.words for it in items), dtype=torch.int32,
                      pin_memory=all(it.is_pinned() for it in items))
    store, out, start = _Store(buf), [], 0
    for it in items:
        buf[start:start + it.words] = it._store.buf[it._start:it._start + it.words]
        out.append(PointTargets(store, start, it.shape, len(it)))
        start += it.words
    return out[0], out[1:]
