"""CLEAR MOD evaluation on the GPU: MODA, MODP, precision and recall.

Drop-ins for the last step of the reference's test loop (``trainer.py:149-160``):
``multiview_detector/evaluation/evaluate.py`` and ``evaluation/pyeval/*`` (same names, arguments
and return order), on the HIP kernels of ``libmvbev.so`` (``mvbev_clear_mod_frames`` for the
Hungarian matching; ``mvbev_threshold_points_xy``, ``mvbev_point_nms_dev`` and
``mvbev_detections_append`` for detections that never leave the device).  No scipy, no files.

* ``CLEAR_MOD_HUN(gt, det) -> (recall, precision, MODA, MODP)``: ``[n, 4]`` rows (frame index, id,
  x, y), numpy arrays or torch tensors on any device.
* ``evaluateDetection_py(res_fpath, gt_fpath, dataset_name)`` / ``evaluate(res_fpath, gt_fpath,
  dataset='wildtrack')``: the file-based entry points (``evaluate`` never tries MATLAB); either
  argument may be an ``[n, 3]`` array or tensor (frame, x, y) instead of a path.
* ``pack_frames`` / ``metrics``: the host halves (the reference's frame rule as CSR point lists; the
  four numbers from the per-frame counters), pure numpy.
* ``clear_mod_frames``: the matching launch on packed frames, per-frame outputs after one readback.
* ``DetectionEvaluator``: the whole path for a test epoch.  ``update(map_res, frame)`` enqueues three
  launches on the map's stream (threshold, NMS, append) with no readback; ``compute()`` is one
  matching launch over the epoch and one readback.

The matching kernel reproduces scipy's ``linear_sum_assignment`` as an optimum, not as a
tie-break: where a frame has several optimal assignments it may pick another one.  The counted
pairs (``d < td``) and both sums are the same for all of them unless two optima differ in how
many pairs sit at exactly ``td``; ``tools/gen_golden_eval.py`` checks that for the fixtures.
"""
from __future__ import annotations

import math
import os
from collections import namedtuple

import numpy as np
import torch

from . import _native
from .ops import _require_cuda, _stream

TD = 50 / 2.5  # CLEAR_MOD_HUN.py:29

PackedFrames = namedtuple("PackedFrames", "frames gt_off gt_xy det_off det_xy")


def _host(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return a.astype(np.float64) if a.dtype.kind != "f" else a


def _rows(a, width: int) -> np.ndarray:
    a = _host(a)
    return a.reshape(-1, width) if a.size == 0 else np.atleast_2d(a)


def _csr(frame_col: np.ndarray, frames: np.ndarray):
    """Rows whose frame is in ``frames`` (sorted, unique), grouped by frame in their own order:
    (offsets int32 [F + 1], row order)."""
    F = len(frames)
    if F == 0 or len(frame_col) == 0:
        return np.zeros(F + 1, np.int32), np.zeros(0, np.int64)
    idx = np.searchsorted(frames, frame_col)
    hit = (idx < F) & (frames[np.minimum(idx, F - 1)] == frame_col)
    sel = np.flatnonzero(hit)
    order = sel[np.argsort(idx[sel], kind="stable")]
    off = np.concatenate([[0], np.cumsum(np.bincount(idx[sel], minlength=F))]).astype(np.int32)
    return off, order


def _pack(gt_frame, gt_xy, det_frame, det_xy, frames) -> PackedFrames:
    for what, xy in (("ground truth", gt_xy), ("detection", det_xy)):
        if not np.isfinite(xy).all():
            raise ValueError(f"{what} coordinates contain NaN or inf")  # as scipy's "matrix contains invalid numeric entries"
    gt_off, go = _csr(gt_frame, frames)
    det_off, do = _csr(det_frame, frames)
    return PackedFrames(frames, gt_off, np.ascontiguousarray(gt_xy[go]), det_off, np.ascontiguousarray(det_xy[do]))


def pack_frames(gt_rows, det_rows) -> PackedFrames:
    """evaluateDetection.py:52-94 as point lists: ``[n, 3]`` rows (frame, x, y) -> the frames that occur
    in the detections (``np.unique`` order, which is their renumbering), and per frame its GT and its
    detections in row order, as CSR offsets (int32) and ``[N, 2]`` coordinates.  GT of other frames is
    dropped.  Pure numpy."""
    gt, det = _rows(gt_rows, 3), _rows(det_rows, 3)
    frames = np.unique(det[:, 0])
    return _pack(gt[:, 0], gt[:, 1:3], det[:, 0], det[:, 1:3], frames)


def metrics(c, fp, m, g, modp_sum):
    """CLEAR_MOD_HUN.py:93-98 from the per-frame counters (arrays over the frames, or totals): fp64, the
    reference's expressions, each 0 unless > 0 (so NaN from 0 / 0 is 0).  -> (recall, precision, MODA, MODP)."""
    def total(a):
        t = np.float64(0)
        for v in np.asarray(a, np.float64).reshape(-1):  # frames in order
            t = t + v
        return t
    c, fp, m, g, s = (total(a) for a in (c, fp, m, g, modp_sum))
    with np.errstate(divide="ignore", invalid="ignore"):
        modp = s / c * 100
        moda = (1 - ((m + fp) / g)) * 100
        recall = c / g * 100
        precision = c / (fp + c) * 100
    return tuple(float(v) if v > 0 else 0 for v in (recall, precision, moda, modp))


def _device(device=None) -> torch.device:
    return torch.device(device if device is not None else "cuda:0")


def clear_mod_frames(gt_xy, gt_off, det_xy, det_off, td: float = TD, want_match: bool = False, device=None):
    """``mvbev_clear_mod_frames`` on CSR point lists (numpy arrays or tensors; fp32 or fp64 points of
    one dtype, or fp64 GT with fp32 detections): one launch, one readback.  -> dict of per-frame numpy
    arrays ``n_gt``, ``n_det``, ``matched`` (int32), ``modp_sum``, ``cost`` (fp64) and, if asked for,
    ``match`` ([Ng] int32: each GT's frame-local detection or -1)."""
    def pts(a):
        if not isinstance(a, torch.Tensor):
            a = np.asarray(a)
            a = torch.from_numpy(np.ascontiguousarray(a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)))
        if a.dtype not in (torch.float32, torch.float64):
            a = a.double()
        return a.reshape(-1, 2)
    gt, det = pts(gt_xy), pts(det_xy)
    if gt.dtype == det.dtype:
        dtype = _native.EVAL_F64 if gt.dtype == torch.float64 else _native.EVAL_F32
    elif gt.dtype == torch.float64:
        dtype = _native.EVAL_GT_F64_DET_F32
    else:
        gt, dtype = gt.double(), _native.EVAL_GT_F64_DET_F32 if det.dtype == torch.float32 else _native.EVAL_F64
    dev = next((t.device for t in (gt, det) if t.is_cuda), None) or _device(device)
    go = torch.as_tensor(gt_off).to(torch.int32).cpu().numpy()
    do = torch.as_tensor(det_off).to(torch.int32).cpu().numpy()
    if go.shape != do.shape or go.ndim != 1 or len(go) < 2:
        raise ValueError("gt_off and det_off are [F + 1] offsets of the same F >= 1 frames")
    ng, nd = np.diff(go), np.diff(do)
    small, large = int(np.minimum(ng, nd).max()), int(np.maximum(ng, nd).max())
    gt, det = gt.to(dev).contiguous(), det.to(dev).contiguous()
    out = _launch_matching(gt, det, dtype, torch.from_numpy(go).to(dev), torch.from_numpy(do).to(dev), len(go) - 1,
                           small, large, td, want_match, None)
    return out.read()


class _MatchOutputs:
    """The matching launch's outputs in one device buffer (one readback): int32 ``n_gt``, ``n_det``,
    ``matched`` [F], then fp64 ``modp_sum``, ``cost`` [F]."""

    def __init__(self, F: int, device, head_words: int = 0):
        self.F, self.head = F, head_words
        self.ints = head_words + 3 * F
        self.f64_at = -(-self.ints * 4 // 8) * 8
        self.buf = torch.zeros(self.f64_at + 16 * F, dtype=torch.uint8, device=device)
        self.match = None

    def int_ptr(self, k: int) -> int:
        return self.buf.data_ptr() + 4 * (self.head + k * self.F)

    def f64_ptr(self, k: int) -> int:
        return self.buf.data_ptr() + self.f64_at + 8 * k * self.F

    def read(self, F: int | None = None) -> dict:
        F = self.F if F is None else F
        host = self.buf.cpu().numpy()  # the readback
        ints = host[:self.ints * 4].view(np.int32)
        f64 = host[self.f64_at:].view(np.float64)
        out = {"head": ints[:self.head].copy()}
        for k, name in enumerate(("n_gt", "n_det", "matched")):
            out[name] = ints[self.head + k * self.F:self.head + k * self.F + F].copy()
        for k, name in enumerate(("modp_sum", "cost")):
            out[name] = f64[k * self.F:k * self.F + F].copy()
        if self.match is not None:
            out["match"] = self.match.cpu().numpy()
        return out


def _launch_matching(gt, det, dtype, gt_off, det_off, F, max_small, max_large, td, want_match, out, ws=None,
                     Nd=None):
    _require_cuda(gt_off, det_off)
    dev = gt_off.device
    lib = _native.load()
    Ng, Nd = gt.shape[0], det.shape[0] if Nd is None else Nd
    out = out if out is not None else _MatchOutputs(F, dev)
    if want_match:
        out.match = torch.empty(max(Ng, 1), dtype=torch.int32, device=dev)[:Ng]
    need = int(lib.mvbev_clear_mod_workspace_bytes(Ng, Nd, max_large))
    if need and (ws is None or ws.numel() * 8 < need):
        ws = torch.empty(-(-need // 8), dtype=torch.float64, device=dev)
    st = lib.mvbev_clear_mod_frames(
        gt.data_ptr() if Ng else None, det.data_ptr() if Nd else None, dtype, gt_off.data_ptr(), det_off.data_ptr(),
        F, Ng, Nd, max_small, max_large, float(td), out.int_ptr(0), out.int_ptr(1), out.int_ptr(2), out.f64_ptr(0),
        out.f64_ptr(1), out.match.data_ptr() if want_match and Ng else None, ws.data_ptr() if need else None,
        ws.numel() * 8 if need else 0, _stream(gt_off))
    _native.check(st, "mvbev_clear_mod_frames")
    out.ws = ws
    return out


def _check_solved(matched: np.ndarray) -> None:
    if (matched < 0).any():
        raise RuntimeError(f"mvbev_clear_mod_frames gave up {int((matched < 0).sum())} frame(s): sizes past the bounds "
                           "the call stated")


def _score(p: PackedFrames, td: float, device=None):
    """The four numbers of packed frames; frames without detections are not in ``p``."""
    if len(p.frames) == 0:
        return 0, 0, 0, 0
    r = clear_mod_frames(p.gt_xy, p.gt_off, p.det_xy, p.det_off, td, device=device)
    _check_solved(r["matched"])
    c = r["matched"]
    return metrics(c, r["n_det"] - c, r["n_gt"] - c, r["n_gt"], r["modp_sum"])


def CLEAR_MOD_HUN(gt, det, device=None):
    """``pyeval/CLEAR_MOD_HUN.py``: ``[n, 4]`` rows (frame index, id, x, y) -> (recall, precision, MODA,
    MODP).  As there, the frames are 0 .. max(gt frame): a frame with GT and no detection counts its misses,
    detections past the last GT frame are ignored."""
    gt, det = _rows(gt, 4), _rows(det, 4)
    if gt.shape[0] == 0:
        raise ValueError("CLEAR_MOD_HUN needs at least one ground-truth row")
    frames = np.arange(int(gt[:, 0].max()) + 1, dtype=np.float64)
    return _score(_pack(gt[:, 0], gt[:, 2:4], det[:, 0], det[:, 2:4], frames), TD, device)


def _load(rows_or_path) -> np.ndarray:
    if isinstance(rows_or_path, (str, os.PathLike)):
        if os.path.getsize(rows_or_path) == 0:
            return np.zeros((0, 3))
        return np.loadtxt(rows_or_path, ndmin=2)
    return _rows(rows_or_path, 3)


def evaluateDetection_py(res_fpath, gt_fpath, dataset_name=None, device=None):
    """``pyeval/evaluateDetection.py``: detections and GT as text files of (frame, x, y) rows, or as
    ``[n, 3]`` arrays / tensors -> (recall, precision, MODA, MODP).  Only frames that occur in the detections
    are evaluated; no detections at all: four zeros."""
    gt, det = _load(gt_fpath), _load(res_fpath)
    if det.shape[0] == 0:
        return 0, 0, 0, 0
    return _score(pack_frames(gt, det), TD, device)


def evaluate(res_fpath, gt_fpath, dataset="wildtrack", device=None):
    """``evaluation/evaluate.py`` without the MATLAB attempt -> (recall, precision, moda, modp)."""
    return evaluateDetection_py(res_fpath, gt_fpath, dataset, device)


class DetectionEvaluator:
    """A test epoch's evaluation without a host sync per frame.

    ``gt_rows`` ([n, 3]: frame, x, y) is packed once as CSR by frame and uploaded once (at the first ``compute()``).  ``update(map_res,
    frame)`` turns one output map into detections on the map's stream — ``map_res > cls_thres`` as positions
    ``* grid_reduce`` (``trainer.py:97-105``), the NMS of ``trainer.py:154`` (``dist_thres``, ``top_k``) and
    an append to the epoch's buffer — in three launches, with no readback and, after the first call for
    a map size, no allocation.  ``compute()`` matches every updated frame in one launch, reads the
    counters back once and returns (recall, precision, MODA, MODP) as ``evaluate`` does on ``results()``:
    frames without a detection are left out.  The buffer holds ``max_dets`` detections and ``max_frames``
    frames per epoch; a frame may be updated once.  GT coordinates are kept in fp64, detections in fp32.
    """

    _HEAD = 2  # cursor, overflow: the first words of the output buffer, so one readback covers them

    def __init__(self, gt_rows, cls_thres=0.4, grid_reduce=4, indexing="ij", dist_thres=20, top_k=math.inf, td=TD,
                 max_frames=1 << 12, max_dets=1 << 20):
        gt = _rows(gt_rows, 3)
        if not np.isfinite(gt).all():
            raise ValueError("ground truth rows contain NaN or inf")
        self._gt_frames = np.unique(gt[:, 0])
        self._gt_off, order = _csr(gt[:, 0], self._gt_frames)
        self._gt_xy = np.ascontiguousarray(gt[order, 1:3], dtype=np.float64)
        self.cls_thres, self.grid_reduce, self.indexing = float(cls_thres), grid_reduce, indexing
        self.dist_thres, self.td = float(dist_thres), float(td)
        self.top_k = (1 << 62) if (isinstance(top_k, float) and math.isinf(top_k)) else max(int(top_k), 1)
        self.max_frames, self.max_dets = int(max_frames), int(max_dets)
        self._frames: list = []
        self._dev = None
        self._map = {}  # (H, W) -> per-map buffers
        self._ws = self._gt_dev = None

    def _setup(self, device):
        self._dev = device
        self._buf = torch.zeros((self.max_dets, 2), dtype=torch.float32, device=device)
        self._det_off = torch.zeros(self.max_frames + 1, dtype=torch.int32, device=device)
        self._out = _MatchOutputs(self.max_frames, device, head_words=self._HEAD)

    def _map_buffers(self, H, W, device):
        b = self._map.get((H, W))
        if b is None:
            cap = H * W
            lib = _native.load()
            nws = int(lib.mvbev_point_nms_workspace_bytes(cap, cap))
            b = dict(cap=cap, cnt=torch.zeros(1, dtype=torch.int32, device=device),
                     xy=torch.empty((cap, 2), dtype=torch.float32, device=device),
                     val=torch.empty(cap, dtype=torch.float32, device=device),
                     keep=torch.empty(cap, dtype=torch.int64, device=device),
                     kept=torch.zeros(1, dtype=torch.int32, device=device),
                     ws=torch.empty(nws, dtype=torch.uint8, device=device), nws=nws)
            self._map[(H, W)] = b
        return b

    def update(self, map_res: torch.Tensor, frame) -> None:
        m = map_res.detach().squeeze().float().contiguous()
        _require_cuda(m)
        if m.dim() != 2:
            raise ValueError(f"expected one H x W map, got {tuple(map_res.shape)}")
        if self._dev is None:
            self._setup(m.device)
        elif m.device != self._dev:
            raise ValueError(f"the evaluator lives on {self._dev}, the map on {m.device}")
        frame = float(frame)
        if frame in self._frames:
            raise ValueError(f"frame {frame:g} was already updated in this epoch")
        slot = len(self._frames)
        if slot >= self.max_frames:
            raise RuntimeError(f"more than max_frames = {self.max_frames} frames in one epoch")
        H, W = m.shape
        b = self._map_buffers(H, W, m.device)
        lib, st = _native.load(), _stream(m)
        _native.check(lib.mvbev_threshold_points_xy(m.data_ptr(), H, W, self.cls_thres, float(self.grid_reduce),
                                                    1 if self.indexing == "xy" else 0, b["cnt"].data_ptr(),
                                                    b["xy"].data_ptr(), b["val"].data_ptr(), b["cap"], st),
                      "mvbev_threshold_points_xy")
        _native.check(lib.mvbev_point_nms_dev(b["xy"].data_ptr(), b["val"].data_ptr(), b["cnt"].data_ptr(), b["cap"],
                                              self.dist_thres, self.top_k, b["keep"].data_ptr(), b["kept"].data_ptr(),
                                              b["ws"].data_ptr(), b["nws"], st), "mvbev_point_nms_dev")
        _native.check(lib.mvbev_detections_append(b["xy"].data_ptr(), b["keep"].data_ptr(), b["kept"].data_ptr(),
                                                  b["cap"], self._buf.data_ptr(), self.max_dets, self._out.int_ptr(0) - 8,
                                                  self._det_off.data_ptr() + 4 * (slot + 1),
                                                  self._out.int_ptr(0) - 4, st), "mvbev_detections_append")
        self._frames.append(frame)

    def reset(self) -> None:
        """Clear the epoch: the frames, the detection buffer's cursor and the overflow word."""
        self._frames = []
        if self._dev is not None:
            self._out.buf.zero_()
            self._det_off.zero_()

    def _raise_overflow(self):
        raise RuntimeError(f"the epoch's detections do not fit max_dets = {self.max_dets}: construct the "
                           "DetectionEvaluator with a larger max_dets")

    def compute(self):
        F = len(self._frames)
        if F == 0:
            return 0, 0, 0, 0
        # the updated frames' GT, in update order, from the device copy: an index and offsets go up
        frames, G = np.asarray(self._frames), len(self._gt_frames)
        lo = n = np.zeros(F, np.int64)
        if G:
            k = np.minimum(np.searchsorted(self._gt_frames, frames), G - 1)
            has = self._gt_frames[k] == frames  # a frame without GT: an empty range
            lo = np.where(has, self._gt_off[k], 0).astype(np.int64)
            n = np.where(has, self._gt_off[k + 1] - self._gt_off[k], 0).astype(np.int64)
        gt_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        index = np.concatenate([np.arange(a, a + c) for a, c in zip(lo, n)] + [np.zeros(0, np.int64)]).astype(np.int64)
        if self._gt_dev is None:  # the one upload of the GT (update() issues launches only)
            self._gt_dev = torch.from_numpy(self._gt_xy).to(self._dev)
        gt = self._gt_dev.index_select(0, torch.from_numpy(index).to(self._dev))
        cap = min(max(b["cap"] for b in self._map.values()), self.max_dets)
        max_gt = int(n.max())
        out = _launch_matching(gt, self._buf, _native.EVAL_GT_F64_DET_F32, torch.from_numpy(gt_off).to(self._dev),
                               self._det_off, F, min(max_gt, cap), max(max_gt, cap), self.td, False, self._out,
                               ws=self._ws, Nd=self.max_dets)
        self._ws = out.ws
        r = out.read(F)
        if r["head"][1]:
            self._raise_overflow()
        _check_solved(r["matched"])
        order = np.argsort(np.asarray(self._frames), kind="stable")
        order = order[r["n_det"][order] > 0]  # the reference's frame rule: only frames that have detections
        if len(order) == 0:
            return 0, 0, 0, 0
        c, g, d = r["matched"][order], r["n_gt"][order], r["n_det"][order]
        return metrics(c, d - c, g - c, g, r["modp_sum"][order])

    def results(self) -> torch.Tensor:
        """The (frame, x, y) rows ``trainer.py:156`` writes to the result file, frames ascending: ``[m, 3]`` fp32
        on the device."""
        F = len(self._frames)
        if F == 0:
            return torch.empty((0, 3), device=self._dev)
        state = self._out.buf[:8].cpu().numpy().view(np.int32)
        if state[1]:
            self._raise_overflow()
        off = self._det_off[:F + 1].cpu().numpy()
        out = []
        for s in np.argsort(np.asarray(self._frames), kind="stable"):
            xy = self._buf[off[s]:off[s + 1]]
            out.append(torch.cat([torch.full((xy.shape[0], 1), self._frames[s], device=self._dev), xy], dim=1))
        return torch.cat(out, 0)
