"""Shared test helpers: golden-fixture loading and the parity gate.

Parity gate (north_star "within 1e-3 relative fp32"):
per tensor  |got - ref| <= 1e-3 * |ref| + 1e-3 * max|ref|   elementwise, and
normwise    max|got - ref| / max|ref| <= 1e-3.
"""
import json
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"
RTOL = 1e-3
ATOL_FRAC = 1e-3


def load_golden(name):
    """``golden/<name>.npz`` and the arrays kept in files of their own (no fixture file passes 1 MiB):
    ``<name>.<key>.npz`` holds the whole array, ``<name>.<key>.v<i>.npz`` its view i (axis 1)."""
    d = dict(np.load(GOLDEN / f"{name}.npz", allow_pickle=False))
    views = {}
    for p in GOLDEN.glob(f"{name}.*.npz"):
        key, *view = p.name[len(name) + 1:-len(".npz")].split(".")
        a = np.load(p, allow_pickle=False)[key]
        if view:
            views.setdefault(key, {})[int(view[0][1:])] = a
        else:
            d[key] = a
    for key, parts in views.items():
        d[key] = np.stack([parts[i] for i in range(len(parts))], 1)
    if "meta" in d:
        d["meta"] = json.loads(str(d["meta"]))
    return d


def to_np(x):
    if isinstance(x, torch.Tensor):
        return x.detach().to("cpu", torch.float64).numpy()
    return np.asarray(x, dtype=np.float64)


def parity_stats(got, ref):
    """Stats over the finite entries; the NaN/inf pattern itself must match exactly."""
    got, ref = to_np(got), to_np(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nf_g, nf_r = ~np.isfinite(got), ~np.isfinite(ref)
    assert np.array_equal(nf_g, nf_r), f"non-finite pattern differs ({int(nf_g.sum())} vs {int(nf_r.sum())})"
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    fin = ~nf_r
    got, ref = got[fin], ref[fin]
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    diff = np.abs(got - ref)
    if diff.size == 0:
        return dict(normwise=0.0, n_bad=0, max_abs=0.0, scale=scale)
    normwise = float(diff.max() / scale) if scale > 0 else float(diff.max())
    bound = RTOL * np.abs(ref) + ATOL_FRAC * scale
    n_bad = int((diff > bound).sum())
    return dict(normwise=normwise, n_bad=n_bad, max_abs=float(diff.max()) if diff.size else 0.0, scale=scale)


def assert_parity(got, ref, what="", normwise_tol=1e-3):
    s = parity_stats(got, ref)
    assert s["n_bad"] == 0 and s["normwise"] <= normwise_tol, f"{what}: parity failed {s}"
    return s


def parity_stats_sliced(got, ref, dims):
    """``parity_stats`` with the scale max|ref| taken over ``dims`` only: every index of the other dimensions
    is a slice judged on its own scale (elementwise bound and normwise error alike).  Returns the worst
    slice's normwise error, the elementwise count over all slices and the smallest / largest slice scale.  A
    slice whose reference is identically zero must be exactly zero."""
    got, ref = to_np(got), to_np(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    dims = sorted(d % ref.ndim for d in dims)
    keep = [d for d in range(ref.ndim) if d not in dims]
    nsl = int(np.prod([ref.shape[d] for d in keep])) if keep else 1
    got = np.transpose(got, keep + dims).reshape(nsl, -1)
    ref = np.transpose(ref, keep + dims).reshape(nsl, -1)
    nf_g, nf_r = ~np.isfinite(got), ~np.isfinite(ref)
    assert np.array_equal(nf_g, nf_r), f"non-finite pattern differs ({int(nf_g.sum())} vs {int(nf_r.sum())})"
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    fin = ~nf_r
    scale = np.where(fin, np.abs(ref), 0.0).max(axis=1)
    diff = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)), 0.0)
    zero = scale == 0
    assert not diff[zero].any(), f"{int((diff[zero] != 0).sum())} non-zero entries in slices whose reference is zero"
    nz = ~zero
    if not nz.any():
        return dict(normwise=0.0, n_bad=0, max_abs=0.0, scale_min=0.0, scale_max=0.0, slices=nsl)
    normwise = float((diff[nz].max(axis=1) / scale[nz]).max())
    bound = RTOL * np.where(fin, np.abs(ref), 0.0) + ATOL_FRAC * scale[:, None]
    n_bad = int((diff > bound).sum())
    return dict(normwise=normwise, n_bad=n_bad, max_abs=float(diff.max()), scale_min=float(scale[nz].min()),
                scale_max=float(scale.max()), slices=nsl)


def assert_parity_sliced(got, ref, dims, what="", normwise_tol=1e-3):
    """``assert_parity`` per slice: the same gate with max|ref| taken over ``dims`` instead of the whole tensor,
    so a small-magnitude slice cannot hide behind a large one."""
    s = parity_stats_sliced(got, ref, dims)
    assert s["n_bad"] == 0 and s["normwise"] <= normwise_tol, f"{what}: sliced parity failed {s}"
    return s


def masked_relu(pre, m):
    """torch's ReLU with the sign decision of a given 0/1 pattern ``m`` where ``pre`` is not NaN (the GPU's
    activation pattern: a pre-activation within fp32 rounding of 0 may fall either way): value
    where(m, pre, 0) with NaN kept as NaN (and -0.0 kept as -0.0, as torch's clamp does); gradient 1 where
    m or where ``pre`` is NaN, 0 elsewhere — ``nn.ReLU``'s backward is ``threshold_backward``,
    ``y <= 0 ? 0 : grad``, which passes the gradient at a NaN output.  With m = (pre > 0) it is ``F.relu``
    bit for bit, value and gradient (``test_oracle.py::test_masked_relu_is_torch_relu_nan_included``)."""
    p = pre.detach()
    off = torch.where(p == 0, p, torch.zeros_like(p))  # no gradient here; a signed zero keeps its sign
    return torch.where((m > 0) | torch.isnan(p), pre, off)


def parity_stats_t(got: torch.Tensor, ref: torch.Tensor, chunk: int = 1 << 26):
    """``parity_stats`` on torch tensors where they live (e.g. the GPU: full-size configs hold
    GB-sized tensors), in float64 chunks; the same gate and NaN/inf rule."""
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    g, r = got.reshape(-1), ref.reshape(-1).to(got.device)
    scale = 0.0
    for i in range(0, r.numel(), chunk):
        rc = r[i:i + chunk].double()
        gc = g[i:i + chunk].double()
        assert torch.equal(~torch.isfinite(gc), ~torch.isfinite(rc)), "non-finite pattern differs"
        assert torch.equal(torch.isnan(gc), torch.isnan(rc)), "NaN pattern differs"
        fin = torch.isfinite(rc)
        if fin.any():
            scale = max(scale, rc[fin].abs().max().item())
    n_bad, dmax = 0, 0.0
    for i in range(0, r.numel(), chunk):
        rc = r[i:i + chunk].double()
        gc = g[i:i + chunk].double()
        fin = torch.isfinite(rc)
        d = (gc[fin] - rc[fin]).abs()
        if d.numel():
            dmax = max(dmax, d.max().item())
            n_bad += int((d > RTOL * rc[fin].abs() + ATOL_FRAC * scale).sum().item())
    normwise = dmax / scale if scale > 0 else dmax
    return dict(normwise=normwise, n_bad=n_bad, max_abs=dmax, scale=scale)


def assert_parity_t(got, ref, what="", normwise_tol=1e-3):
    s = parity_stats_t(got, ref)
    assert s["n_bad"] == 0 and s["normwise"] <= normwise_tol, f"{what}: parity failed {s}"
    return s
