"""The non-finite PARAMETER cases of ``test_gpu_nonfinite_weights.py`` and of the oracle pin in ``test_oracle.py``:
one NaN / inf written into ``map_classifier`` (a diverging ``optimizer.step()``), always at a CENTRE tap (1, 1).

What a non-finite weight does against zero padding is the conv back end's business, not the model's (on this torch a
1-channel 6 x 6 ``F.conv2d`` with a NaN corner tap is NaN at all 36 pixels, while the 512-channel dilation-4 conv3 of
the oracle pass leaves the pixels whose tap (0, 0) falls in the padding finite); a centre tap never reads padding,
so the expected pattern is the model's.

The rig is ``test_gpu_nonfinite._rig(64, seed=0)`` (N = 3, sources 54 x 96, grid 24 x 72, C = 64), the features
``synthetic_features(1, 64, hb, up, seed=500 + v)``, the head ``fixtures.head_params(3, seed=11, C=64)``.  ``kind``:
what the oracle map is — "nan" (all NaN), "partial" (NaN and finite pixels: the discriminating rows, a fast path that
turns inf into NaN gives all-NaN there) or "finite" (a dead channel: -inf in a bias is ReLU'd to 0).
"""
import math

import torch

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
RIG_C, RIG_N, RIG_SEED, FEAT_SEED = 64, 3, 0, 500

# name: (parameter of map_classifier, index, value, kind)
CASES = {
    "w1_view_nan": ("0.weight", (5, 64 + 3, 1, 1), NAN, "nan"),
    "w1_view_ninf": ("0.weight", (5, 64 + 3, 1, 1), NINF, "partial"),
    "w1_coord_ninf": ("0.weight", (5, 192, 1, 1), NINF, "partial"),
    "b1_ninf": ("0.bias", (7,), NINF, "finite"),
    "b1_pinf": ("0.bias", (7,), PINF, "nan"),
    "w2_ninf": ("2.weight", (9, 17, 1, 1), NINF, "partial"),
    "w2_far_ninf": ("2.weight", (100, 200, 1, 1), NINF, "partial"),
    "b2_ninf": ("2.bias", (7,), NINF, "finite"),
}
CASES.update({f"w3_c{c}_pinf": ("4.weight", (0, c, 1, 1), PINF, "nan") for c in (0, 1, 2, 3, 100, 200)})


def rig(C=RIG_C, N=RIG_N, seed=RIG_SEED):
    """(dataset, params) — as ``test_gpu_nonfinite._rig`` (kept importable without a GPU)."""
    from mvdet_amd import synthetic
    from oracle import fixtures
    ds = synthetic.wildtrack_like(N, 4, seed=seed, img_shape=(216, 384), worldgrid_shape=(96, 288))
    return ds, fixtures.head_params(N, seed=11, C=C)


def features(ds, C=RIG_C, device="cpu", seed=FEAT_SEED):
    from mvdet_amd import synthetic
    up = tuple(ds.upsample_shape)
    return [synthetic.synthetic_features(1, C, [u // 3 for u in up], up, seed=seed + v, device=device)
            for v in range(ds.num_cam)]


def poisoned(params, case):
    """``params`` (numpy, ``fixtures.head_params``) as torch tensors with ``case``'s value written in."""
    key, idx, val, _ = CASES[case] if isinstance(case, str) else case
    tp = {k: torch.from_numpy(v).clone() for k, v in params.items()}
    tp["map_classifier." + key][idx] = val
    return tp


def check_kind(ref: torch.Tensor, kind: str) -> None:
    """The oracle map is what the case table says it is (so a case cannot silently become trivial)."""
    fin = int(torch.isfinite(ref).sum())
    assert int(torch.isinf(ref).sum()) == 0
    if kind == "nan":
        assert fin == 0
    elif kind == "finite":
        assert fin == ref.numel()
    else:
        assert 0 < fin < ref.numel(), fin
        assert not math.isnan(float(ref[torch.isfinite(ref)].abs().max()))
