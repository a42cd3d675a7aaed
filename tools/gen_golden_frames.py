"""Golden vectors for the camera-frame front (``mvdet_amd.frames``) from Pillow itself.

Needs Pillow (what torchvision's ``T.Resize`` calls for a ``PIL.Image``: ``img.resize((w, h), Image.BILINEAR)``).
Records two small images and Pillow's own resize of them, with the Pillow version, so that the restatement in
``tests/frames_ref.py`` stays pinned to Pillow where Pillow is not installed:

* a random 54 x 96 x 3 uint8 image and its 36 x 64 resize (the 1080 x 1920 -> 720 x 1280 ratio);
* a 23 x 41 image of alternating 0 / 255 rows and its 23 x 17 resize (one axis unchanged: Pillow skips that pass).

Usage:  python tools/gen_golden_frames.py        (writes tests/golden/frames_pil.npz, a few tens of kB)
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
OUT = ROOT / "tests" / "golden" / "frames_pil.npz"
sys.path.insert(0, str(ROOT / "tests"))


def pil_resize(img: np.ndarray, size) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((size[1], size[0]), Image.BILINEAR))


def main():
    import PIL

    import frames_ref as fr
    random_in = fr.random_frames((54, 96, 3), seed=20)
    rows_in = fr.alternating(23, 41, rows=True)
    arrays = {"random_in": random_in, "random_out": pil_resize(random_in, (36, 64)),
              "rows_in": rows_in, "rows_out": pil_resize(rows_in, (23, 17)),
              "pillow_version": np.array(PIL.__version__)}
    # the restatement is Pillow on these and on every shape pair of the frame tests, before anything is written
    assert np.array_equal(fr.resize(random_in, (36, 64)), arrays["random_out"])
    assert np.array_equal(fr.resize(rows_in, (23, 17)), arrays["rows_out"])
    for (H, W), size in fr.SHAPE_PAIRS:
        img = fr.random_frames((H, W, 3), seed=H + W)
        assert np.array_equal(fr.resize(img, size), pil_resize(img, size)), ((H, W), size)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, Pillow {PIL.__version__})")


if __name__ == "__main__":
    main()
