"""The HR frames the LR tests run on, and their float64 reference values (tests/lr_ref.py), computed once per process and shared.
TEST INFRASTRUCTURE.

The seeds are part of the cases: with integer pixels and the dyadic tap weights of x2 (and x4) an output can be an exact rounding tie
(about 0.2 % of the x2 values of a random frame are), and the byte-for-byte tests want inputs without one.  tests/test_lr_ref.py checks
on the CPU that no reference value of any case lies within TIE_BAND of a half-integer.
"""
import functools
import json
import os

import numpy as np

from tests import lr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE_BAND = 1e-9

# id -> (scale, frames, H, W, seed).  16 x 16: every x4 output mirrors on some side; 148 x 212 -> 37 x 53: partial 16 x 16 tiles on both
# edges, several tiles; 48 x 60 for the other scales; one 720 x 1280.
CASES = {
    "x4-16x16": (4, 2, 16, 16, 1),
    "x4-64x96": (4, 2, 64, 96, 2),
    "x4-148x212": (4, 2, 148, 212, 3),
    "x4-720x1280": (4, 1, 720, 1280, 4),
    "x2-48x60": (2, 2, 48, 60, 3),
    "x3-48x60": (3, 2, 48, 60, 6),
}


def synth_hr(h, w, seed):
    """(h, w, 3) uint8: a smooth textured scene, a region of hard-edged 0 / 255 cells (the filter overshoots the uint8 range there) and a
    region of noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(x / 17.0 + seed) * np.cos(y / 13.0), 40 + 170.0 * x / w + 20 * np.sin(y / 5.0), 230 - 200.0 * y / h], -1)
    img = np.clip(np.rint(base + rng.normal(0, 4, base.shape)), 0, 255).astype(np.uint8)
    ch, cw = h // 2, w // 2
    cells = rng.integers(0, 2, (ch // 5 + 1, cw // 5 + 1, 3), dtype=np.uint8) * 255
    block = cells.repeat(5, 0).repeat(5, 1)[:ch, :cw].astype(np.int32)
    dither = rng.integers(0, 3, block.shape) * rng.integers(0, 2, block.shape)
    img[:ch, w - cw:] = np.where(block == 0, dither, 255 - dither).astype(np.uint8)
    img[h - h // 4:, :cw] = rng.integers(0, 256, (h // 4, cw, 3), dtype=np.uint8)
    return img


@functools.lru_cache(maxsize=None)
def case(cid):
    """(scale, hr, ref): hr (T, H, W, 3) uint8, ref (T, H/s, W/s, 3) float64 (0..255, not rounded).  Read-only: shared between tests."""
    s, t, h, w, seed = CASES[cid]
    hr = np.stack([synth_hr(h, w, seed * 100 + i) for i in range(t)])
    ref = np.stack([R.bicubic_down(f, s) for f in hr])
    hr.setflags(write=False)
    ref.setflags(write=False)
    return s, hr, ref


@functools.lru_cache(maxsize=None)
def fixture():
    """(meta, arrays) of tests/golden/lr_bicubic.npz: the reference's own float32 outputs."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "lr_bicubic.npz"))
    return json.loads(str(z["meta"])), {k: z[k] for k in z.files if k != "meta"}
