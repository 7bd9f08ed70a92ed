"""Writes tests/golden/lr_bicubic.npz: small seeded uint8 frames and what the REFERENCE's own imresize_np (utils/image_resize.py, imported
unmodified at run time; it needs only math and torch) returns for them at 1/2, 1/3 and 1/4, called as datasets/generate_LR.py calls it:
the uint8 frame, scale 1 / s, antialiasing on.  Build container only; TEST INFRASTRUCTURE.  Only data is recorded.

The frames: noise (its LR stays within about 30..225), a smooth scene, blocks of 0 and 255 (up to 2 levels of dither) with hard edges
(the filter overshoots below 0 and above 255 there, so the clamp of the uint8 store matters), a 64 x 96 mix of the three, and a 16 x 16
frame of such blocks whose every x4 output mirrors on some side.  Per frame and scale the script prints the share of reference values within HALF_BAND of a half-integer (where the
float32 reference and a float64 evaluation may round to different bytes) and asserts it stays under HALF_CAP, and that the hard-edge frames
have outputs beyond both ends of the uint8 range.

    VMG_REFERENCE=<path of the reference checkout> python tools/gen_lr_golden.py
"""
import importlib.util
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("VMG_REFERENCE", "")
HALF_BAND, HALF_CAP = 1e-3, 0.01
CLAMPED = ("edges", "mix")  # frames whose outputs must leave the uint8 range at both ends, at every scale


def import_reference_resize():
    if not os.path.isdir(REF):
        raise SystemExit("reference not present: the fixture can only be regenerated in the build container")
    spec = importlib.util.spec_from_file_location("vmg_ref_image_resize", os.path.join(REF, "utils", "image_resize.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def smooth(h, w):
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 100 * np.sin(x / 11.0) * np.cos(y / 7.0), 30 + 2.0 * x + 0.5 * y, 250 - 3.0 * y + 0.2 * x], -1)
    return np.clip(np.rint(base), 0, 255).astype(np.uint8)


def hard_edges(rng, h, w, cell):
    """Cells of 0 and 255 per channel, `cell` pixels wide, none aligned to the scale grids.  Half of the pixels are moved 1 or 2 levels
    inwards: with pure 0 / 255 every output is 255 * (a sum of the dyadic tap weights), and 6 % of them are exact rounding ties at x2."""
    cells = rng.integers(0, 2, (h // cell + 2, w // cell + 2, 3), dtype=np.uint8) * 255
    img = np.ascontiguousarray(cells.repeat(cell, 0).repeat(cell, 1)[1:h + 1, 2:w + 2]).astype(np.int32)
    dither = rng.integers(0, 3, img.shape) * rng.integers(0, 2, img.shape)
    return np.where(img == 0, dither, 255 - dither).astype(np.uint8)


def frames():
    """name -> ((H, W, 3) uint8, scales), at most 64 x 96."""
    rng = np.random.default_rng(20241017)
    out = {}
    out["noise"] = (rng.integers(0, 256, (48, 60, 3), dtype=np.uint8), (2, 3, 4))
    out["smooth"] = (smooth(48, 60), (2, 3, 4))
    out["edges"] = (hard_edges(rng, 48, 60, 7), (2, 3, 4))
    mix = smooth(64, 96)
    mix[8:40, 50:90] = hard_edges(rng, 32, 40, 5)
    mix[44:64, 0:48] = rng.integers(0, 256, (20, 48, 3), dtype=np.uint8)
    out["mix"] = (mix, (2, 4))
    out["tiny_edges"] = (hard_edges(rng, 16, 16, 6), (2, 4))
    return out


def main():
    ref = import_reference_resize()
    data, cases = {}, []
    for name, (img, scales) in frames().items():
        assert img.dtype == np.uint8 and img.shape[0] <= 64 and img.shape[1] <= 96
        data[name + "/hr"] = img
        for s in scales:
            lr = ref.imresize_np(img.copy(), 1 / s, True)
            assert lr.dtype == np.float32 and lr.shape == (img.shape[0] // s, img.shape[1] // s, 3)
            share = float(np.mean(np.abs(lr.astype(np.float64) - np.floor(lr.astype(np.float64)) - 0.5) <= HALF_BAND))
            print(f"{name} x{s}: {img.shape} -> {lr.shape}  min {lr.min():.3f} max {lr.max():.3f}  within {HALF_BAND} of a half-integer: {share:.4%}")
            assert share <= HALF_CAP, (name, s, share)
            if name in CLAMPED:
                assert lr.min() < -0.5 and lr.max() > 255.5, (name, s, "the clamp is not exercised")
            data[f"{name}/x{s}"] = lr
            cases.append([name, s])
    meta = {
        "cases": cases, "clamped": list(CLAMPED), "half_band": HALF_BAND, "half_cap": HALF_CAP,
        "values": "<name>/hr: the (H, W, 3) uint8 frame; <name>/x<s>: imresize_np(frame, 1 / s, True), float32 (H/s, W/s, 3), 0..255 scale, not rounded",
        "source": "imresize_np of the reference's utils/image_resize.py, imported unmodified, called as datasets/generate_LR.py:35 calls it",
    }
    data["meta"] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "lr_bicubic.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
