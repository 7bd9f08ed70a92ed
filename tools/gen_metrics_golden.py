"""Writes tests/golden/metrics_frames.npz: small seeded uint8 frame pairs and what the REFERENCE's own calculate_psnr /
structural_similarity (utils/metrics.py, imported unmodified at run time) return for them.  Build container only; TEST INFRASTRUCTURE.

OpenCV and scikit-image are absent from the image.  The reference module imports cv2 at module level and calls two of its primitives,
which this script gives the empty stand-in module (oracle/_standins/cv2) in THIS process only:
  getGaussianKernel(ksize, sigma)   exp(-x^2 / (2 sigma^2)), scaled by the reciprocal of the sum, as a (ksize, 1) float64 column
  filter2D(src, -1, kernel)         a float64 correlation anchored at the kernel centre (scipy.ndimage.correlate; how the border is
                                    filled does not matter, the caller crops [5:-5, 5:-5])
scikit-image's rgb2ycbcr(uint8)[..., 0], which tools/test_reds4.py:208-209 feeds to the metrics, is restated the way the package spells
it: (rgb / 255) @ [65.481, 128.553, 24.966] + 16, float64, not rounded.  The fixture's `meta` entry says so.

Per pair the eight values are [psnr, psnr_y, ssim, ssim_y] of the frames and the same four of the frames cut by BORDER pixels on every side.

    python tools/gen_metrics_golden.py        (VMG_REFERENCE = path of the reference checkout)
"""
import importlib.util
import json
import math
import os
import sys

import numpy as np
import scipy.ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("VMG_REFERENCE", "/root/reference")
BORDER = 4


def _gaussian_kernel(ksize, sigma):
    t = [math.exp(-((i - (ksize - 1) / 2.0) ** 2) / (2.0 * sigma * sigma)) for i in range(ksize)]
    s = 1.0 / sum(t)
    return np.array([v * s for v in t], dtype=np.float64).reshape(ksize, 1)


def _filter2d(src, ddepth, kernel):
    assert ddepth == -1 and src.dtype == np.float64
    return scipy.ndimage.correlate(src, np.asarray(kernel, dtype=np.float64), mode="mirror")


def _rgb_to_y(img):
    return (img.astype(np.float64) / 255.0) @ np.array([65.481, 128.553, 24.966], dtype=np.float64) + 16.0


def import_reference_metrics():
    if not os.path.isdir(REF):
        raise SystemExit("reference not present: the fixture can only be regenerated in the build container")
    sys.path.insert(0, os.path.join(ROOT, "oracle", "_standins"))
    import cv2
    cv2.getGaussianKernel, cv2.filter2D = _gaussian_kernel, _filter2d
    spec = importlib.util.spec_from_file_location("vmg_ref_metrics", os.path.join(REF, "utils", "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def frame_pairs():
    """name -> (out, gt), (H, W, 3) uint8 each, at most 64 x 96."""
    rng = np.random.default_rng(20241008)
    pairs = {}
    gt = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    pairs["noise"] = (np.clip(gt.astype(np.int32) + rng.integers(-8, 9, gt.shape), 0, 255).astype(np.uint8), gt)
    y, x = np.mgrid[0:64, 0:96]
    base = np.stack([127 + 100 * np.sin(x / 11.0) * np.cos(y / 7.0), 30 + 2.0 * x + 0.5 * y, 250 - 3.0 * y + 0.2 * x], -1)
    gt = np.clip(np.rint(base), 0, 255).astype(np.uint8)
    pairs["smooth"] = (np.clip(gt.astype(np.int32) + rng.integers(-3, 4, gt.shape), 0, 255).astype(np.uint8), gt)
    blocks = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1)[:37, :53]
    out = blocks.copy()
    out[10:30, 20:45] = 255 - out[10:30, 20:45]
    pairs["blocks_odd"] = (out, np.ascontiguousarray(blocks))
    gt = rng.integers(0, 6, (21, 33, 3), dtype=np.uint8)
    pairs["dark"] = (np.clip(gt.astype(np.int32) + rng.integers(-1, 2, gt.shape), 0, 255).astype(np.uint8), gt)
    return pairs


def main():
    ref = import_reference_metrics()
    data, names = {}, []
    for name, (out, gt) in frame_pairs().items():
        vals = []
        for b in (0, BORDER):
            o, g = (out, gt) if b == 0 else (out[b:-b, b:-b], gt[b:-b, b:-b])
            oy, gy = _rgb_to_y(o), _rgb_to_y(g)
            vals += [ref.calculate_psnr(out, gt, border=b), ref.calculate_psnr(_rgb_to_y(out), _rgb_to_y(gt), border=b),
                     ref.structural_similarity(o, g), ref.structural_similarity(oy, gy)]
        data[name + "/out"], data[name + "/gt"] = out, gt
        data[name + "/values"] = np.array(vals, dtype=np.float64)
        names.append(name)
        print(name, out.shape, vals)
    meta = {
        "pairs": names, "border": BORDER,
        "values": "[psnr, psnr_y, ssim, ssim_y] of the frames, then the same four of the frames cut by `border` pixels on every side",
        "source": "calculate_psnr / structural_similarity of the reference's utils/metrics.py, imported unmodified",
        "restated": "cv2.getGaussianKernel and cv2.filter2D (float64 correlation, scipy.ndimage.correlate) and scikit-image's "
                    "rgb2ycbcr(uint8)[..., 0] = (rgb / 255) @ [65.481, 128.553, 24.966] + 16 are restated by tools/gen_metrics_golden.py: "
                    "neither package is installed where the fixture is built",
    }
    data["meta"] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "metrics_frames.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
