"""Float64 numpy restatement of the reference's antialiased bicubic downscale (utils/image_resize.py imresize_np(img, 1 / s, True)) for an
integer factor s.  TEST INFRASTRUCTURE: the yardstick vmg_bicubic_down is held to; tests/test_lr_ref.py holds this file to the
reference's own outputs (tests/golden/lr_bicubic.npz).

Per axis: the output length is n / s.  Output sample o (0-based) sits at the 1-based input coordinate u = (o + 1) s + 0.5 (1 - s) and
reads the P = 4s + 2 samples j = floor(u - 2s) + p, p = 0 .. P-1, each with the weight k((u - j) / s) divided by the sum of the P
weights; k is Keys' cubic with a = -0.5.  A sample outside the input is mirrored with edge repeat (1-based 0 -> 1, -1 -> 2, n+1 -> n).
The reference reaches the same values through padded copies of the image, in float32.
"""
import math

import numpy as np


def cubic(x):
    x = abs(x)
    if x <= 1:
        return 1.5 * x ** 3 - 2.5 * x ** 2 + 1
    if x <= 2:
        return -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2
    return 0.0


def weight_table(s):
    """(first, w): output sample o reads the 0-based input samples o*s + first + p with the normalised weights w[p], p = 0 .. 4s+1.
    For an integer s the table is the same for every o."""
    u = s + 0.5 * (1 - s)                    # o = 0
    left = math.floor(u - 2 * s)             # 1-based
    w = np.array([cubic((u - (left + p)) / s) for p in range(4 * s + 2)], dtype=np.float64)
    return left - 1, w / w.sum()


def mirror(i, n):
    """0-based index of sample i of a length-n axis: -1 -> 0, -2 -> 1, n -> n-1, n+1 -> n-2."""
    if i < 0:
        i = -i - 1
    if i >= n:
        i = 2 * n - 1 - i
    assert 0 <= i < n, "the axis is shorter than the filter's support"
    return i


def axis_matrix(n, s):
    """(n / s, n) float64: row o holds the weights of output sample o on the input samples (mirrored taps add up)."""
    assert n % s == 0 and n >= 4 * s
    first, w = weight_table(s)
    m = np.zeros((n // s, n), dtype=np.float64)
    for o in range(n // s):
        for p, wp in enumerate(w):
            if wp != 0.0:
                m[o, mirror(o * s + first + p, n)] += wp
    return m


def bicubic_down(img, s):
    """img: (H, W) or (H, W, C) of any real dtype, values as they are (uint8 frames: 0..255).  Returns float64 (H/s, W/s[, C]), not rounded:
    rows first, then columns, as the reference orders its two passes."""
    x = np.asarray(img, dtype=np.float64)
    mh, mw = axis_matrix(x.shape[0], s), axis_matrix(x.shape[1], s)
    rows = np.tensordot(mh, x, axes=(1, 0))                      # (h, W[, C])
    out = np.tensordot(rows, mw, axes=(1, 1))                    # (h[, C], w)
    return np.moveaxis(out, -1, 1) if x.ndim == 3 else out


def to_uint8(v):
    """What cv2.imwrite stores: round half to even, then saturate."""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def half_integer_distance(v):
    """|v - nearest half-integer| per value: how far v is from a rounding tie."""
    return np.abs(v - np.floor(v) - 0.5)
