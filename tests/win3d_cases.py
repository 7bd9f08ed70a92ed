"""Geometries, inputs, error metrics and bounds shared by tests/test_win3d_ref.py (CPU) and tests/test_win3d_gpu.py.  Plain module.

A geometry is (id, B, D, H, W, C, heads, wt, shift, biased, routes, cls).  routes: which kernel / dtype routes meet the fp64 reference on
it, M = MFMA kernels on bf16, V = VALU kernel on bf16, F = VALU kernel on fp32.  cls: the class whose members must together make every
wrong variant of the reference visible (tests/test_win3d_ref.py)."""
import collections

import torch

from oracle import recipe as R
from tests.win3d_ref import NAMES, reference_all

Geom = collections.namedtuple("Geom", "id B D H W C heads wt shift biased routes cls")

GEOMS = [
    # ---- no shift, no padding
    Geom("d18-wt4-16x16-noshift", 1, 4, 16, 16, 144, 8, 4, (0, 0, 0), True, "MVF", "plain"),
    Geom("d28-wt8-c448h16-onewindow", 1, 8, 8, 8, 448, 16, 8, (0, 0, 0), True, "MF", "plain"),
    Geom("d64-wt4-noshift", 1, 4, 8, 16, 128, 2, 4, (0, 0, 0), True, "V", "plain"),
    # ---- no shift, padded
    Geom("d8-wt2-20x20-pad-noshift", 1, 2, 20, 20, 32, 4, 2, (0, 0, 0), True, "MF", "padded"),
    Geom("d36-wt2-D3x13x9-pad-noshift", 2, 3, 13, 9, 144, 4, 2, (0, 0, 0), True, "VF", "padded"),
    # ---- shifted, no padding
    Geom("d18-wt4-16x16-shift244", 1, 4, 16, 16, 144, 8, 4, (2, 4, 4), True, "MVF", "shifted"),
    Geom("d16-wt8-8x16-shift444", 1, 8, 8, 16, 64, 4, 8, (4, 4, 4), True, "MV", "shifted"),
    Geom("d18-wt4-train_swin-4x8x64x64", 4, 8, 64, 64, 144, 8, 4, (2, 4, 4), True, "M", "big"),
    # ---- one shifted dimension each (the region-2 branch of the other two)
    Geom("d8-wt2-shiftD", 1, 4, 16, 13, 32, 4, 2, (1, 0, 0), True, "MF", "oneshift"),
    Geom("d8-wt2-shiftH", 1, 4, 13, 16, 32, 4, 2, (0, 4, 0), True, "MV", "oneshift"),
    Geom("d8-wt2-shiftW", 1, 4, 16, 13, 32, 4, 2, (0, 0, 4), True, "M", "oneshift"),
    Geom("d28-wt8-c448h16-shiftD", 1, 16, 8, 8, 448, 16, 8, (4, 0, 0), True, "M", "oneshift"),
    Geom("d16-wt4-shiftD-8x8", 1, 8, 8, 8, 64, 4, 4, (2, 0, 0), True, "M", "oneshift"),
    # ---- shifted, pad == shift (the suite's earlier cases, kept): with wt > 2 the roll puts the padded rows into a mask slab of their own
    Geom("d4-wt2-D5-padeqshift", 2, 5, 8, 16, 32, 8, 2, (1, 4, 4), True, "MV", "shiftpad"),
    Geom("d8-wt2-20x12-padeqshift", 1, 2, 20, 12, 32, 4, 2, (1, 4, 4), True, "MF", "shiftpad"),
    Geom("d24-wt6-8x8-shift344", 1, 6, 8, 8, 48, 2, 6, (3, 4, 4), True, "M", "shifted"),
    Geom("d28-wt6-20x12-padeqshift", 1, 6, 20, 12, 112, 4, 6, (3, 4, 4), True, "M", "shiftpad"),
    # ---- shifted, padding the mask does not isolate (H, W remainders not in {0, 4}; D padding != sd)
    Geom("d32-wt4-B2-D5x23x13-win2x3x2", 2, 5, 23, 13, 64, 2, 4, (2, 4, 4), True, "MV", "shiftpad"),
    Geom("d18-wt4-D6x13x9", 1, 6, 13, 9, 144, 8, 4, (2, 4, 4), True, "MVF", "shiftpad"),
    Geom("d28-wt6-D7x13x9", 1, 7, 13, 9, 112, 4, 6, (3, 4, 4), True, "MF", "shiftpad"),
    Geom("d16-wt8-D9x9x8", 1, 9, 9, 8, 64, 4, 8, (4, 4, 4), True, "M", "shiftpad"),
    Geom("d36-wt2-13x9", 1, 4, 13, 9, 144, 4, 2, (1, 4, 4), True, "VF", "shiftpad"),
    Geom("d36-wt6-D7x9x9", 1, 7, 9, 9, 144, 4, 6, (3, 4, 4), True, "V", "shiftpad"),
    Geom("d9-odd-wt2-B2-9x23", 2, 3, 9, 23, 36, 4, 2, (1, 4, 4), True, "V", "shiftpad"),
    Geom("d64-wt4-D5x9x8", 1, 5, 9, 8, 128, 2, 4, (2, 4, 4), True, "V", "shiftpad"),
    # ---- bias-free Linears: padded tokens are zeros, no bias gradients
    Geom("d32-wt4-B2-D5x23x13-nobias", 2, 5, 23, 13, 64, 2, 4, (2, 4, 4), False, "MV", "nobias"),
    Geom("d36-wt2-13x9-nobias", 1, 4, 13, 9, 144, 4, 2, (1, 4, 4), False, "VF", "nobias"),
    Geom("d18-wt4-16x20-nobias-noshift", 1, 4, 16, 20, 144, 8, 4, (0, 0, 0), False, "M", "nobias"),
]
BY_ID = {g.id: g for g in GEOMS}

ROUTES = {"M": (1, torch.bfloat16), "V": (0, torch.bfloat16), "F": (0, torch.float32)}


def isolated(g):
    """Padding == shift in H / W, none in D, wt > 2: after the roll the padded rows fill one mask slab alone, and every real query has keys of
    its own region, so it sees the padded ones at e^-100.  (wt = 2 does not isolate: the last temporal window's two slices are different
    regions along D, every logit there carries the same -100, and the padded keys weigh as much as the real ones.)"""
    ph, pw = -g.H % 8, -g.W % 8
    return g.wt > 2 and g.D % g.wt == 0 and ph + pw > 0 and all(p in (0, s) for p, s in ((ph, g.shift[1]), (pw, g.shift[2])))


def padded(g):
    return g.D % g.wt != 0 or g.H % 8 != 0 or g.W % 8 != 0


def mfma_expected(g, variant, dtype):
    """win3d_mfma_ok's rule (csrc/win3d.hip)."""
    d = g.C // g.heads
    return variant == 1 and dtype == torch.bfloat16 and d <= 32 and d % 2 == 0 and g.C % 2 == 0 and g.wt >= 2


def make_inputs(g, dtype):
    """q, kv, dout pre-rounded to `dtype` (kept as fp32 values); bq, bkv, table fp32 -- both sides start from these numbers."""
    rd = lambda t: t.to(dtype).float()
    shp = (g.B, g.D, g.H, g.W)
    q = rd(R.seeded(shp + (g.C,), 1300, 0.7))
    kv = rd(R.seeded(shp + (2 * g.C,), 1301, 0.7))
    bq = R.seeded((g.C,), 1302, 0.3) if g.biased else None
    bkv = R.seeded((2 * g.C,), 1303, 0.3) if g.biased else None
    table = R.seeded(((2 * g.wt - 1) * 225, g.heads), 1304, 0.5)
    dout = rd(R.seeded(shp + (g.C,), 1305))
    return q, kv, bq, bkv, table, dout


# Stated ceilings: no bound below is ever looser than these, whatever the floor says.
CAP = {torch.bfloat16: dict(out=2e-2, grad=3e-2), torch.float32: dict(out=1e-4, grad=1e-4)}
MARGIN = 4.0
# Smallest floor a tensor can have, from the number formats alone.  Every kernel accumulates in fp32 (unit roundoff u = 2^-24) and takes
# exp as exp2(x * log2 e) with the product rounded to fp32, |x| u per probability (8 u at a logit spread of 8); sums of a few hundred
# such terms: 16 u = 2^-20 of the tensor's scale.  It matters where the measured floor is (nearly) zero: fp32 tensors, and gradients
# that are ~0 because every contribution carries e^-100.
EPS_REL = 2.0 ** -20
# lse in nats: a logit that carries -100 lies in [64, 128), where fp32 numbers are 2^-17 apart; it is rounded there once when the mask
# is added and once more as max + log(sum).  2 spacings = 2^-16.
EPS_LSE = 2.0 ** -16


def scales(ref):
    """Per tensor (max-norm scale, L2 scale).  dbkv: floored at 1e-3 of dkv's (its own is ~0 when the mask isolates every padded token);
    everything else: the tensor's own max / norm (dtable has thinly populated ends: hence the second, L2, metric)."""
    sc = {}
    for n in NAMES:
        t = ref[n]
        if t is None or n in ("lse", "dbq"):
            continue
        mx, l2 = float(t.abs().max()), float(t.norm())
        if n == "dbkv":
            fl = 1e-3 * float(ref["dkv"].abs().max())
            mx, l2 = max(mx, fl), max(l2, fl * t.numel() ** 0.5)
        sc[n] = (mx, l2)
    return sc


def errors(got, ref, sc):
    """{tensor: (max |got - ref| / max-norm scale, ||got - ref|| / L2 scale)}; lse: (max |got - ref| in nats, the same)."""
    e = {}
    for n in NAMES:
        if ref[n] is None or n == "dbq":
            continue
        diff = got[n].double().reshape(ref[n].shape) - ref[n]
        if n == "lse":
            e[n] = (float(diff.abs().max()),) * 2
        else:
            e[n] = (float(diff.abs().max()) / sc[n][0], float(diff.norm()) / sc[n][1])
    return e


def bounds(floor, dtype):
    """margin x floor per tensor and metric, the floor never below what the formats give, the bound never above the stated ceiling."""
    b = {}
    for n, (fm, fl) in floor.items():
        if n == "lse":
            b[n] = (MARGIN * max(fm, EPS_LSE),) * 2
        else:
            cap = CAP[dtype]["out" if n == "out" else "grad"]
            b[n] = (min(MARGIN * max(fm, EPS_REL), cap), min(MARGIN * max(fl, EPS_REL), cap))
    return b


_cache = {}


def reference_and_bounds(g, dtype):
    """fp64 reference of geometry g on inputs pre-rounded to dtype, its scales, the rounding floor (bf16: |reference - reference with the
    documented roundings|; fp32: |reference - reference evaluated in fp32|) and the bounds that follow.  Cached per (geometry, dtype)."""
    key = (g.id, dtype)
    if key in _cache:
        return _cache[key]
    inp = make_inputs(g, dtype)
    kw = dict(emulate=torch.bfloat16) if dtype == torch.bfloat16 else dict(dtype=torch.float32)
    if g.cls == "big":  # windows never span clips: one clip at a time keeps the fp64 autograd graph small
        ref, low = _per_clip(g, inp), _per_clip(g, inp, **kw)
    else:
        ref, low = reference_all(*inp, g.heads, g.wt, g.shift), reference_all(*inp, g.heads, g.wt, g.shift, **kw)
    sc = scales(ref)
    floor = errors(low, ref, sc)
    res = (inp, ref, sc, floor, bounds(floor, dtype))
    if g.cls != "big":
        _cache[key] = res
    return res


def _per_clip(g, inp, **kw):
    q, kv, bq, bkv, table, dout = inp
    parts = [reference_all(q[b:b + 1], kv[b:b + 1], bq, bkv, table, dout[b:b + 1], g.heads, g.wt, g.shift, **kw) for b in range(g.B)]
    res = {n: torch.cat([p[n] for p in parts], 0) for n in ("out", "lse", "dq", "dkv")}  # (lse: windows are clip-major)
    for n in ("dtable", "dbq", "dbkv"):
        res[n] = None if parts[0][n] is None else sum(p[n] for p in parts)
    return res
