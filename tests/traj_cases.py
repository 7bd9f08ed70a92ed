"""Cases, inputs and bounds shared by tests/test_traj_ref.py (CPU) and tests/test_traj_ops_gpu.py.  Plain module.

Bounds, per element: the fp32 bound is KAPPA[kind] * 2^-24 * S with S the element's natural scale
    out: max |vals|;  lse: max(1, |lse|);  dq: the tensor's max |reference|;
    dk / dv / drpe / dx / dflow: the sum of the |addends| the reference summed into the element (tests/traj_ref.py returns it);
bf16 adds ONE rounding, 2^-8 |reference|, on the tensors that are stored in bf16 (out, dq, the warp's out and dx) and nothing on the fp32
sums (dk, dv, drpe, dflow).  KAPPA is four times the worst ratio measured over this case list on the MI355X; CEILING is what the fp32 bounds may never exceed: the whole-tensor tolerances of tests/test_traj_kernels_gpu.py."""
import collections

import torch

from tests import traj_ref as TR

U = 2.0 ** -24
BF = 2.0 ** -8
# worst |kernel - reference| / (2^-24 S) measured over the whole case list, both dtypes, on the MI355X; KAPPA = 4 x MEASURED, rounded up
MEASURED = dict(out=1.79, lse=4.13, dq=5.70, dk=41.27, dv=7.29, drpe=7.03, wout=1.47, dx=4.82, dflow=2.21)
KAPPA = dict(out=8.0, lse=17.0, dq=23.0, dk=166.0, dv=30.0, drpe=29.0, wout=6.0, dx=20.0, dflow=9.0)
# today's fp32 tolerances, as multiples of 2^-24 of the tensor's scale: 2e-5 forward, 2e-4 gradients, 1e-3 dflow
CEILING = dict(out=2e-5 / U, lse=2e-5 / U, dq=2e-4 / U, dk=2e-4 / U, dv=2e-4 / U, drpe=2e-4 / U, wout=1e-5 / U, dx=1e-4 / U, dflow=1e-3 / U)
ROUNDED = ("out", "dq", "wout", "dx")  # stored in the tensor dtype: one bf16 rounding on top


def bound(kind, S, ref, dtype):
    """Per-element bound for a tensor of `kind`: S its scale (tensor or number), ref the fp64 reference."""
    b = KAPPA[kind] * U * S
    if dtype == torch.bfloat16 and kind in ROUNDED:
        b = b + BF * ref.abs()
    return b


def rnd(t, dtype):
    """t rounded to dtype, as float64: the value both sides start from."""
    return t.to(dtype).double()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0):
    return scale * torch.randn(tuple(shape), generator=_gen(seed))


# ------------------------------------------------------------------------------------------------------------------ trajectory attention
Ltam = collections.namedtuple("Ltam", "id n h w c wh ww t fam")

LTAM = [
    Ltam("2x2-c16-t1-identity", 1, 2, 2, 16, 2, 2, 1, "identity"),
    Ltam("8x8-c32-t2-int", 2, 8, 8, 32, 2, 2, 2, "int"),
    Ltam("10x12-c112-t7-frac", 1, 10, 12, 112, 2, 2, 7, "frac"),
    Ltam("16x8-c112-t2-int", 2, 16, 8, 112, 2, 2, 2, "int"),
    Ltam("18x6-c144-t2-oneframe-out", 1, 18, 6, 144, 2, 2, 2, "frameout"),
    Ltam("10x12-c144-t1-frac", 2, 10, 12, 144, 2, 2, 1, "frac"),
    Ltam("16x8-c16-t17-int", 2, 16, 8, 16, 2, 2, 17, "int"),
    Ltam("8x8-c16-t32-frac", 1, 8, 8, 16, 2, 2, 32, "frac"),
    Ltam("10x12-c32-t2-onepixel", 1, 10, 12, 32, 2, 2, 2, "onepixel"),
    Ltam("18x6-c16-t2-window-on-one-pixel", 1, 18, 6, 16, 2, 2, 2, "winpixel"),
    Ltam("8x8-c16-w1x1-t2-int", 1, 8, 8, 16, 1, 1, 2, "int"),
    Ltam("10x12-c32-w2x4-t2-int", 1, 10, 12, 32, 2, 4, 2, "int"),
    Ltam("16x8-c16-w4x2-t7-frac", 1, 16, 8, 16, 4, 2, 7, "frac"),
    Ltam("16x8-c32-w4x4-t2-int", 2, 16, 8, 32, 4, 4, 2, "int"),
    Ltam("16x8-c16-w1x8-t2-frac", 1, 16, 8, 16, 1, 8, 2, "frac"),
    Ltam("16x8-c32-w8x1-t2-int", 1, 16, 8, 32, 8, 1, 2, "int"),
    Ltam("18x6-c32-w2x2-t7-identity", 1, 18, 6, 32, 2, 2, 7, "identity"),
]
LTAM_BY_ID = {g.id: g for g in LTAM}
HEADS = 4


def ltam_locations(g, seed=2100):
    """(n, 2t, h, w) float32 tracked positions, x then y per key-frame, of the case's family."""
    n, t, h, w = g.n, g.t, g.h, g.w
    gen = _gen(seed)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    ident = torch.stack([xs, ys], 0)[None, None].expand(n, t, 2, h, w).clone()
    if g.fam == "identity":
        loc = ident
    elif g.fam in ("int", "frameout"):  # integers in [-2, size + 2): about a third of the rows / columns of the range lie outside the map
        x = torch.randint(-2, w + 2, (n, t, 1, h, w), generator=gen).float()
        y = torch.randint(-2, h + 2, (n, t, 1, h, w), generator=gen).float()
        loc = torch.cat([x, y], 2)
        if g.fam == "frameout":  # the OLDEST key-frame: every position outside (left of / below the map)
            loc[:, 0, 0] = -3.0 - xs
            loc[:, 0, 1] = h + 1.0 + ys
    elif g.fam == "frac":  # a third exact .5 ties (both neighbours' parities occur), a third 2^-18 beside a tie, a third anywhere
        base_x = torch.randint(-1, w, (n, t, h, w), generator=gen).float()
        base_y = torch.randint(-1, h, (n, t, h, w), generator=gen).float()
        kind = torch.randint(0, 3, (n, t, h, w), generator=gen)
        off = torch.rand((n, t, 2, h, w), generator=gen)
        near = 0.5 + (torch.randint(0, 2, (n, t, 2, h, w), generator=gen).float() * 2 - 1) * 2.0 ** -18
        fx = torch.where(kind == 0, torch.full_like(base_x, 0.5), torch.where(kind == 1, near[:, :, 0], off[:, :, 0]))
        fy = torch.where(kind == 0, torch.full_like(base_y, 0.5), torch.where(kind == 1, near[:, :, 1], off[:, :, 1]))
        loc = torch.stack([base_x + fx, base_y + fy], 2)
    elif g.fam == "onepixel":  # every query of an image gathers the same source row: h * w * wq additions into one row
        loc = torch.zeros((n, t, 2, h, w))
        for j in range(t):
            loc[:, j, 0] = float((3 + 5 * j) % w)
            loc[:, j, 1] = float((h - 2 - 3 * j) % h)
    elif g.fam == "winpixel":  # the positions of one window share one source pixel (its top-left one, shifted by the key-frame)
        wx, wy = (xs // g.ww) * g.ww, (ys // g.wh) * g.wh
        loc = torch.stack([torch.stack([(wx + j) % w, (wy + 2 * j) % h], 0) for j in range(t)], 0)[None].expand(n, t, 2, h, w).clone()
    else:
        raise ValueError(g.fam)
    return loc.reshape(n, 2 * t, h, w).contiguous()


def ltam_inputs(g, dtype, zero_rows=False):
    """q, keys, vals, dout rounded to dtype (float64 values); loc, rpe, decay float32.  decay per head in [0.9, 0.999]: powers up to 32 matter.
    zero_rows: query row (0, 1, 2) is zero, and so is source row (0, 3, 1) of key-frame 0, which locations (0, 0..3) of that key-frame gather."""
    shp = (g.n, g.h, g.w, g.c)
    q = rnd(randn(shp, 2000), dtype)
    keys = [rnd(randn(shp, 2010 + j), dtype) for j in range(g.t)]
    vals = [rnd(randn(shp, 2050 + j), dtype) for j in range(g.t)]
    dout = rnd(randn(shp, 2090), dtype)
    wq = g.wh * g.ww
    rpe = randn((HEADS, wq, wq), 2091, 0.5)
    decay = torch.tensor([0.9, 0.95, 0.98, 0.999], dtype=torch.float32)
    loc = ltam_locations(g)
    if zero_rows:
        q[0, 1, 2] = 0
        keys[0][0, 3, 1] = 0
        loc[0, 0, 0, :4] = 1.0
        loc[0, 1, 0, :4] = 3.0
    return q, keys, vals, loc, rpe, decay, dout


# ------------------------------------------------------------------------------------------------------------------ flow warp
Warp = collections.namedtuple("Warp", "id n h w c dtype fam")
_B, _F = torch.bfloat16, torch.float32

WARP = [
    Warp("bf16-1x1-c8-random", 2, 1, 1, 8, _B, "random"),
    Warp("bf16-1x9-c8-half", 1, 1, 9, 8, _B, "half"),
    Warp("bf16-9x1-c136-half", 1, 9, 1, 136, _B, "half"),
    Warp("bf16-2x2-c8-onborder", 2, 2, 2, 8, _B, "onborder"),
    Warp("bf16-9x7-c112-random", 1, 9, 7, 112, _B, "random"),
    Warp("bf16-9x7-c128-int", 1, 9, 7, 128, _B, "int"),
    Warp("bf16-9x7-c136-random", 2, 9, 7, 136, _B, "random"),
    Warp("bf16-16x24-c144-clamped", 1, 16, 24, 144, _B, "clamped"),
    Warp("bf16-9x7-c256-onborder", 1, 9, 7, 256, _B, "onborder"),
    Warp("bf16-9x7-c264-half", 1, 9, 7, 264, _B, "half"),
    Warp("bf16-16x24-c264-huge", 1, 16, 24, 264, _B, "huge"),
    Warp("bf16-16x24-c8-random", 2, 16, 24, 8, _B, "random"),
    Warp("fp32-1x1-c4-random", 2, 1, 1, 4, _F, "random"),
    Warp("fp32-1x9-c4-int", 1, 1, 9, 4, _F, "int"),
    Warp("fp32-9x1-c68-random", 1, 9, 1, 68, _F, "random"),
    Warp("fp32-2x2-c68-half", 2, 2, 2, 68, _F, "half"),
    Warp("fp32-9x7-c68-random", 1, 9, 7, 68, _F, "random"),
    Warp("fp32-9x7-c132-onborder", 1, 9, 7, 132, _F, "onborder"),
    Warp("fp32-9x7-c4-half", 2, 9, 7, 4, _F, "half"),
    Warp("fp32-16x24-c144-random", 2, 16, 24, 144, _F, "random"),
    Warp("fp32-16x24-c4-huge", 1, 16, 24, 4, _F, "huge"),
    Warp("fp32-16x24-c68-clamped", 1, 16, 24, 68, _F, "clamped"),
    Warp("fp32-9x7-c132-int", 1, 9, 7, 132, _F, "int"),
]
WARP_BY_ID = {g.id: g for g in WARP}
WARP_MAPS = [(1, 1), (1, 9), (9, 1), (2, 2), (9, 7), (16, 24)]


def warp_flow(fam, n, h, w, seed=2200):
    """(n, h, w, 2) float32 pixel offsets of a family."""
    gen = _gen(seed)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    if fam == "zero":
        return torch.zeros((n, h, w, 2))
    if fam == "random":  # incl. far out-of-range samples
        return 3.0 * torch.randn((n, h, w, 2), generator=gen)
    if fam == "int":  # whole-pixel shifts, a good part of them past the borders
        return torch.randint(-3, 4, (n, h, w, 2), generator=gen).float()
    if fam == "half":  # whole pixels + exactly .5
        return torch.randint(-2, 3, (n, h, w, 2), generator=gen).float() + 0.5
    if fam == "onborder":  # half of the pixels sample EXACTLY column W-1 / 0 or row H-1 / 0; the others anywhere inside
        f = torch.rand((n, h, w, 2), generator=gen)
        f[..., 0] = f[..., 0] * max(w - 1, 0) - xs
        f[..., 1] = f[..., 1] * max(h - 1, 0) - ys
        pick = torch.randint(0, 6, (n, h, w), generator=gen)
        f[..., 0] = torch.where(pick == 0, (w - 1) - xs, torch.where(pick == 1, -xs, f[..., 0]))
        f[..., 1] = torch.where(pick == 2, (h - 1) - ys, torch.where(pick == 3, -ys, f[..., 1]))
        return f.contiguous()
    if fam == "huge":
        return (torch.randint(0, 2, (n, h, w, 2), generator=gen).float() * 2 - 1) * 1e4
    if fam == "clamped":  # whole blocks of output pixels clamp onto column 0 / row 0: a border pixel collects dozens of contributions
        f = torch.randn((n, h, w, 2), generator=gen)
        f[:, :, : w // 2, 0] -= 60.0
        f[:, : h // 3, :, 1] -= 40.0
        return f
    raise ValueError(fam)


def warp_inputs(g):
    """x, dy rounded to the case's dtype (float64 values), flow float32.  clamped: same-sign dy, so the border sums grow."""
    shp = (g.n, g.h, g.w, g.c)
    x = rnd(randn(shp, 2201), g.dtype)
    dy = randn(shp, 2202)
    if g.fam == "clamped":
        dy = dy.abs() + 0.5
    return x, warp_flow(g.fam, g.n, g.h, g.w), rnd(dy, g.dtype)


# ------------------------------------------------------------------------------------------------------------------ location advection
Near = collections.namedtuple("Near", "id n k2 h w fam")
NEAREST = [Near(f"{h}x{w}-k{k2}-{fam}", n, k2, h, w, fam)
           for (n, k2, h, w) in [(1, 2, 1, 9), (2, 64, 9, 1), (1, 2, 1, 1), (2, 2, 9, 7), (1, 64, 16, 24), (1, 2, 20, 28)]
           for fam in ("zero", "int", "half", "random", "huge", "onborder")]


def nearest_inputs(g):
    loc = randn((g.n, g.k2, g.h, g.w), 2301, 10.0)
    return loc, warp_flow(g.fam, g.n, g.h, g.w, seed=2302)


# ------------------------------------------------------------------------------------------------------------------ references, computed once
_ltam_cache = {}


def ltam_reference(g, dtype, zero_rows=False):
    """Inputs, the fp64 forward, the rounded out / lse the backward is handed, the fp64 backward from them and its scales.  Computed once."""
    key = (g.id, dtype, zero_rows)
    if key not in _ltam_cache:
        q, keys, vals, loc, rpe, decay, dout = ltam_inputs(g, dtype, zero_rows)
        scale = (g.c // HEADS) ** -0.5
        out, lse = TR.ltam_reference(q, keys, vals, loc, rpe, decay, g.wh, g.ww, scale)
        out_r, lse_r = rnd(out, dtype), lse.float().double()
        dq, dk, dv, drpe, sc = TR.ltam_reference_backward(q, keys, vals, loc, rpe, decay, g.wh, g.ww, scale, out_r, dout, lse=lse_r, with_scales=True)
        vmax = max(float(v.abs().max()) for v in vals)
        _ltam_cache[key] = dict(inp=(q, keys, vals, loc, rpe, decay, dout), scale=scale, out=out, lse=lse, out_r=out_r, lse_r=lse_r, dq=dq, dk=dk, dv=dv,
                                drpe=drpe, sc=sc, vmax=vmax)
    return _ltam_cache[key]


_warp_cache = {}


def warp_reference(g):
    if g.id not in _warp_cache:
        x, flow, dy = warp_inputs(g)
        out = TR.warp_bilinear_reference(x, flow)
        dx, df, sc = TR.warp_bilinear_reference_backward(x, flow, dy, with_scales=True)
        _warp_cache[g.id] = dict(x=x, flow=flow, dy=dy, out=out, dx=dx, dflow=df, sc=sc)
    return _warp_cache[g.id]
