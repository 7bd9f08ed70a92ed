"""Cases, inputs and bounds shared by tests/test_ltam_max_ref.py (CPU) and tests/test_ltam_max_kernels_gpu.py.  Plain module.

Geometries: those of tests/traj_cases.py LTAM (window fields ignored: the max mode has no windows) plus the cases below -- a 1 x 1 map, odd maps,
partial tiles, two table-route cases (t = 33, 40) and a clip whose key-frame 1 DUPLICATES key-frame 0 with other values (exact ties everywhere: the
earlier frame must win).  Inputs come from traj_cases.ltam_inputs / ltam_locations.

Bounds, per element, in the form of traj_cases.bound: KAPPA[kind] * 2^-24 * S (+ 2^-8 |reference| on the bf16-stored out and dq), S = max |vals| for
out, 1 for score, the tensor's max for dq, the sum of |addends| for dk and dv (down to the scalar products of the two dot products inside, see
tests/ltam_max_ref.py).  KAPPA is four times the worst ratio measured over this case list on
the MI355X, both dtypes, rounded up (MEASURED beside it); every fp32 bound is asserted to stay under traj_cases.CEILING (2e-5 forward, 2e-4 gradients).

TAU = 2e-5 is that forward ceiling: a kernel score may differ from the reference's by less, so where two key-frames' reference scores lie closer
than TAU the kernel may pick either; elsewhere its index must be the reference's first maximum.  NEAR_TIE_CAP bounds the share of such (pixel, head)
pairs per case (asserted on the CPU by tests/test_ltam_max_ref.py)."""
import torch

from tests import ltam_max_ref as MR
from tests import traj_cases as TC

Ltam = TC.Ltam
ADDED = [
    Ltam("1x1-c16-t3-identity", 1, 1, 1, 16, 1, 1, 3, "identity"),
    Ltam("3x5-c32-t4-frac", 2, 3, 5, 32, 1, 1, 4, "frac"),
    Ltam("9x7-c144-t7-int", 1, 9, 7, 144, 1, 1, 7, "int"),
    Ltam("8x8-c16-t40-frac", 1, 8, 8, 16, 1, 1, 40, "frac"),
    Ltam("9x17-c112-t33-int", 1, 9, 17, 112, 1, 1, 33, "int"),
    Ltam("10x12-c32-t3-dup", 1, 10, 12, 32, 1, 1, 3, "identity"),
]
CASES = list(TC.LTAM) + ADDED
BY_ID = {g.id: g for g in CASES}
BOTH_ROUTES = "16x8-c16-t17-int"  # 17 key-frames through the argument route AND the table route: the same bits
HEADS = TC.HEADS
TAU = 2e-5
NEAR_TIE_CAP = 0.01

U, BF = TC.U, TC.BF
# worst |kernel - reference| / (2^-24 S) over the whole case list, both dtypes, on the MI355X; KAPPA = 4 x MEASURED, rounded up
MEASURED = dict(score=1.604, out=0.607, dq=4.044, dk=6.608, dv=3.835)
KAPPA = dict(score=7.0, out=3.0, dq=17.0, dk=27.0, dv=16.0)
CEILING = dict(score=2e-5 / U, out=2e-5 / U, dq=2e-4 / U, dk=2e-4 / U, dv=2e-4 / U)
ROUNDED = ("out", "dq")


def bound(kind, S, ref, dtype):
    b = KAPPA[kind] * U * S
    if dtype == torch.bfloat16 and kind in ROUNDED:
        b = b + BF * ref.abs()
    return b


def route(g):
    return "args" if g.t <= 32 else "table"


def inputs(g, dtype):
    """q, keys, vals, loc, dout: values rounded to dtype (float64), loc float32."""
    q, keys, vals, loc, _, _, dout = TC.ltam_inputs(g, dtype)
    if g.id.endswith("-dup"):  # key-frame 1 = key-frame 0 (identity locations: the same source row), other values
        keys[1] = keys[0].clone()
    return q, keys, vals, loc, dout


def near_ties(table, tau=TAU):
    """table (n,h,w,t,heads) reference scores -> bool (n,h,w,heads): some key-frame lies strictly below the maximum by less than tau."""
    gap = table.max(dim=3, keepdim=True).values - table
    return ((gap > 0) & (gap < tau)).any(dim=3)


def allowed(table, tau=TAU):
    """bool (n,h,w,t,heads): the key-frames within tau of the maximum (the set E)."""
    return (table.max(dim=3, keepdim=True).values - table) < tau


_cache = {}


def reference(g, dtype):
    """Inputs, the fp64 forward (with the score table), the fp64 backward at the reference's own selection and its scales.  Computed once."""
    key = (g.id, dtype)
    if key not in _cache:
        q, keys, vals, loc, dout = inputs(g, dtype)
        out, idx, score, table = MR.forward(q, keys, vals, loc, HEADS)
        dq, dk, dv, sc = MR.backward(q, keys, vals, loc, idx, dout, HEADS, with_scales=True)
        _cache[key] = dict(inp=(q, keys, vals, loc, dout), out=out, idx=idx, score=score, table=table, dq=dq, dk=dk, dv=dv, sc=sc,
                           vmax=max(float(v.abs().max()) for v in vals))
    return _cache[key]
