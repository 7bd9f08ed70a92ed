"""The kernels of csrc/tab_ops.hip (group_reduce, group_reduce3, tab_elementwise, maxpool) and avgpool2 (csrc/spynet.hip) on their own,
against the fp64 reference of tests/tab_ops_ref.py (itself checked on the CPU by tests/test_tab_ops_ref.py).

Inputs are made on the CPU, rounded to the tested dtype, and the reference sees the rounded values.  Where the arithmetic is exact in
fp32 (integer-valued inputs, maxima, copies) the comparison is torch.equal; elsewhere the bound is a rounding-error bound derived from
the number formats and written next to the assertion -- none of them is a measured figure."""
import functools

import numpy as np
import pytest
import torch

from tests import tab_ops_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
U = 2.0 ** -24      # unit roundoff of fp32
UB = 2.0 ** -8      # unit roundoff of bf16: the final round-to-nearest of a bf16 output
DT_ID = {F32: "fp32", BF16: "bf16"}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, seed):
    """Integer values in {-4 .. 4} without 0 (exact in bf16 and fp32), as fp32."""
    g = _gen(seed)
    mag = torch.randint(1, 5, tuple(shape), generator=g, dtype=torch.int8)
    sign = torch.randint(0, 2, tuple(shape), generator=g, dtype=torch.int8) * 2 - 1
    return (mag * sign).float()


def normal(shape, seed, dtype, scale=1.0):
    """Seeded normal values rounded to `dtype`, as fp32 (which holds every bf16 value)."""
    return (scale * torch.randn(tuple(shape), generator=_gen(seed))).to(dtype).float()


def dev(t, dtype, offset=0):
    """The CPU tensor on the device in `dtype`; offset > 0: as a contiguous view `offset` elements into a larger buffer, which is not
    16-byte aligned (torch's allocations are)."""
    t = t.to(dtype)
    if not offset:
        out = t.cuda()
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.zeros(t.numel() + 16, dtype=dtype, device="cuda")
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def same(a, b):
    """torch.equal that takes NaN at the same place as equal."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ================================================================================================ reductions
# (G, R, C, element offset of the operands).  chunks = min(max(1, 1024 // G), max(1, R // 64)) blocks per group; threads per row tpr = C / VN,
# rows per block iteration rpb = 256 // tpr, VN = 8 (bf16) / 4 (fp32) channels per thread, VN = 2 when C is no multiple of that or a pointer is
# not 16-byte aligned.
REDUCE_CASES = [
    (1, 2119, 144, 0),     # chunks = 33: the final kernel's loop over chunks runs three times, uneven chunk bounds
    (3, 25605, 144, 0),    # chunks = 341, 1023 blocks
    (1, 65539, 8, 0),      # chunks = 1024; bf16: tpr = 1, rpb = 256
    (2000, 3, 16, 0),      # G > 1024, chunks = 1, fewer rows than rpb
    (4, 24, 64, 0),        # the multi-scale skip's GroupNorm
    (2, 360, 144, 0),      # the shape of the module tests
    (2, 70, 512, 0),       # tpr = 64 (bf16) / 128 (fp32)
    (2, 70, 2, 0), (2, 70, 6, 0), (2, 130, 150, 0),   # VN = 2
    (1, 70, 510, 0),       # VN = 2, tpr = 255, rpb = 1: one idle thread
    (1, 70, 512, 2),       # contiguous, not 16-byte aligned: VN = 2, tpr = 256
]
REDUCE3_CASES = [(2, 360, 144), (1, 2119, 144), (3, 25605, 144), (1, 65539, 8), (5, 70, 512), (2000, 3, 16)]
MODES = ("a", "a+b", "a+b+c3", "a*b", "a*a")


def _mode_args(mode, a, b, c):
    """(b, c3, mode) of the call; a*a passes the SAME tensor twice, as GroupNorm does."""
    return {"a": (None, None, 0), "a+b": (b, None, 0), "a+b+c3": (b, c, 0), "a*b": (b, None, 1), "a*a": (a, None, 1)}[mode]


def _case_id(c):
    return "x".join(str(v) for v in c[:3]) + ("+off%d" % c[3] if len(c) > 3 and c[3] else "")


@functools.lru_cache(maxsize=2)
def int_reduce_case(G, Rr, C):
    """Integer operands (a, b, c, d) of one shape and the fp64 references of the five modes and of group_reduce3 at scale 1, made once."""
    ops = [ints((G * Rr, C), 300 + i) for i in range(4)]
    refs = {m: R.group_reduce_ref(ops[0], G, *_mode_args(m, *ops[:3]), 1.0)[0] for m in MODES}
    refs["3"] = R.group_reduce3_ref(ops[0], ops[1], ops[2], ops[3], G, 1.0)[0]
    return ops, refs


@pytest.mark.parametrize("case,dtype", [(c, d) for c in REDUCE_CASES for d in DTYPES], ids=lambda v: DT_ID.get(v) or _case_id(v))
def test_group_reduce_exact_on_integers(case, dtype):
    """Terms are integers of magnitude <= 16 (a * b) and R * 16 < 2^24: every fp32 partial sum is an integer below 2^24, exact in any
    order, and scale 1 or 0.5 keeps it exact.  So the result IS the fp64 sum: a dropped, doubled or misplaced row or channel shows."""
    from vmg_amd import kernels as K
    G, Rr, C, off = case
    assert Rr * 16 < 2 ** 24
    ops, refs = int_reduce_case(G, Rr, C)
    a, b, c = (dev(t, dtype, off) for t in ops[:3])
    for mode in MODES:
        kb, kc, km = _mode_args(mode, a, b, c)
        for scale in (1.0, 0.5):
            got = K.group_reduce(a, G, b=kb, c3=kc, mode=km, scale=scale)
            assert got.dtype == F32 and got.shape == (G, C)
            want = (refs[mode] * scale).float()
            bad = (got.cpu() != want).nonzero()
            assert bad.numel() == 0, f"{mode} scale {scale}: {bad.shape[0]} of {want.numel()} wrong, first (g, c) = {bad[0].tolist()}"
    again = K.group_reduce(a, G, b=b, c3=c, mode=0, scale=0.5)
    assert torch.equal(again, K.group_reduce(a, G, b=b, c3=c, mode=0, scale=0.5))


@pytest.mark.parametrize("case,dtype", [(c, d) for c in REDUCE3_CASES for d in DTYPES], ids=lambda v: DT_ID.get(v) or _case_id(v))
def test_group_reduce3_exact_on_integers(case, dtype):
    from vmg_amd import kernels as K
    G, Rr, C = case
    assert Rr * 16 < 2 ** 24
    ops, refs = int_reduce_case(G, Rr, C)
    a, b0, b1, b2 = (dev(t, dtype) for t in ops)
    for scale in (1.0, 0.5):
        got = K.group_reduce3(a, b0, b1, b2, G, scale=scale)
        assert got.dtype == F32 and got.shape == (G, C, 3)
        want = (refs["3"] * scale).float()
        bad = (got.cpu() != want).nonzero()
        assert bad.numel() == 0, f"scale {scale}: {bad.shape[0]} of {want.numel()} wrong, first (g, c, k) = {bad[0].tolist()}"
    assert torch.equal(got, K.group_reduce3(a, b0, b1, b2, G, scale=0.5))


@functools.lru_cache(maxsize=2)
def real_reduce_case(G, Rr, C, dtype):
    return [normal((G * Rr, C), 320 + i, dtype) for i in range(4)]


REAL_CASES = [REDUCE_CASES[0], REDUCE_CASES[1], REDUCE_CASES[3], REDUCE_CASES[9]]


@pytest.mark.parametrize("case,dtype", [(c, d) for c in REAL_CASES for d in DTYPES], ids=lambda v: DT_ID.get(v) or _case_id(v))
def test_group_reduce_real_valued(case, dtype):
    """Normal inputs, scale = 1/R (the pooled mean).  Any fp32 summation of n terms, in any order, is off by at most (n - 1) u sum|x_i|,
    u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); one more rounding each for the product of mode 1 and for the scale:
    |got - ref| <= (n + 2) u scale sum_r |addend|, n = R, 2R or 3R addends by mode.  The reference gets the fp32 value of the scale."""
    from vmg_amd import kernels as K
    G, Rr, C, off = case
    ops = real_reduce_case(G, Rr, C, dtype)
    a, b, c = (dev(t, dtype, off) for t in ops[:3])
    scale = float(np.float32(1.0 / Rr))
    for mode in MODES:
        kb, kc, km = _mode_args(mode, a, b, c)
        rb, rc, _ = _mode_args(mode, *ops[:3])
        got = K.group_reduce(a, G, b=kb, c3=kc, mode=km, scale=scale).cpu().double()
        ref, mag = R.group_reduce_ref(ops[0], G, rb, rc, km, scale)
        n = Rr * {"a": 1, "a+b": 2, "a+b+c3": 3, "a*b": 1, "a*a": 1}[mode]
        err, bound = (got - ref).abs(), (n + 2) * U * mag
        print(f"{mode}: max err / bound = {float((err / bound).max()):.3g}")
        assert bool((err <= bound).all()), f"{mode}: {float((err / bound).max())} x the bound at {int((err / bound).argmax())}"


@pytest.mark.parametrize("case,dtype", [(c, d) for c in REDUCE3_CASES[:2] for d in DTYPES], ids=lambda v: DT_ID.get(v) or _case_id(v))
def test_group_reduce3_real_valued(case, dtype):
    """As above with n = R products per sum."""
    from vmg_amd import kernels as K
    G, Rr, C = case
    ops = real_reduce_case(G, Rr, C, dtype)
    scale = float(np.float32(1.0 / Rr))
    got = K.group_reduce3(*(dev(t, dtype) for t in ops), G, scale=scale).cpu().double()
    ref, mag = R.group_reduce3_ref(*ops, G, scale)
    err, bound = (got - ref).abs(), (Rr + 2) * U * mag
    print(f"max err / bound = {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())


# ================================================================================================ elementwise
EW_SHAPES = [(3, 37, 144), (1, 1, 8), (2, 5, 16)]
# name, op, s, OP_AFFINE2 with p1
EW_VARIANTS = [("ca_fwd", R.OP_CA_FWD, 0.7, False), ("ca_bwd", R.OP_CA_BWD, 0.7, False), ("mix_fwd", R.OP_MIX_FWD, 1.0, False),
               ("mix_bwd", R.OP_MIX_BWD, 1.0, False), ("gate_fwd", R.OP_GATE_FWD, 1.0, False), ("gate_bwd", R.OP_GATE_BWD, 1.0, False),
               ("affine2_relu", R.OP_AFFINE2, 1.0, False), ("affine2_relu_p1", R.OP_AFFINE2, 1.0, True), ("affine2", R.OP_AFFINE2, 0.0, False),
               ("affine2_p1", R.OP_AFFINE2, 0.0, True), ("scale", R.OP_SCALE, 0.7, False), ("gate_res_fwd", R.OP_GATE_RES_FWD, 0.75, False),
               ("gate_res_bwd", R.OP_GATE_RES_BWD, 0.75, False)]


def ew_inputs(op, G, Rr, C, dtype, s, with_p1=False, seed=500):
    """Operands of one op as CPU fp32 tensors holding `dtype` values, and its fp32 coefficients: normal, so distinct per (g, c, k) -- a wrong
    group or channel index reads a different number."""
    extra, ncoef, has_add, nout = R.OP_USES[op]
    names = ["p0"] + list(extra) + (["p1"] if with_p1 else [])
    kw = {n: normal((G * Rr, C), seed + i, dtype) for i, n in enumerate(names)}
    if ncoef:
        kw["coef"] = normal((G, C, ncoef) if ncoef > 1 else (G, C), seed + 10, F32)
    if has_add:
        kw["add"] = normal((G, C), seed + 11, F32)
    if dtype == BF16 and op in (R.OP_GATE_RES_FWD, R.OP_GATE_RES_BWD):
        # These two ops round an intermediate to bf16 by design.  The kernel's fp32 value of it (at most 7 roundings: within 16 u mag) and the
        # reference's fp64 value round to the same bf16 number unless a rounding tie lies between them: elements that close to a tie are drawn again.
        for attempt in range(8):
            v, m = R.gate_res_intermediate(op, kw["p0"], kw["p1"], kw["p2"], kw["coef"], s, G)
            near = (R.bf16_tie_distance(v) <= 16 * U * m).reshape(kw["p0"].shape)
            if not bool(near.any()):
                break
            for i, n in enumerate(("p0", "p1", "p2")):
                kw[n][near] = normal((G * Rr, C), seed + 100 + 10 * attempt + i, dtype)[near]
        else:
            raise AssertionError("inputs next to a bf16 rounding tie remain")
    return kw, nout


def ew_run(op, kw, G, s, dtype, nout):
    from vmg_amd import kernels as K
    d = {k: dev(v, dtype if k.startswith("p") else F32) for k, v in kw.items()}
    got = K.tab_elementwise(op, d["p0"], d.get("p1"), d.get("p2"), coef=d.get("coef"), add=d.get("add"), s=s, G=G, nout=nout)
    return [got] if nout == 1 else list(got)


def ew_check(op, kw, G, s, dtype, nout, what):
    """fp32: 16 u M; bf16: 2^-8 |ref| + 16 u M per element, M the expression with every term replaced by its absolute value.  16 covers at most
    6 roundings of the expression plus the 5 ulp the OpenCL / OCML specification allows tanhf, entering at most twice; 2^-8 |ref| is the
    final round-to-nearest to bf16."""
    got = ew_run(op, kw, G, s, dtype, nout)
    refs, mags = R.tab_elementwise_ref(op, kw["p0"], kw.get("p1"), kw.get("p2"), coef=kw.get("coef"), add=kw.get("add"), s=s, G=G, dtype=dtype)
    assert len(got) == len(refs) == nout
    for i, (g, ref, mag) in enumerate(zip(got, refs, mags)):
        assert g.dtype == dtype and g.shape == ref.shape
        err = (g.cpu().double() - ref).abs()
        tol = 16 * U * mag + (UB * ref.abs() if dtype == BF16 else 0.0)
        worst = float((err / tol.clamp_min(1e-300)).max())
        print(f"{what} output {i}: max err / tol = {worst:.3g}")
        bad = (err > tol).nonzero()
        assert bad.numel() == 0, f"{what} output {i}: {bad.shape[0]} of {ref.numel()} off, first at {bad[0].tolist()}, {worst} x the tolerance"


@pytest.mark.parametrize("variant,dtype", [(v, d) for v in EW_VARIANTS for d in DTYPES], ids=lambda v: DT_ID.get(v) or v[0])
def test_tab_elementwise_ops(variant, dtype):
    name, op, s, with_p1 = variant
    for G, Rr, C in EW_SHAPES:
        kw, nout = ew_inputs(op, G, Rr, C, dtype, s, with_p1)
        ew_check(op, kw, G, s, dtype, nout, f"{name} {(G, Rr, C)}")


@pytest.mark.parametrize("op", [R.OP_CA_FWD, R.OP_MIX_BWD], ids=lambda o: R.OP_NAMES[o])
def test_tab_elementwise_past_the_block_cap(op):
    """3 * 174789 rows of 4 fp32 vectors = 2,097,468 vectors against 8192 blocks * 256 threads = 2,097,152: the grid-stride loop takes a second
    turn, in the last group."""
    G, Rr, C = 3, 174789, 16
    assert G * Rr * (C // 4) > 8192 * 256
    kw, nout = ew_inputs(op, G, Rr, C, F32, 0.7)
    ew_check(op, kw, G, 0.7, F32, nout, R.OP_NAMES[op])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_tab_elementwise_exact_outputs(dtype):
    """One product, one rounding: OP_SCALE with s = 1 and d_x of OP_CA_BWD with s = 1 equal the fp64 result rounded to the dtype.  (The
    coefficients have 9 significant bits, distinct per (g, c): a bf16 value times one is exact in fp32, so bf16 is rounded once, too.)"""
    for G, Rr, C in EW_SHAPES:
        p0 = normal((G * Rr, C), 600, dtype)
        coef = ((1.0 + torch.arange(G * C, dtype=torch.float32)) / 256.0).reshape(G, C)
        assert G * C < 512
        add = normal((G, C), 601, F32)
        (got,) = ew_run(R.OP_SCALE, {"p0": p0, "coef": coef}, G, 1.0, dtype, 1)
        (ref,), _ = R.tab_elementwise_ref(R.OP_SCALE, p0, coef=coef, s=1.0, G=G)
        assert torch.equal(got.cpu(), ref.to(dtype))
        _, dx = ew_run(R.OP_CA_BWD, {"p0": p0, "coef": coef, "add": add}, G, 1.0, dtype, 2)
        assert torch.equal(dx.cpu(), p0.to(dtype))


# ================================================================================================ max pooling
POOL_CASES = [((2, 8, 12, 5), 2), ((2, 8, 12, 5), 4), ((1, 4, 4, 3), 2), ((1, 4, 4, 3), 4), ((1, 15, 30, 8), 3), ((1, 15, 30, 8), 15),
              ((3, 16, 24, 64), 2), ((3, 16, 24, 64), 4), ((2, 1024, 1032, 4), 2)]


@functools.lru_cache(maxsize=2)
def pool_case(shape, f, with_nan):
    """Values from {-2 .. 2}: most windows have ties.  with_nan: NaNs first and last in a window, two in one window, and a window of -inf."""
    n, h, w, c = shape
    x = torch.randint(-2, 3, shape, generator=_gen(700 + f)).float()
    if with_nan:
        nan, inf = float("nan"), float("inf")
        x[0, 0, 0, 0] = nan
        x[0, f - 1, 2 * f - 1, 1 % c] = nan
        x[n - 1, h - f, w - f + 1, c - 1] = nan
        x[n - 1, h - 1, w - 1, c - 1] = nan
        x[0, h - f:, :f, 0] = -inf
    dy = ints((n, h // f, w // f, c), 710 + f)
    y, idx, dx = R.maxpool_ref(x, f, dy)
    return x, dy, y, idx, dx


@pytest.mark.parametrize("case,dtype,with_nan", [(c, d, False) for c in POOL_CASES for d in DTYPES] + [(POOL_CASES[0], d, True) for d in DTYPES] +
                         [(POOL_CASES[4], d, True) for d in DTYPES],
                         ids=lambda v: DT_ID.get(v) or ("nan" if v is True else "ints" if v is False else "x".join(map(str, v[0])) + "_f%d" % v[1]))
def test_maxpool_forward_backward_exact(case, dtype, with_nan):
    """y and the winner's position (first maximum in row-major order; a NaN is the maximum) equal the reference; the backward writes EVERY input
    position: the window's gradient at the winner, zero elsewhere.  The block the backward's output is allocated from is filled with a
    non-zero value before, so a position that is not written cannot pass as a zero.  (2, 1024, 1032, 4): 8.4 M inputs against 8192 * 256 threads."""
    from vmg_amd import kernels as K
    shape, f = case
    x, dy, wy, widx, wdx = pool_case(shape, f, with_nan)
    if shape[1] > 1000:
        assert x.numel() > 8192 * 256
    y, idx = K.maxpool_forward(dev(x, dtype), f)
    assert y.dtype == dtype and idx.dtype == torch.uint8
    assert torch.equal(idx.cpu(), widx), f"{int((idx.cpu() != widx).sum())} winners differ"
    assert same(y.cpu().double(), wy)
    dyd = dev(dy, dtype)
    stale = torch.full(shape, 7.0, dtype=dtype, device="cuda")
    del stale
    dx = K.maxpool_backward(dyd, idx, f)
    assert dx.dtype == dtype and tuple(dx.shape) == tuple(shape)
    assert torch.equal(dx.cpu().double(), wdx), f"{int((dx.cpu().double() != wdx).sum())} gradient positions differ"


def test_maxpool_refuses_what_it_cannot_do():
    from vmg_amd import kernels as K
    from vmg_amd.hip import HipError
    x = torch.zeros(1, 32, 32, 4, device="cuda")
    with pytest.raises(HipError):
        K.maxpool_forward(x, 16)                          # the winner's position is one byte: f <= 15
    with pytest.raises(HipError):
        K.maxpool_forward(x[:, :30], 4)                   # not contiguous
    with pytest.raises(HipError):
        K.maxpool_forward(x[:, :30].contiguous(), 4)      # 30 is no multiple of 4
    with pytest.raises(HipError):
        K.maxpool_forward(x[:, :, :30].contiguous(), 4)
    with pytest.raises(HipError):
        K.maxpool_backward(torch.zeros(1, 2, 2, 4, device="cuda"), torch.zeros(1, 2, 2, 4, dtype=torch.uint8, device="cuda"), 16)
    xs, dy, wy, widx, wdx = pool_case((1, 4, 4, 3), 2, False)
    y, idx = K.maxpool_forward(dev(xs, F32), 2)
    assert torch.equal(idx.cpu(), widx) and torch.equal(y.cpu().double(), wy)


# ================================================================================================ 2 x 2 average pooling
@pytest.mark.parametrize("shape,dtype", [(s, d) for s in [(2, 8, 12, 8), (1, 7, 9, 8), (1, 2, 2, 3), (2, 64, 96, 8)] for d in DTYPES],
                         ids=lambda v: DT_ID.get(v) or "x".join(map(str, v)))
def test_avgpool2(shape, dtype):
    """Integer inputs: the four-term sum and the quarter of it are exact in fp32 and in bf16.  Normal inputs: three additions and the (exact)
    quarter in fp32, off by at most 4 u M with M the mean of |x|, plus the final rounding to bf16.  Odd sizes drop the last row / column."""
    from vmg_amd import kernels as K
    n, h, w, c = shape
    x = ints(shape, 800)
    got = K.avgpool2(dev(x, dtype))
    assert got.dtype == dtype and tuple(got.shape) == (n, h // 2, w // 2, c)
    assert torch.equal(got.cpu().double(), R.avgpool2_ref(x)[0])
    x = normal(shape, 801, dtype)
    got = K.avgpool2(dev(x, dtype)).cpu().double()
    ref, mag = R.avgpool2_ref(x)
    err = (got - ref).abs()
    tol = 4 * U * mag + (UB * ref.abs() if dtype == BF16 else 0.0)
    print(f"max err / tol = {float((err / tol).max()):.3g}")
    assert bool((err <= tol).all())


# ================================================================================================ refusals
# Each raises on the host, before any launch, and leaves a following valid call correct.
def _valid_reduce_call(dtype=F32):
    from vmg_amd import kernels as K
    ops, refs = int_reduce_case(4, 24, 64)
    a, b, c = (dev(t, dtype) for t in ops[:3])
    assert torch.equal(K.group_reduce(a, 4, b=b, c3=c).cpu(), refs["a+b+c3"].float())
    assert torch.equal(K.group_reduce3(a, b, c, dev(ops[3], dtype), 4).cpu(), refs["3"].float())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_group_reduce_refusals(dtype):
    from vmg_amd import kernels as K
    from vmg_amd.hip import HipError
    z = lambda rows, C: torch.ones(rows, C, dtype=dtype, device="cuda")
    for C in (7, 143, 514):                                # odd, odd, even but > 512
        with pytest.raises(HipError):
            K.group_reduce(z(8, C), 2)
    a = z(8, 16)
    with pytest.raises(HipError):
        K.group_reduce(a, 2, mode=1)                       # the product needs b
    with pytest.raises(HipError):
        K.group_reduce(a, 2, c3=z(8, 16))                  # a third operand without the second (the kernel would ignore it)
    with pytest.raises(HipError):
        K.group_reduce(a, 2, c3=z(8, 16), mode=1)
    with pytest.raises(HipError):
        K.group_reduce(a, 3)                               # 8 rows, 3 groups
    with pytest.raises(HipError):
        K.group_reduce(a, 2, b=z(8, 8))                    # shapes differ
    with pytest.raises(HipError):
        K.group_reduce(a, 2, b=torch.ones(8, 16, dtype=F32 if dtype == BF16 else BF16, device="cuda"))
    _valid_reduce_call(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_group_reduce3_refusals(dtype):
    from vmg_amd import kernels as K
    from vmg_amd.hip import HipError
    z = lambda rows, C: torch.ones(rows, C, dtype=dtype, device="cuda")
    vn = 8 if dtype == BF16 else 4
    for C in (vn // 2, vn + 2, 512 + vn):                  # no multiple of the vector width (this kernel has no narrow form); too wide
        t = z(8, C)
        with pytest.raises(HipError):
            K.group_reduce3(t, t, t, t, 2)
    t = z(8, 16)
    with pytest.raises(HipError):
        K.group_reduce3(t, t, t, t, 3)
    off = dev(torch.ones(8, 16), dtype, 2)
    for i in range(4):
        args = [t, t, t, t]
        args[i] = off                                      # one misaligned operand, each position
        with pytest.raises(HipError):
            K.group_reduce3(*args, 2)
    _valid_reduce_call(dtype)


def _ew_valid(op, G, Rr, C, dtype):
    with_p1 = op == R.OP_AFFINE2
    kw, nout = ew_inputs(op, G, Rr, C, dtype, 1.0, with_p1)
    return kw, nout


def _ew_call(op, d, G, nout, s=1.0):
    from vmg_amd import kernels as K
    return K.tab_elementwise(op, d["p0"], d.get("p1"), d.get("p2"), coef=d.get("coef"), add=d.get("add"), s=s, G=G, nout=nout)


@pytest.mark.parametrize("op,dtype", [(o, d) for o in range(10) for d in DTYPES], ids=lambda v: DT_ID.get(v) or R.OP_NAMES[v])
def test_tab_elementwise_refusals(op, dtype):
    from vmg_amd.hip import HipError
    G, Rr, C = 2, 5, 16
    kw, nout = _ew_valid(op, G, Rr, C, dtype)
    d = {k: dev(v, dtype if k.startswith("p") else F32) for k, v in kw.items()}
    extra, ncoef, has_add, _ = R.OP_USES[op]
    required = list(extra) + (["coef"] if ncoef else []) + (["add"] if has_add else [])
    for name in required:                                  # a missing operand
        with pytest.raises(HipError):
            _ew_call(op, {k: v for k, v in d.items() if k != name}, G, nout)
    for name in d:                                         # a misaligned operand, each in turn (OP_AFFINE2's optional p1 included)
        with pytest.raises(HipError):
            _ew_call(op, {**d, name: dev(kw[name], dtype if name.startswith("p") else F32, 2)}, G, nout)
    if ncoef:                                              # coefficients of another group count / another op's width
        for shape in ((G + 1, C, ncoef), (G, C, ncoef % 3 + 1), (1, C, ncoef)):
            with pytest.raises(HipError):
                _ew_call(op, {**d, "coef": torch.ones(shape, device="cuda")}, G, nout)
        with pytest.raises(HipError):
            _ew_call(op, {**d, "coef": d["coef"].to(BF16)}, G, nout)
    if has_add:
        with pytest.raises(HipError):
            _ew_call(op, {**d, "add": torch.ones(G + 1, C, device="cuda")}, G, nout)
    with pytest.raises(HipError):
        _ew_call(op, d, 3, nout)                           # 10 rows, 3 groups
    with pytest.raises(HipError):
        _ew_call(op, d, 0, nout)
    for wrong in {1, 2, 3} - {nout}:
        with pytest.raises(HipError):
            _ew_call(op, d, G, wrong)
    if "p1" in d:
        with pytest.raises(HipError):
            _ew_call(op, {**d, "p1": d["p1"][:-1]}, G, nout)  # shapes differ
    Cn = 4 if dtype == BF16 else 2                         # C no multiple of the 16-byte vector
    narrow = {k: torch.ones((G * Rr, Cn), dtype=dtype, device="cuda") if k.startswith("p") else
              torch.ones((G, Cn, ncoef) if k == "coef" else (G, Cn), device="cuda") for k in d}
    with pytest.raises(HipError, match="multiple of"):
        _ew_call(op, narrow, G, nout)
    ew_check(op, kw, G, 1.0, dtype, nout, R.OP_NAMES[op] + " after the refusals")


def test_tab_elementwise_entry_refuses_missing_outputs_and_coefficients():
    """The C entry itself (the Python wrapper always allocates the outputs an op writes): a null output or coefficient pointer of an op that
    uses it is an error return, not a launch."""
    from vmg_amd import hip
    G, Rr, C = 2, 5, 16
    t = [torch.ones(G * Rr, C, device="cuda") for _ in range(6)]
    coef, add = torch.ones(G, C, 3, device="cuda"), torch.ones(G, C, device="cuda")
    full = dict(p0=t[0], p1=t[1], p2=t[2], coef=coef, add=add, o0=t[3], o1=t[4], o2=t[5])
    order = ("p0", "p1", "p2", "coef", "add")

    def call(op, args):
        p = lambda n: args[n].data_ptr() if args.get(n) is not None else None
        return hip.lib().vmg_tab_elementwise(hip.F32, op, *(p(n) for n in order), 1.0, p("o0"), p("o1"), p("o2"), G * Rr, Rr, C, hip.stream_ptr())

    for op, (extra, ncoef, has_add, nout) in R.OP_USES.items():
        used = ["p0", "o0"] + list(extra) + (["coef"] if ncoef else []) + (["add"] if has_add else []) + ["o1", "o2"][:nout - 1]
        for name in used:
            rc = call(op, {k: v for k, v in full.items() if k != name})
            assert rc != 0, f"{R.OP_NAMES[op]} accepted a null {name}"
            assert name in hip.lib().vmg_last_error().decode() or name in ("p0", "o0")
    assert call(10, full) != 0 and call(-1, full) != 0
    torch.cuda.synchronize()
    assert call(R.OP_MIX_BWD, full) == 0                   # and the entry still works: o_k = 1 * 1 + 1
    assert all(bool((t[i] == 2.0).all()) for i in (3, 4, 5))
