"""The depthwise 3x3 kernels of the MBConv mixer (csrc/dwconv.hip) on the GPU against the fp64 restatement of tests/mbconv_ref.py: both routes,
both dtypes, the four flag combinations, exact inputs (bit equality), planted ReLU6 boundaries, Gaussian inputs under a derived bound,
misaligned and non-contiguous operands, run-to-run identity of the weight gradient, and refusals that launch nothing."""
import pytest
import torch

from tests import mbconv_ref as MR

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
FLAGS = [(None, None), ("relu6", None), (None, "relu6"), ("relu6", "relu6")]
SHAPES = [(1, 1, 1, 8), (1, 1, 5, 8), (2, 5, 1, 16), (1, 2, 2, 3), (2, 3, 7, 19), (2, 9, 11, 32), (1, 6, 5, 448), (1, 3, 3, 1792)]
CASES = SHAPES + ["tile+1/vector", "tile+1/element"]


def _name(v):
    if isinstance(v, tuple) and v and isinstance(v[0], int):
        return "x".join(map(str, v))
    if isinstance(v, tuple):
        return "+".join(str(x) for x in v)
    return str(v).replace("torch.", "")


def _shape(case, dtype):
    """A listed shape, or the one that exceeds the plan's tile by one row, one column and -- in channels -- by one vector (vector route) or one
    element (element route) beyond the channel block: read from the plan."""
    from vmg_amd import kernels as K
    if isinstance(case, tuple):
        return case
    vn = 8 if dtype == torch.bfloat16 else 4
    if case.endswith("vector"):
        p = K.dwconv3_plan(1, 1, 1, vn, dtype)
        shape = (1, p.tile_h + 1, p.tile_w + 1, p.chan_block + vn)
    else:
        p = K.dwconv3_plan(1, 1, 1, 1, dtype)
        shape = (1, p.tile_h + 1, p.tile_w + 1, p.chan_block + 1)
    q = K.dwconv3_plan(*shape, dtype)
    assert q.route == case.split("/")[1] and q.grid == 2 * 2 * 2 and shape[0] * shape[1] * shape[2] <= 240
    return shape


def _regimes(v):
    """Fractions of v at or below 0, strictly inside (0, 6), at or above 6."""
    n = v.numel()
    return [float((v <= 0).sum()) / n, float(((v > 0) & (v < 6)).sum()) / n, float((v >= 6).sum()) / n]


def _exact_inputs(shape, seed):
    """e, da: multiples of 1/8 in [-8, 8]; w: multiples of 1/32 in [-1, 1]; b: multiples of 1/16 in [-4, 4] (fp64 tensors whose values every
    dtype here holds).  Every product is a multiple of 1/256 below 2^7 and every partial sum of the forward and the data gradient stays
    below 2^24 / 256, so fp32 adds them exactly in any order; with N * H * W <= 240 the same holds for dW (multiples of 1/64 below 2^18)."""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-64, 65, shape, generator=g).double() / 8
    da = torch.randint(-64, 65, shape, generator=g).double() / 8
    w = torch.randint(-32, 33, (C, 1, 3, 3), generator=g).double() / 32
    b = torch.randint(-64, 65, (C,), generator=g).double() / 16
    return e, da, w, b


def _exact_case(shape):
    """The first seed whose draw puts at least 10 % of the source elements and of the pre-activation outputs (with the source ReLU6) into each
    ReLU6 regime -- a property of the inputs alone, asserted by the caller; small shapes need a few draws."""
    for seed in range(700, 1000):
        e, da, w, b = _exact_inputs(shape, seed)
        pre = MR.dwconv3(e, w, b, "relu6", None, pre=True)
        if min(_regimes(e)) >= 0.1 and min(_regimes(pre)) >= 0.1:
            return e, da, w, b
    raise AssertionError(f"no seed gives every regime 10 % at {shape}")


def _bits(t):
    """The bit patterns with the sign of zero dropped (x + 0 maps -0 to +0 and changes nothing else): what 'the same bits' means here."""
    t = t + 0
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(got, want, what):
    bad = _bits(got.cpu()) != _bits(want.cpu())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


def _dev(t, dtype):
    return t.to(dtype).cuda().contiguous()


def _run_all(e, da, w, b, a, src_act, act, dtype):
    """forward, data gradient, weight gradient of the kernels for fp64 host inputs; a: the stored output handed to the two gradients."""
    from vmg_amd import kernels as K
    ed, dad, ad = _dev(e, dtype), _dev(da, dtype), _dev(a, dtype)
    wd, bd = _dev(w, torch.float32), _dev(b, torch.float32)
    y = K.dwconv3_forward(ed, wd, bd, src_act, act)
    de = K.dwconv3_backward_data(dad, ad if act else None, ed if src_act else None, wd, src_act, act)
    dW, db = K.dwconv3_backward_weight(dad, ad if act else None, ed, src_act, act)
    torch.cuda.synchronize()
    return y, de, dW, db


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", CASES, ids=_name)
def test_exact_inputs_give_the_bits_of_fp64(case, dtype):
    """Forward and data gradient bit-equal to the dtype rounding of the fp64 value, dW and db bit-equal to fp64 cast to fp32, for all four flag
    combinations; each ReLU6 regime holds at least 10 % of the sources and of the outputs."""
    from vmg_amd import kernels as K
    shape = _shape(case, dtype)
    assert shape[0] * shape[1] * shape[2] <= 240
    e, da, w, b = _exact_case(shape)
    pre = MR.dwconv3(e, w, b, "relu6", None, pre=True)
    assert min(_regimes(e)) >= 0.1 and min(_regimes(pre)) >= 0.1, (_regimes(e), _regimes(pre))
    route = K.dwconv3_route(shape[3], dtype)
    assert route == MR.expected_route(shape[3], dtype)
    for src_act, act in FLAGS:
        a = MR.dwconv3(e, w, b, src_act, act).to(dtype).double()  # the stored output: rounded once
        de, dW, db = MR.dwconv3_grads(e, w, a, da, src_act, act)
        y, gde, gdW, gdb = _run_all(e, da, w, b, a, src_act, act, dtype)
        tag = f"{_name(shape)} {route} {src_act}/{act}"
        _same_bits(y, a.to(dtype), f"forward {tag}")
        _same_bits(gde, de.to(dtype), f"data gradient {tag}")
        _same_bits(gdW, dW.float(), f"dW {tag}")
        _same_bits(gdb, db.float(), f"db {tag}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_weight_gradient_repeats_adds_into_and_fills_many_partials(dtype):
    """Two runs give the same bits (no atomics, a grid that depends on the geometry alone); with into= the sums are added to the buffers; a
    shape with more tiles than one workgroup's share (several partials per channel block) is exact too."""
    from vmg_amd import kernels as K
    # 240 pixels in five tiles, one per first-stage workgroup; 129 one-pixel images, one more tile than there are partials: a workgroup walks two
    for shape, partials in (((5, 6, 8, 40), 5), ((129, 1, 1, 8), 128)):
        C = shape[3]
        assert K.dwconv3_plan(*shape, dtype).partials == partials
        e, da, w, b = _exact_case(shape)
        a = MR.dwconv3(e, w, b, "relu6", "relu6").to(dtype).double()
        _, dW, db = MR.dwconv3_grads(e, w, a, da, "relu6", "relu6")
        ed, dad, ad = _dev(e, dtype), _dev(da, dtype), _dev(a, dtype)
        r1 = K.dwconv3_backward_weight(dad, ad, ed, "relu6", "relu6")
        r2 = K.dwconv3_backward_weight(dad, ad, ed, "relu6", "relu6")
        for x, y, want in zip(r1, r2, (dW, db)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
            _same_bits(x, want.float(), "weight gradient")
        gW, gb = torch.full((C, 1, 3, 3), 0.5, device="cuda"), torch.full((C,), -2.0, device="cuda")
        oW, ob = K.dwconv3_backward_weight(dad, ad, ed, "relu6", "relu6", into=(gW, gb))
        assert oW is gW and ob is gb
        _same_bits(gW, (dW + 0.5).float(), "dW added")
        _same_bits(gb, (db - 2.0).float(), "db added")


# ------------------------------------------------------------------------------------------------ planted boundaries
def _planted(dtype):
    six = torch.tensor(6.0, dtype=dtype)
    lo = torch.nextafter(six.float(), torch.tensor(0.0)) if dtype == torch.float32 else torch.tensor(6.0 - 2.0 ** -5)
    hi = torch.nextafter(six.float(), torch.tensor(9.0)) if dtype == torch.float32 else torch.tensor(6.0 + 2.0 ** -5)
    vals = torch.tensor([0.0, -0.0, 6.0, float(lo), float(hi), -100.0, 100.0, 1.0, 5.0, -1.0, 2.0 ** -20, -(2.0 ** -20)], dtype=torch.float64)
    assert torch.equal(vals.to(dtype).double(), vals)  # every planted value is a value of the dtype
    return vals


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("C", [8, 5], ids=["vector", "element"])
def test_planted_boundaries(C, dtype):
    """Sources and outputs exactly 0, -0, 6, the two neighbours of 6 in the dtype, -100, 100.  With a centre-only unit weight and no bias every
    sum has one term, so the forward is relu6 of the planted value and the data gradient is da times the two masks, exactly: 0 at exactly 0
    and at exactly 6, da at the neighbour below 6, 0 at the neighbour above.  The stored output a handed to the gradients is planted too,
    independently of e (a shifted copy), so the output mask is read from a and not recomputed."""
    vals = _planted(dtype)
    N, H, W = 1, 4, 6
    n = N * H * W * C
    e = vals.repeat(n // len(vals) + 1)[:n].reshape(N, H, W, C)
    a_planted = vals.roll(5).repeat(n // len(vals) + 1)[:n].reshape(N, H, W, C)
    da = torch.arange(n, dtype=torch.float64).reshape(N, H, W, C) % 7 / 8 + 0.125
    w = torch.zeros(C, 1, 3, 3, dtype=torch.float64)
    w[:, 0, 1, 1] = 1.0
    b = torch.zeros(C, dtype=torch.float64)
    for src_act, act in FLAGS:
        y, de, dW, db = _run_all(e, da, w, b, a_planted, src_act, act, dtype)
        want = MR._act(MR._act(e, src_act), act)
        _same_bits(y, want.to(dtype), f"forward {src_act}/{act}")
        mask = MR._act_grad(a_planted, act) * MR._act_grad(e, src_act)
        _same_bits(de, (da * mask).to(dtype), f"data gradient {src_act}/{act}")
        if act:
            flat_a, flat = a_planted.reshape(-1), de.cpu().double().reshape(-1)
            assert float(flat[(flat_a == 0) | (flat_a == 6)].abs().max()) == 0.0
        # the sums of dW and db have many inexact terms here (6 -+ 1 ulp): the bound of the Gaussian cases
        _, rW, rb = MR.dwconv3_grads(e, w, a_planted, da, src_act, act)
        _, _, tW, tb = MR.abs_term_sums(e, w, b, a_planted, da, src_act, act)
        _within(dW, rW, tW, N * H * W, torch.float32, "dW")
        _within(db, rb, tb, N * H * W, torch.float32, "db")


# ------------------------------------------------------------------------------------------------ Gaussian cases
def _ulp(want, dtype):
    """Spacing of the dtype's values at |want| (normal range; the smallest normal's spacing below it)."""
    p = 23 if dtype == torch.float32 else 7
    ex = torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), ex - p)


def _within(got, want, terms, n, dtype, what):
    """|got - want| <= ulp_dtype(want) / 2 + (n + 1) 2^-24 sum|terms|: one rounding at the store plus n fp32 operations, each within 2^-24 of
    its result, whose magnitudes the sum of the terms' magnitudes bounds."""
    got = got.detach().cpu().double()
    bound = 0.5 * _ulp(want, dtype) + (n + 1) * 2.0 ** -24 * terms
    err = (got - want).abs()
    bad = err > bound
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} beyond the bound, worst ratio {worst:.3f}"


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", CASES, ids=_name)
def test_gaussian_inputs_within_the_derived_bound(case, dtype):
    shape = _shape(case, dtype)
    N, H, W, C = shape
    g = torch.Generator().manual_seed(811 + C)
    e = (3 * torch.randn(shape, generator=g)).to(dtype).double()
    da = torch.randn(shape, generator=g).to(dtype).double()
    w = (torch.randn(C, 1, 3, 3, generator=g) / 3).double()
    b = torch.randn(C, generator=g).double()
    for src_act, act in FLAGS:
        a = MR.dwconv3(e, w, b, src_act, act)
        a_st = a.to(dtype).double()
        de, dW, db = MR.dwconv3_grads(e, w, a_st, da, src_act, act)
        tf, td, tW, tb = MR.abs_term_sums(e, w, b, a_st, da, src_act, act)
        y, gde, gdW, gdb = _run_all(e, da, w, b, a_st, src_act, act, dtype)
        tag = f"{_name(shape)} {src_act}/{act}"
        _within(y, a, tf, 10, dtype, f"forward {tag}")
        _within(gde, de, td, 9, dtype, f"data gradient {tag}")
        _within(gdW, dW, tW, N * H * W, torch.float32, f"dW {tag}")
        _within(gdb, db, tb, N * H * W, torch.float32, f"db {tag}")


# ------------------------------------------------------------------------------------------------ operands
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_misaligned_and_non_contiguous_operands_give_the_same_bits(dtype):
    """An operand one element off a 16-byte boundary takes the element route (the plan with aligned = False says so) and gives the bits of the
    vector route; a permuted (non-contiguous) input through the autograd entry is made contiguous and gives them too."""
    from vmg_amd import functional as FH
    from vmg_amd import kernels as K
    shape = (2, 9, 11, 32)
    assert K.dwconv3_route(32, dtype) == "vector" and K.dwconv3_plan(*shape, dtype, aligned=False).route == "element"
    e, da, w, b = _exact_case(shape)
    ed, dad, wd, bd = _dev(e, dtype), _dev(da, dtype), _dev(w, torch.float32), _dev(b, torch.float32)

    def off(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 != 0 and t.data_ptr() % 16 == 0
        return v

    y = K.dwconv3_forward(ed, wd, bd, "relu6", "relu6")
    y2 = K.dwconv3_forward(off(ed), wd, bd, "relu6", "relu6")
    assert torch.equal(_bits(y), _bits(y2))
    de = K.dwconv3_backward_data(dad, y, ed, wd, "relu6", "relu6")
    assert torch.equal(_bits(de), _bits(K.dwconv3_backward_data(off(dad), y, ed, wd, "relu6", "relu6")))
    assert torch.equal(_bits(de), _bits(K.dwconv3_backward_data(dad, off(y), off(ed), wd, "relu6", "relu6")))
    dW, db = K.dwconv3_backward_weight(dad, y, ed, "relu6", "relu6")
    dW2, db2 = K.dwconv3_backward_weight(off(dad), off(y), off(ed), "relu6", "relu6")
    _same_bits(dW2, dW, "dW")  # (exact inputs: any summation order gives the same sums)
    _same_bits(db2, db, "db")
    # the autograd entry: (B, T, H, W, C), a permuted input, parameter gradients through autograd
    x5 = ed.reshape(1, 2, 9, 11, 32).permute(0, 1, 3, 2, 4).contiguous().permute(0, 1, 3, 2, 4).requires_grad_(True)
    assert not x5.is_contiguous()
    wp, bp = wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    out = FH.depthwise_conv3x3(x5, wp, bp, "relu6", "relu6")
    assert out.shape == x5.shape and torch.equal(_bits(out.reshape(shape)), _bits(y))
    out.backward(dad.reshape(out.shape))
    assert torch.equal(_bits(x5.grad.reshape(shape)), _bits(de))
    _same_bits(wp.grad, dW, "dW through autograd")
    _same_bits(bp.grad, db, "db through autograd")


def test_entries_refuse_null_pointers_and_bad_flags_without_a_launch():
    """With real device tensors: every refusal returns -1 (a failed launch would be -2) and leaves the outputs untouched."""
    from vmg_amd import hip
    l = hip.lib()
    N, H, W, C = 1, 3, 4, 8
    x = torch.ones(N, H, W, C, device="cuda")
    w, b = torch.ones(C, 1, 3, 3, device="cuda"), torch.ones(C, device="cuda")
    y = torch.full_like(x, -7.0)
    dW, db, ws = torch.full_like(w, -7.0), torch.full_like(b, -7.0), torch.empty(1 << 16, device="cuda")
    p = lambda t: t.data_ptr()
    st = hip.stream_ptr()
    rcs = [l.vmg_dwconv3_fwd(hip.F32, 0, 0, None, p(w), p(b), p(y), N, H, W, C, st), l.vmg_dwconv3_fwd(hip.F32, 0, 0, p(x), None, p(b), p(y), N, H, W, C, st),
           l.vmg_dwconv3_fwd(hip.F32, 0, 0, p(x), p(w), None, p(y), N, H, W, C, st), l.vmg_dwconv3_fwd(hip.F32, 2, 0, p(x), p(w), p(b), p(y), N, H, W, C, st),
           l.vmg_dwconv3_fwd(hip.F32, 0, 7, p(x), p(w), p(b), p(y), N, H, W, C, st), l.vmg_dwconv3_fwd(5, 0, 0, p(x), p(w), p(b), p(y), N, H, W, C, st),
           l.vmg_dwconv3_fwd(hip.F32, 0, 0, p(x), p(w), p(b), p(y), N, 0, W, C, st),
           l.vmg_dwconv3_bwd_data(hip.F32, 1, 1, p(x), None, p(x), p(w), p(y), N, H, W, C, st),
           l.vmg_dwconv3_bwd_data(hip.F32, 1, 1, p(x), p(x), None, p(w), p(y), N, H, W, C, st),
           l.vmg_dwconv3_bwd_data(hip.F32, 0, 2, p(x), p(x), p(x), p(w), p(y), N, H, W, C, st),
           l.vmg_dwconv3_bwd_weight(hip.F32, 1, 1, p(x), None, p(x), p(dW), p(db), N, H, W, C, 0, p(ws), ws.numel() * 4, st),
           l.vmg_dwconv3_bwd_weight(hip.F32, 1, 1, p(x), p(x), p(x), p(dW), p(db), N, H, W, C, 0, None, ws.numel() * 4, st),
           l.vmg_dwconv3_bwd_weight(hip.F32, 1, 1, p(x), p(x), p(x), p(dW), p(db), N, H, W, C, 0, p(ws), 8, st),
           l.vmg_dwconv3_bwd_weight(hip.F32, -1, 1, p(x), p(x), p(x), p(dW), p(db), N, H, W, C, 0, p(ws), ws.numel() * 4, st)]
    torch.cuda.synchronize()
    assert all(rc == -1 for rc in rcs), rcs
    assert l.vmg_last_error()
    assert bool((y == -7).all()) and bool((dW == -7).all()) and bool((db == -7).all())
