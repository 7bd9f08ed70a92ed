"""The max-mode kernels of csrc/ltam.hip (hard trajectory attention) against the float64 reference of tests/ltam_max_ref.py (pinned on the CPU by
tests/test_ltam_max_ref.py) on the cases of tests/ltam_max_cases.py, both dtypes, both routes (key-frame pointers in the kernel arguments / in the
device table).  bf16 inputs are rounded first and the reference sees those values.

Index: with TAU = 2e-5 the kernel's idx must lie within TAU of the reference's maximum, and where no other key-frame lies strictly within TAU of
it, it must EQUAL the reference's first maximum -- the exact ties at score 0 of out-of-range key-frames and the duplicated key-frame included.
Values: score, out, dq, dk, dv per element against the reference evaluated AT THE KERNEL'S OWN idx (so nothing is left out); the backward is handed
the reference's idx.  Bounds: KAPPA[kind] * 2^-24 * S (+ 2^-8 |reference| on the bf16-stored out and dq), see tests/ltam_max_cases.py; every comparison
prints its worst ratio |kernel - reference| / (2^-24 S) first.
Measured on the MI355X over the whole case list, both dtypes (worst ratio per kind) -> KAPPA = 4 x measured, rounded up (ltam_max_cases.MEASURED / KAPPA):
    score 1.604 -> 7   out 0.607 -> 3   dq 4.044 -> 17   dk 6.608 -> 27   dv 3.835 -> 16
All fp32 bounds stay under the whole-tensor ceilings of the window kernels (2e-5 forward, 2e-4 gradients); check() asserts that."""
import pytest
import torch

from tests import ltam_max_cases as MC
from tests import ltam_max_ref as MR

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
_ids = [g.id for g in MC.CASES]
_dn = lambda dt: "bf16" if dt == torch.bfloat16 else "fp32"


def _K():
    from vmg_amd import kernels as K
    from vmg_amd.hip import HipError
    return K, HipError


def check(kind, got, ref, S, dtype, label):
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{label} {kind}: non-finite values"
    err = (got - ref).abs()
    S = S if torch.is_tensor(S) else torch.full_like(ref, float(S))
    b = MC.bound(kind, S, ref, dtype)
    extra = MC.BF * ref.abs() if (dtype == torch.bfloat16 and kind in MC.ROUNDED) else torch.zeros_like(ref)
    ratio = torch.where(S > 0, (err - extra).clamp_min(0) / (MC.U * S.clamp_min(1e-300)), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    print(f"RATIO {kind} {_dn(dtype)} {label} {float(ratio.max()):.3f}")
    if dtype == torch.float32:  # never looser than the whole-tensor tolerance of the window kernels
        assert float((MC.KAPPA[kind] * MC.U * S).max()) <= MC.CEILING[kind] * MC.U * max(1.0, float(ref.abs().max())), f"{label} {kind}: bound above the ceiling"
    bad = err > b
    assert not bad.any(), f"{label} {kind}: {int(bad.sum())} elements over the bound, worst ratio {float(ratio.max()):.3f} (kappa {MC.KAPPA[kind]})"


def device(r, dtype):
    q, keys, vals, loc, dout = r["inp"]
    d = lambda t: t.to(dtype).cuda().contiguous()
    return dict(q=d(q), keys=[d(k) for k in keys], vals=[d(v) for v in vals], loc=loc.cuda(), dout=d(dout), idx=r["idx"].to(torch.int32).cuda().contiguous())


def fwd(g, dv_, tab=None):
    K, _ = _K()
    tab = (MC.route(g) == "table") if tab is None else tab
    return (K.ltam_max_forward_tab if tab else K.ltam_max_forward)(dv_["q"], dv_["keys"], dv_["vals"], dv_["loc"], MC.HEADS)


def bwd(g, dv_, tab=None, **into):
    K, _ = _K()
    tab = (MC.route(g) == "table") if tab is None else tab
    return (K.ltam_max_backward_tab if tab else K.ltam_max_backward)(dv_["q"], dv_["keys"], dv_["vals"], dv_["loc"], dv_["idx"], dv_["dout"], MC.HEADS, **into)


def check_index(g, dtype, r, idx):
    idx = idx.cpu().long()
    assert int(idx.min()) >= 0 and int(idx.max()) < g.t
    table = r["table"]
    assert bool(MC.allowed(table).gather(3, idx[:, :, :, None, :]).all()), f"{g.id}: an index outside the TAU set"
    near = MC.near_ties(table)
    flips = int((idx != r["idx"]).sum())
    print(f"INDEX {_dn(dtype)} {g.id} near-ties {int(near.sum())} of {near.numel()}, differing from the reference {flips}")
    assert float(near.double().mean()) <= MC.NEAR_TIE_CAP
    assert torch.equal(idx[~near], r["idx"][~near]), f"{g.id}: not the first maximum where there is no near-tie"


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("g", MC.CASES, ids=_ids)
def test_forward_index_score_and_output(g, dtype):
    r = MC.reference(g, dtype)
    dv_ = device(r, dtype)
    out, idx, score = fwd(g, dv_)
    assert out.dtype == dtype and idx.dtype == torch.int32 and score.dtype == torch.float32
    check_index(g, dtype, r, idx)
    q, keys, vals, loc, _ = r["inp"]
    ref_out, _, ref_score, _ = MR.forward(q, keys, vals, loc, MC.HEADS, idx=idx.cpu().long())  # the reference at the kernel's own selection
    check("score", score, ref_score, 1.0, torch.float32, g.id)
    check("out", out, ref_out, r["vmax"], dtype, g.id)
    out2, idx2, score2 = fwd(g, dv_)  # no atomics on this path: the same bits
    assert torch.equal(out, out2) and torch.equal(idx, idx2) and torch.equal(score, score2)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("g", MC.CASES, ids=_ids)
def test_backward(g, dtype):
    r = MC.reference(g, dtype)
    dv_ = device(r, dtype)
    dq, dk, dv = bwd(g, dv_)
    assert dq.dtype == dtype and all(t.dtype == torch.float32 for t in dk + dv)
    check("dq", dq, r["dq"], float(r["dq"].abs().max()), dtype, g.id)
    for j in range(g.t):
        check("dk", dk[j], r["dk"][j], r["sc"]["dk"][j], torch.float32, f"{g.id}[{j}]")
        check("dv", dv[j], r["dv"][j], r["sc"]["dv"][j], torch.float32, f"{g.id}[{j}]")
    assert torch.equal(dq, bwd(g, dv_)[0])  # dq has no atomics


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_both_routes_give_the_same_bits(dtype):
    """17 key-frames through the argument route and through the table route: one kernel, a template parameter apart."""
    g = MC.BY_ID[MC.BOTH_ROUTES]
    r = MC.reference(g, dtype)
    dv_ = device(r, dtype)
    a, b = fwd(g, dv_, tab=False), fwd(g, dv_, tab=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    check_index(g, dtype, r, b[1])
    ga, gb = bwd(g, dv_, tab=False), bwd(g, dv_, tab=True)
    assert torch.equal(ga[0], gb[0])
    for j in range(g.t):  # (atomics: the order of the additions into one element is not fixed; both are within the bound)
        check("dk", gb[1][j], r["dk"][j], r["sc"]["dk"][j], torch.float32, f"table {g.id}[{j}]")
        check("dv", gb[2][j], r["dv"][j], r["sc"]["dv"][j], torch.float32, f"table {g.id}[{j}]")


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_dense_key_row_from_a_single_head(dtype):
    """One head alone selects key-frame 1 (idx forced): its row of dk[1] is non-zero in the other heads' channels, within the bound of the reference."""
    g = MC.BY_ID["1x1-c16-t3-identity"]
    r = MC.reference(g, dtype)
    dv_ = device(r, dtype)
    idx = torch.tensor([1, 0, 0, 0]).reshape(1, 1, 1, 4)
    dv_["idx"] = idx.to(torch.int32).cuda()
    q, keys, vals, loc, dout = r["inp"]
    rq, rk, rv, sc = MR.backward(q, keys, vals, loc, idx, dout, MC.HEADS, with_scales=True)
    dq, dk, dv = bwd(g, dv_)
    D = g.c // MC.HEADS
    assert (dk[1][0, 0, 0, D:] != 0).all() and (rk[1][0, 0, 0, D:] != 0).all()
    check("dq", dq, rq, float(rq.abs().max()), dtype, "single-head")
    for j in range(g.t):
        check("dk", dk[j], rk[j], sc["dk"][j], torch.float32, f"single-head[{j}]")
        check("dv", dv[j], rv[j], sc["dv"][j], torch.float32, f"single-head[{j}]")


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("gid", ["8x8-c32-t2-int", "9x7-c144-t7-int", "9x17-c112-t33-int"])
def test_backward_adds_into_the_accumulators_it_is_given(gid, dtype):
    """dk_into / dv_into hold non-zero fp32 values: afterwards prefill + gradient, within the gradient's bound plus one fp32 rounding of the sum."""
    g = MC.BY_ID[gid]
    r = MC.reference(g, dtype)
    dv_ = device(r, dtype)
    shp = (g.n, g.h, g.w, g.c)
    pk = [MC.TC.randn(shp, 2400 + j, max(float(r["dk"][j].std()), 1e-3)) for j in range(g.t)]
    pv = [MC.TC.randn(shp, 2440 + j, max(float(r["dv"][j].std()), 1e-3)) for j in range(g.t)]
    ik, iv = [p.float().cuda().contiguous() for p in pk], [p.float().cuda().contiguous() for p in pv]
    _, dk, dv = bwd(g, dv_, dk_into=ik, dv_into=iv)
    for j in range(g.t):
        assert dk[j].data_ptr() == ik[j].data_ptr() and dv[j].data_ptr() == iv[j].data_ptr()
        for kind, got, pre, ref, S in (("dk", dk[j], pk[j], r["dk"][j], r["sc"]["dk"][j]), ("dv", dv[j], pv[j], r["dv"][j], r["sc"]["dv"][j])):
            want = pre.float().double() + ref
            err = (got.double().cpu() - want).abs()
            lim = MC.bound(kind, S, ref, torch.float32) + 2.0 ** -23 * want.abs().clamp_min(pre.abs().double())
            assert bool((err <= lim).all()), f"{gid} {kind}[{j}]"
            untouched = S == 0
            assert torch.equal(got.cpu()[untouched], pre.float()[untouched])  # no addend, no write


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_an_unselected_key_frame_is_left_bit_untouched(dtype):
    """The duplicated key-frame 1 is never selected: its accumulators (filled with a NaN pattern) come back bit-identical -- no atomic touched them."""
    g = MC.BY_ID["10x12-c32-t3-dup"]
    r = MC.reference(g, dtype)
    assert not (r["idx"] == 1).any()
    dv_ = device(r, dtype)
    shp = (g.n, g.h, g.w, g.c)
    ik = [torch.zeros(shp, device="cuda") for _ in range(g.t)]
    iv = [torch.zeros(shp, device="cuda") for _ in range(g.t)]
    ik[1] = torch.full(shp, float("nan"), device="cuda")
    iv[1] = torch.full(shp, float("nan"), device="cuda")
    before = (ik[1].view(torch.int32).clone(), iv[1].view(torch.int32).clone())
    bwd(g, dv_, dk_into=ik, dv_into=iv)
    assert torch.equal(ik[1].view(torch.int32), before[0]) and torch.equal(iv[1].view(torch.int32), before[1])
    assert torch.isfinite(ik[0]).all() and torch.isfinite(ik[2]).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_rows_outside_partial_tiles_are_not_written(dtype):
    """9 x 7 map = 2 x 1 tiles of 8 x 8: the kernels are handed the first image of a two-image buffer whose second image (the memory right behind the
    rows a partial tile would run into) holds a pattern; out, idx, score and dq leave it alone."""
    K, _ = _K()
    g = MC.BY_ID["9x7-c144-t7-int"]
    r = MC.reference(g, dtype)
    dv_ = device(r, dtype)
    out, idx, score = fwd(g, dv_)
    dq, _, _ = bwd(g, dv_)
    # the wrappers allocate exact-size outputs: write the same launches into guarded buffers through the C entry points
    from vmg_amd import hip
    n, h, w, c, t = g.n, g.h, g.w, g.c, g.t
    pad = 64 * c
    gout = torch.full((n * h * w * c + pad,), 7.0, dtype=dtype, device="cuda")
    gidx = torch.full((n * h * w * 4 + 256,), -5, dtype=torch.int32, device="cuda")
    gsc = torch.full((n * h * w * 4 + 256,), 7.0, dtype=torch.float32, device="cuda")
    gdq = torch.full((n * h * w * c + pad,), 7.0, dtype=dtype, device="cuda")
    ptrs = K._ptrs
    hip.check(hip.lib().vmg_ltam_max_fwd(hip.dtype_code(dtype), dv_["q"].data_ptr(), ptrs(dv_["keys"]), ptrs(dv_["vals"]), dv_["loc"].data_ptr(), gout.data_ptr(),
                                         gidx.data_ptr(), gsc.data_ptr(), n, h, w, c, 4, t, hip.stream_ptr()), "vmg_ltam_max_fwd")
    acc = torch.zeros((2 * t, n, h, w, c), device="cuda")
    hip.check(hip.lib().vmg_ltam_max_bwd(hip.dtype_code(dtype), dv_["q"].data_ptr(), ptrs(dv_["keys"]), ptrs(dv_["vals"]), dv_["loc"].data_ptr(),
                                         dv_["idx"].data_ptr(), dv_["dout"].data_ptr(), gdq.data_ptr(), ptrs(list(acc[:t])), ptrs(list(acc[t:])), n, h, w, c, 4, t,
                                         hip.stream_ptr()), "vmg_ltam_max_bwd")
    torch.cuda.synchronize()
    assert torch.equal(gout[:n * h * w * c].reshape(out.shape), out) and (gout[n * h * w * c:] == 7.0).all()
    assert torch.equal(gidx[:n * h * w * 4].reshape(idx.shape), idx) and (gidx[n * h * w * 4:] == -5).all()
    assert torch.equal(gsc[:n * h * w * 4].reshape(score.shape), score) and (gsc[n * h * w * 4:] == 7.0).all()
    assert torch.equal(gdq[:n * h * w * c].reshape(dq.shape), dq) and (gdq[n * h * w * c:] == 7.0).all()


def test_bad_arguments_raise_without_a_launch():
    K, HipError = _K()
    mk = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    n, h, w, c = 1, 4, 4, 16
    q, loc1 = mk(n, h, w, c), mk(n, 2, h, w)

    def frames(t, cc=c):
        return [mk(n, h, w, cc) for _ in range(t)]

    idx = torch.zeros((n, h, w, 4), dtype=torch.int32, device="cuda")
    with pytest.raises(HipError, match="key-frames"):  # the 33rd key-frame on the argument route
        K.ltam_max_forward(q, frames(33), frames(33), mk(n, 66, h, w), 4)
    with pytest.raises(HipError, match="key-frames"):
        K.ltam_max_backward(q, frames(33), frames(33), mk(n, 66, h, w), idx, q, 4)
    K.ltam_max_forward_tab(q, frames(33), frames(33), mk(n, 66, h, w), 4)  # (the table route takes them)
    with pytest.raises(HipError, match="head dim"):
        K.ltam_max_forward(mk(n, h, w, 48), frames(1, 48), frames(1, 48), loc1, 4)
    with pytest.raises(HipError, match="head dim"):
        K.ltam_max_forward_tab(mk(n, h, w, 48), frames(1, 48), frames(1, 48), loc1, 4)
    with pytest.raises(HipError, match="heads"):
        K.ltam_max_forward(q, frames(1), frames(1), loc1, 2)
    with pytest.raises(HipError, match="contiguous"):
        K.ltam_max_forward(mk(n, h, w, 2 * c)[..., ::2], frames(1), frames(1), loc1, 4)
    with pytest.raises(HipError, match="contiguous"):
        K.ltam_max_forward(q, [mk(n, h, w, 2 * c)[..., ::2]], frames(1), loc1, 4)
    with pytest.raises(HipError, match="loc"):
        K.ltam_max_forward(q, frames(1), frames(1), mk(n, 2, h, w, dt=torch.float64), 4)
    with pytest.raises(HipError, match="loc"):
        K.ltam_max_backward(q, frames(1), frames(1), mk(n, 2, h, w, dt=torch.bfloat16), idx, q, 4)
    with pytest.raises(HipError, match="idx"):
        K.ltam_max_backward(q, frames(1), frames(1), loc1, idx.long(), q, 4)
    with pytest.raises(HipError, match="key-frame"):
        K.ltam_max_forward_tab(q, [], [], mk(n, 0, h, w), 4)
    with pytest.raises(HipError, match="accumulators"):
        K.ltam_max_backward(q, frames(1), frames(1), loc1, idx, q, 4, dk_into=[mk(n, h, w, c, dt=torch.bfloat16)], dv_into=[None])
