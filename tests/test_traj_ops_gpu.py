"""csrc/ltam.hip and csrc/warp.hip, kernel by kernel, against the float64 reference of tests/traj_ref.py (pinned on the CPU by
tests/test_traj_ref.py) on the cases of tests/traj_cases.py.

The attention is called through kernels.ltam_forward / ltam_backward, so dK, dV and dRPE come back as the fp32 sums the kernel wrote.  bf16
inputs are rounded first and the reference gets those values; the backward is handed the REFERENCE's out (rounded to the tensor dtype) and
lse (rounded to fp32), and the reference backward forms its delta from that same rounded out: both sides see the same numbers, bf16 adds
one rounding on out / dq (the warp: out / dx) and none on the fp32 sums.

Bounds are per element, KAPPA[kind] * 2^-24 * S (+ 2^-8 |reference| for the bf16-stored tensors), see tests/traj_cases.py.  Every
comparison prints its worst ratio |kernel - reference| / (2^-24 S) before it asserts.
Measured on the MI355X over the whole case list, both dtypes (worst ratio per kind) -> the chosen KAPPA = 4 x measured, rounded up
(traj_cases.MEASURED / KAPPA):
    out 1.79 -> 8   lse 4.13 -> 17   dq 5.70 -> 23   dk 41.27 -> 166   dv 7.29 -> 30   drpe 7.03 -> 29
    warp out 1.47 -> 6   dx 4.82 -> 20   dflow 2.21 -> 9
dk's ratio is the largest because its addends P (dp - delta) q hide a cancellation: where dp and delta nearly agree the fp32 kernel keeps the
roundings of the two dot products, which the sum of |addends| does not see.  All bounds stay far inside the earlier whole-tensor tolerances
(2e-5 forward, 2e-4 gradients, 1e-3 dflow); check() asserts that for every fp32 comparison."""
import numpy as np
import pytest
import torch

from tests import traj_cases as TC
from tests import traj_ref as TR

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
_ids = lambda gs: [g.id for g in gs]
_dn = lambda dt: "bf16" if dt == torch.bfloat16 else "fp32"


def _K():
    from vmg_amd import kernels as K
    from vmg_amd.hip import HipError
    return K, HipError


def check(kind, got, ref, S, dtype, label, skip=None):
    """|got - ref| <= bound(kind) per element; prints the worst ratio to 2^-24 S first (bf16-stored kinds: after taking 2^-8 |ref| off).
    skip: boolean mask of elements that another assertion covers."""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{label} {kind}: non-finite values"
    err = (got - ref).abs()
    S = S if torch.is_tensor(S) else torch.full_like(ref, float(S))
    b = TC.bound(kind, S, ref, dtype)
    extra = TC.BF * ref.abs() if (dtype == torch.bfloat16 and kind in TC.ROUNDED) else torch.zeros_like(ref)
    ratio = torch.where(S > 0, (err - extra).clamp_min(0) / (TC.U * S.clamp_min(1e-300)), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    if skip is not None:
        ratio, err, b = ratio[~skip], err[~skip], b[~skip]
    print(f"RATIO {kind} {_dn(dtype)} {label} {float(ratio.max()):.3f}")
    if dtype == torch.float32:  # never looser than the whole-tensor tolerance this kind had before
        assert float((TC.KAPPA[kind] * TC.U * S).max()) <= TC.CEILING[kind] * TC.U * max(1.0, float(ref.abs().max())), f"{label} {kind}: bound above the ceiling"
    bad = err > b
    assert not bad.any(), f"{label} {kind}: {int(bad.sum())} elements over the bound, worst ratio {float(ratio.max()):.3f} (kappa {TC.KAPPA[kind]})"


# ------------------------------------------------------------------------------------------------------------------ trajectory attention
def ltam_device(r, dtype):
    q, keys, vals, loc, rpe, decay, dout = r["inp"]
    d = lambda t: t.to(dtype).cuda().contiguous()
    return dict(q=d(q), keys=[d(k) for k in keys], vals=[d(v) for v in vals], loc=loc.cuda(), rpe=rpe.cuda(), decay=decay.cuda(), dout=d(dout),
                out=d(r["out_r"]), lse=r["lse_r"].float().contiguous().cuda())


def ltam_fwd(g, dv_, r):
    K, _ = _K()
    return K.ltam_forward(dv_["q"], dv_["keys"], dv_["vals"], dv_["loc"], dv_["rpe"], dv_["decay"], TC.HEADS, g.wh, g.ww, r["scale"])


def ltam_bwd(g, dv_, r, **into):
    K, _ = _K()
    return K.ltam_backward(dv_["q"], dv_["keys"], dv_["vals"], dv_["loc"], dv_["rpe"], dv_["decay"], dv_["out"], dv_["lse"], dv_["dout"], TC.HEADS,
                           g.wh, g.ww, r["scale"], **into)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("g", TC.LTAM, ids=_ids(TC.LTAM))
def test_ltam_forward_and_lse(g, dtype):
    r = TC.ltam_reference(g, dtype)
    dv_ = ltam_device(r, dtype)
    out, lse = ltam_fwd(g, dv_, r)
    check("out", out, r["out"], r["vmax"], dtype, g.id)
    check("lse", lse, r["lse"], r["lse"].abs().clamp_min(1.0), torch.float32, g.id)
    out2, lse2 = ltam_fwd(g, dv_, r)  # no atomics on this path: the same bits
    assert torch.equal(out, out2) and torch.equal(lse, lse2)


def _check_ltam_grads(g, dtype, r, got, dq_skip=None):
    dq, dk, dv, drpe = got
    check("dq", dq, r["dq"], float(r["dq"][~dq_skip].abs().max()) if dq_skip is not None else float(r["dq"].abs().max()), dtype, g.id, skip=dq_skip)
    for j in range(g.t):
        check("dk", dk[j], r["dk"][j], r["sc"]["dk"][j], torch.float32, f"{g.id}[{j}]")
        check("dv", dv[j], r["dv"][j], r["sc"]["dv"][j], torch.float32, f"{g.id}[{j}]")
    check("drpe", drpe, r["drpe"], r["sc"]["drpe"], torch.float32, g.id)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("g", TC.LTAM, ids=_ids(TC.LTAM))
def test_ltam_backward(g, dtype):
    r = TC.ltam_reference(g, dtype)
    dv_ = ltam_device(r, dtype)
    got = ltam_bwd(g, dv_, r)
    assert all(t.dtype == torch.float32 for t in got[1] + got[2]) and got[3].dtype == torch.float32 and got[0].dtype == dtype
    _check_ltam_grads(g, dtype, r, got)
    again = ltam_bwd(g, dv_, r)  # dq has no atomics
    assert torch.equal(got[0], again[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_ltam_zero_query_row_and_zero_key_row(dtype):
    """A zero query row and a zero key source row (gathered by four positions) meet the 1e-12 norm clamp: forward and lse are finite and
    within bound; in the backward the zero rows' OWN gradients carry the clamp's factor 1e12 and are compared relatively -- the query row
    against its own maximum, the key row through its scale S, which is a sum of |addends| and so relative already."""
    g = TC.LTAM_BY_ID["8x8-c32-t2-int"]
    r = TC.ltam_reference(g, dtype, zero_rows=True)
    dv_ = ltam_device(r, dtype)
    out, lse = ltam_fwd(g, dv_, r)
    check("out", out, r["out"], r["vmax"], dtype, "zero-rows")
    check("lse", lse, r["lse"], r["lse"].abs().clamp_min(1.0), torch.float32, "zero-rows")
    got = ltam_bwd(g, dv_, r)
    zq = torch.zeros(r["dq"].shape, dtype=torch.bool)
    zq[0, 1, 2] = True
    _check_ltam_grads(g, dtype, r, got, dq_skip=zq)
    row = r["dq"][0, 1, 2]
    assert float(row.abs().max()) > 1e9 and float(r["dk"][0][0, 3, 1].abs().max()) > 1e9  # the clamp factor really is in these rows
    check("dq", got[0][0, 1, 2], row, float(row.abs().max()), dtype, "zero-rows-own-row")


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("gid", ["8x8-c32-t2-int", "10x12-c32-w2x4-t2-int", "10x12-c32-t2-onepixel"])
def test_ltam_backward_adds_into_the_accumulators_it_is_given(gid, dtype):
    """dk_into / dv_into / drpe_into hold non-zero fp32 values: afterwards they hold prefill + gradient, within the gradient's bound plus one
    fp32 rounding of the sum."""
    g = TC.LTAM_BY_ID[gid]
    r = TC.ltam_reference(g, dtype)
    dv_ = ltam_device(r, dtype)
    shp = (g.n, g.h, g.w, g.c)
    # (what an accumulator holds in the recurrence: earlier calls' sums, of the size of the gradient it is added to)
    pk = [TC.randn(shp, 2400 + j, float(r["dk"][j].std())) for j in range(g.t)]
    pv = [TC.randn(shp, 2440 + j, float(r["dv"][j].std())) for j in range(g.t)]
    pr = TC.randn(r["drpe"].shape, 2480, float(r["drpe"].std()))
    dk_into, dv_into, drpe_into = [p.cuda() for p in pk], [p.cuda() for p in pv], pr.cuda()
    dq, dk, dv, drpe = ltam_bwd(g, dv_, r, dk_into=dk_into, dv_into=dv_into, drpe_into=drpe_into)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(dk + dv + [drpe], dk_into + dv_into + [drpe_into]))
    for kind, gots, pre, refs, scs in (("dk", dk, pk, r["dk"], r["sc"]["dk"]), ("dv", dv, pv, r["dv"], r["sc"]["dv"]),
                                       ("drpe", [drpe], [pr], [r["drpe"]], [r["sc"]["drpe"]])):
        for j, (a, p, ref, S) in enumerate(zip(gots, pre, refs, scs)):
            want = p.double() + ref
            err = (a.double().cpu() - want).abs()
            b = TC.bound(kind, S, ref, torch.float32) + TC.U * want.abs()
            print(f"RATIO {kind}+prefill {_dn(dtype)} {gid}[{j}] {float((err / (TC.U * (S + want.abs()).clamp_min(1e-300))).max()):.3f} worst err/bound {float((err / b.clamp_min(1e-300)).max()):.3f}")
            assert not (err > b).any(), f"{kind}[{j}]: {int((err > b).sum())} elements over bound + one rounding"


def test_ltam_refuses_33_key_frames_and_wrong_arguments():
    """Each refusal is a HipError raised before any launch."""
    K, HipError = _K()
    g = TC.LTAM_BY_ID["8x8-c32-t2-int"]
    r = TC.ltam_reference(g, torch.float32)
    d = ltam_device(r, torch.float32)
    hd, sc = TC.HEADS, r["scale"]
    fwd = lambda **kw: K.ltam_forward(*[kw.get(k, d[k]) for k in ("q", "keys", "vals", "loc", "rpe", "decay")], hd, kw.get("wh", 2), kw.get("ww", 2), sc)
    bwd = lambda **kw: K.ltam_backward(*[kw.get(k, d[k]) for k in ("q", "keys", "vals", "loc", "rpe", "decay", "out", "lse", "dout")], hd, 2, 2, sc)
    fwd(), bwd()  # the unchanged arguments pass
    k33 = [d["keys"][0]] * 33
    with pytest.raises(HipError):
        fwd(keys=k33, vals=k33, loc=torch.zeros((g.n, 66, g.h, g.w), device="cuda"))
    with pytest.raises(HipError):  # a table made for a 2x4 window
        fwd(rpe=torch.zeros((hd, 8, 8), device="cuda"))
    with pytest.raises(HipError):  # ... and the 2x2 table under a 2x4 window
        fwd(ww=4)
    with pytest.raises(HipError):
        fwd(rpe=torch.zeros((hd, 16), device="cuda"))
    with pytest.raises(HipError):
        fwd(decay=torch.ones(3, device="cuda"))
    with pytest.raises(HipError):
        fwd(decay=torch.ones(8, device="cuda")[::2])
    for bad in (dict(rpe=torch.zeros((hd, 8, 8), device="cuda")), dict(decay=torch.ones(1, device="cuda")),
                dict(out=d["out"][:, :4]), dict(out=d["out"].bfloat16()), dict(dout=d["dout"][:1]), dict(dout=d["dout"].bfloat16()),
                dict(lse=d["lse"].double()), dict(lse=d["lse"][..., :2]), dict(lse=d["lse"].reshape(g.n, g.h * g.w, hd))):
        with pytest.raises(HipError):
            bwd(**bad)


# ------------------------------------------------------------------------------------------------------------------ flow warp
def _check_warp(g, r, label):
    K, _ = _K()
    xd, fd, gd = r["x"].to(g.dtype).cuda(), r["flow"].cuda(), r["dy"].to(g.dtype).cuda()
    out = K.warp_bilinear_forward(xd, fd)
    check("wout", out, r["out"], float(r["x"].abs().max()), g.dtype, label)
    dx, df = K.warp_bilinear_backward(xd, fd, gd)
    assert dx.dtype == g.dtype and df.dtype == torch.float32
    check("dx", dx, r["dx"], r["sc"]["dx"], g.dtype, label)
    check("dflow", df, r["dflow"], r["sc"]["dflow"], torch.float32, label)
    return out, dx, df


@pytest.mark.parametrize("g", TC.WARP, ids=_ids(TC.WARP))
def test_warp_bilinear_forward_and_backward(g):
    r = TC.warp_reference(g)
    out, dx, df = _check_warp(g, r, g.id)
    ix, iy, gmx, gmy = TR.warp_coords(r["flow"].numpy(), g.h, g.w)
    if g.fam == "onborder":  # a sample exactly on a border: the clamp's gradient is zero there, exactly
        on = torch.from_numpy((gmx == 0) | (gmy == 0))
        assert int(on.sum()) >= on.numel() // 8
        assert float(df.cpu()[..., 0][torch.from_numpy(gmx == 0)].abs().max()) == 0.0 and float(df.cpu()[..., 1][torch.from_numpy(gmy == 0)].abs().max()) == 0.0
    if g.fam in ("int", "huge"):  # where the fp32 sample position is a whole pixel the result is a COPY of that pixel (clamped outside)
        whole = torch.from_numpy((ix == np.floor(ix)) & (iy == np.floor(iy)))
        assert int(whole.sum()) >= whole.numel() // 4
        src = torch.from_numpy((iy * g.w + ix).astype(np.int64))
        want = TR._rows(r["x"].reshape(g.n, g.h * g.w, g.c), torch.where(whole, src, torch.zeros_like(src)))
        assert torch.equal(out.double().cpu()[whole], want[whole])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("hw", TC.WARP_MAPS, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_warp_with_zero_flow_is_the_identity(hw, dtype):
    """Zero flow: wherever the fp32 round trip pixel -> normalised grid -> pixel returns the pixel itself (tests/test_traj_ref.py says on which
    of these maps that is every pixel) out is a bit-exact copy of x; where it does so on the whole map, the fp32 dx is a bit-exact copy of
    dy.  The rest is within bound."""
    h, w = hw
    g = TC.Warp(f"{_dn(dtype)}-{h}x{w}-zero", 2, h, w, 8 if dtype == torch.bfloat16 else 4, dtype, "zero")
    r = TC.warp_reference(g)
    out, dx, df = _check_warp(g, r, g.id)
    ix, iy, _, _ = TR.warp_coords(r["flow"].numpy(), h, w)
    same = torch.from_numpy((ix == np.arange(w, dtype=np.float32)[None, None, :]) & (iy == np.arange(h, dtype=np.float32)[None, :, None]))
    assert torch.equal(out.double().cpu()[same], r["x"][same])
    if bool(same.all()) and dtype == torch.float32:
        assert torch.equal(dx.double().cpu(), r["dy"])


def test_warp_refuses_wrong_arguments():
    K, HipError = _K()
    x = torch.zeros((1, 4, 4, 8), device="cuda")
    flow = torch.zeros((1, 4, 4, 2), device="cuda")
    K.warp_bilinear_backward(x, flow, torch.zeros_like(x))
    for dy in (torch.zeros((1, 4, 4, 4), device="cuda"), torch.zeros((1, 4, 2, 8), device="cuda"), torch.zeros_like(x).bfloat16()):
        with pytest.raises(HipError):
            K.warp_bilinear_backward(x, flow, dy)
    # the backward entry applies the forward's channel multiple (bf16: 8, fp32: 4) and 16-byte alignment
    for xb in (torch.zeros((1, 4, 4, 6), device="cuda", dtype=torch.bfloat16), torch.zeros((1, 4, 4, 2), device="cuda")):
        with pytest.raises(HipError):
            K.warp_bilinear_forward(xb, flow)
        with pytest.raises(HipError):
            K.warp_bilinear_backward(xb, flow, torch.zeros_like(xb))
    off = torch.zeros(4 * 4 * 8 + 2, device="cuda", dtype=torch.bfloat16)[2:].reshape(1, 4, 4, 8)  # 4 bytes past a 16-byte boundary
    with pytest.raises(HipError):
        K.warp_bilinear_backward(off, flow, torch.zeros((1, 4, 4, 8), device="cuda", dtype=torch.bfloat16))


# ------------------------------------------------------------------------------------------------------------------ location advection
@pytest.mark.parametrize("g", TC.NEAREST, ids=_ids(TC.NEAREST))
def test_location_advection_equals_the_reference_bit_for_bit(g):
    K, _ = _K()
    loc, flow = TC.nearest_inputs(g)
    got = K.warp_nearest_planes(loc.cuda(), flow.cuda()).cpu()
    assert torch.equal(got, TR.warp_nearest_reference(loc, flow))


# ------------------------------------------------------------------------------------------------------------------ grid-stride loops
def test_grid_stride_bilinear_backward_past_8192_blocks():
    """184 x 180 = 33 120 pixels, one wave each, four per block: 8 280 blocks wanted, 8 192 launched -- the last 352 pixels are second trips."""
    g = TC.Warp("bf16-184x180-c8-stride", 1, 184, 180, 8, torch.bfloat16, "random")
    assert g.h * g.w > 8192 * 4
    _check_warp(g, TC.warp_reference(g), g.id)
    TC._warp_cache.pop(g.id)


def test_grid_stride_bilinear_forward_past_8192_blocks():
    """184 x 180 pixels x 64 four-float vectors = 2 119 680 threads' worth against 8 192 x 256; compared on the last 16 rows (the second trip is
    the last two) and the first 8."""
    K, _ = _K()
    n, h, w, c = 1, 184, 180, 256
    assert h * w * (c // 4) > 8192 * 256
    x, flow = TC.randn((n, h, w, c), 2501).double(), TC.warp_flow("random", n, h, w, seed=2502)
    out = K.warp_bilinear_forward(x.float().cuda(), flow.cuda()).double().cpu()
    ref = TR.warp_bilinear_reference(x, flow)
    rows = list(range(8)) + list(range(h - 16, h))
    check("wout", out[:, rows], ref[:, rows], float(x.abs().max()), torch.float32, "fp32-184x180-c256-stride")


def test_grid_stride_nearest_planes_past_8192_blocks():
    K, _ = _K()
    n, k2, h, w = 1, 2, 1448, 1449
    assert h * w > 8192 * 256
    loc, flow = TC.randn((n, k2, h, w), 2511, 10.0), TC.warp_flow("random", n, h, w, seed=2512)
    got = K.warp_nearest_planes(loc.cuda(), flow.cuda()).cpu()
    assert torch.equal(got, TR.warp_nearest_reference(loc, flow))


def test_grid_stride_flow_smooth_past_8192_blocks():
    """2 planes of 1024 x 1030, r = 4 (the width is padded by 2 reflected columns), forward and backward, against numpy's pad / mean / spread /
    crop and its adjoint.  Bound: the worst case of an fp32 sum of n terms in any order, n * 2^-24 * sum |addends| (n = 16 forward; backward an
    input pixel and its mirror images collect up to 4 blocks of 16).  The addends are x / 16, so their |.| sum is the same reference applied
    to |x| (the division by r^2, a power of two, is exact)."""
    K, _ = _K()
    p, h, w, r = 2, 1024, 1030, 4
    assert p * h * w > 8192 * 256
    x, gy = TC.randn((p, h, w), 2521), TC.randn((p, h, w), 2522)
    got = K.flow_smooth(x.cuda(), r).double().cpu().numpy()
    want, scale = TR.flow_smooth_reference(x.numpy(), r), TR.flow_smooth_reference(x.abs().numpy(), r)
    print(f"RATIO flow_smooth fwd {float((np.abs(got - want) / (TC.U * np.maximum(scale, 1e-300))).max()):.3f} (bound 16)")
    assert np.all(np.abs(got - want) <= 16 * TC.U * scale)
    gb = K.flow_smooth(gy.cuda(), r, backward=True).double().cpu().numpy()
    wb, sb = TR.flow_smooth_reference_backward(gy.numpy(), r), TR.flow_smooth_reference_backward(gy.abs().numpy(), r)
    print(f"RATIO flow_smooth bwd {float((np.abs(gb - wb) / (TC.U * np.maximum(sb, 1e-300))).max()):.3f} (bound 64)")
    assert np.all(np.abs(gb - wb) <= 64 * TC.U * sb)
