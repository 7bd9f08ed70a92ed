"""3-D shifted-window attention kernels (csrc/win3d.hip; models/swin_3d.py:167-252) against an fp64 reference of the OPERATION
(tests/win3d_ref.py: padded volume, torch.roll, the oracle's window_partition / shift_mask / relative_position_index / window_reverse,
a softmax per time slice; pinned to the oracle's swin_block and shown to discriminate in tests/test_win3d_ref.py).  Three routes:
the MFMA kernels on bf16 (even head dimension <= 32), the VALU kernel on bf16, the VALU kernel on fp32.  Geometries: tests/win3d_cases.py.

Bounds (tests/win3d_cases.py::bounds).  Per tensor two metrics, max |got - ref| / max |ref| and ||got - ref|| / ||ref||; lse: max |got - ref|
in nats, absolute.  bound = 4 x floor, floor = the same metric between the fp64 reference and (bf16) the reference re-rounded where the
kernels document a rounding -- padded tokens' biases, probabilities before P.V and the gradient arriving there, stored out / dq / dkv --
or (fp32) the reference evaluated in fp32; the floor is never taken below what fp32 arithmetic itself gives (2^-20 relative, 2^-16 nat),
the bound never above the stated 2e-2 (out) / 3e-2 (gradients) for bf16 and 1e-4 for fp32.  dbkv's scale is floored at 1e-3 of dkv's
(with pad == shift and wt > 2 every padded key is seen at e^-100 and dbkv ~ 0); dtable is scaled by its own max and norm.

Measured on MI355X, worst over the geometries of a route: max-metric / L2 metric, and the largest share of its bound any case used.
    tensor   MFMA bf16                 VALU bf16                 VALU fp32
    out      6.2e-3 / 2.4e-3  0.31     3.3e-3 / 1.8e-3  0.25     2.9e-6 / 1.6e-6  0.28
    lse      2.3e-3 nat       0.25     5.0e-6 nat       0.08     5.1e-6 nat       0.08
    dq       4.6e-3 / 2.7e-3  0.34     3.4e-3 / 2.3e-3  0.28     4.2e-6 / 3.0e-6  0.51
    dkv      3.8e-3 / 2.4e-3  0.26     3.0e-3 / 1.7e-3  0.25     4.8e-6 / 3.1e-6  0.51
    dtable   2.7e-3 / 1.9e-3  0.47     8.7e-4 / 6.6e-4  0.12     2.6e-6 / 2.9e-6  0.44
    dbkv     4.9e-4 / 5.4e-4  0.09     7.1e-4 / 4.9e-4  0.07     2.6e-6 / 2.1e-6  0.69
Floors (CPU, per geometry): bf16 out 2.3e-3 .. 6.9e-3, dq / dkv / dtable / dbkv 7e-4 .. 5.0e-3 (L2: 1.4e-3 .. 2.5e-3), lse 0 (no padding)
.. 2.3e-3 nat; fp32 1e-7 .. 2.7e-6, lse 5e-7 .. 5e-6 nat (the larger figures where logits carry -100).  No kernel needed more than margin 4,
no rounding point had to be added to the emulation.  dbq: exactly 0 added, everywhere."""
import pytest
import torch

from tests import win3d_cases as WC

pytestmark = pytest.mark.gpu

CASES = [(g.id, r) for g in WC.GEOMS for r in g.routes]
ROUTE_NAME = {"M": "mfma-bf16", "V": "valu-bf16", "F": "valu-fp32"}


def _dev(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).cuda().contiguous()


def _check(tag, got, ref, sc, floor, bnd):
    err = WC.errors(got, ref, sc)
    bad = []
    for n, (em, el) in err.items():
        assert torch.isfinite(got[n]).all(), f"{tag}: {n} is not finite"
        unit = "nat" if n == "lse" else "rel"
        print(f"[win3d] {tag} {n}: max {em:.3e} l2 {el:.3e} {unit} | floor {floor[n][0]:.3e} {floor[n][1]:.3e} | bound {bnd[n][0]:.3e} {bnd[n][1]:.3e}"
              f" | used {max(em / bnd[n][0], el / bnd[n][1]):.2f}")
        if em > bnd[n][0] or el > bnd[n][1]:
            bad.append(f"{n}: max {em:.3e} > {bnd[n][0]:.3e} or l2 {el:.3e} > {bnd[n][1]:.3e}")
    return bad


@pytest.mark.parametrize("gid,route", CASES, ids=[f"{ROUTE_NAME[r]}-{i}" for i, r in CASES])
def test_win3d_kernel_matches_the_fp64_reference(gid, route):
    """out, lse, dq, dkv, dtable, dbq, dbkv of one kernel route vs fp64 autograd of the reference, through vmg_amd.kernels.  The bias gradient
    buffers are handed in pre-filled (into=): dbq must stay bit-equal (a padded query's output row is cropped: exactly 0 is added), dbkv is
    compared after the pattern is taken off again (the kernel accumulates).  Bias-free: padded tokens are zeros, no bias gradients come back."""
    from oracle import recipe as R
    from vmg_amd import hip, kernels as K
    g = WC.BY_ID[gid]
    variant, dtype = WC.ROUTES[route]
    assert WC.mfma_expected(g, variant, dtype) == (route == "M")  # which kernel the entry picks for this call (win3d_mfma_ok)
    inp, ref, sc, floor, bnd = WC.reference_and_bounds(g, dtype)
    q, kv, bq, bkv, table, dout = inp
    qd, kvd, doutd = _dev(q, dtype), _dev(kv, dtype), _dev(dout, dtype)
    bqd, bkvd, tabd = _dev(bq), _dev(bkv), _dev(table)
    pat_q, pat_kv = R.seeded((g.C,), 1306, 0.5).cuda(), R.seeded((2 * g.C,), 1307, 0.5).cuda()
    into = (pat_q.clone(), pat_kv.clone()) if g.biased else None
    lib = hip.lib()
    prev = lib.vmg_win3d_variant(-1)
    try:
        lib.vmg_win3d_variant(variant)
        assert lib.vmg_win3d_variant(-1) == variant
        out, lse = K.win3d_attn_forward(qd, kvd, bqd, bkvd, tabd, g.heads, g.wt, g.shift)
        dq, dkv, dtable, dbq, dbkv = K.win3d_attn_backward(qd, kvd, bqd, bkvd, tabd, out, lse, doutd, g.heads, g.wt, g.shift, into=into)
        torch.cuda.synchronize()
    finally:
        lib.vmg_win3d_variant(prev)
    assert prev == 1
    assert out.dtype == dtype and dq.dtype == dtype and dkv.dtype == dtype and lse.dtype == torch.float32 and dtable.dtype == torch.float32
    if g.biased:
        assert torch.equal(dbq, pat_q), f"dbq moved by {float((dbq - pat_q).abs().max()):.3e}"
        dbkv = dbkv - pat_kv
    else:
        assert dbq is None and dbkv is None
    got = dict(out=out, lse=lse, dq=dq, dkv=dkv, dtable=dtable, dbq=None, dbkv=dbkv)
    got = {n: (None if t is None else t.double().cpu()) for n, t in got.items()}
    bad = _check(f"{ROUTE_NAME[route]} {gid}", got, ref, sc, floor, bnd)
    assert not bad, f"{ROUTE_NAME[route]} {gid}: " + "; ".join(bad)


ABI_CASES = [("d32-wt4-B2-D5x23x13-win2x3x2", "M"), ("d16-wt8-D9x9x8", "M"), ("d28-wt6-D7x13x9", "M"), ("d36-wt2-13x9", "V"), ("d18-wt4-D6x13x9", "F")]


@pytest.mark.parametrize("gid,route", ABI_CASES, ids=[f"{ROUTE_NAME[r]}-{i}" for i, r in ABI_CASES])
def test_win3d_abi_properties(gid, route):
    """Properties include/vmg_hip.h documents, through direct calls of the entry points:
    * out, lse, dq, dkv are written in full: poisoned with NaN before the launch, finite after it (padded geometries: only real tokens have rows);
    * dtable ACCUMULATES: started from a pattern, the result minus the pattern meets the reference within the bounds of the module docstring;
    * with a workspace the table gradient is bit-reproducible (two runs, equal bits).  This found the MFMA backward at wt = 8 adding each
      workgroup's table with LDS float atomics from four waves (9.5e-7 between two runs on d16-wt8-D9x9x8); it now gathers there as well
      (the same fp32 values, in a fixed order);
    * without one (float atomics into dtable) it is the same sum in another order: per entry within 2 n u sum_w |partial_w|, n = windows,
      u = 2^-24, the partials read back from the workspace (the bound on two fp32 summation orders of the same n numbers)."""
    from oracle import recipe as R
    from vmg_amd import hip
    g = WC.BY_ID[gid]
    variant, dtype = WC.ROUTES[route]
    inp, ref, sc, floor, bnd = WC.reference_and_bounds(g, dtype)
    q, kv, bq, bkv, table, dout = inp
    qd, kvd, doutd = _dev(q, dtype), _dev(kv, dtype), _dev(dout, dtype)
    bqd, bkvd, tabd = _dev(bq), _dev(bkv), _dev(table)
    lib = hip.lib()
    nrel = (2 * g.wt - 1) * 225
    nwin = g.B * -(-g.D // g.wt) * -(-g.H // 8) * -(-g.W // 8)
    assert int(lib.vmg_win3d_attn_bwd_ws_bytes(g.B, g.D, g.H, g.W, g.heads, g.wt)) == nwin * g.heads * nrel * 4
    nan = float("nan")
    out = torch.full_like(qd, nan)
    lse = torch.full((nwin, g.heads, g.wt * 64), nan, dtype=torch.float32, device="cuda")
    pattern = R.seeded((nrel, g.heads), 1308, 0.5).cuda()
    args = (g.B, g.D, g.H, g.W, g.C, g.heads, g.wt, g.shift[0], g.shift[1], g.shift[2], hip.stream_ptr())

    def backward(dtable, ws):
        dq, dkv = torch.full_like(qd, nan), torch.full_like(kvd, nan)
        dbq, dbkv = torch.zeros(g.C, device="cuda"), torch.zeros(2 * g.C, device="cuda")
        hip.check(lib.vmg_win3d_attn_bwd(hip.dtype_code(dtype), qd.data_ptr(), kvd.data_ptr(), bqd.data_ptr(), bkvd.data_ptr(), tabd.data_ptr(), out.data_ptr(),
                                         lse.data_ptr(), doutd.data_ptr(), dq.data_ptr(), dkv.data_ptr(), dtable.data_ptr(), dbq.data_ptr(), dbkv.data_ptr(),
                                         None if ws is None else ws.data_ptr(), *args), "vmg_win3d_attn_bwd")
        torch.cuda.synchronize()
        return dq, dkv

    prev = lib.vmg_win3d_variant(-1)
    try:
        lib.vmg_win3d_variant(variant)
        hip.check(lib.vmg_win3d_attn_fwd(hip.dtype_code(dtype), qd.data_ptr(), kvd.data_ptr(), bqd.data_ptr(), bkvd.data_ptr(), tabd.data_ptr(), out.data_ptr(),
                                         lse.data_ptr(), *args), "vmg_win3d_attn_fwd")
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and torch.isfinite(lse).all()
        ws1 = torch.full((nwin, g.heads, nrel), nan, dtype=torch.float32, device="cuda")
        ws2 = torch.full_like(ws1, nan)
        acc, ordered1, ordered2, atomic = pattern.clone(), torch.zeros_like(pattern), torch.zeros_like(pattern), torch.zeros_like(pattern)
        dq, dkv = backward(acc, ws1)
        assert torch.isfinite(dq).all() and torch.isfinite(dkv).all() and torch.isfinite(ws1).all()
        backward(ordered1, ws1)
        backward(ordered2, ws2)
        backward(atomic, None)
    finally:
        lib.vmg_win3d_variant(prev)
    tag = f"{ROUTE_NAME[route]} {gid}"
    got = dict(out=out, lse=lse, dq=dq, dkv=dkv, dtable=acc - pattern)
    got = {n: t.double().cpu() for n, t in got.items()}
    keep = lambda d: {n: v for n, v in d.items() if n in got}
    bad = _check(tag + " (dtable onto a pattern)", dict(got, dbq=None, dbkv=None), dict(keep(ref), dbq=None, dbkv=None), sc, keep(floor), keep(bnd))
    assert not bad, tag + ": " + "; ".join(bad)
    assert torch.equal(ordered1, ordered2), f"{tag}: ordered table gradient differs between two runs by {float((ordered1 - ordered2).abs().max()):.3e}"
    room = 2.0 * nwin * 2.0 ** -24 * ws1.double().abs().sum(0).t()  # (nrel, heads)
    over = (atomic.double() - ordered1.double()).abs() - room
    print(f"[win3d] {tag} atomics vs ordered: max |diff| {float((atomic - ordered1).abs().max()):.3e}, least room left {float(-over.max()):.3e}")
    assert float(over.max()) <= 0.0, f"{tag}: float-atomics table gradient is {float(over.max()):.3e} beyond two summation orders of the same partials"


def test_win3d_refuses_what_it_cannot_run():
    """Host-side checks of the entry: a shift outside the window, a temporal window above 8 and a head dimension above 64 are errors, not launches."""
    from vmg_amd import hip, kernels as K
    mk = lambda C, wt, heads: (torch.zeros(1, wt, 8, 8, C, device="cuda"), torch.zeros(1, wt, 8, 8, 2 * C, device="cuda"),
                               None, None, torch.zeros((2 * wt - 1) * 225, heads, device="cuda"), heads, wt)
    with pytest.raises(hip.HipError):
        K.win3d_attn_forward(*mk(32, 2, 4), (2, 0, 0))
    with pytest.raises(hip.HipError):
        K.win3d_attn_forward(*mk(32, 2, 4), (0, 8, 0))
    with pytest.raises(hip.HipError):
        K.win3d_attn_forward(*mk(32, 9, 4), (0, 0, 0))
    with pytest.raises(hip.HipError):
        K.win3d_attn_forward(*mk(130, 2, 2), (0, 0, 0))


@pytest.mark.parametrize("geom", [(1, 4, 16, 16, 144, 8, 4, (0, 0, 0)), (1, 4, 16, 16, 144, 8, 4, (2, 4, 4)), (2, 5, 8, 16, 32, 4, 2, (1, 4, 4)),
                                  (1, 2, 20, 20, 32, 4, 2, (0, 0, 0)), (1, 2, 20, 12, 32, 4, 2, (1, 4, 4)), (1, 8, 8, 8, 64, 8, 4, (2, 0, 0)),
                                  (1, 6, 8, 8, 48, 2, 6, (3, 4, 4)), (1, 8, 8, 16, 64, 4, 8, (4, 4, 4))])
def test_win3d_mfma_matches_the_valu_kernel(geom):
    """Forward output and log-sum-exp, and every gradient (q, kv, bias table, the q / kv Linear biases through padded positions), of the MFMA
    kernels vs the VALU kernel on the same bf16 tensors.  Shapes: head dimensions 18, 8, 4, 24, 16; temporal windows 2, 4, 6, 8; shifted and
    unshifted blocks; frames and maps that need padding (D = 5 with wt = 2, 20 x 20, 20 x 12).  Stated: output within 2e-2 of its scale (the
    probabilities enter the PV product as bf16), gradients within 3e-2 of each tensor's scale.  lse: ABSOLUTE, in nats, 4 x the floor of this
    geometry (what rounding the padded positions' biases to bf16 does to the fp64 reference's lse: the VALU kernel takes them in fp32, the MFMA
    operands round them like every real token's; never below 2^-16 nat), and never above the earlier 1e-3 of max |lse| (which is 0.097 nat where
    a query sees masked keys only, lse ~ -96.8)."""
    from oracle import recipe as R
    from vmg_amd import hip, kernels as K
    B, D, H, W, C, heads, wt, shift = geom
    dt = torch.bfloat16
    q = R.seeded((B, D, H, W, C), 1300, 0.7).to(dt).cuda()
    kv = R.seeded((B, D, H, W, 2 * C), 1301, 0.7).to(dt).cuda()
    bq = R.seeded((C,), 1302, 0.3).cuda()
    bkv = R.seeded((2 * C,), 1303, 0.3).cuda()
    table = R.seeded(((2 * wt - 1) * 225, heads), 1304, 0.5).cuda()
    dout = R.seeded((B, D, H, W, C), 1305).to(dt).cuda()
    lib = hip.lib()
    prev = lib.vmg_win3d_variant(-1)
    res = []
    try:
        for variant in (0, 1):
            lib.vmg_win3d_variant(variant)
            out, lse = K.win3d_attn_forward(q, kv, bq, bkv, table, heads, wt, shift)
            dq, dkv, dtable, dbq, dbkv = K.win3d_attn_backward(q, kv, bq, bkv, table, out, lse, dout, heads, wt, shift)
            res.append([t.float().cpu() for t in (out, lse, dq, dkv, dtable, dbq, dbkv)])
    finally:
        lib.vmg_win3d_variant(prev)
    assert prev == 1
    g = WC.Geom("mfma-vs-valu-" + "-".join(str(v) for v in geom), B, D, H, W, C, heads, wt, shift, True, "", "")
    lse_bound = WC.reference_and_bounds(g, dt)[4]["lse"][0]  # (make_inputs draws the tensors above from the same seeds)
    names = ["out", "lse", "dq", "dkv", "dtable", "dbq", "dbkv"]
    tols = [2e-2, 1e-3, 3e-2, 3e-2, 3e-2, 3e-2, 3e-2]
    for n, tol, a, b in zip(names, tols, res[0], res[1]):
        assert torch.isfinite(b).all(), n
        scale = max(float(a.abs().max()), 1e-6)
        err = float((a - b).abs().max())
        if n == "lse":
            print(f"[win3d] mfma vs valu {geom} lse: {err:.3e} nat | bound {lse_bound:.3e} | earlier bound {tol * scale:.3e}")
            assert err <= min(lse_bound, tol * scale), f"lse: max |valu - mfma| = {err:.3e} nat > {min(lse_bound, tol * scale):.3e} ({geom})"
            continue
        assert err <= tol * scale, f"{n}: max |valu - mfma| = {err:.3e} at scale {scale:.3e} ({geom})"
