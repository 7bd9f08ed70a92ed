"""Every instantiation of the LayerNorm kernels (csrc/elementwise.hip: layernorm_fwd_kernel, layernorm_bwd_kernel, the space<->depth forms
and their launchers) against the fp64 reference and the derived per-element bounds of tests/layernorm_ref.py (checked on the CPU by
tests/test_layernorm_ref.py).  Inputs are made on the CPU with fixed seeds and rounded to the tested dtype; the reference sees the
rounded values; every element of every output is compared; no bound is a measured figure.  The backward is handed the fp32-rounded
REFERENCE statistics, not those of the kernel's own forward, so its bound does not depend on the forward.

Case ids read `dtype-C-V-G-NV[via nv]-M-blocks<forward>f<backward>b-<atomics|ws>` (tests/layernorm_ref.py: case_id).

  channel cases, M = 3 * 8 * rpb + 5 (rpb = 256 / G rows per block: 3 full backward blocks + 5 rows, 7 forward blocks, clamped second rows)
    bf16  144 (8,16,2)      112 (8,16,1)       128 (8,16,1, every lane full)   384 (8,16,4 via nv=3)   512 (8,16,4)
          576 (8,32,4 via 3)  1032 (8,64,4 via 3)  2048 (8,64,4, the maximum; 64 KiB of LDS in the backward)
          36 (4,16,1)   180 (4,16,4 via 3)   6 (2,16,1)   70 (2,16,4 via 3)   45 (1,16,4 via 3)   129 (1,64,4 via 3)   1 (1,16,1)
    fp32  144 (4,16,4 via 3)   36 (4,16,1)   384 (4,32,4 via 3)   576 (4,64,4 via 3)   1024 (4,64,4, the maximum)   6 (2,16,1)
          45 (1,16,4 via 3)   1 (1,16,1)
    backward forms: all six at bf16 144 (SPEC 2 for one+add, SPEC 3 for five+add, SPEC 0 else), fp32 144 and bf16 36 (run-time SPEC 0
    for all); `one` and `five+add` everywhere else.
  row sweeps at bf16 144, fp32 144, bf16 1032:
    M = 1 (one live row, its partner clamped onto itself: `keep`), 2, rpb + 1 (second block, one row), 8 rpb + 1 (second backward block),
    32 * 8 * rpb (32 backward blocks: the last launch on plain atomics), 32 * 8 * rpb + 1 (33: sub-accumulator workspace + ticket).
    Each also with integer gradients (one, and five summed): db is then exact.
  past the block caps: fp32 129 (1,64,4 via 3) at M = 512 * 8 * 4 + 35 (1024 forward / 512 backward blocks, several trips of the row loop,
    a clamped last pair); the forward at the bench shape 114 688 x 144 bf16 (1024 blocks, 7 rows per lane group).
  space<->depth (N = 2): the table at MAPPED; `down 96x88x36` has 4224 rows: 33 backward blocks, the workspace path through the map.
  autograd nodes, refusals, and contiguous-but-misaligned tensors through the functional entries: at the end."""
import functools

import pytest
import torch

from tests import layernorm_ref as R

pytestmark = pytest.mark.gpu

F64, F32, BF16 = R.F64, R.F32, R.BF16
EPS = R.EPS
DT = {BF16: "bf16", F32: "fp32"}

CHANNELS = [(BF16, c) for c in (144, 112, 128, 384, 512, 576, 1032, 2048, 36, 180, 6, 70, 45, 129, 1)] + \
           [(F32, c) for c in (144, 36, 384, 576, 1024, 6, 45, 1)]
ALL_FORMS = [(BF16, 144), (F32, 144), (BF16, 36)]
# name -> (number of output gradients, with the skip gradient)
FORMS = {"one": (1, False), "one_add": (1, True), "two_add": (2, True), "three": (3, False), "five": (5, False), "five_add": (5, True)}
SWEEP = [(BF16, 144), (F32, 144), (BF16, 1032)]


def ragged(dtype, C):
    return 3 * 8 * R.instantiation(dtype, C, 1).rpb + 5


def sweep_rows(dtype, C):
    rpb = R.instantiation(dtype, C, 1).rpb
    return [1, 2, rpb + 1, 8 * rpb + 1, 32 * 8 * rpb, 32 * 8 * rpb + 1]


CHANNEL_CASES = [(d, c, ragged(d, c)) for d, c in CHANNELS]
SWEEP_CASES = [(d, c, m) for d, c in SWEEP for m in sweep_rows(d, c)]
CAP_CASE = (F32, 129, 512 * 8 * 4 + 35)
BENCH_CASE = (BF16, 144, 28 * 64 * 64)
BWD_CASES = [(cs, f) for cs in CHANNEL_CASES for f in (FORMS if cs[:2] in ALL_FORMS else ("one", "five_add"))] + \
            [(cs, f) for cs in SWEEP_CASES + [CAP_CASE] for f in ("one", "five_add")]


def cid(cs):
    return R.case_id(*cs)


@functools.lru_cache(maxsize=4)
def fwd_case(dtype, C, M):
    """Inputs and forward reference of one case, made once and shared (never modified) by the tests that need it."""
    x = R.make_rows(M, C, dtype, 11 * C + (dtype == BF16) + 7 * M)
    w, b = R.make_affine(C, C + 1)
    fb = R.ln_fwd_bounds(x, w, b)
    return x, w, b, fb, fb.mean.to(F32), fb.rstd.to(F32)


def check(tag, name, got, ref, bound):
    """Every element within its bound; prints the worst error / bound ratio (the RATIO lines of a run with -s)."""
    got = got.detach().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got.to(F32)).all()), f"{tag} {name}: non-finite values"
    ratio = R.worst_ratio(got, ref, bound)
    print(f"RATIO {tag} {name} {ratio:.3f}")
    if ratio > 1.0:
        err = (got.to(F64) - ref).abs()
        bad = (err > bound).nonzero()
        k = tuple(bad[0].tolist())
        raise AssertionError(f"{tag} {name}: {bad.shape[0]} of {ref.numel()} elements out of bound, worst ratio {ratio:.3f}; first at {k}: "
                             f"got {float(got[k])!r} want {float(ref[k])!r} bound {float(bound[k]):.3e}")


def workspace_is_zero(K, device):
    ws = K._layernorm_workspace(device)
    assert ws is not None and ws.numel() == K.hip.lib().vmg_layernorm_bwd_ws_bytes() and ws.data_ptr() % 16 == 0
    assert not bool(ws.any()), "the LayerNorm backward left its workspace (or its arrival counter) non-zero"


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


# ================================================================================================ forward
@pytest.mark.parametrize("cs", CHANNEL_CASES + SWEEP_CASES + [CAP_CASE, BENCH_CASE], ids=cid)
def test_forward(cs):
    from vmg_amd import kernels as K
    dtype, C, M = cs
    x, w, b, fb, _, _ = fwd_case(*cs)
    gx, gw, gb = x.cuda(), w.cuda(), b.cuda()
    y, mean, rstd = K.layernorm_forward(gx, gw, gb, EPS)
    assert y.dtype == dtype and y.shape == (M, C) and mean.dtype == F32 and mean.shape == (M,) and rstd.shape == (M,)
    tag = f"fwd {DT[dtype]} {cid(cs)}"
    check(tag, "mean", mean, fb.mean, fb.Bmean)
    check(tag, "rstd", rstd, fb.rstd, fb.Brstd)
    check(tag, "y", y, fb.y, fb.By)
    c = R.const_row(M)
    if c is not None:  # the exactly constant row: xh = 0 in the reference, so y = b up to the mean's error (and the storage rounding)
        tol = (w.to(F64).abs() * fb.rstd[c] * fb.Emu[c]) * (1 + R.unit(dtype)) + (R.unit(dtype) if dtype == BF16 else R.U) * b.to(F64).abs()
        assert bool(((y[c].cpu().to(F64) - b.to(F64)).abs() <= tol).all()), "constant row: y is not b"
    y2, mean2, rstd2 = K.layernorm_forward(gx, gw, gb, EPS)
    assert torch.equal(bits(y2), bits(y)) and torch.equal(bits(mean2), bits(mean)) and torch.equal(bits(rstd2), bits(rstd))
    y3, m3, r3 = K.layernorm_forward(gx, gw, gb, EPS, want_stats=False)
    assert m3 is None and r3 is None and torch.equal(bits(y3), bits(y)), "want_stats=False changes y"
    assert torch.equal(gx.cpu(), x)


# ================================================================================================ backward
def make_backward(cs, form, integers=False):
    dtype, C, M = cs
    ndy, with_add = FORMS[form]
    seed = 1000 * C + 10 * M + sorted(FORMS).index(form)
    make = R.int_grads if integers else R.make_grads
    dys = make((M, C), dtype, seed, ndy)
    add = make((M, C), dtype, seed + 5)[0] if with_add else None
    return dys, add


def run_backward(K, cs, form, integers=False):
    dtype, C, M = cs
    x, w, b, fb, mean32, rstd32 = fwd_case(*cs)
    dys, add = make_backward(cs, form, integers)
    bb = R.ln_bwd_bounds(dys, x, mean32, rstd32, w, add)
    inst = R.instantiation(dtype, C, M)
    gx, gw, gm, gr = x.cuda(), w.cuda(), mean32.cuda(), rstd32.cuda()
    gdys, gadd = [t.cuda() for t in dys], None if add is None else add.cuda()
    arg = gdys[0] if len(gdys) == 1 else gdys
    tag = f"bwd {DT[dtype]} {cid(cs)} {form}{' int' if integers else ''}"

    dx, dw, db = K.layernorm_backward(arg, gx, gm, gr, gw, add=gadd)
    workspace_is_zero(K, gx.device)
    assert dx.dtype == dtype and dx.shape == (M, C) and dw.dtype == F32 and dw.shape == (C,) and db.shape == (C,)
    check(tag, "dx+add" if add is not None else "dx", dx, bb.dx, bb.Bdx)
    check(tag, "dw", dw, bb.dw, bb.Bdw)
    check(tag, "db", db, bb.db, bb.Bdb)
    if integers:  # sums of integers below 2^24: exact in any order, so a dropped, doubled or misplaced row shows
        assert torch.equal(db.cpu().to(F64), bb.db), f"{tag}: db is not the exact integer sum"

    # caller-owned (dw, db) that already hold something: each call ADDS one gradient.  dx has no atomics: equal bits every time
    g = torch.Generator().manual_seed(7)
    dw0 = torch.randn(C, generator=g) if not integers else torch.randint(-8, 9, (C,), generator=g).float()
    db0 = torch.randn(C, generator=g) if not integers else torch.randint(-8, 9, (C,), generator=g).float()
    into = (dw0.cuda(), db0.cuda())
    nadd = R.bwd_adds_into_buffer(inst)
    for k in (1, 2):
        dxk, dwk, dbk = K.layernorm_backward(arg, gx, gm, gr, gw, into=into, add=gadd)
        workspace_is_zero(K, gx.device)
        assert dwk is into[0] and dbk is into[1]
        assert torch.equal(bits(dxk), bits(dx)), f"{tag}: dx differs between two launches"
        check(tag, f"dw_into{k}", dwk, dw0.to(F64) + k * bb.dw, R.into_bound(bb.Bdw, bb.Mdw, dw0, k, nadd))
        check(tag, f"db_into{k}", dbk, db0.to(F64) + k * bb.db, R.into_bound(bb.Bdb, bb.Mdb, db0, k, nadd))
        if integers:
            assert torch.equal(dbk.cpu().to(F64), db0.to(F64) + k * bb.db), f"{tag}: db (into, call {k}) is not the exact integer sum"
    for t, t0 in zip(gdys + [gx], dys + [x]):
        assert torch.equal(t.cpu(), t0), "the backward wrote to an input"


@pytest.mark.parametrize("cs,form", BWD_CASES, ids=[f"{cid(cs)}-{f}" for cs, f in BWD_CASES])
def test_backward(cs, form):
    from vmg_amd import kernels as K
    run_backward(K, cs, form)


@pytest.mark.parametrize("cs", SWEEP_CASES + [CAP_CASE], ids=cid)
def test_backward_integer_gradients_db_exact(cs):
    """Gradients in {-4 .. 4} \\ {0}: exact in bf16, five of them sum to at most 20 (exact again after the storage rounding), and M * 20 < 2^24:
    db must EQUAL the fp64 sum, on both sides of the 32-block threshold, fresh and added into integer-valued buffers."""
    from vmg_amd import kernels as K
    assert cs[2] * 20 + 16 < 2 ** 24
    run_backward(K, cs, "one", integers=True)
    run_backward(K, cs, "five", integers=True)


# ================================================================================================ space<->depth
# (mode, input H, W, Cin, dtype), N = 2
MAPPED = [("down", 6, 10, 36, BF16), ("down", 6, 10, 144, BF16), ("down", 6, 10, 144, F32), ("down", 6, 10, 6, BF16), ("down", 6, 10, 9, BF16),
          ("up", 3, 5, 144, BF16), ("up", 3, 5, 576, BF16), ("up", 3, 5, 576, F32), ("up", 3, 5, 24, BF16), ("down", 96, 88, 36, BF16)]


def mapped_geometry(mc):
    mode, H, W, Cin, dtype = mc
    C, cseg, M = (4 * Cin, Cin, 2 * (H // 2) * (W // 2)) if mode == "down" else (Cin // 4, Cin // 4, 2 * 4 * H * W)
    return C, M, R.ln_vec(dtype, cseg)


def mapped_id(mc):
    C, M, vmax = mapped_geometry(mc)
    return f"{mc[0]}-{mc[1]}x{mc[2]}x{mc[3]}-" + R.case_id(mc[4], C, M, vmax)


@pytest.mark.parametrize("mc", MAPPED, ids=mapped_id)
def test_space_depth(mc):
    from vmg_amd import kernels as K
    mode, H, W, Cin, dtype = mc
    C, M, vmax = mapped_geometry(mc)
    tag = f"map {DT[dtype]} {mapped_id(mc)}"
    # the rows are made by the usual recipe and scattered to the feature map, so the row kinds (and the constant row) are as everywhere
    rows = R.make_rows(M, C, dtype, 31 * Cin + H).reshape((2, H // 2, W // 2, C) if mode == "down" else (2, 2 * H, 2 * W, C))
    x = R.input_of(rows, mode)
    assert x.shape == (2, H, W, Cin) and torch.equal(R.rows_of(x, mode), rows)
    w, b = R.make_affine(C, C + 2)
    fb = R.ln_fwd_bounds(rows, w, b)
    gx, gw, gb = x.cuda(), w.cuda(), b.cuda()
    y, mean, rstd = K.space_depth_ln_forward(gx, mode, gw, gb, EPS)
    assert y.shape == rows.shape and y.dtype == dtype
    check(tag, "mean", mean, fb.mean.reshape(-1), fb.Bmean.reshape(-1))
    check(tag, "rstd", rstd, fb.rstd.reshape(-1), fb.Brstd.reshape(-1))
    check(tag, "y", y, fb.y, fb.By)
    assert torch.equal(bits(K.space_depth_ln_forward(gx, mode, gw, gb, EPS)[0]), bits(y))

    mean32, rstd32 = fb.mean.to(F32).reshape(-1), fb.rstd.to(F32).reshape(-1)
    dy = R.make_grads(rows.shape, dtype, 77 + Cin)[0]
    bb = R.ln_bwd_bounds([dy], rows, mean32, rstd32, w)
    gdy, gm, gr = dy.cuda(), mean32.cuda(), rstd32.cuda()
    dx, dw, db = K.space_depth_ln_backward(gdy, gx, mode, gm, gr, gw)
    workspace_is_zero(K, gx.device)
    assert dx.shape == x.shape and dx.dtype == dtype
    check(tag, "dx", dx, R.input_of(bb.dx, mode), R.input_of(bb.Bdx, mode))   # the scattered gradient over the WHOLE input tensor
    check(tag, "dw", dw, bb.dw, bb.Bdw)
    check(tag, "db", db, bb.db, bb.Bdb)
    g = torch.Generator().manual_seed(9)
    dw0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    into = (dw0.cuda(), db0.cuda())
    nadd = R.bwd_adds_into_buffer(R.instantiation(dtype, C, M, vmax))
    for k in (1, 2):
        dxk, dwk, dbk = K.space_depth_ln_backward(gdy, gx, mode, gm, gr, gw, into=into)
        workspace_is_zero(K, gx.device)
        assert dwk is into[0] and dbk is into[1] and torch.equal(bits(dxk), bits(dx))
        check(tag, f"dw_into{k}", dwk, dw0.to(F64) + k * bb.dw, R.into_bound(bb.Bdw, bb.Mdw, dw0, k, nadd))
        check(tag, f"db_into{k}", dbk, db0.to(F64) + k * bb.db, R.into_bound(bb.Bdb, bb.Mdb, db0, k, nadd))
    # integer gradients through the map: db exact
    idy = R.int_grads(rows.shape, dtype, 78 + Cin)[0]
    _, _, idb = K.space_depth_ln_backward(idy.cuda(), gx, mode, gm, gr, gw)
    assert torch.equal(idb.cpu().to(F64), idy.to(F64).reshape(-1, C).sum(0))


# ================================================================================================ autograd nodes
# One backward block (M <= 8 * rpb rows), so dw / db are one atomic add per channel onto zero: the kernel's sums are then reproducible bit
# for bit and the nodes, which add no arithmetic, must return exactly what the direct kernel calls return.
def _leaf(t):
    return t.cuda().requires_grad_()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=DT.get)
def test_autograd_nodes_equal_the_direct_calls(dtype):
    from vmg_amd import functional as FH
    from vmg_amd import kernels as K
    M, C = 77, 144
    assert R.instantiation(dtype, C, M).bwd_blocks == 1
    xc = R.make_rows(M, C, dtype, 5)
    wc, bc = R.make_affine(C, 6)
    gs = [t.cuda() for t in R.make_grads((M, C), dtype, 8, 4)]
    y0, mean, rstd = K.layernorm_forward(xc.cuda(), wc.cuda(), bc.cuda(), EPS)

    def same(x, w, b, y, want):
        assert torch.equal(bits(y.detach()), bits(y0))
        dx, dw, db = want
        assert torch.equal(bits(x.grad), bits(dx)) and torch.equal(w.grad, dw) and torch.equal(b.grad, db)

    # layer_norm: one gradient
    x, w, b = _leaf(xc), _leaf(wc), _leaf(bc)
    y = FH.layer_norm(x, w, b, EPS)
    y.backward(gs[0])
    same(x, w, b, y, K.layernorm_backward(gs[0], xc.cuda(), mean, rstd, wc.cuda()))

    # layer_norm_skip: the skip gradient summed inside the kernel
    x, w, b = _leaf(xc), _leaf(wc), _leaf(bc)
    y, xs = FH.layer_norm_skip(x, w, b, EPS)
    assert torch.equal(bits(xs.detach()), bits(x.detach()))
    torch.autograd.backward([y, xs], [gs[0], gs[3]])
    same(x, w, b, y, K.layernorm_backward(gs[0], xc.cuda(), mean, rstd, wc.cuda(), add=gs[3]))

    # layer_norm_fan, n = 3, all handles used
    x, w, b = _leaf(xc), _leaf(wc), _leaf(bc)
    ys, xs = FH.layer_norm_fan(x, w, b, EPS, 3)
    assert len(ys) == 3 and all(torch.equal(bits(t.detach()), bits(y0)) for t in ys)
    torch.autograd.backward([*ys, xs], [gs[0], gs[1], gs[2], gs[3]])
    same(x, w, b, ys[0], K.layernorm_backward(gs[:3], xc.cuda(), mean, rstd, wc.cuda(), add=gs[3]))

    # n = 3 with the middle handle unused: its gradient is None and is left out of the sum
    x, w, b = _leaf(xc), _leaf(wc), _leaf(bc)
    ys, xs = FH.layer_norm_fan(x, w, b, EPS, 3)
    torch.autograd.backward([ys[0], ys[2], xs], [gs[0], gs[2], gs[3]])
    same(x, w, b, ys[0], K.layernorm_backward([gs[0], gs[2]], xc.cuda(), mean, rstd, wc.cuda(), add=gs[3]))

    # all handles unused: the skip gradient alone comes back unchanged, the parameters get nothing
    x, w, b = _leaf(xc), _leaf(wc), _leaf(bc)
    ys, xs = FH.layer_norm_fan(x, w, b, EPS, 3)
    xs.backward(gs[3])
    assert torch.equal(bits(x.grad), bits(gs[3]))
    assert all(p.grad is None or not bool(p.grad.any()) for p in (w, b))


@pytest.mark.parametrize("mode", ["down", "up"])
def test_space_depth_autograd_node_equals_the_direct_calls(mode):
    from vmg_amd import functional as FH
    from vmg_amd import kernels as K
    shape = (1, 2, 6, 10, 36) if mode == "down" else (1, 2, 3, 5, 144)
    xc = R.make_grads(shape, BF16, 3)[0]
    C = 144 if mode == "down" else 36
    wc, bc = R.make_affine(C, 4)
    x4 = xc.reshape(2, *shape[2:]).cuda()
    y0, mean, rstd = K.space_depth_ln_forward(x4, mode, wc.cuda(), bc.cuda(), EPS)
    assert R.instantiation(BF16, C, y0.numel() // C, R.ln_vec(BF16, 36)).bwd_blocks == 1
    x, w, b = _leaf(xc), _leaf(wc), _leaf(bc)
    y = FH.space_depth_layer_norm(x, w, b, EPS, mode)
    assert y.shape == (1, 2, *y0.shape[1:]) and torch.equal(bits(y.detach().reshape(y0.shape)), bits(y0))
    dy = R.make_grads(y.shape, BF16, 5)[0].cuda()
    y.backward(dy)
    dx, dw, db = K.space_depth_ln_backward(dy.reshape(y0.shape), x4, mode, mean, rstd, wc.cuda())
    assert torch.equal(bits(x.grad.reshape(dx.shape)), bits(dx)) and torch.equal(w.grad, dw) and torch.equal(b.grad, db)


# ================================================================================================ refusals
def _offset_view(t, dtype, offset):
    """t on the device as a contiguous view `offset` elements into a larger buffer: contiguous, not 16-byte aligned."""
    buf = torch.zeros(t.numel() + 16, dtype=dtype, device="cuda")
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def test_c_entries_refuse_what_the_kernels_cannot_run():
    """Too many channels for 64 lanes x 4 vectors, and misaligned pointers, are refused before anything is launched: a non-zero return, a
    message in vmg_last_error, and the pre-filled outputs unchanged."""
    from vmg_amd import hip
    from vmg_amd import kernels as K
    lib = hip.lib()
    M = 3

    def tensors(dtype, C):
        x = torch.ones((M, C), dtype=dtype, device="cuda")
        outs = [torch.full((M, C), 7.0, dtype=dtype, device="cuda"), torch.full((M,), 7.0, device="cuda"), torch.full((M,), 7.0, device="cuda"),
                torch.full((C,), 7.0, device="cuda"), torch.full((C,), 7.0, device="cuda")]
        return x, torch.ones(C, device="cuda"), outs

    def unchanged(outs):
        torch.cuda.synchronize()
        return all(bool((t == 7.0).all()) for t in outs)

    def fwd(dtype, x, w, y, mean, rstd, C):
        return lib.vmg_layernorm_fwd(hip.dtype_code(dtype), x.data_ptr(), w.data_ptr(), w.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                     M, C, EPS, hip.stream_ptr())

    def bwd(dtype, dy, x, mean, rstd, w, dx, dw, db, C):
        ws = K._layernorm_workspace(x.device)
        return lib.vmg_layernorm_bwd(hip.dtype_code(dtype), 1, K._ptrs([dy]), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), None,
                                     dx.data_ptr(), dw.data_ptr(), db.data_ptr(), M, C, ws.data_ptr(), hip.stream_ptr())

    for dtype, C in ((BF16, 2056), (F32, 1028), (BF16, 257), (F32, 257)):
        assert R.instantiation(dtype, C, M) is None
        x, w, (y, mean, rstd, dw, db) = tensors(dtype, C)
        assert fwd(dtype, x, w, y, mean, rstd, C) != 0
        assert "too large" in lib.vmg_last_error().decode(), (dtype, C)
        stats = torch.ones(M, device="cuda")
        assert bwd(dtype, x, x, stats, stats, w, y, dw, db, C) != 0
        assert "too large" in lib.vmg_last_error().decode(), (dtype, C)
        assert unchanged([y, mean, rstd, dw, db]), (dtype, C)

    # misaligned pointers (C = 36 bf16: contiguous 72-byte rows, 8 bytes past a 16-byte boundary)
    dtype, C = BF16, 36
    x, w, (y, mean, rstd, dw, db) = tensors(dtype, C)
    xo, yo = _offset_view(x, dtype, 4), _offset_view(y, dtype, 4)
    stats = torch.ones(M, device="cuda")
    for rc in (fwd(dtype, xo, w, y, mean, rstd, C), fwd(dtype, x, w, yo, mean, rstd, C)):
        assert rc != 0 and "16-byte" in lib.vmg_last_error().decode()
    for rc in (bwd(dtype, x, xo, stats, stats, w, y, dw, db, C), bwd(dtype, x, x, stats, stats, w, yo, dw, db, C),
               bwd(dtype, xo, x, stats, stats, w, y, dw, db, C)):
        assert rc != 0 and "16-byte" in lib.vmg_last_error().decode()
    # ... and by the space<->depth backward, which shares the check
    x4 = x.reshape(1, 1, 3, 36)  # 'up': rows (1, 2, 6, 9)
    dy4 = torch.ones((1, 2, 6, 9), dtype=dtype, device="cuda")
    st4 = torch.ones(12, device="cuda")
    ws = K._layernorm_workspace(x.device)
    dw9, db9 = torch.full((9,), 7.0, device="cuda"), torch.full((9,), 7.0, device="cuda")
    rc = lib.vmg_space_depth_ln_bwd(hip.BF16, 2, dy4.data_ptr(), xo.data_ptr(), st4.data_ptr(), st4.data_ptr(), w.data_ptr(), y.data_ptr(),
                                    dw9.data_ptr(), db9.data_ptr(), 1, 2, 6, 9, ws.data_ptr(), hip.stream_ptr())
    assert rc != 0 and "16-byte" in lib.vmg_last_error().decode()
    assert unchanged([y, mean, rstd, dw, db, dw9, db9]) and bool((yo == 7.0).all())
    workspace_is_zero(K, x.device)


def test_functional_entries_take_contiguous_misaligned_tensors():
    """x[1:] of 72-byte rows is contiguous but 8 bytes off a 16-byte boundary: nn.LayerNorm takes it, and so do the functional entries (one
    copy to aligned storage, forward and gradient path); the kernel entry itself keeps refusing.  Checked per element like everything else."""
    from vmg_amd import functional as FH
    from vmg_amd import hip
    from vmg_amd import kernels as K
    dtype, C, M = BF16, 36, 44
    xc = R.make_rows(M, C, dtype, 3)
    wc, bc = R.make_affine(C, 4)
    dyc, addc = R.make_grads((M + 1, C), dtype, 5, 2)
    gx_all, gdy_all, gadd_all = (torch.cat([xc[:1], xc]).cuda()), dyc.cuda(), addc.cuda()
    xv, dyv, addv = gx_all[1:], gdy_all[1:], gadd_all[1:]
    assert all(t.is_contiguous() and t.data_ptr() % 16 == 8 for t in (xv, dyv, addv))
    with pytest.raises(hip.HipError, match="16-byte"):
        K.layernorm_forward(xv, wc.cuda(), bc.cuda(), EPS)
    fb = R.ln_fwd_bounds(xc, wc, bc)
    x, w, b = xv.detach().requires_grad_(), _leaf(wc), _leaf(bc)
    y, xs = FH.layer_norm_skip(x, w, b, EPS)
    check("misaligned", "y", y, fb.y, fb.By)
    assert torch.equal(xs.detach().cpu(), xc)
    torch.autograd.backward([y, xs], [dyv, addv])
    # the node's backward runs on the statistics of its own forward: compare with the reference on exactly those
    _, mean, rstd = K.layernorm_forward(xc.cuda(), wc.cuda(), bc.cuda(), EPS)
    bb = R.ln_bwd_bounds([dyc[1:]], xc, mean.cpu(), rstd.cpu(), wc, addc[1:])
    check("misaligned", "dx+add", x.grad, bb.dx, bb.Bdx)
    check("misaligned", "dw", w.grad, bb.dw, bb.Bdw)
    check("misaligned", "db", b.grad, bb.db, bb.Bdb)
    # the plain node and the mapped one
    x = xv.detach().requires_grad_()
    y = FH.layer_norm(x, wc.cuda(), bc.cuda(), EPS)
    y.backward(dyv)
    check("misaligned", "y", y, fb.y, fb.By)
    bb = R.ln_bwd_bounds([dyc[1:]], xc, mean.cpu(), rstd.cpu(), wc)
    check("misaligned", "dx", x.grad, bb.dx, bb.Bdx)
    x5 = xv.reshape(1, 1, 4, 11, 36)  # 'up': rows (1, 1, 8, 22, 9)
    w9, b9 = R.make_affine(9, 5)
    y = FH.space_depth_layer_norm(x5, w9.cuda(), b9.cuda(), EPS, "up")
    rows = R.rows_of(xc.reshape(1, 4, 11, 36), "up")
    fb9 = R.ln_fwd_bounds(rows, w9, b9)
    check("misaligned", "y_up", y.reshape(rows.shape), fb9.y, fb9.By)
