"""CPU checks of tests/layernorm_ref.py, the fp64 reference and the rounding-error bounds that tests/test_layernorm_kernels_gpu.py holds the
LayerNorm kernels to: the references equal torch's fp64 layer_norm and its autograd, the row maps equal the oracle's rearrangement, an
fp32 emulation of the kernels' arithmetic (four summation orders, storage roundings, the rsqrtf allowance in both directions) stays
within every bound, and the bounds reject six seeded wrong implementations.

One storage ulp on one element is rejected where the storage rounding is the bound (bf16 y and dx).  In fp32 the derived bound of y and
dx is about C / 2 ulp by construction, so no a-priori bound can see one ulp there; fp32 is covered by the exact integer db sums of the
GPU test instead."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import layernorm_ref as R

F64, F32, BF16 = R.F64, R.F32, R.BF16
U = R.U

# (dtype, C): every channel case of the GPU test
CHANNELS = [(BF16, c) for c in (144, 112, 128, 384, 512, 576, 1032, 2048, 36, 180, 6, 70, 45, 129, 1)] + \
           [(F32, c) for c in (144, 36, 384, 576, 1024, 6, 45, 1)]
IDS = [f"{'bf16' if d == BF16 else 'fp32'}-{c}" for d, c in CHANNELS]
ORDERS = ("seq", "rev", "tree", "perm")


def ragged_rows(dtype, C):
    i = R.instantiation(dtype, C, 1)
    return 3 * 8 * i.rpb + 5


@functools.lru_cache(maxsize=None)
def case(dtype, C):
    M = ragged_rows(dtype, C)
    x = R.make_rows(M, C, dtype, 11 * C + (dtype == BF16))
    w, b = R.make_affine(C, C + 1)
    return M, x, w, b


# ------------------------------------------------------------------------------------------------ the references themselves
@pytest.mark.parametrize("dtype,C", [(BF16, 144), (F32, 45), (F32, 1), (BF16, 6)])
def test_reference_equals_torch_fp64(dtype, C):
    M, x, w, b = case(dtype, C)
    dys = R.make_grads((M, C), dtype, 5, 3)
    add = R.make_grads((M, C), dtype, 6)[0]
    xr, wr, br = x.to(F64).requires_grad_(), w.to(F64).requires_grad_(), b.to(F64).requires_grad_()
    y = F.layer_norm(xr, (C,), wr, br, R.EPS)
    y.backward(R.sum_grads(dys).to(F64))
    ry, rmu, rrs = R.ln_fwd_ref(x, w, b)
    scale = float(y.detach().abs().max())
    assert float((ry - y.detach()).abs().max()) <= 1e-12 * scale
    assert float((rmu - x.to(F64).mean(-1)).abs().max()) <= 1e-13 * float(x.to(F64).abs().max())
    # the backward takes the statistics as given: hand it the exact ones (fp64) to compare with autograd
    dx, dw, db = R.ln_bwd_ref(dys, x, rmu, rrs, w, add)
    for got, want in ((dx, xr.grad + add.to(F64)), (dw, wr.grad), (db, br.grad)):
        # (1e-9: torch's own fp64 rounding on rows of magnitude 1e3 with rstd up to 316 -- still seven orders below any fp32 bound)
        assert float((got - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max()))


def test_sum_grads_is_fp32_in_list_order_rounded_once():
    a, b, c = (t.to(BF16) for t in (torch.tensor([1.0]), torch.tensor([2.0 ** -9]), torch.tensor([2.0 ** -9])))
    # 256 + 1 + 1: fp32 keeps 258, which bf16 holds; bf16 adds would lose each 1 in turn (256 + 1 -> 256)
    assert R.sum_grads([a]) is a
    assert float(R.sum_grads([a, b, c])) == float((a.float() + b.float() + c.float()).to(BF16))
    assert float(R.sum_grads([torch.tensor([256.0]).to(BF16), torch.tensor([1.0]).to(BF16), torch.tensor([1.0]).to(BF16)])) == 258.0


@pytest.mark.parametrize("mode,shape", [("down", (2, 6, 10, 9)), ("up", (2, 3, 5, 24)), ("down", (1, 2, 2, 1)), ("up", (1, 1, 1, 4))])
def test_row_maps_equal_the_oracle_spelling(mode, shape):
    from oracle import vmg_oracle as O
    N, H, W, C = shape
    x = torch.arange(N * H * W * C, dtype=F64).reshape(shape)
    rows = R.rows_of(x, mode)
    Cr = rows.shape[-1]
    sd = {"p.norm.weight": torch.ones(Cr, dtype=F64), "p.norm.bias": torch.zeros(Cr, dtype=F64),
          "p.linear.weight": torch.eye(Cr, dtype=F64), "p.linear.bias": torch.zeros(Cr, dtype=F64)}
    want = O.updown(sd, "p.", x[None], mode)[0]
    got = F.layer_norm(rows, (Cr,), None, None, 1e-5)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12
    # the same order, element by element, as ln_src_elem spells it
    for n, y, xx, c in ((0, 0, 0, 0), (N - 1, rows.shape[1] - 1, rows.shape[2] - 1, Cr - 1), (0, rows.shape[1] - 1, 0, Cr // 2)):
        if mode == "down":
            sg, cc = divmod(c, C)
            src = x[n, 2 * y + (sg & 1), 2 * xx + (sg >> 1), cc]
        else:
            src = x[n, y // 2, xx // 2, ((xx & 1) * 2 + (y & 1)) * Cr + c]
        assert rows[n, y, xx, c] == src
    assert torch.equal(R.input_of(rows, mode), x)


def test_launcher_restatement():
    """The (V, G, NV) the issue's enumeration lists, the never-launched pairs, the refusals and the block counts."""
    want = {(BF16, 144): (8, 16, 2, 2), (BF16, 112): (8, 16, 1, 1), (BF16, 128): (8, 16, 1, 1), (BF16, 384): (8, 16, 4, 3),
            (BF16, 512): (8, 16, 4, 4), (BF16, 576): (8, 32, 4, 3), (BF16, 1032): (8, 64, 4, 3), (BF16, 2048): (8, 64, 4, 4),
            (BF16, 36): (4, 16, 1, 1), (BF16, 180): (4, 16, 4, 3), (BF16, 6): (2, 16, 1, 1), (BF16, 70): (2, 16, 4, 3),
            (BF16, 45): (1, 16, 4, 3), (BF16, 129): (1, 64, 4, 3), (F32, 144): (4, 16, 4, 3), (F32, 384): (4, 32, 4, 3),
            (F32, 576): (4, 64, 4, 3), (F32, 1024): (4, 64, 4, 4), (F32, 36): (4, 16, 1, 1)}
    for (dt, C), t in want.items():
        assert tuple(R.instantiation(dt, C, 100)[:4]) == t, (dt, C)
    pairs = {(i.G, i.NV) for dt in (BF16, F32) for C in range(1, 2049) for i in [R.instantiation(dt, C, 1)] if i}
    assert pairs == {(16, 1), (16, 2), (16, 4), (32, 4), (64, 4)}
    assert all(R.instantiation(dt, C, 1) is None for dt, C in ((BF16, 2056), (F32, 1028), (BF16, 257), (F32, 257)))
    i = R.instantiation(BF16, 144, 32 * 8 * 16)
    assert (i.bwd_blocks, R.bwd_adds_into_buffer(i)) == (32, 32)
    i = R.instantiation(BF16, 144, 32 * 8 * 16 + 1)
    assert (i.bwd_blocks, R.bwd_adds_into_buffer(i)) == (33, 1)
    assert R.instantiation(BF16, 144, 114688)[-2:] == (1024, 512) and R.instantiation(F32, 129, 512 * 8 * 4 + 35)[-2:] == (1024, 512)
    assert R.instantiation(BF16, 24, 10, vmax=R.ln_vec(BF16, 6)).V == 2


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels
def esum(t, order, dim=-1, seed=0):
    """The fp32 sum of t along dim in one order: sequential, reversed, pairwise tree, or a seeded permutation."""
    t = t.movedim(dim, 0)
    n = t.shape[0]
    if order == "perm":
        t = t[torch.randperm(n, generator=torch.Generator().manual_seed(seed))]
    if order == "rev":
        t = t.flip(0)
    if order == "tree":
        while t.shape[0] > 1:
            if t.shape[0] % 2:
                t = torch.cat([t, torch.zeros_like(t[:1])])
            t = t[0::2] + t[1::2]
        return t[0]
    acc = t[0].clone()
    for i in range(1, n):
        acc = acc + t[i]
    return acc


def emul_rsqrt(q, direction):
    """An rsqrtf that uses the whole allowance: the exact value moved by U relative in `direction`, then rounded to fp32 (<= 2 U in all)."""
    return ((q.to(F64) ** -0.5) * (1.0 + direction * U)).to(F32)


def emul_fwd(x, w, b, order, direction, one_pass=False, drop_slot=None, seed=0):
    """The forward kernel's arithmetic in fp32 CPU ops (every one IEEE, none fused).  one_pass / drop_slot: the seeded mutations."""
    C = x.shape[-1]
    xf = x.to(F32)
    live = torch.ones(C, dtype=torch.bool) if drop_slot is None else ~drop_slot
    mu = esum(xf[:, live], order, seed=seed) / C
    if one_pass:
        q = esum(xf * xf, order, seed=seed + 1) / C - mu * mu
    else:
        d = xf[:, live] - mu[:, None]
        q = esum(d * d, order, seed=seed + 1) / C
    rs = emul_rsqrt(q + R.EPS, direction)
    y = ((xf - mu[:, None]) * rs[:, None]) * w + b
    return y.to(x.dtype), mu, rs


def emul_bwd(dys, x, mean, rstd, w, add, order, twice_last=False, seed=0):
    xf, dy = x.to(F32), R.sum_grads(dys).to(F32)
    C = x.shape[-1]
    xh = (xf - mean[:, None]) * rstd[:, None]
    g = dy * w
    s1 = esum(g, order, seed=seed) / C
    s2 = esum(g * xh, order, seed=seed + 1) / C
    dx = (rstd[:, None] * ((g - s1[:, None]) - xh * s2[:, None])).to(x.dtype)
    if add is not None:
        dx = (dx.to(F32) + add.to(F32)).to(x.dtype)
    pw, pb = dy * xh, dy
    if twice_last:
        pw, pb = torch.cat([pw, pw[-1:]]), torch.cat([pb, pb[-1:]])
    return dx, esum(pw, order, dim=0, seed=seed + 2), esum(pb, order, dim=0, seed=seed + 3)


def within(got, ref, bound):
    return R.worst_ratio(got, ref, bound) <= 1.0


@pytest.mark.parametrize("dtype,C", CHANNELS, ids=IDS)
def test_emulation_stays_within_every_bound(dtype, C):
    M, x, w, b = case(dtype, C)
    fb = R.ln_fwd_bounds(x, w, b)
    ratios = {}
    for order in ORDERS:
        for direction in (-1, 1):
            y, mu, rs = emul_fwd(x, w, b, order, direction, seed=C)
            for name, got, ref, bound in (("y", y, fb.y, fb.By), ("mean", mu, fb.mean, fb.Bmean), ("rstd", rs, fb.rstd, fb.Brstd)):
                ratios[name] = max(ratios.get(name, 0.0), R.worst_ratio(got, ref, bound))
    # the backward on the fp32-rounded REFERENCE statistics, as the GPU test runs it
    mean32, rstd32 = fb.mean.to(F32), fb.rstd.to(F32)
    for ndy, with_add in ((1, False), (1, True), (5, True), (3, False)):
        dys = R.make_grads((M, C), dtype, 100 + ndy, ndy)
        add = R.make_grads((M, C), dtype, 200)[0] if with_add else None
        bb = R.ln_bwd_bounds(dys, x, mean32, rstd32, w, add)
        for order in ORDERS:
            dx, dw, db = emul_bwd(dys, x, mean32, rstd32, w, add, order, seed=C)
            for name, got, ref, bound in (("dx+add" if with_add else "dx", dx, bb.dx, bb.Bdx), ("dw", dw, bb.dw, bb.Bdw), ("db", db, bb.db, bb.Bdb)):
                ratios[name] = max(ratios.get(name, 0.0), R.worst_ratio(got, ref, bound))
    print(IDS[CHANNELS.index((dtype, C))], " ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    c = R.const_row(M)
    assert float(fb.y[c].sub(b.to(F64)).abs().max()) == 0.0  # the exactly constant row: xh = 0, y = b, the bound is |w| rs Emu (+ rounding)


def test_integer_db_is_exact_in_the_emulation():
    for dtype in (BF16, F32):
        dys = R.int_grads((4097, 6), dtype, 3, 5)
        x = R.make_rows(4097, 6, dtype, 1)
        _, mu, rs = R.ln_fwd_ref(x, *R.make_affine(6, 1))
        for order in ORDERS:
            db = emul_bwd(dys, x, mu.to(F32), rs.to(F32), R.make_affine(6, 1)[0], None, order)[2]
            assert torch.equal(db.to(F64), R.ln_bwd_ref(dys, x, mu.to(F32), rs.to(F32), R.make_affine(6, 1)[0])[2])


# ------------------------------------------------------------------------------------------------ the bounds reject wrong kernels
@pytest.mark.parametrize("dtype,C", [c for c in CHANNELS if c[1] > 1], ids=[i for i, c in zip(IDS, CHANNELS) if c[1] > 1])
def test_bounds_reject_wrong_implementations(dtype, C):
    M, x, w, b = case(dtype, C)
    fb = R.ln_fwd_bounds(x, w, b)
    mean32, rstd32 = fb.mean.to(F32), fb.rstd.to(F32)
    dys = R.make_grads((M, C), dtype, 101, 1)
    bb = R.ln_bwd_bounds(dys, x, mean32, rstd32, w)
    y, mu, rs = emul_fwd(x, w, b, "tree", 1)
    dx, dw, db = emul_bwd(dys, x, mean32, rstd32, w, None, "tree")
    assert within(y, fb.y, fb.By) and within(dx, bb.dx, bb.Bdx) and within(dw, bb.dw, bb.Bdw) and within(db, bb.db, bb.Bdb)

    # 1. the affine weight (and bias) of channel c + 1
    wn, bn = torch.roll(w, -1), torch.roll(b, -1)
    assert not within(emul_fwd(x, wn, b, "tree", 1)[0], fb.y, fb.By), "forward with the neighbour's weight passes"
    assert not within(emul_fwd(x, w, bn, "tree", 1)[0], fb.y, fb.By), "forward with the neighbour's bias passes"
    assert not within(emul_bwd(dys, x, mean32, rstd32, wn, None, "tree")[0], bb.dx, bb.Bdx), "backward with the neighbour's weight passes"

    # 2. the statistics of the next row
    m2, r2 = torch.roll(mu, -1), torch.roll(rs, -1)
    assert not within(m2, fb.mean, fb.Bmean) and not within(r2, fb.rstd, fb.Brstd)
    y2 = (((x.to(F32) - m2[:, None]) * r2[:, None]) * w + b).to(dtype)
    assert not within(y2, fb.y, fb.By), "forward on the next row's statistics passes"
    assert not within(emul_bwd(dys, x, torch.roll(mean32, -1), torch.roll(rstd32, -1), w, None, "tree")[0], bb.dx, bb.Bdx)

    # 3. a one-pass variance E[x^2] - mu^2: x^2 ~ 2500 on the offset rows loses the variance (1) to rounding
    _, _, rs3 = emul_fwd(x, w, b, "tree", 1, one_pass=True)
    off = slice(1, None, 4)
    assert not within(rs3[off], fb.rstd[off], fb.Brstd[off]), "one-pass variance passes on the offset rows (rstd)"
    # (y alone would not show it at large C: there the a-priori error of a mean of C values near 50, |w| rs Emu, dominates y's bound)

    # 4. the last row counted twice in dw / db
    _, dw4, db4 = emul_bwd(dys, x, mean32, rstd32, w, None, "tree", twice_last=True)
    assert not within(dw4, bb.dw, bb.Bdw) and not within(db4, bb.db, bb.Bdb)

    # 5. nv == 3 on the 4-vector instantiation: the vectors of the third lane slot (vi in [2G, 3G)) dropped from the row sums
    i = R.instantiation(dtype, C, M)
    if i.nv == 3:
        ch = torch.arange(C) // i.V
        slot = (ch >= 2 * i.G) & (ch < 3 * i.G)
        assert slot.any()
        y5, mu5, rs5 = emul_fwd(x, w, b, "tree", 1, drop_slot=slot)
        assert not within(mu5, fb.mean, fb.Bmean) and not within(rs5, fb.rstd, fb.Brstd) and not within(y5, fb.y, fb.By)
        dys5 = [torch.where(slot, torch.zeros((), dtype=dtype), dys[0])]
        dx5, dw5, db5 = emul_bwd(dys5, x, mean32, rstd32, w, None, "tree")
        assert not within(dx5, bb.dx, bb.Bdx) and not within(dw5[slot], bb.dw[slot], bb.Bdw[slot]) and not within(db5[slot], bb.db[slot], bb.Bdb[slot])

    # 6. one storage ulp on one element, away from the reference.  bf16 only (module docstring); the element is the first whose
    # significand is below 1.5, where one ulp (2^(e-7)) exceeds the half-ulp bound u |v| < 0.75 * 2^(e-7) by more than E32
    if dtype == BF16:
        for got, ref, bound in ((y, fb.y, fb.By), (dx, bb.dx, bb.Bdx)):
            g64 = got.to(F64).flatten()
            mant = g64.abs() / 2.0 ** torch.floor(torch.log2(g64.abs().clamp_min(1e-30)))
            ok = ((mant < 1.5) & (g64.abs() > 2.0 ** -6) & (g64.abs() < 2.0 ** 6)).nonzero()
            assert ok.numel(), "no element to move"
            k = int(ok[0])
            ulp = 2.0 ** (math.floor(math.log2(abs(float(g64[k])))) - 7)
            away = 1.0 if float(g64[k]) >= float(ref.flatten()[k]) else -1.0
            moved = got.clone().flatten()
            moved[k] = float(g64[k]) + away * ulp
            assert float(moved[k]) != float(g64[k])
            assert not within(moved.reshape(got.shape), ref, bound), "one bf16 ulp on one element passes"
