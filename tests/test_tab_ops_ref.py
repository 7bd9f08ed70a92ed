"""CPU checks of tests/tab_ops_ref.py (no GPU): the fp64 reference that tests/test_tab_ops_gpu.py holds the kernels of csrc/tab_ops.hip and
avgpool2 against is itself held against torch.autograd / torch.nn.functional in fp64."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import tab_ops_ref as R

F64 = torch.float64


def rnd(shape, seed, scale=1.0):
    return scale * torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=F64)


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def bcast(k, R_):
    """(G, C[, n]) -> broadcastable over (G, R, C)."""
    return k[:, None]


def test_group_reduce_modes_and_magnitudes():
    G, R_, C = 3, 7, 6
    a, b, c = (rnd((G * R_, C), 10 + i) for i in range(3))
    v = lambda t: t.reshape(G, R_, C)
    for args, want, wmag in (((a,), v(a).sum(1), v(a).abs().sum(1)),
                             ((a, b), v(a + b).sum(1), (v(a).abs() + v(b).abs()).sum(1)),
                             ((a, b, c), v(a + b + c).sum(1), (v(a).abs() + v(b).abs() + v(c).abs()).sum(1))):
        got, mag = R.group_reduce_ref(args[0], G, *args[1:], mode=0, scale=0.5)
        assert got.shape == (G, C) and close(got, 0.5 * want) and close(mag, 0.5 * wmag)
    got, mag = R.group_reduce_ref(a, G, b, None, 1, 2.0)
    assert close(got, 2.0 * v(a * b).sum(1)) and close(mag, 2.0 * v(a * b).abs().sum(1))
    sq, _ = R.group_reduce_ref(a, G, a, None, 1, 1.0)
    assert close(sq, v(a * a).sum(1))
    # groups are consecutive blocks of rows: a group's sum must not see its neighbour's rows
    z = a.clone().reshape(G, R_, C)
    z[1] = 0
    got, _ = R.group_reduce_ref(z.reshape(G * R_, C), G)
    assert float(got[1].abs().max()) == 0.0 and close(got[0], v(a)[0].sum(0)) and close(got[2], v(a)[2].sum(0))


def test_ca_ops_against_autograd():
    """OP_CA_FWD and OP_CA_BWD: out = (r * g + x) * s with g a function of the per-group mean of r (models/function.py:542-558)."""
    G, R_, C, s = 2, 5, 4, 0.7
    r = rnd((G, R_, C), 1).requires_grad_(True)
    x = rnd((G, R_, C), 2).requires_grad_(True)
    q = rnd((G, C), 3)
    dy = rnd((G, R_, C), 4)
    m = r.mean(1)
    g = torch.sigmoid(m * q)
    out = (r * bcast(g, R_) + x) * s
    (want,), _ = R.tab_elementwise_ref(R.OP_CA_FWD, r, x, coef=g, s=s, G=G)
    assert close(want, out.detach())
    dr, dx = torch.autograd.grad(out, (r, x), dy)
    # the pieces of the backward as functional._ChannelAttention strings them together: dg = s * sum_r dy * r, dm through the gate, / R
    dg, _ = R.group_reduce_ref(dy, G, r, None, 1, s)
    dm = dg * (g * (1 - g) * q).detach() / R_
    (d_r, d_x), _ = R.tab_elementwise_ref(R.OP_CA_BWD, dy, coef=g, add=dm, s=s, G=G)
    assert close(d_r, dr) and close(d_x, dx)
    (sc,), _ = R.tab_elementwise_ref(R.OP_SCALE, dy, coef=g, s=s, G=G)
    assert close(sc, (dy * bcast(g, R_) * s).detach())


def test_gate_ops_against_autograd():
    """OP_GATE_FWD / OP_GATE_BWD: (x + y) * tanh(y); OP_GATE_RES_*: res + gate * g (rounding off: dtype fp64)."""
    G, R_, C = 3, 4, 8
    x = rnd((G, R_, C), 5).requires_grad_(True)
    y = rnd((G, R_, C), 6).requires_grad_(True)
    res = rnd((G, R_, C), 7).requires_grad_(True)
    g = rnd((G, C), 8)
    d = rnd((G, R_, C), 9)
    gate = (x + y) * torch.tanh(y)
    (want,), (mag,) = R.tab_elementwise_ref(R.OP_GATE_FWD, x, y)
    assert close(want, gate.detach()) and bool((mag >= want.abs() * (1 - 1e-15)).all())
    wx, wy = torch.autograd.grad(gate, (x, y), d, retain_graph=True)
    (dx, dy), mags = R.tab_elementwise_ref(R.OP_GATE_BWD, d, x, y)
    assert close(dx, wx) and close(dy, wy)
    assert all(bool((m >= o.abs() * (1 - 1e-15)).all()) for m, o in zip(mags, (dx, dy)))
    out = (gate * bcast(g, R_) + res) * 1.0
    (want,), _ = R.tab_elementwise_ref(R.OP_GATE_RES_FWD, x, y, res, coef=g, s=1.0, G=G, dtype=F64)
    assert close(want, out.detach())
    wx, wy, wr = torch.autograd.grad(out, (x, y, res), d)
    (dx, dy), _ = R.tab_elementwise_ref(R.OP_GATE_RES_BWD, d, x, y, coef=g, s=1.0, G=G, dtype=F64)
    assert close(dx, wx) and close(dy, wy) and close(wr, d)


def test_gate_res_rounds_the_intermediate_to_the_tensor_dtype():
    """The one-pass ops equal the two-pass form, which stored the gate (the scaled gradient) in the tensor dtype between its kernels."""
    G, R_, C = 2, 3, 8
    bf = torch.bfloat16
    x, y, res, d = (rnd((G, R_, C), 20 + i).to(bf) for i in range(4))
    g = rnd((G, C), 24).float()
    (gate,), _ = R.tab_elementwise_ref(R.OP_GATE_FWD, x, y)
    (two,), _ = R.tab_elementwise_ref(R.OP_CA_FWD, gate.to(bf), res, coef=g, s=1.0, G=G)
    (one,), _ = R.tab_elementwise_ref(R.OP_GATE_RES_FWD, x, y, res, coef=g, s=1.0, G=G, dtype=bf)
    assert torch.equal(one, two)
    (unrounded,), _ = R.tab_elementwise_ref(R.OP_GATE_RES_FWD, x, y, res, coef=g, s=1.0, G=G, dtype=F64)
    assert not torch.equal(one, unrounded)
    (ds,), _ = R.tab_elementwise_ref(R.OP_SCALE, d, coef=g, s=1.0, G=G)
    two = R.tab_elementwise_ref(R.OP_GATE_BWD, ds.to(bf), x, y)[0]
    one = R.tab_elementwise_ref(R.OP_GATE_RES_BWD, d, x, y, coef=g, s=1.0, G=G, dtype=bf)[0]
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    v, m = R.gate_res_intermediate(R.OP_GATE_RES_FWD, x, y, res, g, 1.0, G)
    assert torch.equal(v.reshape(gate.shape), gate) and bool((m >= v.abs() * (1 - 1e-15)).all())
    v, _ = R.gate_res_intermediate(R.OP_GATE_RES_BWD, d, x, y, g, 1.0, G)
    assert torch.equal(v.reshape(ds.shape), ds)


def test_bf16_tie_distance():
    bf = torch.bfloat16
    one, nxt = 1.0, 1.0 + 2.0 ** -7  # neighbours in bf16
    tie = (one + nxt) / 2
    v = torch.tensor([tie + 1e-9, tie - 1e-9, one, one + 1e-4, 1.0 - 2.0 ** -9 + 1e-9, -tie - 1e-9, 3.0], dtype=F64)
    d = R.bf16_tie_distance(v)
    assert float(d[0]) <= 2e-9 and float(d[1]) <= 2e-9 and float(d[5]) <= 2e-9
    assert float(d[4]) <= 2e-9                     # just above the tie between 1 - 2^-8 and 1, where the spacing is 2^-8
    assert float(d[2]) >= 2.0 ** -10 - 1e-12 and float(d[6]) >= 2.0 ** -9 - 1e-12
    # never more than the true distance: a perturbation smaller than d leaves the rounding unchanged.  (torch converts fp64 to bf16 through
    # fp32, so the 2^-25 next to a tie is left out.)
    w = rnd((4096,), 31)
    dist = R.bf16_tie_distance(w)
    far = dist > 1e-6 * w.abs()
    assert int(far.sum()) > 4000
    for sign in (-1.0, 1.0):
        assert torch.equal((w + sign * 0.9 * dist)[far].to(bf), w[far].to(bf))
    # and not needlessly small: away from powers of two it IS the distance
    inside = (w.abs() > 1.05) & (w.abs() < 1.95) & far
    assert not torch.equal((w + 1.1 * dist)[inside].to(bf), w[inside].to(bf)) or not torch.equal((w - 1.1 * dist)[inside].to(bf), w[inside].to(bf))


def test_mix_ops_and_group_reduce3_against_autograd():
    """y = h a0 + w a1 + c a2 (models/function.py:791-793) with a loss that also sees the per-group mean of h + w + c, as the re-weighting MLP does."""
    G, R_, C = 2, 6, 4
    hs = [rnd((G, R_, C), 40 + i).requires_grad_(True) for i in range(3)]
    a = rnd((G, C, 3), 43).softmax(-1).requires_grad_(True)
    q = rnd((G, C), 44)
    dy = rnd((G, R_, C), 45)
    y = sum(h * a[:, None, :, k] for k, h in enumerate(hs))
    (want,), _ = R.tab_elementwise_ref(R.OP_MIX_FWD, hs[0], hs[1], hs[2], coef=a, G=G)
    assert close(want, y.detach())
    pooled = (hs[0] + hs[1] + hs[2]).mean(1)
    m, _ = R.group_reduce_ref(hs[0], G, hs[1], hs[2], 0, 1.0 / R_)
    assert close(m, pooled.detach())
    loss = (y * dy).sum() + (pooled * q).sum()
    gh0, gh1, gh2, ga = torch.autograd.grad(loss, hs + [a])
    da, mag = R.group_reduce3_ref(dy, hs[0], hs[1], hs[2], G)
    assert da.shape == (G, C, 3) and close(da, ga) and bool((mag >= da.abs() * (1 - 1e-15)).all())
    outs, _ = R.tab_elementwise_ref(R.OP_MIX_BWD, dy, coef=a, add=q / R_, G=G)
    assert close(outs[0], gh0) and close(outs[1], gh1) and close(outs[2], gh2)


def test_affine2_is_groupnorm1_relu_forward_and_backward():
    """relu(GroupNorm(1, C)(x)) and its backward from two grouped reductions and OP_AFFINE2 each way, with the coefficient algebra of
    functional._GroupNorm1ReLU, against F.group_norm + ReLU through autograd."""
    n, h, w_, c, eps = 3, 4, 5, 6, 1e-5
    x = rnd((n, h, w_, c), 50).requires_grad_(True)
    wt = (1 + 0.3 * rnd((c,), 51)).requires_grad_(True)
    bs = rnd((c,), 52, 0.3).requires_grad_(True)
    dy = rnd((n, h, w_, c), 53)
    want = F.relu(F.group_norm(x.permute(0, 3, 1, 2), 1, wt, bs, eps)).permute(0, 2, 3, 1)
    gx, gw, gb = torch.autograd.grad(want, (x, wt, bs), dy)
    xd, w, b = x.detach(), wt.detach(), bs.detach()
    cnt = h * w_ * c
    s1 = R.group_reduce_ref(xd, n)[0].sum(1)
    s2 = R.group_reduce_ref(xd, n, xd, None, 1)[0].sum(1)
    mu = s1 / cnt
    rs = torch.rsqrt((s2 / cnt - mu * mu).clamp_min(0) + eps)
    coef = torch.stack([rs[:, None] * w[None], torch.zeros(n, c, dtype=F64)], -1)
    add = b[None] - mu[:, None] * rs[:, None] * w[None]
    (y,), _ = R.tab_elementwise_ref(R.OP_AFFINE2, xd, coef=coef, add=add, s=1.0, G=n)
    assert close(y, want.detach(), 1e-10) and float(y.min()) == 0.0
    (lin,), _ = R.tab_elementwise_ref(R.OP_AFFINE2, xd, coef=coef, add=add, s=0.0, G=n)
    assert float(lin.min()) < 0.0 and torch.equal(lin.clamp_min(0), y)
    g = dy * (y > 0)
    S1 = R.group_reduce_ref(g, n)[0]
    S2 = R.group_reduce_ref(g, n, xd, None, 1)[0]
    gxh = rs[:, None] * (S2 - mu[:, None] * S1)
    assert close(gxh.sum(0), gw, 1e-10) and close(S1.sum(0), gb, 1e-10)
    m1 = (S1 * w[None]).sum(1) / cnt
    m2 = (gxh * w[None]).sum(1) / cnt
    coef = torch.stack([(rs[:, None] * w[None]).expand(n, c), (-rs * rs * m2)[:, None].expand(n, c)], -1)
    add = (rs * (mu * rs * m2 - m1))[:, None].expand(n, c)
    (dx,), (mag,) = R.tab_elementwise_ref(R.OP_AFFINE2, g, xd, coef=coef, add=add, s=0.0, G=n)
    assert close(dx, gx, 1e-10) and bool((mag >= dx.abs() * (1 - 1e-15)).all())


def test_maxpool_against_torch_on_tie_free_input():
    for (n, h, w, c), f in (((2, 8, 12, 5), 2), ((2, 8, 12, 5), 4), ((1, 15, 30, 3), 3), ((1, 15, 30, 3), 15)):
        count = n * h * w * c
        x = torch.randperm(count, generator=torch.Generator().manual_seed(60 + f)).to(F64).reshape(n, h, w, c).requires_grad_(True)
        dy = rnd((n, h // f, w // f, c), 61)
        want, flat = F.max_pool2d(x.permute(0, 3, 1, 2), f, f, return_indices=True)
        (gx,) = torch.autograd.grad(want, x, dy.permute(0, 3, 1, 2))
        y, idx, dx = R.maxpool_ref(x, f, dy)
        assert idx.dtype == torch.uint8 and torch.equal(y, want.permute(0, 2, 3, 1)) and torch.equal(dx, gx)
        iy, ix = flat // w, flat % w                                   # ATen's index is flat over the (h, w) plane
        assert torch.equal(idx.long(), ((iy % f) * f + ix % f).permute(0, 2, 3, 1))


def test_maxpool_ties_and_nan():
    """The first maximum in row-major order wins, a NaN beats every number and the first NaN wins; the gradient goes to that one position."""
    nan = float("nan")
    x = torch.tensor([[1.0, 3.0, 2.0, 2.0],
                      [3.0, 0.0, 2.0, 2.0],
                      [5.0, nan, -1.0, -1.0],
                      [nan, 9.0, -1.0, float("-inf")]], dtype=F64).reshape(1, 4, 4, 1)
    dy = torch.tensor([[10.0, 20.0], [30.0, 40.0]], dtype=F64).reshape(1, 2, 2, 1)
    y, idx, dx = R.maxpool_ref(x, 2, dy)
    assert idx.reshape(-1).tolist() == [1, 0, 1, 0]
    assert y.reshape(-1)[:2].tolist() == [3.0, 2.0] and bool(torch.isnan(y.reshape(-1)[2])) and float(y.reshape(-1)[3]) == -1.0
    want = torch.zeros(4, 4, dtype=F64)
    want[0, 1], want[0, 2], want[2, 1], want[2, 2] = 10.0, 20.0, 30.0, 40.0
    assert torch.equal(dx.reshape(4, 4), want)
    # ATen agrees on ties and on a window with one NaN (among several NaNs of one window it keeps the last; the kernel and numpy the first)
    x[0, 3, 0, 0] = 7.0
    ty, tflat = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2, return_indices=True)
    assert tflat.reshape(-1).tolist() == [1, 2, 9, 10] and bool(torch.isnan(ty.reshape(-1)[2]))
    assert R.maxpool_ref(x, 2)[1].reshape(-1).tolist() == [1, 0, 1, 0]


def test_avgpool2_against_torch():
    for shape in ((2, 8, 12, 8), (1, 7, 9, 8), (1, 2, 2, 3), (1, 3, 2, 1)):
        x = rnd(shape, 70)
        y, mag = R.avgpool2_ref(x)
        want = F.avg_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        assert y.shape == want.shape and close(y, want, 1e-15)
        assert close(mag, F.avg_pool2d(x.abs().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1), 1e-15)


def test_op_table_matches_the_reference_branches():
    """OP_USES (what the GPU tests derive their refusals from): an op works with exactly its listed operands and asserts without one of them."""
    G, R_, C = 2, 3, 4
    t = [rnd((G * R_, C), 80 + i) for i in range(3)]
    for op, (extra, ncoef, has_add, nout) in R.OP_USES.items():
        kw = {"p1": t[1] if "p1" in extra else None, "p2": t[2] if "p2" in extra else None,
              "coef": rnd((G, C, ncoef), 83) if ncoef else None, "add": rnd((G, C), 84) if has_add else None}
        outs, mags = R.tab_elementwise_ref(op, t[0], s=1.0, G=G, **kw)
        assert len(outs) == len(mags) == nout and all(o.shape == t[0].shape for o in outs)
        for name in [k for k, v in kw.items() if v is not None]:
            try:
                R.tab_elementwise_ref(op, t[0], s=1.0, G=G, **{**kw, name: None})
            except AssertionError:
                continue
            raise AssertionError(f"{R.OP_NAMES[op]} ran without {name}")
    assert np.array_equal(sorted(R.OP_USES), np.arange(10))
