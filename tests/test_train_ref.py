"""tests/train_ref.py against independent references, on the CPU: adamw_step_ref against torch.optim.AdamW on fp64 parameters, clip_ref
against torch.nn.utils.clip_grad_norm_ in fp32, the matrix form of the loss's Laplacian pyramid against the oracle's loss (value and autograd
gradient) and its adjoint pieces against autograd of the forward matrices."""
import math

import numpy as np
import pytest
import torch

from tests import train_ref as R

F64, F32, U = R.F64, R.F32, R.U


# ================================================================================================ AdamW
@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_adamw_step_ref_is_torch_adamw(wd):
    """Six steps from a fresh state with a changing learning rate (0 on the first two steps of one run), gradients from 1e-10 to 1: the
    chained one-step reference and torch.optim.AdamW(foreach=False) on fp64 parameters agree to fp64 rounding."""
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(257, generator=gen, dtype=F64) * 0.1
    for lrs in ([2e-4 * (1 - 0.1 * s) for s in range(6)], [0.0, 0.0, 1e-6, 1e-3, 1e-3, 5e-4]):
        par = torch.nn.Parameter(p0.clone())
        opt = torch.optim.AdamW([par], lr=lrs[0], betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, foreach=False)
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for t, lr in enumerate(lrs, 1):
            g = torch.randn(257, generator=gen, dtype=F64) * 10.0 ** torch.randint(-10, 1, (257,), generator=gen).double()
            opt.param_groups[0]["lr"] = lr
            par.grad = g.clone()
            opt.step()
            p, m, v, _ = R.adamw_step_ref(p, g, m, v, lr, wd, 0.9, 0.99, 1e-8, t)
            st = opt.state[par]
            assert float((p - par.detach()).abs().max()) <= 1e-14 * float(p.abs().max())
            assert float(((m - st["exp_avg"]).abs() / m.abs().clamp_min(1e-300)).max()) <= 1e-13
            assert float(((v - st["exp_avg_sq"]).abs() / v.abs().clamp_min(1e-300)).max()) <= 1e-13
        assert wd == 0.0 or not torch.equal(p, p0)


def test_adamw_bounds_tell_the_mutations_apart():
    """The bounds are far below what the three arithmetic mistakes of an AdamW kernel change, at the state classes the GPU test plants: decay
    after the update (p = 0), eps dropped, eps inside the bias correction (|g| near eps, t = 1)."""
    lr, wd, b1, b2, eps, t = 2e-3, 0.05, 0.9, 0.99, 1e-8, 1
    z = torch.zeros(3, dtype=F64)
    g = torch.tensor([1e-8, -1e-9, 1e-2], dtype=F64)
    p, m, v, k = R.adamw_step_ref(z, g, z, z, lr, wd, b1, b2, eps, t)
    Bp, Bm, Bv = R.adamw_bounds(k)
    bc1, sq = 1 - b1 ** t, math.sqrt(1 - b2 ** t)
    after = (z - (lr / bc1) * m / (v.sqrt() / sq + eps)) * (1 - lr * wd)
    no_eps = z * (1 - lr * wd) - (lr / bc1) * m / (v.sqrt() / sq)
    inside = z * (1 - lr * wd) - (lr / bc1) * m / ((v.sqrt() + eps) / sq)
    assert bool(((after - p).abs() > 10 * Bp).all())
    assert bool(((no_eps - p).abs() > 10 * Bp)[:2].all()) and bool(((inside - p).abs() > 10 * Bp)[:2].all())
    assert bool((Bp <= 40 * U * k["upd"]).all()) and bool((Bm <= 14 * U * m.abs()).all())


# ================================================================================================ clip
def _torch_clip(g, max_norm):
    par = torch.nn.Parameter(torch.zeros_like(g))
    par.grad = g.clone()
    norm = torch.nn.utils.clip_grad_norm_([par], max_norm, norm_type=2)
    return norm, par.grad


@pytest.mark.parametrize("max_norm", [1e-3, 0.7, 1e6])
@pytest.mark.parametrize("n", [1, 5, 4099])
def test_clip_ref_is_torch_clip_grad_norm(n, max_norm):
    """torch forms the coefficient as reciprocal(norm + 1e-6) * max_norm (Tensor.__rtruediv__): two roundings where clip_ref and the kernel
    divide once, so the coefficients may differ by one unit and the products by U (coefficient) + U (their own rounding) relative.  Below
    the cap the comparison is that; at the cap both leave the gradient's bits alone."""
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen) * 0.02
    tn, tg = _torch_clip(g, max_norm)
    norm, coef, scaled = R.clip_ref(g, max_norm, norm32=float(tn))
    assert abs(float(tn) - float(norm)) <= 4 * U * float(norm)  # (torch's own fp32 reduction)
    if coef < 1:
        assert float(((scaled - tg).abs() / tg.abs().clamp_min(1e-30)).max()) <= 2.01 * U * 2  # (U of a value is up to 2 U of its power of two)
    else:
        assert coef == 1 and torch.equal(R.bits(scaled), R.bits(g)) and torch.equal(R.bits(tg), R.bits(g))


def test_clip_ref_specials_are_torch_s():
    """The cases of the issue: a NaN makes the norm and every element NaN; an Inf makes the norm Inf, the finite elements +-0 and the Inf NaN;
    an all-zero gradient keeps its bits under max_norm 1 and its signed zeros under max_norm 1e-7 (coefficient about 0.1)."""
    nan, inf = float("nan"), float("inf")
    for vals, max_norm in (([1, -2, nan, 0, -0.0], 1.0), ([1, -2, nan, 0, -0.0], 100.0), ([1, -2, inf, 0, -0.0], 1.0), ([0, -0.0, 0, -0.0], 1.0),
                           ([0, -0.0, 0, -0.0], 1e-7)):
        g = torch.tensor(vals, dtype=F32)
        tn, tg = _torch_clip(g, max_norm)
        norm, coef, scaled = R.clip_ref(g, max_norm)
        assert torch.equal(torch.isnan(scaled), torch.isnan(tg)), vals
        ok = ~torch.isnan(tg)
        assert torch.equal(R.bits(scaled)[ok], R.bits(tg)[ok]), vals
        assert (math.isnan(float(tn)) and math.isnan(float(norm))) or float(tn) == float(norm)
    g = torch.tensor([1, -2, nan, 0, -0.0], dtype=F32)
    assert bool(torch.isnan(R.clip_ref(g, 1.0)[2]).all()) and np.isnan(R.clip_ref(g, 1.0)[1])
    g = torch.tensor([1, -2, inf, 0, -0.0], dtype=F32)
    norm, coef, scaled = R.clip_ref(g, 1.0)
    assert float(norm) == inf and coef == 0 and R.bits(scaled).tolist()[:2] == [0, -2 ** 31] and math.isnan(float(scaled[2]))
    z = torch.tensor([0, -0.0, 0, -0.0], dtype=F32)
    assert R.clip_ref(z, 1.0)[1] == 1 and abs(float(R.clip_ref(z, 1e-7)[1]) - 0.1) < 1e-6
    assert torch.equal(R.bits(R.clip_ref(z, 1e-7)[2]), R.bits(z))


def test_clip_coef_ref_at_the_cap():
    n32 = np.float32(0.37)
    den = n32 + np.float32(1e-6)
    assert R.clip_coef_ref(n32, den) == 1 and R.clip_coef_ref(n32, np.nextafter(den, np.float32(np.inf))) == 1
    below = R.clip_coef_ref(n32, np.nextafter(den, np.float32(-np.inf)))
    assert below < 1 and below.dtype == np.float32


# ================================================================================================ Laplacian pyramid
SIZES = [(h, w) for h in (3, 4, 5, 6, 7) for w in (3, 4, 5, 6, 7)] + [(18, 33)]


def _lap_t_abs(pyr, e):
    return e + pyr.blur_t(pyr.stuff(pyr.blur_t(e)))


@pytest.mark.parametrize("aux_ratio", [0.005, 1.0])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matrix_pyramid_is_the_oracle_s_loss(hw, aux_ratio):
    """Value and autograd gradient of oracle.vmg_oracle.charbonnier_edge_loss in fp64 against the matrices.  The oracle convolves with the
    5 x 5 tensor fl32(k_i k_j), the matrices apply the fp32 taps per axis with exact products: every weight differs by at most U relative
    per blur.  So lap(d) differs by delta <= 2 U S_gz2 (both blurs), the value by aux_ratio * mean(delta), and the gradient by
    gs2 * ( |lap^T| (slope * delta) + 2 U S_t2 ), slope = eps / (ld^2 + eps)^1.5 at the |ld| nearest 0 within delta: derived, not fitted."""
    from oracle import vmg_oracle as O
    H, W = hw
    eps = 1e-12
    gen = torch.Generator().manual_seed(100 * H + W)
    x = (torch.rand(1, 2, 3, H, W, generator=gen, dtype=F64) * 0.6 + 0.2)
    y = (torch.rand(1, 2, 3, H, W, generator=gen, dtype=F64) * 0.6 + 0.2)
    xo = x.clone().requires_grad_(True)
    lo = O.charbonnier_edge_loss(xo, y, eps, aux_ratio)
    lo.backward()
    n = x.numel()
    xf, yf = x.reshape(-1, H, W), y.reshape(-1, H, W)
    r = R.lap_fwd_ref(xf, yf, eps)
    pyr = r["pyr"]
    delta = 2 * U * r["S_gz2"] * R.ORDER2
    got = (r["sum1"] + aux_ratio * r["sum2"]) / n
    assert abs(float(got) - float(R.loss_ref(x, y, eps, aux_ratio))) == 0.0
    assert abs(float(got) - float(lo.detach())) <= aux_ratio * float(delta.sum()) / n + 1e-15
    b = R.lap_bwd_ref(xf, yf, r["ld"], eps, 1.0 / n, aux_ratio / n, pyr)
    near = (r["ld"].abs() - delta).clamp_min(0)
    slope = eps / (near * near + eps) ** 1.5
    tol = (aux_ratio / n) * (_lap_t_abs(pyr, slope * delta) + 2 * U * (b["w"].abs() + b["S_t2"])) * R.ORDER2 + 1e-17
    err = (b["dx"].reshape(x.shape) - xo.grad).abs()
    assert bool((err <= tol.reshape(x.shape)).all()), float((err / tol.reshape(x.shape)).max())
    # the tolerance is far below the gradient itself: the comparison is not vacuous
    assert float(tol.median()) <= 1e-5 * float(xo.grad.abs().max())


@pytest.mark.parametrize("hw", [(3, 3), (3, 4), (4, 3), (4, 4), (5, 3), (6, 7), (18, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_adjoint_pieces_are_autograd_of_the_forward_matrices(hw):
    """u and G^T(z[u]) of lap_bwd_ref against autograd through the forward operators: for a -> G place(a) G^T (a quarter size, placed at the
    even positions) the gradient of <w, .> with respect to a is (G^T w G) at the even positions, a quarter of u; for
    d -> d - lap(d) = G z[4 (G d G^T) even] G^T the gradient with respect to d is G^T(z[u])."""
    H, W = hw
    gen = torch.Generator().manual_seed(7 * H + W)
    pyr = R.Pyramid(H, W)
    x = torch.rand(2, H, W, generator=gen, dtype=F64)
    y = torch.rand(2, H, W, generator=gen, dtype=F64)
    ld = torch.randn(2, H, W, generator=gen, dtype=F64) * 1e-3
    b = R.lap_bwd_ref(x, y, ld, 1e-6, 0.0, 1.0, pyr)
    w = b["w"]
    # (a) u: the gradient of <w, G z[a] G^T> with respect to the quarter-size a, where z places a at (even, even) -- a1 already holds the 4
    a = torch.zeros(2, (H + 1) // 2, (W + 1) // 2, dtype=F64, requires_grad=True)
    full = torch.zeros(2, H, W, dtype=F64)
    full = full.index_put((torch.arange(2)[:, None, None], torch.arange(0, H, 2)[None, :, None], torch.arange(0, W, 2)[None, None, :]), a)
    (pyr.blur(full) * w).sum().backward()
    assert float((4 * a.grad - b["u"]).abs().max()) <= 1e-14 * max(1.0, float(b["u"].abs().max()))
    # (b) G^T(z[u]): the gradient of <w, d - lap(d)> with respect to d
    d = (x - y).clone().requires_grad_(True)
    ((d - pyr.lap(d)) * w).sum().backward()
    assert float((d.grad - b["t"]).abs().max()) <= 1e-14 * max(1.0, float(b["t"].abs().max()))
    # (c) dx with gs = (0, 1) is lap^T w
    assert float((b["dx"] - pyr.lap_t(w)).abs().max()) <= 1e-15 * max(1.0, float(w.abs().max())) * 8


def test_blur_matrix_rows_and_the_small_sizes():
    """Rows of G sum to 1 (the fp32 taps sum to 1 within U); at n = 3 the middle column collects nothing from the padding and the edge
    columns collect the folded taps: written out by hand."""
    for n in (3, 4, 5, 9):
        G = R.blur_matrix(n)
        assert float((G.sum(1) - 1).abs().max()) <= 2 * U
    a, b, c = R.TAPS[0], R.TAPS[1], R.TAPS[2]
    want = torch.tensor([[a + b + c, b, a], [a + b, c, b + a], [a, b, c + b + a]], dtype=F64)
    assert float((R.blur_matrix(3) - want).abs().max()) <= 1e-16
    assert torch.equal(R.even_matrix(4), torch.diag(torch.tensor([2.0, 0, 2.0, 0], dtype=F64)))
