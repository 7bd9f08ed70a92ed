"""tests/wgrad_ref.py checked on the CPU: the fp64 weight-gradient reference against fp64 autograd of F.conv2d, the claim that the two
value families make fp32 accumulation exact in any order, and the NaN-guarded operand views.  (The kernels themselves:
tests/test_wgrad_kernels_gpu.py.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wgrad_ref as WR


@pytest.mark.parametrize("ks", [1, 3, 7])
@pytest.mark.parametrize("shape", [(2, 5, 6, 3, 4, 1), (1, 1, 9, 5, 2, 3), (3, 4, 1, 2, 3, 2), (1, 1, 1, 4, 4, 2)])
def test_wgrad_ref_equals_fp64_autograd_of_conv2d(ks, shape):
    N, H, W, Ci, Co, P = shape
    g = torch.Generator().manual_seed(7 * ks + H)
    xs = [torch.randn(N, H, W, Ci, generator=g, dtype=torch.float64) for _ in range(P)]
    dys = [torch.randn(N, H, W, Co, generator=g, dtype=torch.float64) for _ in range(P)]
    w = torch.zeros(Co, Ci, ks, ks, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    loss = sum((F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=ks // 2) * dy.permute(0, 3, 1, 2)).sum() for x, dy in zip(xs, dys))
    gw, gb = torch.autograd.grad(loss, [w, b])
    dW, db = WR.wgrad_ref(xs, dys, ks)
    assert dW.dtype == torch.float64 and tuple(dW.shape) == (Co, Ci, ks, ks)
    assert float((dW - gw).abs().max()) <= 1e-12 * max(1.0, float(gw.abs().max()))
    assert float((db - gb).abs().max()) <= 1e-12 * max(1.0, float(gb.abs().max()))


def _largest_terms(family):
    lo, hi = 1, 2 ** 24
    while lo < hi:  # largest count assert_exact accepts without an initial value
        mid = (lo + hi + 1) // 2
        try:
            WR.assert_exact(family, mid, 0)
            lo = mid
        except AssertionError:
            hi = mid - 1
    return lo


def test_assert_exact_accepts_what_the_families_promise_and_no_more():
    assert _largest_terms("full") >= 256 and 255 * 255 * (_largest_terms("full") + 1) >= 2 ** 24
    assert _largest_terms("small") == 2 ** 18 - 1
    WR.assert_exact("full", 256)       # with the family's own initial values
    WR.assert_exact("small", 2 ** 17)
    with pytest.raises(AssertionError):
        WR.assert_exact("full", 300)
    with pytest.raises(AssertionError):
        WR.assert_exact("small", 2 ** 18)
    with pytest.raises(AssertionError):
        WR.assert_exact("full", 16, 2)  # an initial value the family does not account for


@pytest.mark.parametrize("family", ["full", "small"])
def test_fp32_accumulation_is_exact_in_any_order(family):
    """At the largest term count of each family: the products, added one by one in fp32 -- forward, reversed, in a seeded permutation -- give
    the bits of the fp64 sum at EVERY prefix, for dense seeded values (16 columns) and for the worst case (every product kmax^2, one
    sign).  And init + scale * sum is exact for each scale at the largest count the family's initial values allow."""
    kmax, s = WR.FAMILIES[family]
    T = _largest_terms(family)
    x = WR.exact_values((T, 16), 11, family)
    dy = WR.exact_values((T, 16), 12, family)
    assert float(x.abs().max()) == kmax / 2 ** s and torch.equal(x, x.bfloat16().float())  # the whole range, and bf16 numbers
    assert torch.equal(x * 2 ** s, (x * 2 ** s).round())
    x[:, 0] = kmax / 2 ** s
    dy[:, 0] = -kmax / 2 ** s
    prod32 = (x * dy).numpy()
    prod64 = x.double().numpy() * dy.double().numpy()
    assert np.array_equal(prod32.astype(np.float64), prod64)  # every product is an fp32 number
    perm = np.random.default_rng(5).permutation(T)
    for order in (np.arange(T), np.arange(T)[::-1], perm):
        run32 = np.cumsum(prod32[order], axis=0, dtype=np.float32)  # sequential fp32 additions
        run64 = np.cumsum(prod64[order], axis=0, dtype=np.float64)
        assert run32.dtype == np.float32 and np.array_equal(run32.astype(np.float64), run64)
    # the initial value and the scale, at the count that leaves room for them
    Ti = T - WR.INIT_MAX[family] * 2 ** (2 * s + 2) // (kmax * kmax) - 1
    WR.assert_exact(family, Ti)
    with pytest.raises(AssertionError):
        WR.assert_exact(family, T)
    init = float(WR.INIT_MAX[family])
    for scale in (1.0, 0.5, -0.25):
        for sign in (1.0, -1.0):
            run32 = np.cumsum(prod32[:Ti, 0], dtype=np.float32)
            got = (np.float32(sign * init) + np.float32(scale) * run32).astype(np.float32)
            want = sign * init + scale * np.cumsum(prod64[:Ti, 0])
            assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("geom", [((2, 3, 5, 3), 8, 4, 0), ((1, 2, 7, 40), 43, 9, 0), ((7, 24), 24, 3, 1), ((1, 1, 4, 17), 32, 20, 0),
                                  ((2, 2, 2, 3), 3, 5, 0), ((3, 5, 16), 16, 0, 3)])
def test_embed_views_are_aligned_strided_and_surrounded_by_nan(dtype, geom):
    shape, ps, guard, offset = geom
    C = shape[-1]
    M = int(np.prod(shape[:-1]))
    t = WR.exact_values(shape, 3, "full").to(dtype)
    v = WR.embed(t, ps, guard, offset=offset)
    es = t.element_size()
    assert tuple(v.shape) == tuple(shape) and v.dtype == dtype and torch.equal(v, t)
    assert v.stride(-1) == 1 and v.stride(-2) == ps
    assert torch.equal(v.reshape(M, C), t.reshape(M, C))  # dense over the pixels: one stride serves every leading dimension
    assert v.data_ptr() % 16 == (offset * es) % 16
    flat = v._base.reshape(-1)
    first, last = v.storage_offset(), v.storage_offset() + (M - 1) * ps + C
    assert first >= guard * ps and flat.numel() - (first + M * ps) >= guard * ps
    assert torch.isnan(flat[:first]).all() and torch.isnan(flat[first + M * ps:]).all()
    body = flat[first:first + M * ps].view(M, ps)
    c8 = min((C + 7) // 8 * 8, ps)
    assert torch.isfinite(body[:, :c8]).all()         # the "computed and dropped" channels hold finite junk
    if c8 > C:
        assert float(body[:, C:c8].abs().min()) > 0   # ... that is not zero: a kernel that keeps them shows
    assert torch.isnan(body[:, c8:]).all()
    out = WR.embed_outside(v)
    assert out.numel() == flat.numel() - M * C and int(torch.isfinite(out).sum()) == M * (c8 - C)
    assert last <= flat.numel()


def test_first_mismatch_reports_nan_and_the_first_index():
    a = torch.zeros(2, 3)
    b = a.clone()
    assert WR.first_mismatch(a, b)[0] == 0
    a[1, 1] = float("nan")
    a[1, 2] = 2.0
    n, idx, g, w = WR.first_mismatch(a, b)
    assert n == 2 and idx == (1, 1) and g != g and w == 0.0
