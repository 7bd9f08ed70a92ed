"""tests/conv_ref.py checked on the CPU: the fp64 convolution and data-gradient references against F.conv2d and its autograd, the order of
the epilogue on hand-computed one-pixel examples, the claim that the exact cases of tests/test_conv_chain_kernels_gpu.py have no
rounding in fp32 in any order, the shift probes and the real-valued bound.  (The kernels themselves: tests/test_conv_chain_kernels_gpu.py.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as CR
from tests import test_conv_chain_kernels_gpu as G
from tests import wgrad_ref as WR


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _close(a, b):
    assert a.dtype == torch.float64 and tuple(a.shape) == tuple(b.shape)
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def _conv2d(x, w, groups=1):
    return F.conv2d(x.permute(0, 3, 1, 2), w, padding=1, groups=groups).permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", [(2, 5, 6, 3, 4), (1, 1, 1, 5, 2), (3, 4, 1, 2, 3), (1, 1, 9, 4, 4)])
def test_conv_ref_equals_fp64_conv2d(shape):
    N, H, W, Ci, Co = shape
    x, w = _rand((N, H, W, Ci), 1), _rand((Co, Ci, 3, 3), 2)
    _close(CR.conv_ref([x], w), _conv2d(x, w))


def test_conv_ref_concat_slices_and_groups_equal_fp64_conv2d():
    N, H, W = 2, 4, 5
    a, b, w = _rand((N, H, W, 3), 3), _rand((N, H, W, 5), 4), _rand((6, 8, 3, 3), 5)
    full = _conv2d(torch.cat([a, b], -1), w)
    _close(CR.conv_ref([a, b], w), full)                                       # virtual concat
    _close(CR.conv_ref([a, b], w, o0=1, on=4), full[..., 1:5])                 # output slice
    _close(CR.conv_ref([b], w, src_off=[3]), _conv2d(b, w[:, 3:8].contiguous()))  # a K slice of a wider weight
    _close(CR.conv_ref([b, a], w, src_off=[3, 0]), full)                       # the sources in another order than the weight's channels
    wg = _rand((6, 4, 3, 3), 6)                                                # groups = 2: 8 dense inputs, 4 per group
    _close(CR.conv_ref([a, b], wg, groups=2), _conv2d(torch.cat([a, b], -1), wg, groups=2))


@pytest.mark.parametrize("shape", [(2, 5, 6, 3, 4), (1, 1, 1, 5, 2), (3, 4, 1, 2, 3), (1, 1, 9, 4, 4)])
def test_dgrad_ref_equals_fp64_autograd(shape):
    N, H, W, Ci, Co = shape
    x = _rand((N, H, W, Ci), 7).requires_grad_(True)
    w, dy = _rand((Co, Ci, 3, 3), 8), _rand((N, H, W, Co), 9)
    gx, = torch.autograd.grad((_conv2d(x, w) * dy).sum(), [x])
    _close(CR.dgrad_ref(dy, w), gx)
    if Ci > 2:
        _close(CR.dgrad_ref(dy, w, i0=1, inn=2), gx[..., 1:3])


def _one_pixel(acc, **kw):
    t = lambda v: None if v is None else torch.tensor(v, dtype=torch.float32).reshape(1, 1, 1, 1)  # noqa: E731
    for k in ("res", "aux"):
        kw[k] = t(kw.get(k))
    kw["bias"] = None if kw.get("bias") is None else torch.tensor([kw["bias"]], dtype=torch.float32)
    out, pre = CR.epilogue_ref(torch.tensor(acc, dtype=torch.float64).reshape(1, 1, 1, 1), **kw)
    return float(out), float(pre)


def test_epilogue_order_on_hand_computed_pixels():
    """v = acc + bias; out_pre = bf16(v); act; * alpha; * mask; + res; bf16 -- each wrong order gives another number."""
    # the sum itself, from a one-pixel image: only the centre tap sees it
    w = torch.zeros(1, 1, 3, 3)
    w[0, 0] = torch.arange(1.0, 10.0).reshape(3, 3)
    w[0, 0, 1, 1] = -1.5
    assert float(CR.conv_ref([torch.full((1, 1, 1, 1), 2.0)], w)) == -3.0
    kw = dict(bias=1.0, act=CR.ACT_LRELU, slope=0.5, alpha=0.25, aux=-1.0, actgrad=2, res=4.0)
    # -3 + 1 = -2 -> out_pre;  lrelu: -1;  * 0.25: -0.25;  mask (aux < 0, mode 2): * 0.5 = -0.125;  + 4 = 3.875
    assert _one_pixel(-3.0, **kw) == (3.875, -2.0)
    assert 3.875 != (-1.0 * 0.5 + 4.0) * 0.25                      # alpha behind the residual
    assert 3.875 != (-1.5 + 1.0) * 0.25 * 0.5 + 4.0                # the activation in front of the bias
    assert 3.875 != (-1.0 + 4.0) * 0.25 * 0.5                      # the residual in front of the scalings
    # acc < 0 < acc + bias: the activation sees v, and +0.0 / -0.0 in aux are not positive
    for zero in (0.0, -0.0):
        assert _one_pixel(-0.5, **dict(kw, aux=zero)) == (0.5 * 0.25 * 0.5 + 4.0, 0.5)
        assert _one_pixel(-0.5, **dict(kw, aux=zero, actgrad=1)) == (4.0, 0.5)
    assert _one_pixel(-0.5, **dict(kw, aux=0.25, actgrad=1)) == (0.5 * 0.25 + 4.0, 0.5)
    assert _one_pixel(-3.0, **dict(kw, act=CR.ACT_RELU)) == (4.0, -2.0)
    # out is computed from v, not from the rounded out_pre: v = 1 + 3 * 2^-9 rounds to 1 + 2^-7, v - 1 is a bf16 number
    v = 1.0 + 3 * 2.0 ** -9
    assert _one_pixel(v, res=-1.0) == (3 * 2.0 ** -9, 1.0 + 2.0 ** -7)
    # slope 0.1: ONE rounding of v * float32(0.1) to fp32, then bf16
    want = float(torch.tensor(float(np.float32(-3.0) * np.float32(0.1))).bfloat16())
    assert _one_pixel(-3.0, act=CR.ACT_LRELU, slope=0.1) == (want, -3.0)
    out, pre = CR.epilogue_ref(torch.tensor([[[[-3.0]]]], dtype=torch.float64), act=CR.ACT_GELU)
    assert out is None and float(pre) == -3.0


def test_round_bf16_rounds_to_nearest_even_and_refuses_what_is_no_fp32_number():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    got = CR.round_bf16(t(1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -(1 + 2.0 ** -8)))
    assert got.dtype == torch.bfloat16 and got.tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -1.0]
    with pytest.raises(AssertionError):
        CR.round_bf16(t(1 + 2.0 ** -30))
    assert float(CR.round_bf16(t(1 + 2.0 ** -30), exact=False)) == 1.0


def test_assert_exact_accepts_every_gpu_case_and_no_more():
    cases = G.exact_cases()
    assert len(cases) > 100
    for _, _, spec in cases:
        CR.assert_exact(*G.exact_args(spec))
    CR.assert_exact("small", 448, bias=True, res=True, scales=(0.25, 0.125, 0.25))  # 64 * 4032 is far below 2^24
    CR.assert_exact("full", 16, bias=True, res=True, scales=(0.125,))                # 144 terms
    with pytest.raises(AssertionError):
        CR.assert_exact("full", 32)                                                  # 288 terms of 255^2
    with pytest.raises(AssertionError):
        CR.assert_exact("full", 16, res=True, scales=(2.0 ** -10,))                  # the residual on too fine a grid
    with pytest.raises(AssertionError):
        CR.assert_exact("small", 2 ** 15)
    CR.assert_exact("small", 144, scales=(0.1,))                                     # one odd scale, nothing behind it
    with pytest.raises(AssertionError):
        CR.assert_exact("small", 144, res=True, scales=(0.1,))
    with pytest.raises(AssertionError):
        CR.assert_exact("small", 144, scales=(0.1, 0.125))
    with pytest.raises(AssertionError):
        CR.assert_exact("small", 144, scales=(2.0,))


def test_gpu_case_table_covers_what_it_says():
    G.test_ws_case_table_reaches_both_ring_sizes()
    for route in (G.WS, G.KSPLIT):
        cases = G._channel_cases(route)
        assert {g for g, s in cases if s.src_ch == (144,) and s.co == 144 and s.epi == "bias" and not (s.o_total or s.i_total or s.groups > 1)} == set(G.GEOMS)
        assert all(N * H * W <= 2000 for (N, H, W), _ in cases)
    assert sorted({s.tiles for s in G.KS_SPECS}) == [1, 3, 4, 5]
    # (1, 24, 81): 18 weight-streaming tiles, at least the largest stage count of a source block (160 channels: 45 k-steps = 15 stages)
    assert 3 * 6 == 18 and max(9 * (b // 32) + (6 if b % 32 else 0) for s in G.WS_SPECS for c in s.src_ch for b in G._blocks(c)) // 3 == 15


def _terms(x, w):
    """Every product of the convolution, in fp32: (N, H, W, Co, 9 * Ci)."""
    N, H, W, Ci = x.shape
    xpad = F.pad(x, (0, 0, 1, 1, 1, 1))
    cols = torch.stack([xpad[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], -2)  # N, H, W, 9, Ci
    wt = w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, Ci)
    p32 = (cols[:, :, :, None] * wt[None, None, None]).reshape(N, H, W, w.shape[0], 9 * Ci)
    p64 = (cols.double()[:, :, :, None] * wt.double()[None, None, None]).reshape(p32.shape)
    assert p32.dtype == torch.float32 and torch.equal(p32.double(), p64)  # every product is an fp32 number
    return p32.numpy()


@pytest.mark.parametrize("case", [("full", 16, 8, (1, 3, 4), dict(alpha=0.125, res=True)),
                                  ("small", 448, 4, (1, 2, 3), dict(act=CR.ACT_LRELU, slope=0.25, alpha=0.125, actgrad=2, res=True)),
                                  ("small", 288, 4, (2, 2, 2), dict(act=CR.ACT_LRELU, slope=0.1))], ids=lambda c: f"{c[0]}-{c[1]}")
def test_fp32_partial_sums_in_any_order_reproduce_the_fp64_value(case):
    """An exact case, every partial sum reordered randomly and added one by one in fp32 (numpy), then the epilogue step by step in fp32:
    every prefix has the bits of the fp64 sum and the bf16 result those of the reference."""
    family, Ci, Co, (N, H, W), e = case
    scales = [e["slope"]] if e.get("act") == CR.ACT_LRELU else []
    scales += [e.get("alpha", 1.0)] + ([e["slope"]] if e.get("actgrad") == 2 else [])
    CR.assert_exact(family, Ci, True, e.get("res", False), tuple(scales))
    x, w = WR.exact_values((N, H, W, Ci), 21, family), WR.exact_values((Co, Ci, 3, 3), 22, family)
    kmax, s = WR.FAMILIES[family]
    x[0, 0, 0, :], w[0] = kmax / 2 ** s, -kmax / 2 ** s  # the worst case in one element: every product -kmax^2, one sign
    bias = WR.exact_values((Co,), 23, family)
    bias[0] = -kmax / 2 ** s
    res = WR.exact_values((N, H, W, Co), 24, family) if e.get("res") else None
    aux = WR.exact_values((N, H, W, Co), 25, family) if e.get("actgrad") else None
    acc = CR.conv_ref([x], w)
    want, _ = CR.epilogue_ref(acc, bias, act=e.get("act", 0), slope=e.get("slope", 0.0), alpha=e.get("alpha", 1.0), aux=aux, actgrad=e.get("actgrad", 0), res=res)
    p32 = _terms(x, w)
    rng = np.random.default_rng(3)
    for _ in range(3):
        order = rng.permutation(p32.shape[-1])
        run32 = np.cumsum(p32[..., order], axis=-1, dtype=np.float32)
        run64 = np.cumsum(p32[..., order].astype(np.float64), axis=-1)
        assert run32.dtype == np.float32 and np.array_equal(run32.astype(np.float64), run64)
        # the weight-streaming kernel starts its accumulators from the bias, the K-split kernel adds it last: both orders
        first = np.cumsum(np.concatenate([np.broadcast_to(bias.numpy(), p32.shape[:-1])[..., None], p32[..., order]], -1), axis=-1, dtype=np.float32)[..., -1]
        v = (run32[..., -1] + bias.numpy()).astype(np.float32)
        assert np.array_equal(first, v) and np.array_equal(v.astype(np.float64), acc.numpy() + bias.double().numpy())
        slope, alpha = np.float32(e.get("slope", 0.0)), np.float32(e.get("alpha", 1.0))
        if e.get("act") == CR.ACT_LRELU:
            v = np.where(v > 0, v, (v * slope).astype(np.float32))
        v = (v * alpha).astype(np.float32)
        if aux is not None:
            v = (v * np.where(aux.numpy() > 0, np.float32(1), slope)).astype(np.float32)
        if res is not None:
            v = (v + res.numpy()).astype(np.float32)
        got = torch.from_numpy(v).bfloat16()
        assert torch.equal(got, want)


@pytest.mark.parametrize("t", range(9))
def test_shift_probes_are_exact_for_full_mantissa_inputs(t):
    N, H, W, Ci, Co = 2, 3, 5, 16, 24
    x = torch.randn(N, H, W, Ci, generator=torch.Generator().manual_seed(t)).bfloat16().float()
    assert int((x.view(torch.int32) >> 16 & 0x7F).unique().numel()) > 64  # the mantissas are not special
    w, pi, ptap = CR.one_hot_weight(Co, Ci, t)
    assert float(w.sum()) == Co and bool((w.reshape(Co, -1).sum(1) == 1).all())
    assert sorted(set(ptap.tolist())) == list(range(9))  # every tap occurs in every probe
    acc = CR.conv_ref([x], w)
    assert torch.equal(acc, CR.shifted_copy(x, pi, ptap).double())
    out, _ = CR.epilogue_ref(acc)  # asserts that nothing is rounded
    assert torch.equal(out.float(), acc.float())
    # a probe moved by one tap is another tensor: the comparison can name the tap
    assert not torch.equal(CR.shifted_copy(x, pi, (ptap + 1) % 9).double(), acc)


def test_fp32_evaluation_of_real_values_stays_within_the_bound():
    """Seeded normal operands, the products added in fp32 in a random order, the chain's epilogue (alpha 0.1, residual) in fp32 steps: inside
    conv_ref.real_bound, which itself is below two bf16 ulps of the largest value."""
    N, H, W, Ci, Co = 1, 3, 4, 144, 8
    g = torch.Generator().manual_seed(31)
    x = torch.randn(N, H, W, Ci, generator=g).bfloat16().float()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5).bfloat16().float()
    bias, res = torch.randn(Co, generator=g) * 0.1, torch.randn(N, H, W, Co, generator=g).bfloat16().float()
    v, _ = CR.epilogue_ref(CR.conv_ref([x], w), bias, alpha=0.1, res=res, exact=False)
    S = CR.conv_ref([x.abs()], w.abs()) + bias.abs().double() + res.abs().double()
    bound = CR.real_bound(v, S, Ci)
    p32 = _terms_real(x, w)
    order = np.random.default_rng(4).permutation(p32.shape[-1])
    acc32 = np.cumsum(p32[..., order], axis=-1, dtype=np.float32)[..., -1]
    got = ((acc32 + bias.numpy()).astype(np.float32) * np.float32(0.1)).astype(np.float32) + res.numpy()
    got = torch.from_numpy(got.astype(np.float32)).bfloat16().double()
    assert float(((got - v).abs() / bound).max()) <= 1.0
    assert float(bound.max()) < 2.0 ** -7 * float(v.abs().max())  # and it is a tight bound: about one bf16 ulp


def _terms_real(x, w):
    N, H, W, Ci = x.shape
    xpad = F.pad(x, (0, 0, 1, 1, 1, 1))
    cols = torch.stack([xpad[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], -2)
    wt = w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, Ci)
    return (cols[:, :, :, None] * wt[None, None, None]).reshape(N, H, W, w.shape[0], 9 * Ci).numpy()


# ------------------------------------------------------------------------------------------------------------------------------------
# ks = 1: the references of tests/test_linear_kernels_gpu.py
# ------------------------------------------------------------------------------------------------------------------------------------
from tests import test_linear_kernels_gpu as GL  # noqa: E402


def _r64(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_linear_ref_equals_fp64_linear():
    x, w = _r64(2, 3, 5, 24, seed=1), _r64(20, 24, seed=2)
    assert float((CR.linear_ref([x], w) - F.linear(x, w)).abs().max()) <= 1e-12
    # sources as channel slices, in another order than the weight's; an output slice
    a, b, c = x[..., :8], x[..., 8:16], x[..., 16:]
    got = CR.linear_ref([c, a, b], w, src_off=[16, 0, 8], o0=3, on=11)
    assert tuple(got.shape) == (2, 3, 5, 11) and float((got - F.linear(x, w)[..., 3:14]).abs().max()) <= 1e-12
    assert float((CR.linear_ref([a, b, c], w) - F.linear(x, w)).abs().max()) <= 1e-12
    # a K slice of a wider weight
    assert float((CR.linear_ref([b], w, src_off=[8]) - F.linear(b, w[:, 8:16])).abs().max()) <= 1e-12
    assert CR.linear_ref([x.float()], w.float()).dtype == torch.float64


def test_dlinear_ref_equals_fp64_autograd():
    x, w, dy = _r64(7, 24, seed=3).requires_grad_(True), _r64(20, 24, seed=4), _r64(7, 20, seed=5)
    F.linear(x, w).backward(dy)
    assert float((CR.dlinear_ref(dy, w) - x.grad).abs().max()) <= 1e-12
    assert float((CR.dlinear_ref(dy, w, i0=8, inn=8) - x.grad[:, 8:16]).abs().max()) <= 1e-12
    assert tuple(CR.dlinear_ref(dy, w).shape) == (7, 24)  # not the weight's other side


def test_pixel_shuffle_ref_equals_torch():
    x = torch.arange(2 * 3 * 5 * 12, dtype=torch.float32).reshape(2, 3, 5, 12)
    want = F.pixel_shuffle(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    got = CR.pixel_shuffle_ref(x)
    assert tuple(got.shape) == (2, 6, 10, 3) and torch.equal(got, want)


def test_gelu_refs_equal_torch_in_fp64():
    x = torch.cat([torch.linspace(-12, 12, 4001, dtype=torch.float64), torch.tensor([0.0, -0.0, 2.0 ** -126, 30.0, -30.0], dtype=torch.float64)])
    xg = x.clone().requires_grad_(True)
    y = F.gelu(xg)
    y.sum().backward()
    # (another spelling of the same fp64 formula: a few ulps of the largest value, ulp(30) = 3.6e-15)
    assert float((CR.gelu_ref(x) - y.detach()).abs().max()) <= 1e-14
    assert float((CR.gelu_grad_ref(x) - xg.grad).abs().max()) <= 1e-14
    assert float(CR.gelu_grad_ref(x).abs().max()) < 1.13 and float(CR.gelu_grad_ref(torch.tensor([2.0 ** 0.5])).item()) > 1.128  # sup |gelu'| = 1.129
    assert CR.gelu_ref(x.float()).dtype == torch.float64
    assert GL.gelu_sweep().numel() >= 65536 + 6 + 4096 and not bool(torch.isnan(GL.gelu_sweep()).any())


def test_assert_exact_with_one_tap_accepts_every_linear_gpu_case_and_no_more():
    cases = GL.exact_cases()
    assert len(cases) > 500
    for c in cases:
        CR.assert_exact(*GL.exact_args(c), taps=1)
        assert c.fam == ("full" if sum(c.src_ch) <= 256 else "small")  # "full" wherever one tap admits it
    CR.assert_exact("full", 256, bias=True, res=True, taps=1)  # 255^2 * 256 + 255 * 2^7 * 2 = 16 711 680 < 2^24
    assert 255 ** 2 * 256 + 255 * 2 ** 7 * 2 == 16711680 < 2 ** 24
    with pytest.raises(AssertionError):
        CR.assert_exact("full", 264, bias=False, taps=1)
    with pytest.raises(AssertionError):
        CR.assert_exact("full", 288, taps=1)
    with pytest.raises(AssertionError):
        CR.assert_exact("full", 32)  # (the default is still nine taps)
    CR.assert_exact("full", 32, taps=1)


def test_epilogue_ref_for_fp32_outputs_is_the_fp64_value():
    acc = torch.tensor([[-1.5, 0.75 + 2.0 ** -20, 3.0]], dtype=torch.float64)
    out, pre = CR.epilogue_ref(acc, torch.tensor([0.5, 0.0, -1.0]), act=CR.ACT_LRELU, slope=0.25, alpha=0.5, out_dtype=torch.float32)
    assert out.dtype == torch.float32 and pre.dtype == torch.float32
    assert torch.equal(pre.double(), torch.tensor([[-1.0, 0.75 + 2.0 ** -20, 2.0]], dtype=torch.float64))
    assert torch.equal(out.double(), torch.tensor([[-0.125, 0.375 + 2.0 ** -21, 1.0]], dtype=torch.float64))
    out16, _ = CR.epilogue_ref(acc, torch.tensor([0.5, 0.0, -1.0]), act=CR.ACT_LRELU, slope=0.25, alpha=0.5)
    assert out16.dtype == torch.bfloat16 and float(out16[0, 1]) == 0.375  # (the bf16 default rounds what fp32 keeps)
    with pytest.raises(AssertionError):
        CR.epilogue_ref(torch.tensor([1 + 2.0 ** -30], dtype=torch.float64), out_dtype=torch.float32)  # no fp32 number
    # a slope that is no power of two rounds once, to fp32
    out, _ = CR.epilogue_ref(torch.tensor([-3.0], dtype=torch.float64), act=CR.ACT_LRELU, slope=0.1, out_dtype=torch.float32)
    assert float(out) == float(np.float32(-3.0) * np.float32(0.1))


def test_permutation_probes_and_the_one_tap_bound():
    for t in range(3):
        w, i = CR.one_hot_linear(144, 288, t)
        assert torch.equal(w.sum(1), torch.ones(144)) and torch.equal(w.argmax(1), i) and len(set(i.tolist())) == 144  # distinct input channels
        x = torch.randn(5, 288, generator=torch.Generator().manual_seed(t))
        assert torch.equal(CR.linear_ref([x], w), x[:, i].double())
    assert not torch.equal(CR.one_hot_linear(16, 8, 0)[1], CR.one_hot_linear(16, 8, 1)[1])
    v, S = torch.tensor([2.0], dtype=torch.float64), torch.tensor([3.0], dtype=torch.float64)
    assert float(CR.sum_bound(S, 144, taps=1)) == 2 * 148 * 2.0 ** -24 * 3 and float(CR.sum_bound(S, 144)) == 2 * (9 * 144 + 4) * 2.0 ** -24 * 3
    e = float(CR.sum_bound(S, 144, taps=1))
    assert float(CR.real_bound(v, S, 144, taps=1)) == 2.0 ** -8 * (2 + e) + e
    assert float(CR.real_bound(v, S, 144, taps=1, out_dtype=torch.float32)) == 2.0 ** -23 * (2 + e) + e
    assert float(CR.real_bound(v, S, 144)) == 2.0 ** -8 * (2 + float(CR.sum_bound(S, 144))) + float(CR.sum_bound(S, 144))


# ------------------------------------------------------------------------------------------------------------------------------------
# ks = 7, and the table of tests/test_conv_general_kernels_gpu.py
# ------------------------------------------------------------------------------------------------------------------------------------
from tests import test_conv_general_kernels_gpu as GG  # noqa: E402


def _conv2d7(x, w):
    return F.conv2d(x.permute(0, 3, 1, 2), w, padding=3).permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", [(2, 5, 6, 3, 4), (1, 1, 1, 5, 2), (3, 4, 1, 2, 3), (1, 3, 3, 4, 4), (2, 6, 21, 2, 3), (1, 9, 8, 3, 2)])
def test_conv_ref_7x7_equals_fp64_conv2d(shape):
    N, H, W, Ci, Co = shape
    x, w = _rand((N, H, W, Ci), 41), _rand((Co, Ci, 7, 7), 42)
    _close(CR.conv_ref([x], w), _conv2d7(x, w))
    with pytest.raises(AssertionError):
        CR.conv_ref([x], _rand((Co, Ci, 5, 5), 43))  # 3 or 7, nothing else
    with pytest.raises(AssertionError):
        CR.conv_ref([x], _rand((Co, Ci, 3, 7), 43))


def test_conv_ref_7x7_concat_and_slices_equal_fp64_conv2d():
    N, H, W = 2, 4, 9
    a, b, w = _rand((N, H, W, 3), 44), _rand((N, H, W, 5), 45), _rand((6, 8, 7, 7), 46)
    full = _conv2d7(torch.cat([a, b], -1), w)
    _close(CR.conv_ref([a, b], w), full)
    _close(CR.conv_ref([a, b], w, o0=1, on=4), full[..., 1:5])
    _close(CR.conv_ref([b], w, src_off=[3]), _conv2d7(b, w[:, 3:8].contiguous()))
    _close(CR.conv_ref([b, a], w, src_off=[3, 0]), full)
    # a weight that is not symmetric under a flip: the tap order (ky, kx) = (row, column) is torch's
    w1 = torch.zeros(1, 1, 7, 7, dtype=torch.float64)
    w1[0, 0, 0, 6] = 1.0  # out[y, x] = in[y - 3, x + 3]
    x = torch.arange(35, dtype=torch.float64).reshape(1, 5, 7, 1)
    got = CR.conv_ref([x], w1)
    assert float(got[0, 3, 2, 0]) == float(x[0, 0, 5, 0]) and float(got[0, 2, 2, 0]) == 0.0 and float(got[0, 4, 4, 0]) == 0.0


@pytest.mark.parametrize("shape", [(2, 5, 6, 3, 4), (1, 1, 1, 5, 2), (3, 4, 1, 2, 3), (1, 3, 3, 4, 4), (2, 6, 21, 2, 3)])
def test_dgrad_ref_7x7_equals_fp64_autograd(shape):
    N, H, W, Ci, Co = shape
    x = _rand((N, H, W, Ci), 47).requires_grad_(True)
    w, dy = _rand((Co, Ci, 7, 7), 48), _rand((N, H, W, Co), 49)
    gx, = torch.autograd.grad((_conv2d7(x, w) * dy).sum(), [x])
    got = CR.dgrad_ref(dy, w)
    assert tuple(got.shape) == (N, H, W, Ci)  # not the weight's other side
    _close(got, gx)
    if Ci > 2:
        _close(CR.dgrad_ref(dy, w, i0=1, inn=2), gx[..., 1:3])
    # the two spellings are independent: the scatter equals the gather with the transposed, mirrored weight
    _close(got, CR.conv_ref([dy], w.flip(2, 3).transpose(0, 1).contiguous()))


@pytest.mark.parametrize("t", [0, 16, 32, 48, 7])
def test_shift_probes_7x7_reproduce_shifted_copy_through_conv_ref(t):
    N, H, W, Ci, Co = 2, 3, 9, 16, 32
    x = torch.randn(N, H, W, Ci, generator=torch.Generator().manual_seed(t)).bfloat16().float()
    w, pi, ptap = CR.one_hot_weight(Co, Ci, t, 7)
    assert tuple(w.shape) == (Co, Ci, 7, 7) and float(w.sum()) == Co and bool((w.reshape(Co, -1).sum(1) == 1).all())
    assert ptap.tolist() == [(o + t) % 49 for o in range(Co)] and pi.tolist() == [(7 * o + 31 * t) % Ci for o in range(Co)]
    acc = CR.conv_ref([x], w)
    want = CR.shifted_copy(x, pi, ptap, 7)
    assert torch.equal(acc, want.double())
    # by hand for one element: tap (ky, kx) reads pixel (y + ky - 3, x + kx - 3)
    o = 5
    ky, kx = int(ptap[o]) // 7, int(ptap[o]) % 7
    y, xx = 1, 4
    yy, xc = y + ky - 3, xx + kx - 3
    assert float(want[1, y, xx, o]) == (float(x[1, yy, xc, int(pi[o])]) if 0 <= yy < H and 0 <= xc < W else 0.0)
    out, _ = CR.epilogue_ref(acc)  # asserts that nothing is rounded
    assert torch.equal(out.float(), acc.float())
    assert not torch.equal(CR.shifted_copy(x, pi, (ptap + 1) % 49, 7).double(), acc)  # a probe moved by one tap is another tensor
    # four probes meet every tap in every 16-channel tile; the 3x3 form is unchanged by the new argument
    taps = [set() for _ in range(Co // 16)]
    for p in GG.PROBES7:
        tp = CR.one_hot_weight(Co, Ci, p, 7)[2]
        for tile in range(Co // 16):
            taps[tile] |= set(tp[16 * tile:16 * tile + 16].tolist())
    assert all(s == set(range(49)) for s in taps)
    w3, i3, t3 = CR.one_hot_weight(Co, Ci, 4)
    assert tuple(w3.shape) == (Co, Ci, 3, 3) and t3.tolist() == [(o + 4) % 9 for o in range(Co)] and torch.equal(i3, CR.one_hot_weight(Co, Ci, 4, 3)[1])


def test_assert_exact_with_49_taps_accepts_every_general_gpu_case_and_no_more():
    cases = GG.exact_cases()
    assert len(cases) > 700
    for c in cases:
        args = GG.exact_args(c)
        assert args[5] == (49 if c.ks == 7 else 9)
        CR.assert_exact(*args[:5], taps=args[5])
        assert c.fam == ("full" if c.ks == 3 and sum(c.src_ch) <= 28 else "small")  # "full" wherever the taps admit it
    assert {sum(c.src_ch) for c in cases if c.fam == "full"} == {8, 16, 24}
    CR.assert_exact("full", 5, bias=True, taps=49)  # 255^2 * 245 + 255 * 2^7 = 15 963 765 < 2^24
    assert 255 ** 2 * 49 * 5 + 255 * 2 ** 7 == 15963765 < 2 ** 24 < 255 ** 2 * 49 * 6
    with pytest.raises(AssertionError):
        CR.assert_exact("full", 6, bias=False, taps=49)
    with pytest.raises(AssertionError):
        CR.assert_exact("full", 8, taps=49)  # the narrowest source a kernel takes
    CR.assert_exact("full", 28, bias=True, res=True, scales=(0.5, 0.25))  # 3x3: 255^2 * 252 + 255 * 2^7 * (1 + 8) < 2^24
    with pytest.raises(AssertionError):
        CR.assert_exact("full", 29)
    CR.assert_exact("small", 64, bias=True, res=True, scales=(0.5, 0.25), taps=49)
    with pytest.raises(AssertionError):
        CR.assert_exact("small", 2 ** 13, taps=49)  # 64 * 49 * 8192 > 2^24
    CR.assert_exact("small", 64, scales=(0.1,), taps=49)
    with pytest.raises(AssertionError):
        CR.assert_exact("small", 64, res=True, scales=(0.1,), taps=49)


def test_fp32_partial_sums_of_a_7x7_case_in_any_order_reproduce_the_fp64_value():
    """As for 3x3 above: 49 * 64 products of the "small" family added one by one in fp32 in random orders."""
    N, H, W, Ci, Co = 1, 3, 8, 64, 3
    CR.assert_exact("small", Ci, True, True, (0.125,), taps=49)
    x, w = WR.exact_values((N, H, W, Ci), 51, "small"), WR.exact_values((Co, Ci, 7, 7), 52, "small")
    x[:], w[0] = 2.0, -2.0  # the worst case in output channel 0: every product -kmax^2 / 16 (the other channels keep their seeded weights)
    bias, res = WR.exact_values((Co,), 53, "small"), WR.exact_values((N, H, W, Co), 54, "small")
    acc = CR.conv_ref([x], w)
    assert float(acc[0, 1, 3, 0]) == -4.0 * Ci * 3 * 7  # three of the seven tap rows lie inside the image
    want, _ = CR.epilogue_ref(acc, bias, alpha=0.125, res=res)
    xpad = F.pad(x, (0, 0, 3, 3, 3, 3))
    cols = torch.stack([xpad[:, ky:ky + H, kx:kx + W] for ky in range(7) for kx in range(7)], -2)  # N, H, W, 49, Ci
    wt = w.permute(0, 2, 3, 1).reshape(Co, 49, Ci)
    p32 = (cols[:, :, :, None] * wt[None, None, None]).reshape(N, H, W, Co, 49 * Ci).numpy()
    rng = np.random.default_rng(5)
    for _ in range(3):
        order = rng.permutation(p32.shape[-1])
        run32 = np.cumsum(p32[..., order], axis=-1, dtype=np.float32)
        assert np.array_equal(run32.astype(np.float64), np.cumsum(p32[..., order].astype(np.float64), axis=-1))
        v = (run32[..., -1] + bias.numpy()).astype(np.float32)
        v = ((v * np.float32(0.125)).astype(np.float32) + res.numpy()).astype(np.float32)
        assert torch.equal(torch.from_numpy(v).bfloat16(), want)


def test_real_bound_with_49_taps():
    v, S = torch.tensor([2.0], dtype=torch.float64), torch.tensor([3.0], dtype=torch.float64)
    e = float(CR.sum_bound(S, 32, taps=49))
    assert e == 2 * (49 * 32 + 4) * 2.0 ** -24 * 3
    assert float(CR.real_bound(v, S, 32, taps=49)) == 2.0 ** -8 * (2 + e) + e
    assert float(CR.real_bound(v, S, 32, taps=49, out_dtype=torch.float32)) == 2.0 ** -23 * (2 + e) + e
