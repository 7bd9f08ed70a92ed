"""tests/glue_ref.py against independent torch spellings, on the CPU: the references of the glue-kernel tests (tests/test_glue_kernels_gpu.py)
are themselves pinned here -- F.pixel_shuffle / F.pixel_unshuffle, F.interpolate(align_corners=True) and its autograd, cat / flip / transpose for
the frame pairing, Tensor.to(bfloat16) for the rounding, F.avg_pool2d."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import glue_ref as G
from tests import tab_ops_ref as TR

F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, dtype=F32):
    return torch.randn(tuple(shape), generator=_gen(seed)).to(dtype)


# ================================================================================================ activation backward
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_act_backward_ref(dtype):
    """Against autograd through torch's own activations (alpha = 1: the chain rule's single product), on +-0, +-inf, a denormal; NaN
    takes the `false` side of ref > 0; the product order ((dy * d) * alpha) is spelled out for an inexact alpha."""
    ref = _randn((64,), 1, dtype)
    ref[:5] = torch.tensor([0.0, -0.0, 2.0 ** -130, float("inf"), -float("inf")]).to(dtype)
    dy = _randn((64,), 2, dtype)
    for act, fn in ((G.ACT_RELU, F.relu), (G.ACT_LRELU, lambda v: F.leaky_relu(v, 0.1))):
        x = ref.float().clone().requires_grad_(True)
        fn(x).backward(dy.float())
        got = G.act_backward_ref(dy, ref, act, 0.1, 1.0, dtype)
        # (values, not bits: autograd SELECTS a +0 where the definition's product dy * 0 keeps dy's sign; the loop below pins the bits)
        assert got.dtype == dtype and torch.equal(got, x.grad.to(dtype))
    assert torch.equal(G.bits(G.act_backward_ref(dy, ref, G.ACT_NONE, 0.1, 1.0, dtype)), G.bits(dy))
    ref[5] = float("nan")
    a = np.float32(1.0 / 3.0)
    for act, lo in ((G.ACT_RELU, 0.0), (G.ACT_LRELU, 0.1)):
        got = G.act_backward_ref(dy, ref, act, 0.1, 1.0 / 3.0, dtype)
        want = [np.float32(np.float32(np.float32(v) * (np.float32(1.0) if r > 0 else np.float32(lo))) * a) for v, r in zip(dy.float().tolist(), ref.float().tolist())]
        assert torch.equal(G.bits(got), G.bits(torch.tensor(np.array(want, dtype=np.float32)).to(dtype)))
        assert float(got[5]) == float((dy[5].float() * np.float32(lo) * a).to(dtype))  # NaN reference: the `else` side
    # GELU: autograd through F.gelu in fp64
    x = ref.double().clone()[6:].requires_grad_(True)
    F.gelu(x).backward(dy.double()[6:] * 0.5)
    want, mag = G.act_backward_ref(dy[6:], ref[6:], G.ACT_GELU, 0.0, 0.5, dtype)
    assert float((want - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    assert torch.equal(mag, (dy.double()[6:] * 0.5).abs())
    want, _ = G.act_backward_ref(dy[:6], ref[:6], G.ACT_GELU, 0.0, 0.5, dtype)
    assert torch.isnan(want).tolist() == [False, False, False, True, True, True]  # +-0, denormal | +-inf (inf * 0), NaN
    assert want[:3].tolist() == (dy.double()[:3] * 0.25).tolist()                    # gelu'(0) = 1/2


# ================================================================================================ depth <-> space
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 5, 7, 12), (1, 3, 130, 96), (2, 3, 2, 4)], ids=lambda s: "x".join(map(str, s)))
def test_pixel_shuffle_refs(shape):
    x = _randn(shape, 3)
    want = F.pixel_shuffle(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    got = G.pixel_shuffle_ref(x)
    assert got.is_contiguous() and torch.equal(got, want)
    back = G.pixel_unshuffle_ref(got)
    assert back.is_contiguous() and torch.equal(back, x)
    assert torch.equal(back, F.pixel_unshuffle(want.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))


# ================================================================================================ frame moves
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,t", [(1, 1), (2, 5), (3, 7)])
def test_frame_pairing_refs(dtype, n, t):
    """The (t, 2n) arrangement of the lock-step sweeps = cat([flip(x^T), x^T], 1) as a one-column gather; its gradient as a two-column
    gather-add; the step tensors of pair_steps_ref are the rows of that arrangement, mode 1 inverts mode 0, mode 2 is the gradient."""
    fe = 24
    x = _randn((n, t, fe), 4, dtype)
    xt = x.transpose(0, 1)
    want = torch.cat([xt.flip(0), xt], 1)  # (t, 2n, fe)
    fi = torch.tensor([[i * t + (t - 1 - j if r == 0 else j)] for j in range(t) for r in range(2) for i in range(n)], dtype=torch.int32)
    got = G.frame_gather_ref(x.reshape(n * t, fe), fi).reshape(t, 2 * n, fe)
    assert got.dtype == dtype and torch.equal(got, want)
    go = _randn((t, 2 * n, fe), 5, dtype)
    gref = (go.float()[:, :n].flip(0) + go.float()[:, n:]).transpose(0, 1).to(dtype)  # (n, t, fe)
    bi = torch.tensor([[(t - 1 - f) * 2 * n + i, f * 2 * n + n + i] for i in range(n) for f in range(t)], dtype=torch.int32)
    assert torch.equal(G.frame_gather_ref(go.reshape(t * 2 * n, fe), bi).reshape(n, t, fe), gref)
    steps = list(want.unbind(0))
    back, fwd = G.pair_steps_ref(0, n, t, steps=steps)
    assert torch.equal(back, x) and torch.equal(fwd, x)
    a, b = _randn((n, t, fe), 6, dtype), _randn((n, t, fe), 7, dtype)
    st = G.pair_steps_ref(1, n, t, a=a, b=b)
    assert len(st) == t and all(s.shape == (2 * n, fe) for s in st)
    assert torch.equal(torch.stack(st, 0), torch.cat([a.transpose(0, 1).flip(0), b.transpose(0, 1)], 1))
    a2, b2 = G.pair_steps_ref(0, n, t, steps=st)
    assert torch.equal(a2, a) and torch.equal(b2, b)
    assert torch.equal(G.pair_steps_ref(2, n, t, steps=list(go.unbind(0))), gref)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_frame_gather_ref_skips_negative_indices(dtype):
    src = _randn((5, 16), 8, dtype)
    idx = torch.tensor([[1, 3], [-1, 2], [4, -1], [-1, -1], [2, 2]], dtype=torch.int32)
    got = G.frame_gather_ref(src, idx)
    assert torch.equal(got[0], (src[1].float() + src[3].float()).to(dtype))
    assert torch.equal(got[1], src[2]) and torch.equal(got[2], src[4])
    assert bool((G.bits(got[3]) == 0).all())
    assert torch.equal(got[4], (2 * src[2].float()).to(dtype))
    assert torch.equal(G.frame_gather_ref(src, torch.tensor([[3], [3], [0]], dtype=torch.int32)), torch.stack([src[3], src[3], src[0]]))


def test_sum_and_cast_refs_round_once():
    """bf16: the fp32 sum rounded ONCE differs from pairwise bf16 adds and equals Tensor.to(bfloat16) of the float sum; fp32: the left-to-right sum."""
    ts = [_randn((4096,), 10 + i, BF16) for i in range(4)]
    want = (((ts[0].float() + ts[1].float()) + ts[2].float()) + ts[3].float())
    got = G.sum_n_ref(ts)
    assert got.dtype == BF16 and torch.equal(got, want.to(BF16))
    assert not torch.equal(got, ((ts[0] + ts[1]) + ts[2]) + ts[3])
    fs = [_randn((4096,), 20 + i) for i in range(3)]
    assert torch.equal(G.sum_n_ref(fs), (fs[0] + fs[1]) + fs[2])
    assert not torch.equal(G.sum_n_ref(fs), fs[0] + (fs[1] + fs[2]))  # the order is part of the definition
    assert torch.equal(G.sum_n_ref([fs[0], fs[0]]), 2 * fs[0])
    acc = _randn((4096,), 30)
    assert torch.equal(G.cast_clear_ref(acc, None, BF16), acc.to(BF16)) and torch.equal(G.cast_clear_ref(acc, None, F32), acc)
    assert torch.equal(G.cast_clear_ref(acc, ts[0], BF16), (acc + ts[0].float()).to(BF16))
    # round to nearest, ties to even, as Tensor.to(bfloat16): 1 + 2^-8 is a tie -> 1; 1 + 3 * 2^-8 is a tie -> 1 + 2^-6
    tie = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])
    assert G.cast_clear_ref(tie, None, BF16).float().tolist() == [1.0, 1.0 + 2.0 ** -6]


# ================================================================================================ SPyNet glue
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_spynet_glue_refs(dtype):
    img = torch.rand((2, 3, 5, 7), generator=_gen(40))
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    got = G.spy_prep_ref(img, mean, std, dtype)
    want = F.pad(((img - mean[None, :, None, None]) / std[None, :, None, None]).permute(0, 2, 3, 1), (0, 5)).to(dtype)
    assert got.dtype == dtype and got.shape == (2, 5, 7, 8) and torch.equal(G.bits(got), G.bits(want))
    assert bool((G.bits(got[..., 3:]) == 0).all())
    px = np.float32(np.float32(img[1, 2, 3, 4].item()) - np.float32(0.406)) / np.float32(0.225)
    assert float(got[1, 3, 4, 2]) == float(torch.tensor(px).to(dtype))

    ref, warped = _randn((2, 5, 7, 8), 41, dtype), _randn((2, 5, 7, 8), 42, dtype)
    up = _randn((2, 5, 7, 2), 43)
    r = ref.clone().requires_grad_(True)
    w = warped.clone().requires_grad_(True)
    u = up.clone().requires_grad_(True)
    want = torch.cat([r[..., :3], w[..., :3], u.to(dtype)], -1)
    assert torch.equal(G.spy_operand_ref(ref, warped, up), want.detach())
    go = _randn((2, 5, 7, 8), 44, dtype)
    want.backward(go)
    dw, du = G.spy_operand_bwd_ref(go)
    assert torch.equal(G.bits(dw), G.bits(w.grad)) and du.dtype == F32 and torch.equal(du, u.grad)
    assert bool((G.bits(dw[..., 3:]) == 0).all())
    res = _randn((2, 5, 7, 2), 45, dtype)
    assert torch.equal(G.spy_flow_add_ref(up, res), up + res.float())


def test_avgpool2_ref():
    x = torch.randint(-4, 5, (2, 7, 9, 3), generator=_gen(50)).float()
    y, mag = TR.avgpool2_ref(x)
    assert torch.equal(y.float(), F.avg_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))
    assert torch.equal(mag.float(), F.avg_pool2d(x.abs().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))


# ================================================================================================ bilinear x2, align_corners=True
UP_SHAPES = [(3, 1, 1, 2), (2, 5, 3, 2), (1, 64, 112, 2), (2, 1, 9, 3), (1, 37, 1, 1)]


def _interp(x):
    return F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_refs_against_interpolate(shape):
    """With fp64 coordinates: F.interpolate on a double tensor and its autograd, within 1e-12 relative.  With fp32 coordinates (what the kernel
    tests use): F.interpolate on the float tensor within the forward bound those tests assert, 8 * 2^-24 * S -- the index choice is torch's."""
    n, h, w, c = shape
    x = _randn(shape, 60).double().requires_grad_(True)
    y = _interp(x)
    val, S = G.upsample2x_ac_ref(x.detach(), 0.75, np.float64)
    assert val.shape == (n, 2 * h, 2 * w, c) and val.dtype == torch.float64
    assert float((val - 0.75 * y.detach()).abs().max()) <= 1e-12 * float(y.detach().abs().max())
    assert bool((S >= val.abs() * (1 - 1e-12)).all())
    g = _randn((n, 2 * h, 2 * w, c), 61).double()
    y.backward(g)
    adj, Sa = G.upsample2x_ac_adjoint_ref(g, 0.75, np.float64)
    assert adj.shape == tuple(shape)
    assert float((adj - 0.75 * x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    assert bool((Sa >= adj.abs() * (1 - 1e-12)).all())
    # the rows of the weights sum to one, with at most two non-zero entries, both in [0, 1]
    for co in (np.float32, np.float64):
        W = G.ac_weights(h, 2 * h, co)
        assert float((W.sum(1) - 1).abs().max()) <= 1e-15 and int((W != 0).sum(1).max()) <= 2 and float(W.min()) >= 0.0
    x32 = x.detach().float()
    v32, S32 = G.upsample2x_ac_ref(x32, 0.75)
    err = (0.75 * _interp(x32).double() - v32).abs()
    assert bool((err <= 8 * U * S32).all()), float((err / (U * S32)).max())


@pytest.mark.parametrize("coord", [np.float32, np.float64], ids=["coord32", "coord64"])
@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_adjoint_dot_product(shape, coord):
    """<U x, g> = <x, U^T g> from the reference alone, to 1e-12 relative."""
    n, h, w, c = shape
    x, g = _randn(shape, 62), _randn((n, 2 * h, 2 * w, c), 63)
    ux, _ = G.upsample2x_ac_ref(x, -1.5, coord)
    utg, _ = G.upsample2x_ac_adjoint_ref(g, -1.5, coord)
    lhs, rhs = float((ux * g.double()).sum()), float((x.double() * utg).sum())
    scale = float((ux.abs() * g.double().abs()).sum())
    assert abs(lhs - rhs) <= 1e-12 * scale
