"""tests/morph_ref.py (index arithmetic, fp64) against the oracle's restatement of the reference's pad + rearrange chain
(oracle.vmg_oracle.morph_tokens / morph_untokens) and against torch autograd of the oracle's branch in fp64.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import morph_ref as MR
from tests import wgrad_ref as WR

# (chunk, Cp, C, H, W): axis lengths that are and are not chunk multiples (remainders 1 and chunk - 1, a line shorter than a chunk), C == Cp and C < Cp,
# even and odd S, S = 1
GEOMS = [(8, 16, 16, 8, 16), (8, 16, 8, 9, 15), (16, 32, 24, 3, 33), (16, 16, 8, 17, 31), (4, 12, 10, 7, 9), (8, 144, 136, 17, 5), (16, 144, 144, 16, 1),
         (3, 9, 8, 5, 4), (12, 228, 224, 13, 11)]
BT = (2, 3)


def _x(g, seed, dtype=torch.float64):
    chunk, Cp, C, H, W = g
    return torch.randn(BT + (H, W, C), generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)


@pytest.mark.parametrize("axis", ["h", "w"])
@pytest.mark.parametrize("g", GEOMS)
def test_tokens_and_untokens_equal_the_oracle(g, axis):
    from oracle import vmg_oracle as O
    chunk, Cp, C, H, W = g
    x = _x(g, 1)
    want = O.morph_tokens(x, axis, chunk, Cp)
    got = MR.tokens_ref(x, axis, chunk, Cp)
    assert got.shape == (MR.token_rows(axis, chunk, BT[0] * BT[1], H, W), Cp)
    assert torch.equal(got, want.reshape(-1, Cp))
    # padded positions / channels are zero, everything else is an element of x exactly once
    assert int((got != 0).sum()) == x.numel()
    t = torch.randn(want.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    back = MR.untokens_ref(t.reshape(-1, Cp), axis, chunk, Cp, H, W, C)
    assert torch.equal(back.reshape(BT + (H, W, C)), O.morph_untokens(t, axis, chunk, Cp, H, W, C))
    assert torch.equal(MR.untokens_ref(got, axis, chunk, Cp, H, W, C).reshape(x.shape), x)
    # a wider row (features [Cp, ld) ignored), and bit patterns as integers
    wide = torch.cat([got, torch.full((got.shape[0], 5), 7.0, dtype=got.dtype)], 1)
    assert torch.equal(MR.untokens_ref(wide, axis, chunk, Cp, H, W, C).reshape(x.shape), x)
    xi = torch.randint(-2 ** 15, 2 ** 15, tuple(x.shape), generator=torch.Generator().manual_seed(3)).to(torch.int16)
    assert torch.equal(MR.tokens_ref(xi, axis, chunk, Cp).double(), MR.tokens_ref(xi.double(), axis, chunk, Cp))


def test_prepare_ref_treats_zeros_and_nan_as_not_positive():
    x = torch.tensor([1.5, 1.5, 1.5, 1.5, -3.0, 1.0 + 2.0 ** -7], dtype=torch.bfloat16)
    m = torch.tensor([0.0, -0.0, float("nan"), -1.0, 2.0 ** -130, 1.0], dtype=torch.bfloat16)
    got = MR.prepare_ref(x, m, 0.125)
    assert got.tolist() == [0.0, 0.0, 0.0, 0.0, -0.375, (1.0 + 2.0 ** -7) / 8]
    assert not torch.signbit(got[:4]).any()
    # a scale that is no power of two: the fp32 product, rounded once to bf16
    got = MR.prepare_ref(x[5:], m[5:], 1.0 / 144)
    assert float(got) == float((x[5:].float() * torch.tensor(1.0 / 144, dtype=torch.float32)).bfloat16())


@pytest.mark.parametrize("axis", ["h", "w"])
@pytest.mark.parametrize("g", [g for g in GEOMS if g[1] <= 144])
def test_branch_ref_equals_autograd_of_the_oracle_branch(g, axis):
    """Forward form: relu(Linear(tokens)) * scale, untokened.  Data-gradient form: the input gradient torch autograd gives for that branch, from
    branch_ref on dy with the transposed matrix and the forward output as the mask.  Operands of the "full" family and power-of-two scales: the
    bf16 roundings of the operand preparation round nothing, so the two must agree to fp64 summation error."""
    from oracle import vmg_oracle as O
    chunk, Cp, C, H, W = g
    shape = BT + (H, W, C)
    x, dy = WR.exact_values(shape, 11, "full"), WR.exact_values(shape, 12, "full")
    w, b = WR.exact_values((Cp, Cp), 13, "full"), WR.exact_values((Cp,), 14, "full")
    sc, isc = 2.0 ** -7, 2.0 ** -3
    xo = x.double().requires_grad_(True)
    want = O.morph_untokens(F.relu(F.linear(O.morph_tokens(xo, axis, chunk, Cp), w.double(), b.double())) * sc, axis, chunk, Cp, H, W, C)
    v, S, tok = MR.branch_ref(x.bfloat16(), w, b, axis, chunk, Cp, True, sc)
    assert v.shape == (BT[0] * BT[1], H, W, C) and S.shape == v.shape and tok.dtype == torch.bfloat16
    assert torch.equal(tok.double(), MR.tokens_ref(x.double(), axis, chunk, Cp))
    assert torch.equal(v.reshape(shape), want.detach())  # (integers of 2^-21 below 2^53: fp64 sums are exact in any order)
    # S: the same sum over magnitudes, before ReLU and scale
    va, _, _ = MR.branch_ref(x.abs().bfloat16(), w.abs(), b.abs(), axis, chunk, Cp, False, 1.0)
    assert torch.equal(S, va) and bool((S * sc >= v.abs()).all())
    (dx,) = torch.autograd.grad(want, [xo], (dy.double() * isc / sc))  # d/dx of <want / sc, dy * isc>
    y = want.detach().bfloat16()
    assert torch.equal((y > 0), (want.detach() > 0))
    gv, gS, gtok = MR.branch_ref(dy.bfloat16(), w.t(), None, axis, chunk, Cp, False, 1.0, mask=y, in_scale=isc)
    assert torch.equal(gv.reshape(shape), dx)
    # the token side output of the data-gradient form: tokens of dy * [y > 0] * in_scale
    assert torch.equal(gtok.double(), MR.tokens_ref(torch.where(want.detach() > 0, dy.double() * isc, torch.zeros((), dtype=torch.float64)), axis, chunk, Cp))
    assert 0.2 < float((y > 0).double().mean()) < 0.8
