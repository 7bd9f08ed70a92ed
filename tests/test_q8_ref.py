"""tests/q8_ref.py checked on the CPU: the records against their own statement (round trip, the (224, 448] property, torch's e4m3 cast and
the emulation of tests/test_fp8_gpu.py), the claim that every exact case of tests/test_conv_q8_kernels_gpu.py keeps its sums of magnitudes
below 2^12, and the probes.  (The kernels themselves: tests/test_conv_q8_kernels_gpu.py.)"""
import numpy as np
import pytest
import torch

from tests import conv_ref as CR
from tests import q8_ref as Q
from tests import test_conv_q8_kernels_gpu as G


def _octaves(shape, seed, lo=-30, hi=30):
    g = torch.Generator().manual_seed(seed)
    C = shape[-1]
    nb = (C + 31) // 32
    s = torch.exp2(torch.randint(lo, hi + 1, tuple(shape[:-1]) + (nb,), generator=g).float()).repeat_interleave(32, -1)[..., :C]
    return (torch.randn(*shape, generator=g) * s).bfloat16().float()


def test_e4m3_table_and_encoder_agree_with_torch():
    codes = torch.arange(256, dtype=torch.uint8)
    t = codes.view(torch.float8_e4m3fn).float().double().numpy()
    assert np.array_equal(t, Q.E4M3, equal_nan=True)
    assert Q.E4M3[0x7E] == 448.0 and Q.E4M3[0x38] == 1.0 and Q.E4M3[0x01] == 2.0 ** -9 and np.isnan(Q.E4M3[0x7F]) and np.isnan(Q.E4M3[0xFF])
    # every code but the NaNs and minus zero encodes to itself
    ok = ~np.isnan(Q.E4M3)
    assert np.array_equal(Q.e4m3_encode(Q.E4M3[ok]), np.arange(256, dtype=np.uint8)[ok])
    # every midpoint between neighbours goes to the even code, a hair to either side of it to the nearer one
    pos = Q.E4M3[:0x7F]
    mid = (pos[:-1] + pos[1:]) / 2
    even = np.where(np.arange(0x7E) % 2 == 0, np.arange(0x7E), np.arange(0x7E) + 1)
    assert np.array_equal(Q.e4m3_encode(mid), even.astype(np.uint8)) and np.array_equal(Q.e4m3_encode(-mid), (even | 0x80).astype(np.uint8))
    assert np.array_equal(Q.e4m3_encode(mid * (1 - 2.0 ** -20)), np.arange(0x7E, dtype=np.uint8))
    assert np.array_equal(Q.e4m3_encode(mid * (1 + 2.0 ** -20)), np.arange(1, 0x7F, dtype=np.uint8))
    # seeded values: torch's cast gives the same codes (the sign of a zero aside)
    v = (torch.randn(20000, generator=torch.Generator().manual_seed(1)) * torch.exp2(torch.randint(-12, 9, (20000,), generator=torch.Generator().manual_seed(2)).float()))
    v = v.clamp(-448, 448)
    mine = torch.from_numpy(Q.e4m3_encode(v.double().numpy()))
    theirs = v.to(torch.float8_e4m3fn).view(torch.uint8)
    z = lambda b: torch.where(b == 0x80, torch.zeros_like(b), b)  # noqa: E731
    assert torch.equal(z(mine), z(theirs))
    with pytest.raises(AssertionError):
        Q.e4m3_encode(np.array([449.0]))


def test_scale_byte_meets_its_statement():
    top = torch.cat([_octaves((4000, 1), 3, -120, 120).abs().reshape(-1), torch.tensor(Q.BOUNDARY_MAXIMA)]).double().numpy()
    top = top[top >= 2.0 ** -118]  # (below that the clamp at 1 takes over)
    sb = Q.scale_byte(top).astype(np.float64)
    scaled = top[top > 0] * np.exp2(127 - sb[top > 0])
    assert (scaled > 224).all() and (scaled <= 448).all() and (sb >= 1).all() and (sb <= 254).all()
    # a mantissa of exactly 1.75 sits on 448, the next bf16 above it just over 224
    for v in (3.5, 7.0, 448.0, 1.75 * 2.0 ** 40):
        assert float(v * 2.0 ** (127 - int(Q.scale_byte(np.array([v]))[0]))) == 448.0
        up = float(torch.tensor(v).bfloat16().view(torch.int16).add(1).view(torch.bfloat16))
        assert up > v and 224 < up * 2.0 ** (127 - int(Q.scale_byte(np.array([up]))[0])) < 226
    assert Q.scale_byte(np.array([0.0, 2.0 ** -126, 2.0 ** -140, 1.0, Q.BF16_MAX])).tolist() == [1, 1, 1, 119, 247]
    assert Q.BF16_MAX == float(torch.tensor(3.0e38).bfloat16().view(torch.int16).fill_(0x7F7F).view(torch.bfloat16))
    with pytest.raises(AssertionError):
        Q.scale_byte(np.array([np.inf]))


@pytest.mark.parametrize("C", [8, 40, 112, 144, 512])
def test_records_layout_round_trip_and_emulation(C):
    x = torch.cat([_octaves((300, C), 10 + C), Q.boundary_rows(C)])
    x[7] = 0
    rec = Q.records(x)
    nb = (C + 31) // 32
    assert rec.dtype == torch.uint8 and tuple(rec.shape) == (x.shape[0], nb * 32 + 16)
    assert int(rec[:, C:nb * 32].max() if C < nb * 32 else 0) == 0 and int(rec[:, nb * 32 + nb:].max() if nb < 16 else 0) == 0
    assert int(rec[7, :nb * 32].max()) == 0 and rec[7, nb * 32:nb * 32 + nb].tolist() == [1] * nb  # the all-zero pixel
    # the largest bf16, 255 * 2^120, rounds UP to 256 * 2^120 = 2^128, which no fp32 holds: its bytes are defined, its dequantised value is not
    big = x.abs().amax(-1) == Q.BF16_MAX
    assert int(big.sum()) == 1 and int((rec[big][:, :C] & 0x7F).max()) == 0x78 and rec[big][0, nb * 32:nb * 32 + nb].tolist() == [247] * nb
    assert bool(torch.isinf(Q.dequant(rec[big], C)).any()) and bool(torch.isinf(Q.quant_emul(x[big])).any())
    x, rec = x[~big], rec[~big]
    xq = Q.dequant(rec, C)
    # the same dequantised values as the emulation of tests/test_fp8_gpu.py (the kernel's bit formula, torch's cast)
    assert torch.equal(xq, Q.quant_emul(x))
    # a fixed point: the dequantised values dequantise to themselves (their bytes may differ: a maximum just above 224 rounds down to 224
    # itself, which the canonical rule stores as 448 under the next scale)
    assert torch.equal(Q.dequant(Q.records(xq), C), xq)
    # e4m3 keeps three mantissa bits under the block's scale: the error is at most 2^-4 of the value or half a subnormal step of the block
    sc = torch.exp2(rec[:, nb * 32:nb * 32 + nb].double() - 127).repeat_interleave(32, -1)[:, :C]
    assert bool(((xq.double() - x.double()).abs() <= torch.maximum(x.double().abs() * 2.0 ** -4, sc * 2.0 ** -10)).all())
    # the largest value of every block lands in (224, 448] of the e4m3 range, so on one of the codes 0x76 (a value just above 224 rounds down to 224) .. 0x7E
    data = rec[:, :nb * 32].reshape(-1, nb, 32)
    top = (data & 0x7F).amax(-1)
    live = x.abs().double().reshape(x.shape[0], -1)
    for b in range(nb):
        amax = live[:, 32 * b:min(C, 32 * b + 32)].amax(-1)
        big = amax >= 2.0 ** -118
        assert bool(((top[:, b] >= 0x76) & (top[:, b] <= 0x7E))[big].all())
    assert Q.E4M3[0x76] == 224.0 and Q.E4M3[0x7E] == 448.0


def test_records_with_scales_honours_any_scale():
    x, e = Q.scaled_x((2, 3, 5), 144, 5)
    sb = (127 + e).to(torch.uint8)
    rec = Q.records_with_scales(x, sb)
    assert torch.equal(Q.dequant(rec, 144), x) and torch.equal(Q.dequant(Q.records(x), 144), x)
    assert set(rec[..., :144].unique().tolist()) == {0x00, 0x38, 0xB8} and torch.equal(rec[..., 160:165], sb)
    assert set(Q.records(x)[..., :144].unique().tolist()) == {0x00, 0x78, 0xF8}  # canonically +-256
    assert sorted(sb.unique().tolist()) == [127, 128, 129]
    with pytest.raises(AssertionError):
        Q.records_with_scales(x, sb[..., :4])


def test_zero_sign_touches_data_bytes_only():
    rec = torch.full((2, 48), 0x80, dtype=torch.uint8)
    out = Q.zero_sign(rec)
    assert int(out[:, :32].max()) == 0 and bool((out[:, 32:] == 0x80).all()) and bool((rec == 0x80).all())
    n, first = Q.first_byte_mismatch(rec, torch.zeros_like(rec), 8)
    assert n == 32 and "scale byte of block 0" in first


def test_every_exact_gpu_case_holds_the_invariant():
    cases = G.exact_cases()
    assert len(cases) == 26 + 40 + 12
    worst = 0.0
    for geom, spec in cases:
        e = G.EPILOGUES[spec.epi]
        op = G.exact_operands(geom, spec.C, spec.family, e.get("dgrad", False))
        bias = op.bias if e.get("bias", True) else None
        top = Q.assert_q8_exact(op.x, op.w, bias, e.get("dgrad", False))
        worst = max(worst, top)
        # the family's own bound
        assert top <= (2 * 9 * spec.C + 8 if spec.family == "narrow" else 4 * 2 * 9 * spec.C + 8)
        assert int(op.x.abs().max()) <= (2 if spec.family == "narrow" else 4) and int(op.w.abs().max()) <= (2 if spec.family == "scaled" else 1)
    assert 1000 < worst < Q.CAP
    print(f"largest sum of magnitudes over {len(cases)} exact cases: {worst:g} (cap {Q.CAP})")
    x, w, b = Q.narrow((1, 2, 2), 144, 0)
    Q.assert_q8_exact(x, w, b)
    with pytest.raises(AssertionError):
        Q.assert_q8_exact(torch.full((1, 3, 3, 144), 2.0), torch.full((144, 144, 3, 3), 2.0))  # the centre pixel: 9 * 144 * 4 = 5184
    with pytest.raises(AssertionError):
        Q.assert_q8_exact(x + 0.5, w, b)            # no integers
    with pytest.raises(AssertionError):
        Q.assert_q8_exact(x, w, b + 4000)


def test_the_scaled_family_varies_the_scale_bytes():
    x, w, _ = Q.scaled((2, 7, 15), 144, 9)
    rec = Q.records(x)
    assert sorted(rec[..., 160:165].unique().tolist()) == [119, 120, 121] and bool((x[..., 0::32] != 0).all())
    assert 0.4 < float((x != 0).float().mean()) < 0.6 and 0.4 < float((w != 0).float().mean()) < 0.6
    assert sorted(w.abs().amax((1, 2, 3)).unique().tolist()) == [1.0, 2.0]


def test_gpu_case_table_covers_what_the_issue_lists():
    geo = G._geometry_cases()
    for C in G.CHANNELS:
        assert [g for g, s in geo if s == G.Spec(C)] == G.GEOMS
        assert [g for g, s in geo if s == G.Spec(C, "scaled")] == G.RAGGED
        assert [g for g, s in geo if s.family == "free" and s.C == C] == [(2, 7, 15)]
        assert {(g, s.epi) for g, s in G._epilogue_cases() if s.C == C} == {(g, e) for g in G.EPI_GEOMS for e in G.EXACT_EPILOGUES}
        assert {(g, s.family) for g, s in G._dgrad_cases() if s.C == C} == {(g, f) for g in G.RAGGED for f in ("narrow", "scaled")}
    assert len(G.EXACT_EPILOGUES) == 10 and len(G.GEOMS) == 9
    tiles = [n * -(-h // 8) * -(-w // 16) for n, h, w in G.GEOMS]
    assert tiles == [1, 1, 4, 2, 9, 3, 8, 16, 18]
    # the XCD remap (taken where the tile count is a multiple of 8) is the identity at 8 tiles and a real permutation at 16
    remap = lambda nblk: [(b & 7) * (nblk >> 3) + (b >> 3) for b in range(nblk)]  # noqa: E731
    assert remap(8) == list(range(8)) and remap(16) != list(range(16)) and sorted(remap(16)) == list(range(16))
    assert all(n * h * w <= 2048 for n, h, w in G.GEOMS)


def test_epilogue_ref_accepts_every_epilogue_of_the_table():
    for geom, spec in G._epilogue_cases() + G._dgrad_cases():
        p = G.exact_problem(geom, spec)
        assert (p.want is not None) == p.want_bf16 and (p.want_rec is not None) == p.want_q8
        if p.want is not None:
            assert p.want.dtype == torch.bfloat16 and tuple(p.want.shape) == geom + (spec.C,) and float(p.want.float().abs().max()) > 0
        if p.want_rec is not None:
            assert tuple(p.want_rec.shape) == geom + ((spec.C + 31) // 32 * 32 + 16,)
    a = G.exact_problem((3, 5, 33), G.Spec(144, epi="fp32_records"))
    assert a.want is None and a.want_rec is not None and G.exact_problem((3, 5, 33), G.Spec(144, epi="no_records")).want_rec is None


@pytest.mark.parametrize("C", [144, 112])
def test_impulse_gather_inverts_the_impulse_convolution(C):
    g = torch.Generator().manual_seed(C)
    x = Q.impulse_image(C)
    assert tuple(x.shape) == (1, 36, 36, C) and float(x.sum()) == C and bool((x.sum((0, 1, 2)) == 1).all())
    w = torch.randn(C, C, 3, 3, generator=g)
    out = CR.conv_ref([x], w)
    assert torch.equal(Q.impulse_gather(out, C), w.double())
    assert int((out != 0).sum()) == w.numel()  # every weight appears once and nothing else does
    wd = torch.randn(C, 24, 3, 3, generator=g)  # a data gradient: dy has C channels, dx 24
    dx = CR.dgrad_ref(x, wd)
    assert torch.equal(Q.impulse_gather(dx, C, dgrad=True), wd.double()) and int((dx != 0).sum()) == wd.numel()
    # every output element holds at most one product: the magnitude sum IS the magnitude
    assert torch.equal(Q.magnitude_sum(x, w), out.abs())


def test_wquant_ref_follows_the_statement_on_both_sides():
    w = G.readback_weight(144, False)
    wq = Q.wquant_ref(w)
    assert torch.equal(wq, Q.wquant_emul(w)) and not torch.equal(wq, w)
    assert float(wq[5].abs().max()) == 0 and float(wq[141].abs().max()) == 1.75 and float(w[141].abs().max()) == 1.75
    wt = G.readback_weight(144, True)
    wtq = Q.wquant_ref(wt, transpose_flip=True)
    assert float(wtq[:, 5].abs().max()) == 0 and float(wtq[:, 141].abs().max()) == 1.75
    # per input channel: the forward rule on the transposed weight
    assert torch.equal(wtq, Q.wquant_emul(wt.permute(1, 0, 2, 3).contiguous()).permute(1, 0, 2, 3))
    assert not torch.equal(wtq, Q.wquant_emul(wt))


def test_probe_activations_are_bf16_numbers_with_full_mantissas():
    for C in G.CHANNELS:
        rec, xq = G.probe_activations(C)
        assert float(xq[1, 3, 7].abs().max()) == 0 and torch.equal(Q.dequant(rec, C), xq)
        w, pi, ptap = CR.one_hot_weight(C, C, 4)
        assert torch.equal(Q.magnitude_sum(xq, w), CR.shifted_copy(xq, pi, ptap).abs().double())  # one product per output element
