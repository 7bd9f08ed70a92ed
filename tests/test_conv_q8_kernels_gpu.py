"""The fp8 path of csrc/conv_fp8.hip -- convq8_kernel<9,5> / <7,4>, the pack kernels convq8_scale_kernel / convq8_pack_kernel,
q8_quantize_kernel and the chain entry vmg_resblock_chain_fwd_q8 -- element by element and byte by byte against the host reference of
tests/q8_ref.py and the fp64 convolution of tests/conv_ref.py.

Exactness invariant.  An e4m3 value times a power of two is a bf16 number and the matrix instruction's products are exact.  The operand
families of q8_ref (small integers, exact in e4m3 under the canonical scale) keep S = sum |x||w| + |bias| below 2^12 per output element --
q8_ref.assert_q8_exact, on the CPU BEFORE the launch --, so every partial sum, the accumulator (which starts from the bias) included, is an
integer below 2^12: the instruction's adder keeps about 14 bits below its largest product, which holds these sums whichever way the
accumulator input is aligned.  The bf16 output must EQUAL round_bf16(fp64 reference) and the record output, byte for byte, the host's
records of the value the kernel quantises (the bf16-rounded one when a bf16 output exists, else the fp32 one).  One dropped or misplaced
(tap, channel) term, a record of the neighbouring row at an image corner, a wrong channel inside one 16-byte half of a slot, a scale byte of
another block changes them.

Probes with ONE nonzero product per output element are exact for ANY values: one-hot weights make the output a shifted copy of the
dequantised records (real-valued activations over twelve octaves: a failure names the tap and the channel), one-hot activations
(q8_ref.impulse_image) make it the dequantised weight image itself -- the scale rule and every byte of the pack, read back without knowing
the layout.

What every launch shares: the source records are a view inside an allocation filled with 0xFF (NaN as e4m3 data and as an E8M0 scale), out
and res views with pixel strides Cout + 8 / Cout + 16 inside NaN-filled allocations (wgrad_ref.embed), the record output a view inside an
allocation filled with 0xAA; two launches must give the same bits, leave everything outside the views alone, no NaN inside, and no byte of
a record unwritten (padding and the unused scale bytes are zero by contract)."""
import functools
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import pytest
import torch

from tests import conv_ref as CR
from tests import q8_ref as Q
from tests import wgrad_ref as WR

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16

# (N, H, W); tiles are 8 x 16 pixels
GEOMS = [(1, 1, 1),     # smaller than a tile: the image lies inside the halo
         (1, 8, 16),    # exactly one tile
         (1, 9, 17),    # one pixel over in both directions
         (2, 7, 15),    # ragged, two images: the halo must not read the other image
         (3, 5, 33),    # ragged, three images
         (1, 17, 3),    # narrower than a tile
         (2, 16, 32),   # 8 tiles: the XCD remap branch is taken but is the identity
         (2, 16, 64),   # 16 tiles: the first count at which the remap permutes
         (1, 24, 81)]   # 18 tiles, not a multiple of 8
RAGGED = [(2, 7, 15), (3, 5, 33), (1, 17, 3)]
EPI_GEOMS = [(2, 7, 15), (3, 5, 33)]
CHANNELS = (144, 112)

# name -> the epilogue of vmg_convq8_fwd.  `dgrad`: a data-gradient pack (transpose_flip), reference conv_ref.dgrad_ref
EPILOGUES = {
    "plain": dict(bias=False),
    "bias": dict(),
    "relu": dict(act=CR.ACT_RELU),
    "lrelu_0.25": dict(act=CR.ACT_LRELU, slope=0.25),
    "lrelu_0.1": dict(act=CR.ACT_LRELU, slope=0.1),            # one rounding of v * float32(0.1), then bf16 (epilogue_ref allows it: nothing follows)
    "relu_alpha_0.5": dict(act=CR.ACT_RELU, alpha=0.5),
    "res_alpha_0.125": dict(alpha=0.125, res=True),            # the chain's conv2 with a power of two for r_scaling
    "res_alpha_1": dict(res=True),
    "fp32_records": dict(act=CR.ACT_RELU, want_bf16=False),    # the chain's conv1 when t is not kept: records from the fp32 values
    "no_records": dict(want_q8=False),
    "dgrad": dict(bias=False, dgrad=True),
}
EXACT_EPILOGUES = [n for n in EPILOGUES if n != "dgrad"]


class Spec(NamedTuple):
    """One convolution C -> C.  family: "narrow" / "scaled" (q8_ref.FAMILIES, canonical records) or "free": scaled activations k * 2^e stored
    as e4m3 +-1.0 with the NON-canonical scale byte 127 + e (a record is e4m3 * 2^(sb - 127) whatever produced it), narrow weights."""
    C: int
    family: str = "narrow"
    epi: str = "bias"

    @property
    def id(self):
        return f"{self.C}-{self.family}-{self.epi}"


def _geometry_cases():
    return [(g, Spec(C)) for C in CHANNELS for g in GEOMS] + [(g, Spec(C, "scaled")) for C in CHANNELS for g in RAGGED] + \
        [((2, 7, 15), Spec(C, "free")) for C in CHANNELS]


def _epilogue_cases():
    return [(g, Spec(C, epi=e)) for e in EXACT_EPILOGUES for C in CHANNELS for g in EPI_GEOMS]


def _dgrad_cases():
    return [(g, Spec(C, f, "dgrad")) for f in ("narrow", "scaled") for C in CHANNELS for g in RAGGED]


def exact_cases():
    """Every (geometry, spec) of the exact tests: tests/test_q8_ref.py checks q8_ref.assert_q8_exact on each without a GPU."""
    return _geometry_cases() + _epilogue_cases() + _dgrad_cases()


def _seed(geom, C):
    return (geom[0] * 7919 + geom[1] * 104729 + geom[2] * 1299709 + C * 31) % (2 ** 31 - 1)


@functools.lru_cache(maxsize=None)
def exact_operands(geom, C, family, dgrad):
    """The CPU side that the epilogues of a (geometry, channel case) share: x, w, the full bias, the source records, the fp64 sums and max S.
    Returns a namespace that nobody changes."""
    seed = _seed(geom, C) + (500 if dgrad else 0)
    if family == "free":
        x, e = Q.scaled_x(geom, C, seed)
        _, w, bias = Q.narrow(geom, C, seed + 1)
        rec = Q.records_with_scales(x, (127 + e).to(torch.uint8))
        data = rec[..., :rec.shape[-1] - 16]
        assert set(data.unique().tolist()) <= {0x00, 0x38, 0xB8}  # e4m3 0 and +-1.0
        assert not torch.equal(rec, Q.records(x))                 # (not the canonical records)
    else:
        x, w, bias = Q.FAMILIES[family](geom, C, seed)
        rec = Q.records(x)
    assert torch.equal(Q.dequant(rec, C), x), "the activations are not exact in their records"
    assert torch.equal(Q.wquant_ref(w, dgrad), w), "the weights are not exact in e4m3 under the canonical scale"
    acc = CR.dgrad_ref(x, w) if dgrad else CR.conv_ref([x], w)
    return SimpleNamespace(x=x, w=w, bias=bias, rec=rec, acc=acc, S=Q.magnitude_sum(x, w, None, dgrad))


def exact_problem(geom, spec):
    """One exact convolution with its epilogue: the invariant, then the expected bf16 output and record bytes (None where not asked for)."""
    e = dict(EPILOGUES[spec.epi])
    dgrad = e.pop("dgrad", False)
    op = exact_operands(geom, spec.C, spec.family, dgrad)
    bias = op.bias if e.pop("bias", True) else None
    top = Q.assert_q8_exact(op.x, op.w, bias, dgrad)  # the invariant, before anything runs on the GPU
    assert top == float((op.S + (bias.abs().double() if bias is not None else 0)).max())
    want_bf16, want_q8 = e.pop("want_bf16", True), e.pop("want_q8", True)
    res = WR.exact_values(geom + (spec.C,), _seed(geom, spec.C) + 2000, "small") if e.pop("res", False) else None
    out16, _ = CR.epilogue_ref(op.acc, bias, res=res, exact=True, **e)
    out32, _ = CR.epilogue_ref(op.acc, bias, res=res, exact=True, out_dtype=torch.float32, **e)
    seen = out16.float() if want_bf16 else out32  # what the kernel quantises
    return SimpleNamespace(geom=geom, C=spec.C, what=f"{geom} {spec.id}", rec=op.rec, w=op.w, dgrad=dgrad, bias=bias, res=res, kw=e,
                           want_bf16=want_bf16, want_q8=want_q8, want=out16 if want_bf16 else None,
                           want_rec=Q.records(seen) if want_q8 else None, name=_pixel)


def _pixel(idx):
    return f"image {idx[0]}, pixel ({idx[1]}, {idx[2]}), output channel {idx[3]}"


def _mods():
    from vmg_amd import hip, kernels as K
    return hip, K


def _guarded_bytes(payload, guard, fill, dev="cuda"):
    """payload (..., rec) uint8 -> a contiguous view of its shape inside a uint8 allocation filled with `fill`, `guard` bytes (a multiple of
    16) on both sides; payload None: the view keeps the fill."""
    shape = tuple(payload.shape) if isinstance(payload, torch.Tensor) else tuple(payload)
    n = int(np.prod(shape))
    assert guard % 16 == 0
    flat = torch.full((guard + n + guard,), fill, dtype=torch.uint8, device=dev)
    view = flat[guard:guard + n].view(shape)
    if isinstance(payload, torch.Tensor):
        view.copy_(payload)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0 and view.data_ptr() == flat.data_ptr() + guard
    return flat, view


def _outside_mask(view):
    C, ps = view.shape[-1], view.stride(-2)
    M = view.numel() // C
    mask = torch.ones(view._base.numel(), dtype=torch.bool)
    idx = (view.storage_offset() + torch.arange(M)[:, None] * ps + torch.arange(C)[None, :]).reshape(-1)
    mask[idx] = False
    return mask


def _launch(p):
    """Pack, place every operand inside its guarded allocation, launch twice.  Returns (out or None, record bytes or None) as CPU tensors
    after the checks every case shares."""
    hip, K = _mods()
    assert (hip.ACT_NONE, hip.ACT_RELU, hip.ACT_LRELU) == (CR.ACT_NONE, CR.ACT_RELU, CR.ACT_LRELU)
    (N, H, W), C = p.geom, p.C
    guard = 10 * W + 32  # pixels: more than a tile with its halo could reach past either end of the image
    rec_b = K.q8_record_bytes(C)
    assert rec_b == p.rec.shape[-1] == (C + 31) // 32 * 32 + 16 and tuple(p.rec.shape[:3]) == (N, H, W)
    src_flat, src = _guarded_bytes(p.rec, guard * rec_b, 0xFF)
    src_before = src_flat.clone()
    pw = K.pack_conv_weight_q8(p.w.cuda().contiguous(), transpose_flip=p.dgrad)
    assert pw.cout == C and pw.cin == C
    res = WR.embed(p.res.to(BF16), C + 16, guard, device="cuda") if p.res is not None else None
    if res is not None:
        assert torch.equal(res.float().cpu(), p.res)
    out = WR.embed(torch.full((N, H, W, C), float("nan"), dtype=BF16), C + 8, guard, device="cuda") if p.want_bf16 else None
    oq_flat, oq = _guarded_bytes((N, H, W, rec_b), guard * rec_b, 0xAA) if p.want_q8 else (None, None)
    out_before = out._base.clone() if out is not None else None
    bias = p.bias.cuda() if p.bias is not None else None
    runs = []
    for _ in range(2):
        if out is not None:
            out._base.copy_(out_before)
        if oq is not None:
            oq_flat.fill_(0xAA)
        o, q = K.conv_q8_forward(src, pw, bias, N, H, W, res=res, want_bf16=p.want_bf16, want_q8=p.want_q8, out=out, outq=oq, **p.kw)
        torch.cuda.synchronize()
        assert (o is None) == (out is None) and (q is None) == (oq is None)
        assert (o is None or o.data_ptr() == out.data_ptr()) and (q is None or q.data_ptr() == oq.data_ptr())
        runs.append((out._base.cpu() if out is not None else None, oq_flat.cpu() if oq is not None else None))
    assert torch.equal(src_flat, src_before), p.what + ": the source allocation changed"
    got = gotq = None
    if out is not None:
        full, again = runs[0][0], runs[1][0]
        assert torch.equal(full.view(torch.int16), again.view(torch.int16)), p.what + ": out: the second launch gave other bits"
        mask = _outside_mask(out)
        assert torch.equal(full.view(torch.int16)[mask], out_before.cpu().view(torch.int16)[mask]), p.what + ": out: the allocation changed outside the view"
        assert bool(torch.isnan(full[mask]).all())
        got = out.cpu()
        nan = torch.isnan(got)
        if bool(nan.any()):
            first = tuple(int(v) for v in torch.nonzero(nan)[0])
            raise AssertionError(f"{p.what}: out: {int(nan.sum())} of {got.numel()} elements are NaN, the first at {p.name(first)}: something outside "
                                 "the operands was read, or the element was never written")
    if oq is not None:
        full, again = runs[0][1], runs[1][1]
        assert torch.equal(full, again), p.what + ": records: the second launch gave other bits"
        g = guard * rec_b
        assert bool((full[:g] == 0xAA).all()) and bool((full[full.numel() - g:] == 0xAA).all()), p.what + ": records: the allocation changed outside the view"
        gotq = full[g:full.numel() - g].view(N, H, W, rec_b)
        # every byte of a record is defined, padding included: a byte that still holds the fill where the reference has another was never written
        left = gotq == 0xAA
        if p.want_rec is not None:
            left &= p.want_rec != 0xAA
            if bool(left.any()):
                first = tuple(int(v) for v in torch.nonzero(left)[0])
                raise AssertionError(f"{p.what}: records: {int(left.sum())} bytes were never written, the first at image {first[0]}, pixel "
                                     f"({first[1]}, {first[2]}), byte {first[3]}")
        db = rec_b - 16
        nb = db // 32
        assert not bool((gotq[..., C:db] != 0).any()), p.what + ": records: data bytes beyond the channel count are not zero"
        assert not bool((gotq[..., db + nb:] != 0).any()), p.what + ": records: scale bytes beyond the block count are not zero"
        assert not bool((gotq[..., :db] & 0x7F == 0x7F).any()), p.what + ": records: NaN data bytes"
    return got, gotq


def _assert_out(got, want, p):
    n, idx, g, w = WR.first_mismatch(got, want)
    if n:
        err = float((got.double() - want.double()).abs().max())
        raise AssertionError(f"{p.what}: out: {n} of {got.numel()} elements differ from the reference, the first at {p.name(idx)}: got {g!r}, want {w!r} "
                             f"(largest error {err:g})")
    assert torch.equal(got, want), p.what


def _assert_records(gotq, want, p):
    n, first = Q.first_byte_mismatch(gotq, want, p.C)
    assert n == 0, f"{p.what}: records: {n} of {gotq.numel()} bytes differ from the host's records, the first at {first}"
    assert torch.equal(Q.zero_sign(gotq), Q.zero_sign(want))


def _run(p):
    got, gotq = _launch(p)
    assert (got is not None) == p.want_bf16 and (gotq is not None) == p.want_q8
    if p.want is not None:
        _assert_out(got, p.want, p)
    if p.want_rec is not None:
        _assert_records(gotq, p.want_rec, p)
    return got, gotq


def _ids(cases):
    return ["x".join(map(str, g)) + "-" + s.id for g, s in cases]


# ------------------------------------------------------------------------------------------------------------------------------------
# exact cases
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,spec", _geometry_cases(), ids=_ids(_geometry_cases()))
def test_q8_geometries_and_operand_families(geom, spec):
    _run(exact_problem(geom, spec))


@pytest.mark.parametrize("geom,spec", _epilogue_cases(), ids=_ids(_epilogue_cases()))
def test_q8_epilogues(geom, spec):
    _run(exact_problem(geom, spec))


@pytest.mark.parametrize("geom,spec", _dgrad_cases(), ids=_ids(_dgrad_cases()))
def test_q8_data_gradient_packs(geom, spec):
    _run(exact_problem(geom, spec))


def test_q8_activation_with_a_residual_is_refused():
    hip, K = _mods()
    p = exact_problem((2, 7, 15), Spec(144, epi="res_alpha_1"))
    N, H, W = p.geom
    pw = K.pack_conv_weight_q8(p.w.cuda().contiguous())
    out = torch.zeros((N, H, W, p.C), dtype=BF16, device="cuda")
    with pytest.raises(hip.HipError):
        K.conv_q8_forward(p.rec.cuda(), pw, p.bias.cuda(), N, H, W, act=hip.ACT_RELU, res=p.res.to(BF16).cuda(), out=out)
    torch.cuda.synchronize()
    assert float(out.float().abs().max()) == 0  # nothing was launched
    # a caller's record buffer is checked like the source: uint8, contiguous, one record per pixel
    rec_b = K.q8_record_bytes(p.C)
    for bad in (torch.zeros((N, H, W, rec_b + 16), dtype=torch.uint8, device="cuda"), torch.zeros((N, H, W - 1, rec_b), dtype=torch.uint8, device="cuda"),
                torch.zeros((N, H, W, rec_b), dtype=torch.int8, device="cuda"), torch.zeros((N, H, W, 2 * rec_b), dtype=torch.uint8, device="cuda")[..., :rec_b]):
        with pytest.raises(hip.HipError):
            K.conv_q8_forward(p.rec.cuda(), pw, p.bias.cuda(), N, H, W, outq=bad)
        assert int(bad.max()) == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# shift probes: one-hot weights, real-valued activations
# ------------------------------------------------------------------------------------------------------------------------------------
PROBE_GEOM = (2, 7, 15)


@functools.lru_cache(maxsize=None)
def probe_activations(C):
    """Seeded normal values times 2^(-6..6) per (pixel, 32-channel block), one all-zero pixel: (records, their dequantised values)."""
    N, H, W = PROBE_GEOM
    g = torch.Generator().manual_seed(4000 + C)
    nb = (C + 31) // 32
    x = torch.randn(N, H, W, C, generator=g) * torch.exp2(torch.randint(-6, 7, (N, H, W, nb), generator=g).float()).repeat_interleave(32, -1)[..., :C]
    x[1, 3, 7] = 0
    rec = Q.records(x)
    xq = Q.dequant(rec, C)
    assert torch.equal(xq.bfloat16().float(), xq)  # an e4m3 value times a power of two is a bf16 number
    assert int((rec[..., :C] & 7).unique().numel()) == 8 and int(rec[..., rec.shape[-1] - 16].unique().numel()) >= 12  # every mantissa, many scales
    return rec, xq


@pytest.mark.parametrize("t", range(9))
@pytest.mark.parametrize("C", CHANNELS)
def test_q8_shift_probes(C, t):
    rec, xq = probe_activations(C)
    w, pi, ptap = CR.one_hot_weight(C, C, t)
    want = CR.shifted_copy(xq, pi, ptap)
    assert torch.equal(CR.conv_ref([xq], w), want.double())  # the probe's reference IS the shifted copy

    def name(idx):
        o = idx[3]
        return _pixel(idx) + f" = the copy of input channel {int(pi[o])} through tap (ky, kx) = ({int(ptap[o]) // 3}, {int(ptap[o]) % 3})"
    p = SimpleNamespace(geom=PROBE_GEOM, C=C, what=f"{PROBE_GEOM} {C}-probe{t}", rec=rec, w=w, dgrad=False, bias=None, res=None, kw={},
                        want_bf16=True, want_q8=True, want=CR.round_bf16(want.double()), want_rec=Q.records(want), name=name)
    _run(p)


# ------------------------------------------------------------------------------------------------------------------------------------
# weight read-back: one-hot activations, real-valued weights
# ------------------------------------------------------------------------------------------------------------------------------------
def readback_weight(C, dgrad):
    """Seeded real-valued (C, C, 3, 3) weight whose scaled channels -- output channels for the forward pack, input channels for the
    data-gradient pack -- each carry 2^(seeded -6..6); one of them is all zero, one has a maximum with mantissa exactly 1.75."""
    g = torch.Generator().manual_seed(5000 + C + (1 if dgrad else 0))
    w = torch.randn(C, C, 3, 3, generator=g) * torch.exp2(torch.randint(-6, 7, (C, 1, 1, 1), generator=g).float())
    w[5] = 0
    w[C - 3] = w[C - 3] / w[C - 3].abs().max() * 0.8125
    w[C - 3, 37, 1, 2] = -1.75
    return w.permute(1, 0, 2, 3).contiguous() if dgrad else w


@pytest.mark.parametrize("dgrad", [False, True], ids=["forward", "transpose_flip"])
@pytest.mark.parametrize("C", CHANNELS)
def test_q8_weight_image_read_back(C, dgrad):
    w = readback_weight(C, dgrad)
    x = Q.impulse_image(C)
    rec = Q.records(x)
    assert torch.equal(Q.dequant(rec, C), x)
    # forward: the scale is per output channel of w (the emulation test_fp8_gpu.py has always used); transpose_flip: per INPUT channel of w,
    # the taps mirrored -- the reference follows dgrad_ref's definition (q8_ref.wquant_ref, q8_ref.impulse_gather)
    wq = Q.wquant_ref(w, True) if dgrad else Q.wquant_emul(w)
    assert not torch.equal(wq, w) and torch.equal(wq.bfloat16().float(), wq)
    want = (CR.dgrad_ref(x, wq) if dgrad else CR.conv_ref([x], wq))
    assert torch.equal(Q.impulse_gather(want, C, dgrad), wq.double())

    def name(idx):
        return _pixel(idx) + " (weight read-back)"
    p = SimpleNamespace(geom=Q.IMPULSE_GEOM, C=C, what=f"weight read-back {C} {'transpose_flip' if dgrad else 'forward'}", rec=rec, w=w, dgrad=dgrad,
                        bias=None, res=None, kw={}, want_bf16=True, want_q8=False, want=None, want_rec=None, name=name)
    got, _ = _run(p)
    gw = Q.impulse_gather(got.float(), C, dgrad)
    n, idx, g_, w_ = WR.first_mismatch(gw, wq)
    assert n == 0, (f"{p.what}: {n} of {gw.numel()} weights differ from the quantised weight, the first at w[{idx[0]}, {idx[1]}, {idx[2]}, {idx[3]}]: "
                    f"read back {g_!r}, want {w_!r} (unquantised {float(w[idx])!r})")
    assert torch.equal(gw, wq)
    _assert_out(got, CR.round_bf16(want), p)  # and nothing anywhere else in the image


# ------------------------------------------------------------------------------------------------------------------------------------
# the quantiser
# ------------------------------------------------------------------------------------------------------------------------------------
def quantiser_values(M, C, seed):
    """Seeded bf16 numbers (M, C) over many octaves (2^(-20..20) per 8 channels), with an all-zero pixel where there are several."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g) * torch.exp2(torch.randint(-20, 21, (M, C // 8), generator=g).float()).repeat_interleave(8, -1)
    if M > 2:
        x[M // 2] = 0
    return x.bfloat16()


def _check_quantiser(x_dev, x_cpu, what):
    _, K = _mods()
    C = x_cpu.shape[-1]
    rec = K.q8_quantize(x_dev)
    torch.cuda.synchronize()
    assert rec.dtype == torch.uint8 and tuple(rec.shape) == tuple(x_cpu.shape[:-1]) + (K.q8_record_bytes(C),)
    got = rec.cpu()
    del rec
    want = Q.records(x_cpu.float())
    n, first = Q.first_byte_mismatch(got, want, C)
    assert n == 0, f"{what}: {n} of {got.numel()} bytes differ from the host's records, the first at {first}"


@pytest.mark.parametrize("M", [1, 1000])
@pytest.mark.parametrize("C", [8, 40, 112, 144, 512])
def test_q8_quantize_bytes(C, M):
    x = quantiser_values(M, C, 6000 + C + M)
    _check_quantiser(x.cuda(), x, f"q8_quantize C={C} M={M}")


@pytest.mark.parametrize("C", [40, 144])
def test_q8_quantize_strided_input(C):
    x = quantiser_values(77, C, 6100 + C)
    v = WR.embed(x, C + 24, 4, device="cuda")  # NaN between the pixels
    assert v.stride(-2) == C + 24 and torch.equal(v.cpu().view(torch.int16), x.view(torch.int16))
    _check_quantiser(v, x, f"q8_quantize C={C} strided")


@pytest.mark.parametrize("C", [8, 40, 144])
def test_q8_quantize_boundary_maxima(C):
    x = Q.boundary_rows(C).bfloat16()
    _check_quantiser(x.cuda(), x, f"q8_quantize C={C} boundary maxima")


def test_q8_quantize_grid_stride_branch():
    """More (pixel, block) items than 8192 workgroups of 256 threads hold: every thread loops."""
    C, M = 8, 8192 * 256 + 777
    g = torch.Generator().manual_seed(6200)
    x = (torch.randn(M, C, generator=g) * torch.exp2(torch.randint(-20, 21, (M, 1), generator=g).float())).bfloat16()
    _check_quantiser(x.cuda(), x, f"q8_quantize C={C} M={M}")


# ------------------------------------------------------------------------------------------------------------------------------------
# the chain entry against the same convolutions issued one by one
# ------------------------------------------------------------------------------------------------------------------------------------
CHAIN_GEOM = (2, 7, 15)


def _bits_equal(a, b, what):
    n, idx, g, w = WR.first_mismatch(a.float().cpu(), b.float().cpu())
    assert n == 0, f"{what}: {n} elements differ from the single launches, the first at {idx}: chain {g!r}, single {w!r}"
    assert torch.equal(a.cpu().view(torch.int16), b.cpu().view(torch.int16)), what + ": other bits than the single launches"


@pytest.mark.parametrize("keep_t", [True, False])
@pytest.mark.parametrize("nblk", [1, 2])
@pytest.mark.parametrize("C", CHANNELS)
def test_q8_chain_entry_equals_the_single_launches(C, nblk, keep_t):
    hip, K = _mods()
    N, H, W = CHAIN_GEOM
    g = torch.Generator().manual_seed(7000 + C + nblk)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    r = 0.1
    y0 = rn(N, H, W, C).to(BF16).cuda()
    pw1 = [K.pack_conv_weight_q8((rn(C, C, 3, 3) / (9 * C) ** 0.5 * 1.4).cuda()) for _ in range(nblk)]
    pw2 = [K.pack_conv_weight_q8((rn(C, C, 3, 3) / (9 * C) ** 0.5).cuda()) for _ in range(nblk)]
    b1, b2 = [(rn(C) * 0.1).cuda() for _ in range(nblk)], [(rn(C) * 0.1).cuda() for _ in range(nblk)]
    # one by one: quantise, conv1 with ReLU writing records, conv2 with the residual writing records for the next block
    y, t = [y0], []
    q = K.q8_quantize(y0)
    for k in range(nblk):
        tk, qb = K.conv_q8_forward(q, pw1[k], b1[k], N, H, W, act=hip.ACT_RELU, want_bf16=keep_t)
        yk, q = K.conv_q8_forward(qb, pw2[k], b2[k], N, H, W, alpha=r, res=y[k], want_q8=k + 1 < nblk)
        t.append(tk)
        y.append(yk)
    ys, ts = K.resblock_chain_forward_q8(y0, pw1, b1, pw2, b2, r, keep_t)
    torch.cuda.synchronize()
    assert len(ys) == nblk + 1 and len(ts) == nblk
    for k in range(nblk + 1):
        assert not bool(torch.isnan(ys[k]).any())
        _bits_equal(ys[k], y[k], f"C={C} ys[{k}]")
    for k in range(nblk):
        if keep_t:
            _bits_equal(ts[k], t[k], f"C={C} ts[{k}]")
            assert float(ts[k].float().abs().max()) > 0
        else:
            assert ts[k] is None and t[k] is None
    assert float((ys[-1].float() - y0.float()).abs().max()) > 0 and float(ys[-1].float().abs().max()) > 0  # (not a comparison of zeros)
