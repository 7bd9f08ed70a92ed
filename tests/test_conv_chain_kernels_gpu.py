"""The two bf16 3x3 kernels under the recurrent residual chains -- conv_ws_kernel<NCT> (route hip.CONV_WS) and conv_ksplit_kernel<bf16, 3, NTB>
(route hip.CONV_KSPLIT) of csrc/conv_igemm.hip -- and the chain entries vmg_resblock_chain_fwd / _bwd, element by element against the fp64
reference of tests/conv_ref.py.

Exactness invariant.  Operands, bias and residual are k * 2^-s with small integer k (wgrad_ref.FAMILIES), alpha and the slopes powers of
two, and conv_ref.assert_exact has checked BEFORE the launch that kmax^2 * 9 * Ci_total plus the bias and residual terms on the finest
grid stays below 2^24: every partial sum in any order and every epilogue intermediate is then an fp32 number, the only rounding is the
final one to bf16, and the output must EQUAL round_bf16(reference) (torch.equal; the first differing element is named).  One wrong tap
at a tile edge, a halo row of the neighbouring image, alpha applied behind the residual, a mask that takes 0 for positive or a
remainder k-step that reads another chunk changes it.  The shift probes (a one-hot weight per output channel: the output is a shifted
copy of one input channel) are exact for ANY bf16 input and name the tap and the channel.

Every source, res, aux, out and out_pre is a view inside a NaN-filled allocation (wgrad_ref.embed) with a pixel stride larger than the
channel count: a read outside the image that is not replaced by zero poisons the result, a write outside the view shows in the
allocation, and both are checked together with a second launch that must give the same bits.  Neither route falls back (vmg_conv_fwd
refuses what the kernel asked for does not cover), so the pack's layout / cout_tiles and the `deep` argument decide the kernel.

Real-valued operands (seeded normal values, the chain's own alpha = slope = 0.1) are held to the per-element bound of conv_ref.real_bound:
with v the fp64 result from the bf16-rounded operands and S = sum |x||w| + |b| + |res|, e32 = 2 * (9 * Ci_total + 4) * 2^-24 * S is the
any-order fp32 summation bound (doubled: the matrix unit's adder may truncate) and |got - v| <= 2^-8 * (|v| + e32) + e32.
Measured on an MI355X: the worst |got - v| / bound over the 24 real-valued cases is 0.82 (112 -> 112 with alpha 0.1 and a residual on
(1, 24, 81), the same element and the same figure on both routes; 0.24 .. 0.78 elsewhere) -- each case prints its own.

Ring slots of the weight-streaming kernel (launch_ws: 4 where halo + 4 stages + bias fit 160 KiB, else 3; cout_tiles = 3 always 3):
ring 3 is reached by 320 -> 144 (160-channel blocks) and by every cout_tiles = 3 case, ring 4 by all the others
(test_ws_case_table_reaches_both_ring_sizes computes it from the same formula)."""
import copy
import functools
from typing import NamedTuple, Tuple

import numpy as np
import pytest
import torch

from tests import conv_ref as CR
from tests import wgrad_ref as WR

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
WS, KSPLIT = "ws", "ksplit"

# (N, H, W): the smallest geometries at which the tiling can go wrong (WS tiles are 8 x 16 pixels, K-split tiles 4 x 16)
GEOMS = [(1, 1, 1),     # the image lies inside the halo
         (1, 8, 16),    # one WS tile
         (1, 9, 17),    # one pixel into the next tile both ways
         (2, 7, 15),    # ragged tile; the halo must not read the other image
         (3, 5, 33), (1, 17, 3),
         (2, 16, 32),   # 8 WS tiles / 16 K-split tiles: the xcd_remap branch
         (1, 24, 81)]   # 18 WS tiles, ragged W: >= the largest stage count of a source block (15), so every bid % stages and bid % NCT occurs; no multiple of 8
RAGGED = [(2, 7, 15), (3, 5, 33), (1, 17, 3)]  # every channel case but 144 -> 144 runs on these three only
EPI_GEOMS = [(2, 7, 15), (3, 5, 33)]

# name -> the epilogue of vmg_conv_fwd.  `dgrad`: the pack is a data-gradient pack (transpose_flip) and the reference conv_ref.dgrad_ref
EPILOGUES = {
    "plain": dict(bias=False),
    "bias": dict(),
    "bias_relu": dict(act=CR.ACT_RELU),
    "bias_lrelu_0.25": dict(act=CR.ACT_LRELU, slope=0.25),
    "conv0_lrelu_0.1": dict(act=CR.ACT_LRELU, slope=0.1),                       # the chain's conv0: one rounding of v * float32(0.1), then bf16
    "res_alpha_0.125": dict(alpha=0.125, res=True),                             # the chain's conv2 with a power of two for r_scaling
    "want_pre": dict(act=CR.ACT_RELU, alpha=0.5, res=True, want_pre=True),
    "gelu_pre_only": dict(act=CR.ACT_GELU, want_pre=True),                      # GELU itself stays with the tolerance tests: out_pre only
    "dgrad_plain": dict(bias=False, dgrad=True),
    "dgrad_res": dict(bias=False, dgrad=True, res=True),                        # the chain's g_y = g_y' + dgrad1(g_t)
    "dgrad_mask1": dict(bias=False, dgrad=True, alpha=0.125, actgrad=1),        # the chain's g_t = r * dgrad2(g_y') * relu'(t)
    "dgrad_mask1_res": dict(bias=False, dgrad=True, alpha=0.125, actgrad=1, res=True),
    "dgrad_mask2": dict(bias=False, dgrad=True, alpha=0.5, slope=0.25, actgrad=2, res=True),
}


EXACT_EPILOGUES = [n for n in EPILOGUES if n not in ("plain", "bias")]  # (those two come with the channel cases and the probes)


class Spec(NamedTuple):
    """One convolution.  Forward: sources of src_ch channels -> co output channels; the weight has o_total outputs (the pack takes [o0, o0 + co))
    and i_total inputs per group (source s meets [src_off[s], + src_ch[s]) and IS that channel slice of an i_total-wide tensor).
    Data gradient (the epilogue says so): src_ch = (K,) channels of dy, co = input channels of the weight (K, co, 3, 3)."""
    src_ch: Tuple[int, ...]
    co: int
    tiles: int
    epi: str = "bias"
    family: str = "small"
    o_total: int = 0
    o0: int = 0
    i_total: int = 0
    src_off: Tuple[int, ...] = ()
    groups: int = 1
    probe: int = -1  # 0..8: shift probe (one-hot weight, full-mantissa input)

    @property
    def id(self):
        s = "+".join(map(str, self.src_ch)) + f"to{self.co}-t{self.tiles}-{self.epi}"
        s += "" if self.family == "small" else "-" + self.family
        s += f"-o{self.o0}of{self.o_total}" if self.o_total else ""
        s += f"-i{self.src_off[0]}of{self.i_total}" if self.i_total else ""
        s += f"-g{self.groups}" if self.groups > 1 else ""
        return s + (f"-probe{self.probe}" if self.probe >= 0 else "")


# ---- weight-streaming channel cases: (sources, Cout, the tile count ws_eligible must state)
WS_CHANNELS = [
    ((144,), 144, 9), ((112,), 112, 7),
    ((144, 144), 144, 9), ((112, 112), 112, 7),   # the chain's conv0: the halo tile is restaged between the sources
    ((144,), 288, 9),                             # two cout blocks
    ((144,), 256, 8), ((64,), 128, 8),
    ((32,), 144, 9),                              # exactly 3 stages, no remainder k-steps
    ((16,), 144, 9),                              # 2 stages, remainder k-steps only
    ((320,), 144, 9),                             # two 160-channel blocks (ring 3)
    ((448,), 112, 7),                             # four 112-channel blocks
]
WS_SPECS = []
for _src, _co, _t in WS_CHANNELS:
    WS_SPECS.append(Spec(_src, _co, _t))
    if _co % 48 == 0:
        WS_SPECS.append(Spec(_src, _co, 3))       # the 48-channel-block instance (three ring slots, several workgroups per CU)
WS_SPECS += [
    Spec((16,), 144, 9, family="full"), Spec((16,), 144, 3, family="full"),
    Spec((144,), 144, 9, o_total=200, o0=40),                    # an output slice of a wider weight
    Spec((144,), 144, 9, i_total=176, src_off=(16,)),            # a channel slice of a wider tensor, a K slice of a wider weight
    Spec((144,), 144, 9, groups=4),                              # the dense block-diagonal pack of a grouped convolution
]
# ---- K-split channel cases
KS_SPECS = [
    Spec((144,), 144, 3), Spec((144, 144), 144, 3), Spec((112,), 112, 4),
    Spec((144,), 144, 5),                                        # partial last cout block
    Spec((144,), 144, 1),
    Spec((8,), 144, 3), Spec((24,), 16, 1), Spec((64,), 112, 4),  # 9 / 9 / 18 k-steps on four waves: uneven quarters, padding steps
    Spec((64,), 3, 1),                                           # Cout = 3: the element-wise (non-vec8) epilogue
]
FULL_GEOM_SPECS = {WS: [Spec((144,), 144, 9), Spec((144,), 144, 3)], KSPLIT: [Spec((144,), 144, 3)]}


def _epi_specs(route):
    t144, t112 = (9, 7) if route == WS else (3, 4)
    out = []
    for name in EXACT_EPILOGUES:
        out += [(g, Spec((144,), 144, t144, epi=name)) for g in EPI_GEOMS] + [(EPI_GEOMS[0], Spec((112,), 112, t112, epi=name))]
    # a data gradient whose weight is not square: dy of 112 channels -> dx of 144 (a transposition that mixes up O and I shows)
    out += [(g, Spec((112,), 144, t144, epi="dgrad_mask1_res")) for g in EPI_GEOMS]
    return out


def _channel_cases(route):
    specs = WS_SPECS if route == WS else KS_SPECS
    full = FULL_GEOM_SPECS[route]
    return [(g, s) for s in full for g in GEOMS] + [(g, s) for s in specs if s not in full for g in RAGGED]


PROBE_GEOM = (2, 7, 15)


def _probe_cases(route):
    t = 9 if route == WS else 3
    return [(PROBE_GEOM, Spec(src, 144, t, epi="plain", probe=p)) for src in ((144,), (144, 144)) for p in range(9)]


def exact_cases():
    """Every (route, geometry, spec) of the exact tests: tests/test_conv_ref.py checks conv_ref.assert_exact on each without a GPU."""
    return [(r, g, s) for r in (WS, KSPLIT) for g, s in _channel_cases(r) + _epi_specs(r) + _probe_cases(r)]


def exact_args(spec):
    """The arguments of conv_ref.assert_exact for a spec."""
    e = EPILOGUES[spec.epi]
    scales = [e["slope"]] if e.get("act") == CR.ACT_LRELU else []
    scales.append(e.get("alpha", 1.0))
    if e.get("actgrad") == 2:
        scales.append(e["slope"])
    return spec.family, sum(spec.src_ch), e.get("bias", True), e.get("res", False), tuple(scales)


def _blocks(c):
    """expand_sources of conv_igemm.hip: equal channel blocks of at most 160 channels, each a multiple of 8."""
    parts = 1
    while c // parts > 160 or c % (8 * parts):
        parts += 1
    return [c // parts] * parts


def ws_ring(spec):
    """launch_ws's choice of ring slots."""
    nct = spec.tiles
    halo = (max(10 * 18 * b * 2 for c in spec.src_ch for b in _blocks(c)) + 1023) // 1024 * 1024
    stg, cob = 3 * nct * 16 * 64, nct * 16
    return 3 if nct <= 3 else (4 if halo + 4 * stg + cob * 4 <= 160 * 1024 else 3)


def _mods():
    from vmg_amd import hip, kernels as K
    return hip, K


def _seed(geom, spec):
    return (geom[0] * 7919 + geom[1] * 104729 + geom[2] * 1299709 + sum(spec.src_ch) * 31 + spec.co * 17 + len(spec.src_ch)) % (2 ** 31 - 1)


def _values(shape, seed, family):
    """Operand values: the exact families, or ("real") seeded normal values that are bf16 numbers."""
    if family == "real":
        return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)).bfloat16().float()
    return WR.exact_values(shape, seed, family)


@functools.lru_cache(maxsize=24)
def _operands(geom, src_ch, co, family, o_total, o0, i_total, src_off, groups, dgrad, probe):
    """The CPU side that the epilogues of a (geometry, channel case) share: sources (wide, where the source is a slice), weight, the fp64 sums
    and, for real-valued cases, the sums of the magnitudes."""
    N, H, W = geom
    seed = _seed(geom, Spec(src_ch, co, 0))
    ci = sum(src_ch)
    wide = [_values((N, H, W, i_total or c), seed + 11 * s, "real" if probe >= 0 else family) for s, c in enumerate(src_ch)]
    off = src_off[0] if i_total else 0
    srcs = [t[..., off:off + c] if i_total else t for t, c in zip(wide, src_ch)]
    if dgrad:
        assert len(src_ch) == 1 and not (o_total or i_total or groups > 1 or probe >= 0)
        w = _values((ci, co, 3, 3), seed + 101, family)
        if family == "real":
            w = (w / (9 * ci) ** 0.5).bfloat16().float()
        acc = CR.dgrad_ref(srcs[0], w)
        mag = CR.dgrad_ref(srcs[0].abs(), w.abs()) if family == "real" else None
        return wide, srcs, w, acc, mag
    if probe >= 0:
        w, pi, ptap = CR.one_hot_weight(co, ci, probe)
        x = torch.cat(srcs, -1)
        acc = CR.conv_ref(srcs, w)
        assert torch.equal(acc, CR.shifted_copy(x, pi, ptap).double())  # the probe's reference IS the shifted copy
        return wide, srcs, w, acc, None
    w = _values((o_total or co, (i_total or ci) // groups, 3, 3), seed + 101, family)
    if family == "real":
        w = (w / (9 * ci) ** 0.5).bfloat16().float()
    kw = dict(src_off=list(src_off) if i_total else None, o0=o0, on=co, groups=groups)
    acc = CR.conv_ref(srcs, w, **kw)
    mag = CR.conv_ref([s.abs() for s in srcs], w.abs(), **kw) if family == "real" else None
    return wide, srcs, w, acc, mag


class _Problem:
    """One convolution with its epilogue: CPU operands, the expected bf16 results (exact) or fp64 value and bound (real-valued)."""

    def __init__(self, geom, spec):
        N, H, W = geom
        e = dict(EPILOGUES[spec.epi])
        self.geom, self.spec, self.e = geom, spec, e
        self.real = spec.family == "real"
        self.dgrad = e.pop("dgrad", False)
        self.want_pre = e.pop("want_pre", False)
        if not self.real:
            CR.assert_exact(*exact_args(spec))  # the invariant, before anything runs on the GPU
        self.wide, self.srcs, self.w, acc, mag = _operands(geom, spec.src_ch, spec.co, spec.family, spec.o_total, spec.o0, spec.i_total, spec.src_off,
                                                           spec.groups, self.dgrad, spec.probe)
        seed = _seed(geom, spec) + 1000
        shape = (N, H, W, spec.co)
        self.bias = (_values((spec.co,), seed + 1, spec.family) * (0.1 if self.real else 1.0)) if e.pop("bias", True) else None
        self.res = _values(shape, seed + 2, spec.family) if e.pop("res", False) else None
        self.aux = None
        if e.get("actgrad"):
            aux = _values(shape, seed + 3, spec.family)
            flat = aux.reshape(-1)
            flat[0::7] = -0.0  # neither zero is positive
            flat[3::11] = 0.0
            assert bool((flat < 0).any()) and bool((flat > 0).any()) and bool(torch.signbit(flat[flat == 0]).any()) and \
                not bool(torch.signbit(flat[flat == 0]).all())
            self.aux = aux
        self.kw = e  # act, slope, alpha, actgrad: as vmg_conv_fwd takes them
        out, pre = CR.epilogue_ref(acc, self.bias, aux=self.aux, res=self.res, exact=not self.real, **e)
        self.want, self.want_pre_value = out, pre
        if self.real:
            S = mag + (self.bias.abs().double() if self.bias is not None else 0) + (self.res.abs().double() if self.res is not None else 0)
            self.bound = CR.real_bound(out, S, sum(spec.src_ch))


def _outside_mask(view):
    C, ps = view.shape[-1], view.stride(-2)
    M = view.numel() // C
    mask = torch.ones(view._base.numel(), dtype=torch.bool)
    idx = (view.storage_offset() + torch.arange(M)[:, None] * ps + torch.arange(C)[None, :]).reshape(-1)
    mask[idx] = False
    return mask


def _name(idx, spec):
    n, y, x, o = idx
    s = f"image {n}, pixel ({y}, {x}), output channel {o}"
    if spec.probe >= 0:
        _, pi, ptap = CR.one_hot_weight(spec.co, sum(spec.src_ch), spec.probe)
        s += f" = the copy of input channel {int(pi[o])} through tap (ky, kx) = ({int(ptap[o]) // 3}, {int(ptap[o]) % 3})"
    return s


def _assert_same(got, want, what, spec):
    nan = torch.isnan(got)
    if bool(nan.any()):
        first = tuple(int(v) for v in torch.nonzero(nan)[0])
        raise AssertionError(f"{what}: {int(nan.sum())} of {got.numel()} elements are NaN, the first at {_name(first, spec)}: something outside the "
                             "operands was read, or the element was never written")
    n, idx, g, w = WR.first_mismatch(got, want)
    if n:
        err, top = float((got.double() - want.double()).abs().max()), float(want.double().abs().max())
        raise AssertionError(f"{what}: {n} of {got.numel()} elements differ from the fp64 reference, the first at {_name(idx, spec)}: got {g!r}, want "
                             f"{w!r} (largest error {err:g}; 2e-2 of the largest value: {2e-2 * max(1.0, top):g})")
    assert torch.equal(got, want), what


def _launch(route, prob):
    """Pack, embed, launch twice.  Returns (out, out_pre or None) as CPU tensors after the checks every case shares: no NaN left inside, nothing
    changed outside the views, the same bits from the second launch."""
    hip, K = _mods()
    assert (hip.ACT_NONE, hip.ACT_RELU, hip.ACT_LRELU, hip.ACT_GELU) == (CR.ACT_NONE, CR.ACT_RELU, CR.ACT_LRELU, CR.ACT_GELU)
    spec, (N, H, W) = prob.spec, prob.geom
    what = f"{route} {prob.geom} {spec.id}"
    guard = 10 * W + 32  # pixels: more than a tile with its halo could reach past either end of the image
    dev = "cuda"
    srcs = []
    for s, (t, c) in enumerate(zip(prob.wide, spec.src_ch)):
        v = WR.embed(t.to(BF16), t.shape[-1] + 8 + 16 * (s % 2), guard, device=dev)
        assert torch.equal(v.float().cpu(), t)  # the values are bf16 numbers
        srcs.append(v[..., spec.src_off[0]:spec.src_off[0] + c] if spec.i_total else v)
    w = prob.w.to(dev).contiguous()
    assert torch.equal(w.bfloat16().float(), w)
    common = dict(src_ch=list(spec.src_ch), src_off=list(spec.src_off) if spec.i_total else None, o0=spec.o0, on=spec.co, transpose_flip=prob.dgrad,
                  cout_tiles=spec.tiles, groups=spec.groups)
    if route == WS:
        if spec.tiles != 3:
            assert K.ws_eligible(spec.co, 3, BF16, list(spec.src_ch)) == spec.tiles
        pw = K.pack_conv_weight_ws(w, **common)
        assert pw.layout == "ws"
        deep = hip.CONV_WS
    else:
        pw = K.pack_conv_weight(w, BF16, **common)
        assert pw.layout == "std"
        deep = hip.CONV_KSPLIT
    assert pw.cout_tiles == spec.tiles and pw.cout == spec.co and pw.src_ch == list(spec.src_ch)
    c8 = (spec.co + 7) // 8 * 8
    emb = lambda t, ps: WR.embed(t.to(BF16), ps, guard, device=dev)  # noqa: E731
    res = emb(prob.res, c8 + 16) if prob.res is not None else None
    aux = emb(prob.aux, c8 + 24) if prob.aux is not None else None
    blank = torch.full((N, H, W, spec.co), float("nan"), dtype=BF16)
    outs = [emb(blank, c8 + 8)] + ([emb(blank, c8 + 8)] if prob.want_pre else [])
    before = [o._base.clone() for o in outs]
    bias = prob.bias.to(dev) if prob.bias is not None else None
    runs = []
    for _ in range(2):
        for o, b in zip(outs, before):
            o._base.copy_(b)
        K.conv_forward(srcs, pw, bias, N, H, W, res=res, aux=aux, out=outs[0], out_pre=outs[1] if prob.want_pre else None, deep=deep, **prob.kw)
        torch.cuda.synchronize()
        runs.append([o._base.cpu() for o in outs])
    for k, (o, b) in enumerate(zip(outs, before)):
        name = what + (": out", ": out_pre")[k]
        full, again = runs[0][k], runs[1][k]
        assert torch.equal(full.view(torch.int16), again.view(torch.int16)), name + ": the second launch gave other bits"
        mask = _outside_mask(o)
        assert torch.equal(full.view(torch.int16)[mask], b.cpu().view(torch.int16)[mask]), name + ": the allocation changed outside the view"
        if spec.co % 8 == 0:
            assert bool(torch.isnan(full[mask]).all()), name + ": not every element outside the view is NaN"
    got = [o.cpu() for o in outs]
    for k, g in enumerate(got):
        nan = torch.isnan(g)
        if bool(nan.any()):
            first = tuple(int(v) for v in torch.nonzero(nan)[0])
            raise AssertionError(f"{what}{(': out', ': out_pre')[k]}: {int(nan.sum())} of {g.numel()} elements are NaN, the first at {_name(first, spec)}")
    return got[0], (got[1] if prob.want_pre else None)


@functools.lru_cache(maxsize=8)
def _problem(geom, spec):
    return _Problem(geom, spec)


def _run_exact(route, geom, spec):
    prob = _problem(geom, spec._replace(tiles=0))  # (the expected values do not depend on the tiling: both routes share them)
    prob = _with_spec(prob, spec)
    out, pre = _launch(route, prob)
    what = f"{route} {geom} {spec.id}"
    if prob.want_pre:
        _assert_same(pre, prob.want_pre_value, what + ": out_pre", spec)
    if prob.want is not None:
        _assert_same(out, prob.want, what + ": out", spec)


def _with_spec(prob, spec):
    p = copy.copy(prob)
    p.spec = spec
    return p


def _ids(cases):
    return ["x".join(map(str, g)) + "-" + s.id for g, s in cases]


# ------------------------------------------------------------------------------------------------------------------------------------
# exact cases
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,spec", _channel_cases(WS), ids=_ids(_channel_cases(WS)))
def test_ws_geometries_and_channel_cases(geom, spec):
    _run_exact(WS, geom, spec)


@pytest.mark.parametrize("geom,spec", _channel_cases(KSPLIT), ids=_ids(_channel_cases(KSPLIT)))
def test_ksplit_geometries_and_channel_cases(geom, spec):
    _run_exact(KSPLIT, geom, spec)


@pytest.mark.parametrize("geom,spec", _epi_specs(WS), ids=_ids(_epi_specs(WS)))
def test_ws_epilogues(geom, spec):
    _run_exact(WS, geom, spec)


@pytest.mark.parametrize("geom,spec", _epi_specs(KSPLIT), ids=_ids(_epi_specs(KSPLIT)))
def test_ksplit_epilogues(geom, spec):
    _run_exact(KSPLIT, geom, spec)


@pytest.mark.parametrize("geom,spec", _probe_cases(WS), ids=_ids(_probe_cases(WS)))
def test_ws_shift_probes(geom, spec):
    _run_exact(WS, geom, spec)


@pytest.mark.parametrize("geom,spec", _probe_cases(KSPLIT), ids=_ids(_probe_cases(KSPLIT)))
def test_ksplit_shift_probes(geom, spec):
    _run_exact(KSPLIT, geom, spec)


def test_ws_case_table_reaches_both_ring_sizes():
    rings = {s.id: ws_ring(s) for s in WS_SPECS}
    assert set(rings.values()) == {3, 4}
    assert rings[Spec((320,), 144, 9).id] == 3 and rings[Spec((144,), 144, 9).id] == 4 and rings[Spec((448,), 112, 7).id] == 4
    assert all(r == 3 for i, r in rings.items() if "-t3-" in i)
    assert all(r == 4 for i, r in rings.items() if "-t3-" not in i and not i.startswith("320"))


# ------------------------------------------------------------------------------------------------------------------------------------
# real-valued cases: the per-element bound
# ------------------------------------------------------------------------------------------------------------------------------------
REAL_GEOMS = [(2, 7, 15), (1, 24, 81)]
REAL_EPILOGUES = {
    "real_conv0": dict(act=CR.ACT_LRELU, slope=0.1),
    "real_conv2": dict(alpha=0.1, res=True),
    "real_dgrad2": dict(bias=False, dgrad=True, alpha=0.1, actgrad=1),
    "real_dgrad0": dict(bias=False, dgrad=True),
}
EPILOGUES.update(REAL_EPILOGUES)


def _real_cases(route):
    t144, t112 = (9, 7) if route == WS else (3, 4)
    out = []
    for g in REAL_GEOMS:
        out += [(g, Spec((144,), 144, t144, epi="real_conv2", family="real")), (g, Spec((112,), 112, t112, epi="real_conv2", family="real")),
                (g, Spec((144, 144), 144, t144, epi="real_conv0", family="real")),
                (g, Spec((144,), 144, t144, epi="real_dgrad2", family="real")), (g, Spec((112,), 112, t112, epi="real_dgrad2", family="real")),
                (g, Spec((144,), 288, t144, epi="real_dgrad0", family="real"))]  # conv0's data gradient: dy of 144 channels -> both sources
    return out


def _run_real(route, geom, spec):
    prob = _with_spec(_problem(geom, spec._replace(tiles=0)), spec)
    out, _ = _launch(route, prob)
    err = (out.double() - prob.want).abs()
    ratio = torch.where(prob.bound > 0, err / prob.bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max())
    i = int(ratio.reshape(-1).argmax())
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))
    print(f"bound ratio {route} {geom} {spec.id}: {worst:.4f} at {idx}")
    assert worst <= 1.0, (f"{route} {geom} {spec.id}: |got - v| = {float(err[idx]):g} at {_name(idx, spec)} is {worst:.3f} of the bound "
                          f"{float(prob.bound[idx]):g} (got {float(out[idx])!r}, v = {float(prob.want[idx])!r})")


@pytest.mark.parametrize("geom,spec", _real_cases(WS), ids=_ids(_real_cases(WS)))
def test_ws_real_values_within_the_per_element_bound(geom, spec):
    _run_real(WS, geom, spec)


@pytest.mark.parametrize("geom,spec", _real_cases(KSPLIT), ids=_ids(_real_cases(KSPLIT)))
def test_ksplit_real_values_within_the_per_element_bound(geom, spec):
    _run_real(KSPLIT, geom, spec)


# ------------------------------------------------------------------------------------------------------------------------------------
# the chain entries against the same convolutions issued one by one
# ------------------------------------------------------------------------------------------------------------------------------------
CHAIN_GEOM = (2, 7, 15)


def _chain_setup(route, C, seed):
    """Seeded normal operands of a chain with two blocks, sources [C, C], and the packs of both directions for the route."""
    hip, K = _mods()
    N, H, W = CHAIN_GEOM
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    tiles = ({144: 9, 112: 7} if route == WS else {144: 3, 112: 4})[C]
    deep = hip.CONV_WS if route == WS else hip.CONV_KSPLIT

    def pack(w, **kw):
        w = w.cuda().contiguous()
        p = K.pack_conv_weight_ws(w, cout_tiles=tiles, **kw) if route == WS else K.pack_conv_weight(w, BF16, cout_tiles=tiles, **kw)
        assert p.layout == ("ws" if route == WS else "std") and p.cout_tiles == tiles
        return p
    srcs = [WR.embed(rn(N, H, W, C).to(BF16), C + 8 + 16 * s, 10 * W + 32, device="cuda") for s in range(2)]
    w0 = rn(C, 2 * C, 3, 3) / (18 * C) ** 0.5
    w1 = [rn(C, C, 3, 3) / (9 * C) ** 0.5 * 1.4 for _ in range(2)]
    w2 = [rn(C, C, 3, 3) / (9 * C) ** 0.5 for _ in range(2)]
    ch = dict(pw0=pack(w0, src_ch=[C, C]), b0=(rn(C) * 0.1).cuda(), pw1=[pack(w) for w in w1], b1=[(rn(C) * 0.1).cuda() for _ in range(2)],
              pw2=[pack(w) for w in w2], b2=[(rn(C) * 0.1).cuda() for _ in range(2)], pd1=[pack(w, transpose_flip=True) for w in w1],
              pd2=[pack(w, transpose_flip=True) for w in w2], g=rn(N, H, W, C).to(BF16).cuda())
    return srcs, ch, deep


def _bits_equal(a, b, what):
    n, idx, g, w = WR.first_mismatch(a.float().cpu(), b.float().cpu())
    assert n == 0, f"{what}: {n} elements differ from the single launch, the first at {idx}: chain {g!r}, single {w!r}"
    assert torch.equal(a.cpu().view(torch.int16), b.cpu().view(torch.int16)), what + ": other bits than the single launch"


@pytest.mark.parametrize("r_scaling", [0.1, 0.125])
@pytest.mark.parametrize("C", [144, 112])
@pytest.mark.parametrize("route", [WS, KSPLIT])
def test_chain_entries_equal_the_single_launches(route, C, r_scaling):
    hip, K = _mods()
    N, H, W = CHAIN_GEOM
    srcs, ch, deep = _chain_setup(route, C, 5 * C + (1 if route == WS else 2))
    slope0 = 0.1
    # forward, one launch per convolution
    y = [K.conv_forward(srcs, ch["pw0"], ch["b0"], N, H, W, act=hip.ACT_LRELU, slope=slope0, deep=deep)[0]]
    t = []
    for k in range(2):
        t.append(K.conv_forward([y[k]], ch["pw1"][k], ch["b1"][k], N, H, W, act=hip.ACT_RELU, deep=deep)[0])
        y.append(K.conv_forward([t[k]], ch["pw2"][k], ch["b2"][k], N, H, W, alpha=r_scaling, res=y[k], deep=deep)[0])
    before = dict(K.CHAIN_STATS["fwd"])
    ys, ts = K.resblock_chain_forward(srcs, ch["pw0"], ch["b0"], slope0, deep, ch["pw1"], ch["b1"], ch["pw2"], ch["b2"], r_scaling, deep)
    assert K.CHAIN_STATS["fwd"].get(deep, 0) == before.get(deep, 0) + 1
    assert {r: c for r, c in K.CHAIN_STATS["fwd"].items() if r != deep} == {r: c for r, c in before.items() if r != deep}
    assert len(ys) == 3 and len(ts) == 2
    for k in range(3):
        assert not bool(torch.isnan(ys[k]).any())
        _bits_equal(ys[k], y[k], f"{route} C={C} ys[{k}]")
    for k in range(2):
        _bits_equal(ts[k], t[k], f"{route} C={C} ts[{k}]")
    ys2, _ = K.resblock_chain_forward(srcs, ch["pw0"], ch["b0"], slope0, deep, ch["pw1"], ch["b1"], ch["pw2"], ch["b2"], r_scaling, deep, own_output=True)
    _bits_equal(ys2[-1], y[-1], f"{route} C={C} own_output")
    assert ys2[-1].data_ptr() != ys[-1].data_ptr() and ys2[-1].is_contiguous()
    # backward: per block g_t[k] = r * dgrad2(g_y[k+1]) * relu'(t_k), g_y[k] = g_y[k+1] + dgrad1(g_t[k])
    gy, gt = [None, None, ch["g"]], [None, None]
    for k in (1, 0):
        gt[k] = K.conv_forward([gy[k + 1]], ch["pd2"][k], None, N, H, W, alpha=r_scaling, aux=t[k], actgrad=1, deep=deep)[0]
        gy[k] = K.conv_forward([gt[k]], ch["pd1"][k], None, N, H, W, res=gy[k + 1], deep=deep)[0]
    before = dict(K.CHAIN_STATS["bwd"])
    gys, gts = K.resblock_chain_backward(ch["g"], ts, ch["pd1"], ch["pd2"], r_scaling, deep)
    assert K.CHAIN_STATS["bwd"].get(deep, 0) == before.get(deep, 0) + 1
    assert len(gys) == 3 and len(gts) == 2
    for k in range(3):
        assert not bool(torch.isnan(gys[k]).any())
        _bits_equal(gys[k], gy[k], f"{route} C={C} g_ys[{k}]")
    for k in range(2):
        _bits_equal(gts[k], gt[k], f"{route} C={C} g_ts[{k}]")
    assert float(gys[0].float().abs().max()) > 0 and float(ts[1].float().abs().max()) > 0  # (not a comparison of zeros)
