"""The 1x1 kernels of csrc/conv_igemm.hip -- vmg_conv_fwd with ks = 1, every nn.Linear and 1x1 conv on the path and their data gradients --
element by element against the fp64 reference of tests/conv_ref.py (linear_ref, dlinear_ref), one case table for all 28 template instances:

    conv_igemm_kernel<bf16, 1, MT, NTB>  MT 1, 2;  NTB 1, 3, 4, 5, 7, 8, 9      (IG, "bf16", MT, NTB)
    conv_igemm_kernel<float, 1, 1, NTB>            NTB 1, 3, 4, 5, 7, 8, 9      (IG, "f32", 1, NTB)
    conv_ksplit_kernel<bf16, 1, NTB>               NTB 1, 3, 4, 5               (KSP, NTB)
    linear_wres_kernel<3>, <5>, <3, 2>                                          (WRES, NTB, NS)

Which kernel a case runs.  hip.CONV_LINEAR_WRES is a hint: a call it does not cover runs the general kernel without a word.  Every case
therefore NAMES the instance it is meant for (Case.kernel), kernels.conv_forward_plan must report that very instance before each launch, and
tests/test_conv_plan.py asserts the same for the whole table without a GPU (and that the table reaches all 28 instances).  A case that
asks for the wave-autonomous kernel and is meant to fall back says so (Case.hint = "wres" with a general-kernel instance): it tests the fallback.

Exactness invariant.  Operands, bias and residual are k * 2^-s (wgrad_ref.FAMILIES), alpha and the slopes powers of two, and
conv_ref.assert_exact(..., taps=1) has checked BEFORE the launch that every partial sum in any order and every epilogue intermediate is an
fp32 number.  With one tap the full-mantissa family "full" (k up to 255, s = 7) is exact up to 256 input channels
(255^2 * 256 + 255 * 2^7 * 2 < 2^24), so 144- and 160-channel sources run with every mantissa bit in use; wider sources use "small".  The
output must EQUAL round_bf16(reference) -- the fp64 value itself for the fp32 kernels -- and a failure names the first differing element.
The permutation probes (one-hot weights: output channel o is a copy of input channel (7 o + 31 t) % I) are exact for any input.

Every source, res, aux, out and out_pre is a view inside a NaN-filled allocation (wgrad_ref.embed) with a pixel stride larger than the channel
count and a guard of 80 rows; every case launches twice: no NaN inside, nothing changed outside, the same bits again.

Real-valued cases (seeded normal values, alpha = 0.1, a residual) are held to conv_ref.real_bound(..., taps=1); each prints its worst
|got - v| / bound.  Measured on an MI355X: the largest is 0.965 (144 -> 288, the same element and figure on every bf16 kernel: the bf16 rounding of a value just
above a power of two, half an ulp = 2^-8 of it; 0.929 .. 0.959 on the other shapes); the fp32 kernels reach 0.0014.

GELU and its gradient have no exact form.  The device functions are measured through the fp32 general kernel (identity weight 8 -> 8: act =
GELU returns gelu_erf(x), a source of ones with actgrad = 3 returns gelu_erf_grad(aux)) over 65 536 values of [-12, 12], +-0, +-2^-126, +-30 and
the 2 048 fp32 values nearest sqrt(2) and -sqrt(2), against conv_ref.gelu_ref / gelu_grad_ref.  Measured on an MI355X (ROCm 7): worst absolute
error 4.465e-7 (GELU, at x = 5.0748: one fp32 ulp of the result; 2.9e-7 over |x| <= 4, 1.6e-7 beside sqrt(2)) and 1.359e-7 (gradient, at
x = 1.6016); the asserted constants are twice that rounded up to one digit, EG = 9e-7 and EGRAD = 3e-7 (erff and __expf change with the
compiler release).  The bf16 cases then hold |got - gelu(v) * alpha| <= 2^-8 (|g| + E) + E with
E = alpha * (1.13 * e32 + EG) (1.13 bounds sup |gelu'| = 1.129), and the masked gradient with E = alpha * (1.13 * e32 + |v| * EGRAD).
Measured: 0.966 of the bound forward, 0.959 on the masked gradient, 0.976 on the forward's out_pre under real_bound -- the largest ratio
of the module; the same elements and figures on all five bf16 kernels.

Every case passes on an MI355X (630 cases + the two measurements, about 4.3 s)."""
import copy
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np
import pytest
import torch

from tests import conv_ref as CR
from tests import wgrad_ref as WR

pytestmark = pytest.mark.gpu

IG, KSP, WRES = "igemm", "ksplit", "wres"
NTBS = (1, 3, 4, 5, 7, 8, 9)
INSTANCES = ([(IG, "bf16", mt, n) for mt in (1, 2) for n in NTBS] + [(IG, "f32", 1, n) for n in NTBS] + [(KSP, n) for n in (1, 3, 4, 5)] +
             [(WRES, 3, 1), (WRES, 5, 1), (WRES, 3, 2)])
assert len(INSTANCES) == 28
GUARD = 80  # rows of NaN before and after every view
EG, EGRAD = 9e-7, 3e-7  # absolute error of the device's gelu_erf / gelu_erf_grad: 2 x the measured worst, rounded up (module docstring)

# ks = 1: the weight gradient aside, the epilogues of the chain module without the 3x3-only ones, and PixelShuffle
EPILOGUES = {
    "plain": dict(bias=False),
    "bias": dict(),
    "bias_relu": dict(act=CR.ACT_RELU),
    "bias_lrelu_0.25": dict(act=CR.ACT_LRELU, slope=0.25),
    "conv0_lrelu_0.1": dict(act=CR.ACT_LRELU, slope=0.1),
    "res_alpha_0.125": dict(alpha=0.125, res=True),
    "want_pre": dict(act=CR.ACT_RELU, alpha=0.5, res=True, want_pre=True),
    "gelu_pre_only": dict(act=CR.ACT_GELU, want_pre=True),
    "dgrad_plain": dict(bias=False, dgrad=True),
    "dgrad_res": dict(bias=False, dgrad=True, res=True),
    "dgrad_mask1_res": dict(bias=False, dgrad=True, alpha=0.125, actgrad=1, res=True),
    "dgrad_mask2": dict(bias=False, dgrad=True, alpha=0.5, slope=0.25, actgrad=2, res=True),
    "pixel_shuffle": dict(act=CR.ACT_LRELU, slope=0.25, pixel_shuffle=True),
    # real-valued
    "real_res": dict(alpha=0.1, res=True),
    "real_gelu": dict(act=CR.ACT_GELU, alpha=0.5, want_pre=True),
    "real_gelu_grad": dict(bias=False, dgrad=True, alpha=0.5, actgrad=3),
}
EXACT_EPILOGUES = [n for n in EPILOGUES if not n.startswith("real_")]


class Case(NamedTuple):
    """One 1x1 convolution.  kernel: the template instance the case is meant for.  Forward: sources of src_ch channels -> co outputs; the weight
    has o_total outputs (the pack takes [o0, o0 + co)) and i_total inputs (the single source IS the channel slice [src_off, + src_ch[0]) of an
    i_total-wide tensor).  Data gradient (the epilogue says so): src_ch = (K,) channels of dy, co = input channels of the weight (K, co).
    geom None: a wave-autonomous case whose row count follows from the compute units, so that a wave owns `tpw` tiles."""
    kernel: tuple
    geom: Optional[Tuple[int, int, int]]
    src_ch: Tuple[int, ...]
    co: int
    epi: str = "bias"
    hint: str = ""       # "wres": hip.CONV_LINEAR_WRES is asked for although `kernel` is the general kernel -- the case tests the fallback
    o_total: int = 0
    o0: int = 0
    i_total: int = 0
    src_off: int = 0
    probe: int = -1      # 0..2: permutation probe
    odd_ps: bool = False  # output pixel stride that is no multiple of 8 (drives the element-wise epilogue)
    res_off: int = 0     # the residual view starts this many elements off 16-byte alignment (the same)
    tpw: int = 0
    family: str = ""     # "" = "full" up to 256 input channels, else "small"; "real": seeded normal values

    @property
    def fam(self):
        return self.family or ("full" if sum(self.src_ch) <= 256 else "small")

    @property
    def id(self):
        k = self.kernel
        s = "-".join(map(str, k)) + ("-hint_" + self.hint if self.hint else "") + "-"
        s += ("x".join(map(str, self.geom)) if self.geom else f"tpw{self.tpw}") + "-" + "+".join(map(str, self.src_ch)) + f"to{self.co}-{self.epi}"
        s += f"-o{self.o0}of{self.o_total}" if self.o_total else ""
        s += f"-i{self.src_off}of{self.i_total}" if self.i_total else ""
        s += "-oddps" if self.odd_ps else ""
        s += f"-resoff{self.res_off}" if self.res_off else ""
        s += "-real" if self.family == "real" else ""
        return s + (f"-probe{self.probe}" if self.probe >= 0 else "")


# ---- what a case asks vmg_conv_fwd for, and what the plan must answer -------------------------------------------------------------------
def request(case):
    """(torch dtype, cout_tiles, mt, route name) of the call."""
    k = case.kernel
    if case.hint:
        assert case.hint == "wres" and k[0] == IG and k[1] == "bf16" and k[2] == 1
        return torch.bfloat16, k[3], 0, "wres"
    if k[0] == IG:
        return (torch.bfloat16 if k[1] == "bf16" else torch.float32), k[3], k[2], "general"
    if k[0] == KSP:
        return torch.bfloat16, k[1], 0, "ksplit"
    assert k[0] == WRES
    return torch.bfloat16, k[1], 0, "wres"


def vec8_of(case):
    """The rule of vmg_conv_fwd for the 16-byte epilogue: bf16, no PixelShuffle, Cout % 16 == 0, every output-side row 16-byte aligned."""
    e = EPILOGUES[case.epi]
    return int(request(case)[0] == torch.bfloat16 and not e.get("pixel_shuffle") and case.co % 16 == 0 and not case.odd_ps and
               not (case.res_off and e.get("res")))


def expected_plan(case):
    """The first seven ints of vmg_conv_fwd_plan for the instance the case names: family, dtype, ks, mt, ntb, variant, vec8 (include/vmg_hip.h)."""
    k = case.kernel
    if k[0] == IG:
        return (1, 1 if k[1] == "bf16" else 0, 1, k[2], k[3], 0, vec8_of(case))
    if k[0] == KSP:
        return (2, 1, 1, 1, k[1], 0, vec8_of(case))
    return (4, 1, 1, 1, k[1], k[2], 1)


def rows_for(case, ncu):
    """(N, H, W) of a case.  tpw cases: the fewest rows at which launch_linear_wres gives a wave `tpw` tiles on ncu compute units --
    waves = max(1, (2 / NS) * ncu / ncb) * 4, tiles = (tpw - 1) * waves + 1, one row in the last tile."""
    if case.geom is not None:
        return case.geom
    _, ntb, ns = case.kernel
    ncb = -(-case.co // (16 * ntb))
    waves = max(1, (2 if ns == 1 else 1) * ncu // ncb) * 4
    return (1, 1, 16 * (case.tpw - 1) * waves + 1)


class Layout(NamedTuple):
    src_ps: Tuple[int, ...]
    out_ch: int
    out_ps: int
    res_ps: int
    aux_ps: int


def layout(case):
    """Pixel strides (elements) of the embedded views; the GPU launch and the host-side plan test share them."""
    ps_shuffle = EPILOGUES[case.epi].get("pixel_shuffle", False)
    oc = case.co // 4 if ps_shuffle else case.co
    c8 = (oc + 7) // 8 * 8
    r8 = (case.co + 7) // 8 * 8
    return Layout(tuple((case.i_total or c) + 8 + 16 * (s % 2) for s, c in enumerate(case.src_ch)), oc, c8 + (9 if case.odd_ps else 8), r8 + 16, r8 + 24)


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
GENERAL = [(IG, "bf16", 1), (IG, "bf16", 2), (IG, "f32", 1)]  # + (NTB,)
WRES_DENSE = (16, 48, 80, 112, 144)  # sources whose LDS pixel stride is dense (include/vmg_hip.h, vmg_conv_desc::deep): channels % 32 == 16
NS2_SOURCES = tuple(range(176, 321, 16))  # single sources that split into two equal blocks, each a multiple of 8 and at most 160 channels


def _rot(i, allowed=NTBS):
    return allowed[i % len(allowed)]


def _row_cases():
    out = []
    small = [(1, 1, m) for m in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)] + [(2, 3, 5), (3, 7, 11)]
    for i, g in enumerate(small):
        out += [Case((IG, "bf16", 1, 9), g, (144,), 144), Case((IG, "bf16", 2, 3), g, (144,), 144), Case((IG, "f32", 1, 5), g, (144,), 144),
                Case((KSP, 3), g, (144,), 144)]
    for g in [(1, 1, m) for m in (1, 17, 64, 65, 80, 255, 256, 257, 1000)] + [(2, 3, 5), (3, 7, 11)]:
        out += [Case((WRES, 3, 1), g, (144,), 144), Case((WRES, 5, 1), g, (144,), 144), Case((WRES, 3, 2), g, (288,), 144)]
    # an odd number of tiles per wave (>= 5): the last tile of a wave lands in buffer 0, and a wave owns more than both buffers once
    out += [Case((WRES, 3, 1), None, (16,), 48, tpw=5), Case((WRES, 5, 1), None, (16,), 80, tpw=5), Case((WRES, 3, 2), None, (288,), 144, tpw=9)]
    return out


CI_CASES = [(8,), (24,), (32,), (40,), (64,), (72,), (96,), (144,), (160,), (168,), (288,), (320,), (576,), (144, 288, 144), (8, 8)]


def _channel_cases():
    out = []
    i = 0
    for src in CI_CASES:
        for epi in ("plain", "bias"):
            g = (1, 1, 129) if i % 2 else (1, 1, 65)
            co = (144, 48, 80, 16)[i % 4]
            for f, fam in enumerate(GENERAL):
                out.append(Case(fam + (_rot(i + 2 * f),), g, src, co, epi))
            out.append(Case((KSP, _rot(i, (1, 3, 4, 5))), g, src, co, epi))
            i += 1
    for f, fam in enumerate(GENERAL + [(KSP,)]):
        n = 3 + (f % 2) * 2  # 3 or 5
        out += [Case(fam + (n,), (1, 1, 65), (144,), 144, i_total=176, src_off=16),   # a channel slice of a wider tensor, a K slice of a wider weight
                Case(fam + (n,), (1, 1, 65), (144,), 144, o_total=200, o0=40)]        # an output slice of a wider weight
    out += [Case((WRES, 3, 1), (1, 1, 80), (144,), 144, i_total=176, src_off=16), Case((WRES, 5, 1), (1, 1, 80), (144,), 144, o_total=200, o0=40),
            Case((WRES, 3, 2), (1, 1, 80), (288,), 144, i_total=320, src_off=16), Case((WRES, 3, 2), (1, 1, 80), (288,), 144, o_total=200, o0=40)]
    # the wave-autonomous kernel: every multiple of 8 from 8 to 160 at M = 80; the sources without a dense LDS stride fall back
    for ci in range(8, 161, 8):
        for n in (3, 5):
            co = 48 if n == 3 else 80
            for epi in ("plain", "bias"):
                if ci in WRES_DENSE:
                    out.append(Case((WRES, n, 1), (1, 1, 80), (ci,), co, epi))
                else:
                    out.append(Case((IG, "bf16", 1, n), (1, 1, 80), (ci,), co, epi, hint="wres"))
    for ci in NS2_SOURCES:
        out += [Case((WRES, 3, 2), (1, 1, 80), (ci,), 48, epi) for epi in ("plain", "bias")]
    out += [Case((IG, "bf16", 1, 3), (1, 1, 80), (184,), 48, hint="wres"),            # 184 = 23 x 8: no two equal blocks
            Case((IG, "bf16", 1, 3), (1, 1, 80), (144, 144), 48, hint="wres"),        # two sources
            Case((IG, "bf16", 1, 5), (1, 1, 80), (288,), 80, hint="wres")]            # the two-block form exists with cout_tiles 3 only
    return out


def _cout_cases():
    out = []
    for i, co in enumerate((8, 16, 48, 80, 144, 288, 3, 20)):
        g = (1, 1, 65) if i % 2 else (1, 1, 129)
        for f, fam in enumerate(GENERAL):
            out += [Case(fam + (_rot(i + 3 * f + 1),), g, (144,), co), Case(fam + (_rot(i + f),), g, (8,), co, "plain")]
        out += [Case((KSP, _rot(i + 1, (1, 3, 4, 5))), g, (144,), co), Case((KSP, _rot(i, (1, 3, 4, 5))), g, (8,), co, "plain")]
    # bf16 kernels that would take the 16-byte epilogue, driven into the element-wise one
    for k in [(IG, "bf16", 1, 9), (IG, "bf16", 2, 5), (KSP, 3)]:
        out += [Case(k, (1, 1, 65), (144,), 144, "want_pre", odd_ps=True), Case(k, (1, 1, 65), (144,), 144, "res_alpha_0.125", res_off=2)]
    # the wave-autonomous kernel: three blocks at NTB 3, a short last block at NTB 5, one block, six blocks
    for co in (16, 48, 80, 144, 288):
        out += [Case((WRES, 3, 1), (1, 1, 80), (144,), co), Case((WRES, 5, 1), (1, 1, 80), (144,), co), Case((WRES, 3, 2), (1, 1, 80), (288,), co)]
    # ... and what it does not cover: no 16-byte rows
    out += [Case((IG, "bf16", 1, 3), (1, 1, 80), (144,), 8, hint="wres"), Case((IG, "bf16", 1, 5), (1, 1, 80), (144,), 20, hint="wres"),
            Case((IG, "bf16", 1, 3), (1, 1, 80), (144,), 144, "want_pre", hint="wres", odd_ps=True),
            Case((IG, "bf16", 1, 3), (1, 1, 80), (144,), 144, "res_alpha_0.125", hint="wres", res_off=2),
            Case((IG, "bf16", 1, 3), (1, 1, 80), (144,), 144, "pixel_shuffle", hint="wres")]
    return out


EPI_KERNELS = [((IG, "bf16", 1, 9), (144,)), ((IG, "bf16", 2, 3), (144,)), ((IG, "f32", 1, 5), (144,)), ((KSP, 3), (144,)), ((WRES, 3, 1), (144,)),
               ((WRES, 5, 1), (144,)), ((WRES, 3, 2), (288,))]
EPI_GEOMS = [(1, 1, 65), (3, 7, 11)]


def _epilogue_cases():
    out = []
    for k, src in EPI_KERNELS:
        for name in EXACT_EPILOGUES:
            if name in ("plain", "bias"):
                continue
            if name == "pixel_shuffle" and k[0] == WRES:
                continue  # (it refuses PixelShuffle: a fallback case of _cout_cases)
            out += [Case(k, g, src, 144, name) for g in EPI_GEOMS]
        # data gradients whose weight is not square (a transposition that mixes up O and I shows)
        if not (k[0] == WRES and k[2] == 2):  # (<3, 2>: its whole list is 288 -> 144 already)
            out.append(Case(k, EPI_GEOMS[0], (144,), 288, "dgrad_mask1_res"))
            if k[0] != WRES:
                out.append(Case(k, EPI_GEOMS[0], (288,), 144, "dgrad_mask1_res"))
    return out


def _probe_cases():
    out = []
    for t in range(3):
        out += [Case(k, (1, 1, 65), src, 144, "plain", probe=t) for k, src in EPI_KERNELS]
        out += [Case(fam + (1,), (1, 1, 17), (8,), 16, "plain", probe=t) for fam in GENERAL + [(KSP,)]]
        out += [Case((IG, "bf16", 1, 3), (1, 1, 17), (8,), 16, "plain", probe=t, hint="wres")]
    return out


def exact_cases():
    return _row_cases() + _channel_cases() + _cout_cases() + _epilogue_cases() + _probe_cases()


def _real_cases():
    out = []
    g = (1, 1, 257)
    for k in [(IG, "bf16", 1, 9), (IG, "bf16", 2, 9), (IG, "f32", 1, 5), (KSP, 3)]:
        out += [Case(k, g, (144,), 144, "real_res", family="real"), Case(k, g, (144,), 288, "real_res", family="real"),
                Case(k, g, (288,), 144, "real_res", family="real")]
    for k in [(WRES, 3, 1), (WRES, 5, 1)]:
        out += [Case(k, g, (144,), 144, "real_res", family="real"), Case(k, g, (144,), 288, "real_res", family="real")]
    out.append(Case((WRES, 3, 2), g, (288,), 144, "real_res", family="real"))
    return out


def _gelu_cases():
    out = []
    for k in [(IG, "bf16", 1, 9), (IG, "bf16", 2, 9), (KSP, 3), (WRES, 3, 1), (WRES, 5, 1)]:
        out += [Case(k, (1, 1, 257), (144,), 288, "real_gelu", family="real"), Case(k, (1, 1, 257), (144,), 288, "real_gelu_grad", family="real")]
    return out


def all_cases():
    return exact_cases() + _real_cases() + _gelu_cases()


def exact_args(case):
    """The arguments of conv_ref.assert_exact(..., taps=1) for a case."""
    e = EPILOGUES[case.epi]
    scales = [e["slope"]] if e.get("act") == CR.ACT_LRELU else []
    scales.append(e.get("alpha", 1.0))
    if e.get("actgrad") == 2:
        scales.append(e["slope"])
    return case.fam, sum(case.src_ch), e.get("bias", True), e.get("res", False), tuple(scales)


# ---- operands and expected values -------------------------------------------------------------------------------------------------------
def _mods():
    from vmg_amd import hip, kernels as K
    return hip, K


def _seed(geom, case):
    return (geom[0] * 7919 + geom[1] * 104729 + geom[2] * 1299709 + sum(case.src_ch) * 31 + case.co * 17 + len(case.src_ch)) % (2 ** 31 - 1)


def _values(shape, seed, family, f32=False):
    """Operand values: the exact families, or ("real") seeded normal values -- bf16 numbers for the bf16 kernels, any fp32 for the fp32 ones."""
    if family == "real":
        v = torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed))
        return v if f32 else v.bfloat16().float()
    return WR.exact_values(shape, seed, family)


@functools.lru_cache(maxsize=16)
def _operands(geom, src_ch, co, family, o_total, o0, i_total, src_off, dgrad, probe, f32):
    seed = _seed(geom, Case((), geom, src_ch, co))
    ci = sum(src_ch)
    wide = [_values(geom + (i_total or c,), seed + 11 * s, "real" if probe >= 0 else family, f32) for s, c in enumerate(src_ch)]
    assert not i_total or len(src_ch) == 1
    srcs = [t[..., src_off:src_off + c] if i_total else t for t, c in zip(wide, src_ch)]
    real = family == "real"
    if dgrad:
        assert len(src_ch) == 1 and not (o_total or i_total or probe >= 0)
        w = _values((ci, co), seed + 101, family, f32)
        if real:
            w = w / ci ** 0.5 if f32 else (w / ci ** 0.5).bfloat16().float()
        return wide, srcs, w, CR.dlinear_ref(srcs[0], w), (CR.dlinear_ref(srcs[0].abs(), w.abs()) if real else None)
    if probe >= 0:
        w, pi = CR.one_hot_linear(co, ci, probe)
        acc = CR.linear_ref(srcs, w)
        assert torch.equal(acc, torch.cat(srcs, -1)[..., pi].double())  # the probe's reference IS the permuted copy
        return wide, srcs, w, acc, None
    w = _values((o_total or co, i_total or ci), seed + 101, family, f32)
    if real:
        w = w / ci ** 0.5 if f32 else (w / ci ** 0.5).bfloat16().float()
    kw = dict(src_off=[src_off] if i_total else None, o0=o0, on=co)
    return wide, srcs, w, CR.linear_ref(srcs, w, **kw), (CR.linear_ref([s.abs() for s in srcs], w.abs(), **kw) if real else None)


class _Problem:
    def __init__(self, geom, case):
        e = dict(EPILOGUES[case.epi])
        dt = request(case)[0]
        f32 = dt == torch.float32
        fam = case.fam
        self.geom, self.case = geom, case
        self.real = fam == "real"
        self.dgrad = e.pop("dgrad", False)
        self.want_pre = e.pop("want_pre", False)
        self.pixel_shuffle = e.pop("pixel_shuffle", False)
        if not self.real:
            CR.assert_exact(*exact_args(case), taps=1)  # the invariant, before anything runs on the GPU
        self.wide, self.srcs, self.w, acc, mag = _operands(geom, case.src_ch, case.co, fam, case.o_total, case.o0, case.i_total, case.src_off, self.dgrad,
                                                           case.probe, f32)
        seed = _seed(geom, case) + 1000
        shape = geom + (case.co,)
        self.bias = (_values((case.co,), seed + 1, fam, f32) * (0.1 if self.real else 1.0)) if e.pop("bias", True) else None
        self.res = _values(shape, seed + 2, fam, f32) if e.pop("res", False) else None
        self.aux = None
        if e.get("actgrad"):
            aux = _values(shape, seed + 3, fam, f32)
            flat = aux.reshape(-1)
            flat[0::7] = -0.0  # neither zero is positive
            flat[3::11] = 0.0
            self.aux = aux
        self.kw = e  # act, slope, alpha, actgrad: as vmg_conv_fwd takes them
        self.acc, self.mag = acc, mag
        if e.get("act") == CR.ACT_GELU or e.get("actgrad") == 3:
            self.want = self.want_pre_value = None  # (the GELU tests compute their own)
            if not self.real:
                _, self.want_pre_value = CR.epilogue_ref(acc, self.bias, act=CR.ACT_GELU, out_dtype=dt)
            return
        out, pre = CR.epilogue_ref(acc, self.bias, aux=self.aux, res=self.res, exact=not self.real, out_dtype=dt, **e)
        if self.pixel_shuffle:
            out = CR.pixel_shuffle_ref(out)
        self.want, self.want_pre_value = out, pre
        if self.real:
            S = mag + (self.bias.abs().double() if self.bias is not None else 0) + (self.res.abs().double() if self.res is not None else 0)
            self.bound = CR.real_bound(out, S, sum(case.src_ch), taps=1, out_dtype=dt)


def _outside_mask(view):
    C, ps = view.shape[-1], view.stride(-2)
    M = view.numel() // C
    mask = torch.ones(view._base.numel(), dtype=torch.bool)
    idx = (view.storage_offset() + torch.arange(M)[:, None] * ps + torch.arange(C)[None, :]).reshape(-1)
    mask[idx] = False
    return mask


def _name(idx, case):
    n, y, x, o = idx
    s = f"image {n}, pixel ({y}, {x}), output channel {o}"
    if case.probe >= 0:
        s += f" = the copy of input channel {int(CR.one_hot_linear(case.co, sum(case.src_ch), case.probe)[1][o])}"
    return s


def _assert_same(got, want, what, case):
    n, idx, g, w = WR.first_mismatch(got, want)
    if n:
        err, top = float((got.double() - want.double()).abs().max()), float(want.double().abs().max())
        raise AssertionError(f"{what}: {n} of {got.numel()} elements differ from the fp64 reference, the first at {_name(idx, case)}: got {g!r}, want "
                             f"{w!r} (largest error {err:g}; 2e-2 of the largest value: {2e-2 * max(1.0, top):g})")
    assert torch.equal(got, want), what


def _launch(prob):
    """Pack, embed, ask the plan, launch twice.  Returns (out, out_pre or None) as CPU tensors after the checks every case shares: the plan names
    the case's instance, no NaN left inside, nothing changed outside the views, the same bits from the second launch."""
    hip, K = _mods()
    assert (hip.ACT_NONE, hip.ACT_RELU, hip.ACT_LRELU, hip.ACT_GELU) == (CR.ACT_NONE, CR.ACT_RELU, CR.ACT_LRELU, CR.ACT_GELU)
    case, (N, H, W) = prob.case, prob.geom
    dt, tiles, mt, route = request(case)
    deep = dict(general=hip.CONV_GENERAL, ksplit=hip.CONV_KSPLIT, wres=hip.CONV_LINEAR_WRES)[route]
    lay = layout(case)
    bits = torch.int16 if dt == torch.bfloat16 else torch.int32
    dev = "cuda"
    srcs = []
    for t, c, ps in zip(prob.wide, case.src_ch, lay.src_ps):
        v = WR.embed(t.to(dt), ps, GUARD, device=dev)
        assert v.stride(-2) > t.shape[-1] and torch.equal(v.float().cpu(), t)  # the values are numbers of the kernel's type
        srcs.append(v[..., case.src_off:case.src_off + c] if case.i_total else v)
    w = prob.w.to(dev).contiguous()
    pw = K.pack_conv_weight(w, dt, src_ch=list(case.src_ch), src_off=[case.src_off] if case.i_total else None, o0=case.o0, on=case.co,
                            transpose_flip=prob.dgrad, cout_tiles=tiles)
    assert pw.layout == "std" and pw.cout_tiles == tiles and pw.cout == case.co and pw.src_ch == list(case.src_ch)
    emb = lambda t, ps, off=0: WR.embed(t.to(dt), ps, GUARD, offset=off, device=dev)  # noqa: E731
    res = emb(prob.res, lay.res_ps, case.res_off) if prob.res is not None else None
    aux = emb(prob.aux, lay.aux_ps) if prob.aux is not None else None
    oshape = (N, 2 * H, 2 * W, lay.out_ch) if prob.pixel_shuffle else (N, H, W, lay.out_ch)
    blank = torch.full(oshape, float("nan"), dtype=dt)
    outs = [emb(blank, lay.out_ps)] + ([emb(blank, lay.out_ps)] if prob.want_pre else [])
    before = [o._base.clone() for o in outs]
    bias = prob.bias.to(dev) if prob.bias is not None else None
    args = (srcs, pw, bias, N, H, W)
    kw = dict(res=res, aux=aux, out=outs[0], out_pre=outs[1] if prob.want_pre else None, deep=deep, mt=mt, pixel_shuffle=prob.pixel_shuffle, **prob.kw)
    what = case.id
    runs = []
    for _ in range(2):
        for o, b in zip(outs, before):
            o._base.copy_(b)
        plan = K.conv_forward_plan(*args, **kw)
        assert tuple(plan[:7]) == expected_plan(case), (f"{what}: the call runs {plan}, not the instance the case names "
                                                        f"(family, dtype, ks, mt, ntb, variant, vec8) = {expected_plan(case)}")
        if case.tpw:
            assert plan.tiles_per_wave == case.tpw and case.tpw % 2 == 1 and case.tpw >= 5, f"{what}: {plan}"
        K.conv_forward(*args, **kw)
        torch.cuda.synchronize()
        runs.append([o._base.cpu() for o in outs])
    for k, (o, b) in enumerate(zip(outs, before)):
        name = what + (": out", ": out_pre")[k]
        full, again = runs[0][k], runs[1][k]
        assert torch.equal(full.view(bits), again.view(bits)), name + ": the second launch gave other bits"
        mask = _outside_mask(o)
        assert torch.equal(full.view(bits)[mask], b.cpu().view(bits)[mask]), name + ": the allocation changed outside the view"
        if lay.out_ch % 8 == 0:
            assert bool(torch.isnan(full[mask]).all()), name + ": not every element outside the view is NaN"
    got = [o.cpu() for o in outs]
    for k, g in enumerate(got):
        nan = torch.isnan(g)
        if bool(nan.any()):
            first = tuple(int(v) for v in torch.nonzero(nan)[0])
            raise AssertionError(f"{what}{(': out', ': out_pre')[k]}: {int(nan.sum())} of {g.numel()} elements are NaN, the first at {_name(first, case)}: "
                                 "something outside the operands was read, or the element was never written")
    return got[0], (got[1] if prob.want_pre else None)


def _geom(case):
    return rows_for(case, torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=4)
def _problem(geom, case):
    return _Problem(geom, case)


def _prob(case):
    """(the expected values depend on the kernel's dtype only: instances of one dtype share them)"""
    key = case._replace(kernel=(IG, "f32" if request(case)[0] == torch.float32 else "bf16", 1, 1), hint="", odd_ps=False, res_off=0, tpw=0)
    p = copy.copy(_problem(_geom(case), key))
    p.case = case
    return p


def _run_exact(case):
    prob = _prob(case)
    out, pre = _launch(prob)
    if prob.want_pre:
        _assert_same(pre, prob.want_pre_value, case.id + ": out_pre", case)
    if prob.want is not None:
        _assert_same(out, prob.want, case.id + ": out", case)


def _ids(cases):
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return ids


@pytest.mark.parametrize("case", _row_cases(), ids=_ids(_row_cases()))
def test_rows(case):
    _run_exact(case)


@pytest.mark.parametrize("case", _channel_cases(), ids=_ids(_channel_cases()))
def test_input_channels(case):
    _run_exact(case)


@pytest.mark.parametrize("case", _cout_cases(), ids=_ids(_cout_cases()))
def test_output_channels(case):
    _run_exact(case)


@pytest.mark.parametrize("case", _epilogue_cases(), ids=_ids(_epilogue_cases()))
def test_epilogues(case):
    _run_exact(case)


@pytest.mark.parametrize("case", _probe_cases(), ids=_ids(_probe_cases()))
def test_permutation_probes(case):
    _run_exact(case)


# ------------------------------------------------------------------------------------------------------------------------------------
# real-valued cases: the per-element bound
# ------------------------------------------------------------------------------------------------------------------------------------
def _worst(err, bound):
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    i = int(ratio.reshape(-1).argmax())
    return float(ratio.reshape(-1)[i]), tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))


def _assert_bound(got, want, bound, what, case):
    err = (got.double() - want).abs()
    worst, idx = _worst(err, bound)
    print(f"bound ratio {what}: {worst:.4f} at {idx}")
    assert worst <= 1.0, (f"{what}: |got - v| = {float(err[idx]):g} at {_name(idx, case)} is {worst:.3f} of the bound {float(bound[idx]):g} "
                          f"(got {float(got[idx])!r}, v = {float(want[idx])!r})")


@pytest.mark.parametrize("case", _real_cases(), ids=_ids(_real_cases()))
def test_real_values_within_the_per_element_bound(case):
    prob = _prob(case)
    out, _ = _launch(prob)
    _assert_bound(out, prob.want, prob.bound, case.id, case)


# ------------------------------------------------------------------------------------------------------------------------------------
# GELU and its gradient
# ------------------------------------------------------------------------------------------------------------------------------------
def gelu_sweep():
    """~70 k fp32 arguments: [-12, 12] evenly, +-0, +-2^-126, +-30, and the 2 048 fp32 numbers nearest sqrt(2) and -sqrt(2) each."""
    near = (np.float32(np.sqrt(2.0)).view(np.int32) + np.arange(-1024, 1024, dtype=np.int32)).view(np.float32)
    v = np.concatenate([np.linspace(-12.0, 12.0, 65536, dtype=np.float32), np.float32([0.0, -0.0, 2.0 ** -126, -2.0 ** -126, 30.0, -30.0]), near, -near])
    v = np.concatenate([v, np.zeros(-len(v) % 8, dtype=np.float32)])
    return torch.from_numpy(v).reshape(1, 1, -1, 8)


def _device_function(grad):
    """gelu_erf (grad False) or gelu_erf_grad of the sweep, through the fp32 general kernel with an identity weight 8 -> 8."""
    hip, K = _mods()
    x = gelu_sweep()
    M = x.shape[2]
    pw = K.pack_conv_weight(torch.eye(8).cuda(), torch.float32, cout_tiles=1)
    if grad:
        got, _ = K.conv_forward([torch.ones_like(x).cuda()], pw, None, 1, 1, M, aux=x.cuda(), actgrad=3)
    else:
        got, _ = K.conv_forward([x.cuda()], pw, None, 1, 1, M, act=hip.ACT_GELU)
    return x, got.cpu().reshape(x.shape)


@pytest.mark.parametrize("grad", [False, True], ids=["gelu", "gelu_grad"])
def test_gelu_device_functions_within_the_asserted_error(grad):
    x, got = _device_function(grad)
    want = CR.gelu_grad_ref(x) if grad else CR.gelu_ref(x)
    err = (got.double() - want).abs()
    i = int(err.reshape(-1).argmax())
    limit = EGRAD if grad else EG
    print(f"gelu device function ({'gradient' if grad else 'value'}): worst absolute error {float(err.max()):.3e} at x = {float(x.reshape(-1)[i])!r}; "
          f"asserted {limit:g}")
    assert not bool(torch.isnan(got).any())
    assert float(err.max()) <= limit, f"x = {float(x.reshape(-1)[i])!r}: got {float(got.reshape(-1)[i])!r}, want {float(want.reshape(-1)[i])!r}"


@pytest.mark.parametrize("case", _gelu_cases(), ids=_ids(_gelu_cases()))
def test_gelu_epilogues_within_the_bound(case):
    prob = _prob(case)
    out, pre = _launch(prob)
    alpha, ci = prob.kw["alpha"], sum(case.src_ch)
    v = prob.acc if prob.bias is None else prob.acc + prob.bias.double()
    S = prob.mag + (prob.bias.abs().double() if prob.bias is not None else 0)
    e32 = CR.sum_bound(S, ci, taps=1)
    if prob.want_pre:
        _assert_bound(pre, v, CR.real_bound(v, S, ci, taps=1), case.id + ": out_pre", case)
    if prob.kw.get("actgrad") == 3:
        g = alpha * v * CR.gelu_grad_ref(prob.aux)
        E = alpha * (1.13 * e32 + v.abs() * EGRAD)
    else:
        g = alpha * CR.gelu_ref(v)
        E = alpha * (1.13 * e32 + EG)
    _assert_bound(out, g, 2.0 ** -8 * (g.abs() + E) + E, case.id + ": out", case)
