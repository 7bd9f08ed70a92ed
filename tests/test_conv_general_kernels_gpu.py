"""The convolutions that none of the special routes takes -- the general pixel-split kernel for 3x3 and 7x7 and the weights-stationary 3x3 kernel
of csrc/conv_igemm.hip -- element by element against the fp64 reference of tests/conv_ref.py (conv_ref, dgrad_ref, pixel_shuffle_ref), one case
table for all 39 template instances:

    conv_igemm_kernel<bf16, 3, MT, NTB>   MT 1, 2;  NTB 1, 3, 4, 5, 7, 8, 9          (IG, "bf16", 3, MT, NTB)
    conv_igemm_kernel<float, 3, 1, NTB>             NTB 1, 3, 4, 5, 7, 8, 9          (IG, "f32", 3, 1, NTB)
    conv_igemm_kernel<bf16 | float, 7, 1, NTB>      NTB 1, 2, 4                      (IG, dtype, 7, 1, NTB)
    conv_wstat_kernel<NCT, NB, FULL>      NCT 1, 3, 4;  NB 1, 2;  FULL 0, 1          (WSTAT, NCT, NB, FULL)

Which kernel a case runs.  hip.CONV_WSTAT is a hint that falls back to the general kernel without a word, and mt = 2 is silently forced to 1
for fp32 and for 7x7.  Every case therefore NAMES the instance it is meant for (Case.kernel), kernels.conv_forward_plan must report that very
instance before each launch, and tests/test_conv_plan.py asserts the same for the whole table without a GPU (and that the table reaches all 39
instances).  A case that asks for something it is not meant to get says so in its name (Case.fallback = "wstat" / "mt2": "-fallback_from_..."):
it tests the fallback.  One fallback the header mentions cannot be reached: a bf16 source pixel stride that is no multiple of 8 is refused by
vmg_conv_fwd for every route (16-byte rows), which tests/test_conv_plan.py asserts.

Exactness invariant.  Operands, bias and residual are k * 2^-s (wgrad_ref.FAMILIES), alpha and the slopes powers of two (the model's lone
lrelu 0.1 is the one exception conv_ref.assert_exact admits), and assert_exact(..., taps = 9 or 49) has checked BEFORE the launch that every
partial sum in any order and every epilogue intermediate is an fp32 number.  The full-mantissa family "full" is exact for 3x3 up to 28 input
channels (8, 16 and 24 use it), for 7x7 only through the shift probes; everything else uses "small".  The output must EQUAL
round_bf16(reference) -- the fp64 value itself for the fp32 kernels -- and a failure names the first differing element.  The shift probes
(one-hot weights: output channel o is the copy of one input channel through one tap) are exact for any input and name the tap and the
channel; probe_taps_missing() asserts that the probe set of every probed channel case meets every tap in every 16-channel output tile.

Every source, res, aux, out and out_pre is a view inside a NaN-filled allocation (wgrad_ref.embed) with a pixel stride larger than the channel
count and guard rows of 12 image rows + 40 pixels before and after; every case launches twice: no NaN inside, nothing changed outside, the same
bits again.

The many-tile weights-stationary cases (geom None) take their size from the grid the plan reports for a launch that fills the device
(wstat_rows): 2 * grid + 1 tiles or a few more, in five tile columns the last of which is partial -- a workgroup then walks three tiles (both
halo buffers, the deferred epilogue of tile t - 1, the drain after the last tile), the tile count is no multiple of 8 (uneven XCD bands), and
wstat_walk() recomputes the kernel's tile assignment to assert all that against the grid of the launch itself.

Real-valued cases (seeded normal values, alpha = slope = 0.1, a residual) are held per element to conv_ref.real_bound(v, S, ci_total, taps,
out_dtype); each prints its worst |got - v| / bound.  GELU results use the constants EG / EGRAD that tests/test_linear_kernels_gpu.py derived
for the device functions (nothing is measured again here).

Measured on an MI355X, the largest |got - v| / bound per family over the real-valued cases: bf16 3x3 0.829 (64 -> 3 with alpha 0.1 and a residual
on (1, 24, 81), MT 2; 0.73 on the GELU out_pre), bf16 7x7 0.745 (32 -> 64 on (1, 24, 81)), weights-stationary 0.983 (the 8 -> 64 data gradient
with mask and residual on (2, 7, 15): the bf16 rounding of a value just above a power of two; 0.84 .. 0.94 on the other shapes), fp32 3x3
0.0023 and fp32 7x7 0.0001 -- nothing in the derivation for 49 taps had to give.  GELU and its masked gradient: 0.70 (general kernel) and 0.84
(weights-stationary) of their bounds.  Every case passes (855 cases, about 5 s)."""
import copy
import functools
from typing import NamedTuple, Optional, Tuple

import pytest
import torch

from tests import conv_ref as CR
from tests import wgrad_ref as WR
from tests.test_linear_kernels_gpu import EG, EGRAD, _outside_mask, _worst

pytestmark = pytest.mark.gpu

IG, WSTAT = "igemm", "wstat"
NTBS3, NTBS7 = (1, 3, 4, 5, 7, 8, 9), (1, 2, 4)
INSTANCES = ([(IG, "bf16", 3, mt, n) for mt in (1, 2) for n in NTBS3] + [(IG, "f32", 3, 1, n) for n in NTBS3] +
             [(IG, d, 7, 1, n) for d in ("bf16", "f32") for n in NTBS7] + [(WSTAT, nct, nb, full) for nct in (1, 3, 4) for nb in (1, 2) for full in (0, 1)])
assert len(INSTANCES) == 39 and len(set(INSTANCES)) == 39

# the chain module's table (tests/test_conv_chain_kernels_gpu.py), alpha alone, and PixelShuffle
EPILOGUES = {
    "plain": dict(bias=False),
    "bias": dict(),
    "bias_relu": dict(act=CR.ACT_RELU),
    "bias_lrelu_0.25": dict(act=CR.ACT_LRELU, slope=0.25),
    "conv0_lrelu_0.1": dict(act=CR.ACT_LRELU, slope=0.1),                       # one rounding of v * float32(0.1), then the output type
    "bias_alpha_0.5": dict(alpha=0.5),
    "res_alpha_0.125": dict(alpha=0.125, res=True),
    "want_pre": dict(act=CR.ACT_RELU, alpha=0.5, res=True, want_pre=True),
    "gelu_pre_only": dict(act=CR.ACT_GELU, want_pre=True),                      # GELU itself has no exact form: out_pre only
    "dgrad_plain": dict(bias=False, dgrad=True),
    "dgrad_res": dict(bias=False, dgrad=True, res=True),
    "dgrad_mask1": dict(bias=False, dgrad=True, alpha=0.125, actgrad=1),
    "dgrad_mask1_res": dict(bias=False, dgrad=True, alpha=0.125, actgrad=1, res=True),
    "dgrad_mask2": dict(bias=False, dgrad=True, alpha=0.5, slope=0.25, actgrad=2, res=True),
    "pixel_shuffle": dict(act=CR.ACT_LRELU, slope=0.25, pixel_shuffle=True),
    "pixel_shuffle_0.1": dict(act=CR.ACT_LRELU, slope=0.1, pixel_shuffle=True),  # the model's up-convs
    # real-valued
    "real_res": dict(alpha=0.1, res=True),
    "real_lrelu": dict(act=CR.ACT_LRELU, slope=0.1),
    "real_dgrad": dict(bias=False, dgrad=True, alpha=0.1, actgrad=1, res=True),
    "real_gelu": dict(act=CR.ACT_GELU, alpha=0.5, want_pre=True),
    "real_gelu_grad": dict(bias=False, dgrad=True, alpha=0.5, actgrad=3),
}
CHAIN_TABLE = ["bias_relu", "bias_lrelu_0.25", "conv0_lrelu_0.1", "res_alpha_0.125", "want_pre", "gelu_pre_only", "dgrad_plain", "dgrad_res", "dgrad_mask1",
               "dgrad_mask1_res", "dgrad_mask2"]  # ("plain" and "bias" come with the channel cases and the probes)
WSTAT_SIMPLE = ["bias_relu", "bias_lrelu_0.25", "conv0_lrelu_0.1", "bias_alpha_0.5"]              # FULL = 0 (and "plain", "bias")
WSTAT_FULL = ["res_alpha_0.125", "want_pre", "gelu_pre_only", "dgrad_res", "dgrad_mask1", "dgrad_mask1_res", "dgrad_mask2"]  # FULL = 1


class Case(NamedTuple):
    """One convolution.  kernel: the template instance the case is meant for.  Forward: sources of src_ch channels -> co outputs; the weight has
    o_total outputs (the pack takes [o0, o0 + co)) and i_total inputs (the single source IS the channel slice [src_off, + src_ch[0]) of an
    i_total-wide tensor).  Data gradient (the epilogue says so): src_ch = (K,) channels of dy, co = input channels of the weight (K, co, ks, ks).
    geom None: a weights-stationary case whose size follows from the grid (wstat_rows)."""
    kernel: tuple
    geom: Optional[Tuple[int, int, int]]
    src_ch: Tuple[int, ...]
    co: int
    epi: str = "bias"
    fallback: str = ""   # "wstat": hip.CONV_WSTAT is asked for although `kernel` is the general kernel; "mt2": mt = 2 is asked for, `kernel` has MT 1
    o_total: int = 0
    o0: int = 0
    i_total: int = 0
    src_off: int = 0
    probe: int = -1      # 0 .. ks * ks - 1: shift probe (one-hot weight, full-mantissa input)
    out_pad: int = 8     # out pixel stride = Cout rounded up to 8, + out_pad: 9 drives the element-wise epilogue, 12 only clears the plan's vec8
    family: str = ""     # "" = "full" for 3x3 up to 28 input channels, else "small"; "real": seeded normal values

    @property
    def ks(self):
        return self.kernel[2] if self.kernel[0] == IG else 3

    @property
    def fam(self):
        return self.family or ("full" if self.ks == 3 and sum(self.src_ch) <= 28 else "small")

    @property
    def id(self):
        s = "-".join(map(str, self.kernel)) + ("-fallback_from_" + self.fallback if self.fallback else "") + "-"
        s += ("x".join(map(str, self.geom)) if self.geom else "manytiles") + "-" + "+".join(map(str, self.src_ch)) + f"to{self.co}-{self.epi}"
        s += f"-o{self.o0}of{self.o_total}" if self.o_total else ""
        s += f"-i{self.src_off}of{self.i_total}" if self.i_total else ""
        s += f"-outpad{self.out_pad}" if self.out_pad != 8 else ""
        s += "-real" if self.family == "real" else ""
        return s + (f"-probe{self.probe}" if self.probe >= 0 else "")


# ---- what a case asks vmg_conv_fwd for, and what the plan must answer -------------------------------------------------------------------
def request(case):
    """(torch dtype, ks, cout_tiles, mt, route name) of the call."""
    k = case.kernel
    if k[0] == WSTAT:
        assert not case.fallback
        return torch.bfloat16, 3, k[1], 0, "wstat"
    dt = torch.bfloat16 if k[1] == "bf16" else torch.float32
    if case.fallback == "wstat":
        assert k[1] == "bf16" and k[2] == 3
        return dt, 3, k[4], k[3], "wstat"
    if case.fallback == "mt2":
        assert k[3] == 1 and (k[1] == "f32" or k[2] == 7)
        return dt, k[2], k[4], 2, "general"
    assert not case.fallback
    return dt, k[2], k[4], k[3], "general"


def vec8_of(case):
    """The rule of vmg_conv_fwd for the plan's vec8: bf16, no PixelShuffle, Cout % 16 == 0, every output-side row 16-byte aligned."""
    e = EPILOGUES[case.epi]
    return int(request(case)[0] == torch.bfloat16 and not e.get("pixel_shuffle") and case.co % 16 == 0 and layout(case).out_ps % 8 == 0)


def expected_plan(case):
    """The first seven ints of vmg_conv_fwd_plan for the instance the case names: family, dtype, ks, mt, ntb, variant, vec8 (include/vmg_hip.h)."""
    k = case.kernel
    if k[0] == IG:
        return (1, 1 if k[1] == "bf16" else 0, k[2], k[3], k[4], 0, vec8_of(case))
    return (5, 1, 3, 1, k[1], k[2] | k[3] << 4, 1)


def expected_grid(case, geom):
    """(grid x, grid y) of the general kernel: a workgroup per tile of 4 * MT rows x 16 pixels and per block of 16 * NTB output channels."""
    assert case.kernel[0] == IG
    N, H, W = geom
    mt, ntb = case.kernel[3], case.kernel[4]
    return N * -(-H // (4 * mt)) * -(-W // 16), -(-case.co // (16 * ntb))


WSTAT_FILL = (64, 8, 1024)  # 4096 tiles: a launch whose grid is the weights-stationary kernel's full one (a workgroup per compute unit)


def wstat_rows(grid):
    """(N, H, W) of a many-tile case for a full grid of `grid` workgroups: five tile columns (W = 75: the last one partial), the fewest tile rows
    that give at least 2 * grid + 1 tiles -- some workgroup then walks three -- and a tile count that is no multiple of 8; the last tile row is
    partial too (H = 8 * rows - 3)."""
    assert grid >= 8 and grid % 8 == 0
    rows = -(-(2 * grid + 1) // 5)
    while (5 * rows) % 8 == 0:
        rows += 1
    return (1, 8 * rows - 3, 75)


def wstat_walk(ntiles, grid):
    """conv_wstat_kernel's tile assignment: tiles per workgroup and tiles per XCD band.  Workgroup b belongs to XCD b % 8 and is number b // 8
    there; XCD j owns the band [j * band, min(ntiles, (j + 1) * band)), band = ceil(ntiles / 8), and its workgroup l walks tiles
    band0 + l, band0 + l + grid / 8, ..."""
    per_xcd, band = grid // 8, -(-ntiles // 8)
    bands = [max(0, min(ntiles, (j + 1) * band) - j * band) for j in range(8)]
    walks = [len(range(b // 8, bands[b % 8], per_xcd)) for b in range(grid)]
    assert sum(walks) == ntiles == sum(bands)
    return walks, bands


def assert_many_tiles(geom, grid):
    """The properties a many-tile case is there for, from the geometry and the grid of the launch."""
    N, H, W = geom
    ntiles = N * -(-H // 8) * -(-W // 16)
    walks, bands = wstat_walk(ntiles, grid)
    assert max(walks) >= 3, f"{geom} on {grid} workgroups: no workgroup walks three tiles"
    assert ntiles % 8 != 0 and len(set(bands)) > 1, f"{geom}: {ntiles} tiles give even XCD bands"
    assert W % 16 != 0 and H % 8 != 0
    return ntiles


class Layout(NamedTuple):
    src_ps: Tuple[int, ...]
    out_ch: int
    out_ps: int
    res_ps: int
    aux_ps: int


def layout(case):
    """Pixel strides (elements) of the embedded views; the GPU launch and the host-side plan test share them."""
    shuffle = EPILOGUES[case.epi].get("pixel_shuffle", False)
    oc = case.co // 4 if shuffle else case.co
    c8 = (oc + 7) // 8 * 8
    r8 = (case.co + 7) // 8 * 8
    return Layout(tuple((case.i_total or c) + 8 + 16 * (s % 2) for s, c in enumerate(case.src_ch)), oc, c8 + case.out_pad, r8 + 16, r8 + 24)


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
G3 = [(IG, "bf16", 3, 1), (IG, "bf16", 3, 2), (IG, "f32", 3, 1)]  # + (NTB,)
G7 = [(IG, "bf16", 7, 1), (IG, "f32", 7, 1)]

# (N, H, W): the smallest geometries at which the tiling can go wrong (tiles of 4 * MT rows x 16 pixels)
GEOMS = [(1, 1, 1),              # the image lies inside the halo
         (1, 4, 16), (1, 8, 16),  # one exact tile for MT 1 / MT 2
         (1, 5, 17), (1, 9, 17),  # one pixel into the next tile both ways
         (2, 7, 15),             # ragged tile; the halo must not read the other image
         (3, 5, 33), (1, 17, 3),
         (2, 16, 32),            # 16 / 8 workgroups: the xcd_remap branch for both MT
         (1, 24, 81)]            # 36 / 18 workgroups: no multiple of 8, more than the largest stage count of a source block (15; 7x7: 14)
GEOMS7 = GEOMS + [(1, 3, 3),     # every tap row is partly outside the image
                  (2, 6, 21)]    # the 22-pixel halo crosses a tile boundary
RAGGED = [(2, 7, 15), (3, 5, 33), (1, 17, 3)]
RAGGED7 = [(2, 7, 15), (1, 3, 3), (2, 6, 21)]
EPI_GEOMS = [(2, 7, 15), (3, 5, 33)]
WGEOMS = [(1, 1, 1), (1, 8, 16), (2, 7, 15),  # fewer tiles than workgroups
          (1, 17, 33),           # 3 x 3 tiles: the middle one takes the interior fast path of the halo copy, its eight neighbours the slow one
          (2, 18, 34),
          (2, 16, 32),           # the halo of tile (1, 1) ends one row and one pixel outside the image: the fast path's `<=` at its threshold
          (1, 9, 40)]            # a last partial column tile
WRAGGED = [(2, 7, 15), (1, 17, 33)]


def _rot(i, allowed):
    return allowed[i % len(allowed)]


def _uniq(cases):
    """(two lists of one table may name the same case: it runs once)"""
    return list(dict.fromkeys(cases))


def _ntbs(fam, src):
    """cout_tiles a family admits for these sources: fp32 stages are twice as large, and beside the halo tile of a block of more than 64
    channels only up to 5 tiles fit 160 KiB of LDS (kernels.cout_tiles_for gives fp32 at most 5 anyway)."""
    return (1, 3, 4, 5) if fam[1] == "f32" and max(src) > 64 else NTBS3


def _geometry_cases():
    """The full geometry list on one channel case per kernel family (40 channels: a 32-channel block and one more chunk)."""
    out = []
    for g in GEOMS:
        out += [Case(G3[0] + (9,), g, (40,), 144), Case(G3[1] + (5,), g, (40,), 144), Case(G3[2] + (5,), g, (40,), 80)]
    for g in GEOMS7:
        out += [Case(fam + (2,), g, (8,), 32) for fam in G7]
    return out


# 3x3 sources: 8 = one chunk and three padding chunks per k-step, 32 = exactly one block, 40 = block + one chunk, 320 = two 160-channel blocks;
# two sources: the halo tile is restaged between them
SRC3 = [(8,), (16,), (24,), (32,), (40,), (64,), (144,), (320,), (144, 144), (64, 8)]
# SPyNet's widths (models/vmg.py:126-173) and 40 -> 32, with the cout_tiles the product uses (kernels.cout_tiles_for(co, dtype, 7))
SPY = [((8,), 32, 2), ((32,), 64, 4), ((64,), 32, 2), ((32,), 16, 1), ((16,), 2, 1), ((40,), 32, 2)]


def _ntbs7(fam, src):
    """7x7, fp32: two stages of 4 tiles (112 KiB) do not fit beside the halo tile of a 64-channel source."""
    return (1, 2) if fam[1] == "f32" and max(src) > 40 else NTBS7


def _channel_cases():
    out = []
    i = 0
    for src in SRC3:
        for g in RAGGED:
            co = (144, 48, 80, 16)[i % 4]
            for f, fam in enumerate(G3):
                out.append(Case(fam + (_rot(i + 2 * f, _ntbs(fam, src)),), g, src, co, "bias" if i % 2 else "plain"))
            i += 1
    for f, fam in enumerate(G3):
        out += [Case(fam + (3,), (2, 7, 15), (144,), 144, i_total=176, src_off=16),   # a channel slice of a wider tensor, a K slice of a wider weight
                Case(fam + (5,), (2, 7, 15), (144,), 144, o_total=200, o0=40)]        # an output slice of a wider weight
    for src, co, tiles in SPY:
        for fam in G7:
            assert tiles in _ntbs7(fam, src)
            out += [Case(fam + (tiles,), g, src, co) for g in RAGGED7]                                           # the product's cout_tiles
            out += [Case(fam + (n,), RAGGED7[j % 3], src, co, "plain") for j, n in enumerate(_ntbs7(fam, src)) if n != tiles]  # the other admitted ones
    for fam in G7:
        out += [Case(fam + (2,), (2, 7, 15), (32,), 32, i_total=48, src_off=8), Case(fam + (2,), (2, 7, 15), (32,), 32, o_total=56, o0=16)]
    return _uniq(out)


def _cout_cases():
    out = []
    # Cout 3 (conv_last), 2 and 20: the element-wise epilogue, short last blocks (nt_real < NTB), a block that ends inside a 4-channel group
    for co in (3, 2, 20):
        for n in (1, 3, 4):
            for g in EPI_GEOMS:
                out += [Case(fam + (n,), g, (64,), co) for fam in G3]
    # a partial last cout block
    for g in EPI_GEOMS:
        for fam in G3:
            out += [Case(fam + (5,), g, (64,), 144), Case(fam + (3,), g, (64,), 112)]
    # Cout % 16 == 0 with an out pixel stride that is no multiple of 8: vec8 = 0 in the plan; + 9: the element-wise epilogue, + 12: the 4-channel one
    for fam in G3:
        n = 5 if fam[1] == "f32" else 9
        out += [Case(fam + (n,), (2, 7, 15), (64,), 144, "want_pre", out_pad=9), Case(fam + (n,), (2, 7, 15), (64,), 144, "res_alpha_0.125", out_pad=12),
                Case(fam + (n,), (2, 7, 15), (64,), 144, "dgrad_mask2", out_pad=9)]
    # PixelShuffle (upconv1 / upconv2): Cout 256 and 12
    for fam in G3:
        n = 4 if fam[1] == "f32" else 8
        for g in [(2, 7, 15), (1, 5, 17)]:
            out += [Case(fam + (n,), g, (64,), 256, "pixel_shuffle"), Case(fam + (1,), g, (64,), 12, "pixel_shuffle_0.1")]
        out += [Case(fam + (n,), (2, 7, 15), (64,), 256, "pixel_shuffle_0.1"), Case(fam + (1,), (2, 7, 15), (64,), 12, "pixel_shuffle")]
    # what mt = 2 silently becomes for fp32 and for 7x7
    out += [Case((IG, "f32", 3, 1, 5), (1, 9, 17), (40,), 80, fallback="mt2"), Case((IG, "bf16", 7, 1, 2), (1, 9, 17), (8,), 32, fallback="mt2"),
            Case((IG, "f32", 7, 1, 2), (1, 9, 17), (8,), 32, fallback="mt2")]
    return _uniq(out)


# (kernel, sources, Cout): both epilogue paths of the general kernel -- Cout % 16 == 0 takes the 4-channel vector path, Cout 20 / 2 the element-wise one
EPI_KERNELS = [((IG, "bf16", 3, 1, 9), (144,), 144), ((IG, "bf16", 3, 2, 3), (144,), 144), ((IG, "f32", 3, 1, 5), (144,), 80),
               ((IG, "bf16", 3, 1, 3), (64,), 20), ((IG, "bf16", 3, 2, 1), (64,), 20), ((IG, "f32", 3, 1, 4), (64,), 20),
               ((IG, "bf16", 7, 1, 4), (32,), 64), ((IG, "f32", 7, 1, 1), (32,), 16), ((IG, "bf16", 7, 1, 1), (16,), 2), ((IG, "f32", 7, 1, 2), (16,), 20)]


def _epilogue_cases():
    out = []
    for k, src, co in EPI_KERNELS:
        for name in CHAIN_TABLE:
            out += [Case(k, g, src, co, name) for g in EPI_GEOMS]
    # data gradients whose weight is not square (a transposition that mixes up O and I shows): dy of 112 channels -> dx of 144 / 80 ...
    out += [Case(k, EPI_GEOMS[0], (112,), co, "dgrad_mask1_res") for k, _, co in EPI_KERNELS[:3]]
    # ... and SPyNet's own data-gradient packs: 8 <- 32, 32 <- 64, 64 <- 32, 32 <- 16 (Cout of the pack = input channels of the conv)
    for fam in G7:
        for g in RAGGED7:
            out += [Case(fam + (1,), g, (32,), 8, "dgrad_plain"), Case(fam + (2,), g, (64,), 32, "dgrad_plain"),
                    Case(fam + (4,), g, (32,), 64, "dgrad_plain"), Case(fam + (2,), g, (16,), 32, "dgrad_res")]
    return _uniq(out)


PROBE_GEOM = (2, 7, 15)
PROBES7 = (0, 16, 32, 48)  # a 16-channel tile meets taps t .. t + 15 (mod 49) in probe t: four probes meet all 49
# (kernel, sources, Cout) of the probed channel cases
PROBED = [((IG, "bf16", 3, 1, 9), (144,), 144), ((IG, "bf16", 3, 2, 9), (144, 144), 144), ((IG, "f32", 3, 1, 5), (64, 8), 80),
          ((IG, "bf16", 7, 1, 2), (8,), 32), ((IG, "f32", 7, 1, 2), (64,), 32), ((IG, "bf16", 7, 1, 4), (32,), 64), ((IG, "f32", 7, 1, 4), (32,), 64)]
WPROBE_GEOM = (1, 17, 33)  # (the interior fast path and the slow path of the halo copy)
WPROBED = [((WSTAT, 1, 1, 0), (8,), 16), ((WSTAT, 3, 1, 0), (24,), 48), ((WSTAT, 4, 1, 0), (32,), 64), ((WSTAT, 1, 2, 0), (40,), 16),
           ((WSTAT, 3, 2, 0), (64,), 48), ((WSTAT, 4, 2, 0), (64,), 64)]


def _probe_cases():
    out = []
    for k, src, co in PROBED:
        out += [Case(k, PROBE_GEOM, src, co, "plain", probe=t) for t in (range(9) if k[2] == 3 else PROBES7)]
    for k, src, co in WPROBED:
        out += [Case(k, WPROBE_GEOM, src, co, "plain", probe=t) for t in range(9)]
    return out


def probe_taps_missing(cases):
    """{(kernel, sources, Cout, 16-channel output tile): taps that no probe of that channel case meets} -- empty for a sound table."""
    seen = {}
    for c in cases:
        if c.probe < 0:
            continue
        _, _, tap = CR.one_hot_weight(c.co, sum(c.src_ch), c.probe, c.ks)
        for tile in range(-(-c.co // 16)):
            seen.setdefault((c.kernel, c.src_ch, c.co, tile), set()).update(tap[16 * tile:16 * tile + 16].tolist())
    return {k: sorted(set(range(k[0][2] ** 2 if k[0][0] == IG else 9)) - v) for k, v in seen.items() if len(v) != (k[0][2] ** 2 if k[0][0] == IG else 9)}


def _nb(ci):
    return 1 if ci <= 32 else 2


def _wstat_cases():
    out = []
    # the full geometry list on the HR head's own shapes (HRconv 64 -> 64; conv_last's data gradient 8 -> 64) and on the narrowest one
    for g in WGEOMS:
        for src, co in (((64,), 64), ((8,), 16)):
            k = (WSTAT, co // 16, _nb(src[0]))
            out += [Case(k + (0,), g, src, co, "bias_relu"), Case(k + (1,), g, src, co, "res_alpha_0.125")]
        out += [Case((WSTAT, 4, 1, 1), g, (8,), 64, "dgrad_mask1_res")]
    # input channels 8 .. 64 (NB 1 and 2, chunk counts below a full block) x output channels 16, 48, 64
    i = 0
    for ci in (8, 24, 32, 40, 64):
        for co in (16, 48, 64):
            for g in WRAGGED:
                k = (WSTAT, co // 16, _nb(ci))
                out += [Case(k + (0,), g, (ci,), co, "bias" if i % 2 else "plain"), Case(k + (1,), g, (ci,), co, "dgrad_res" if i % 2 else "res_alpha_0.125")]
                i += 1
    # several output-channel blocks, the last one short (the kernel takes them although the model never asks)
    for g in WRAGGED:
        out += [Case((WSTAT, 3, 2, 0), g, (64,), 80, "bias_relu"), Case((WSTAT, 3, 2, 1), g, (64,), 80, "want_pre"),
                Case((WSTAT, 4, 1, 0), g, (32,), 128, "bias_relu"), Case((WSTAT, 4, 1, 1), g, (32,), 128, "res_alpha_0.125")]
    out += [Case((WSTAT, 4, 2, 0), (1, 17, 33), (64,), 64, i_total=96, src_off=16), Case((WSTAT, 4, 2, 1), (1, 17, 33), (64,), 64, "res_alpha_0.125", o_total=100, o0=20)]
    # the epilogues: FULL = 0 has bias / ReLU / LeakyReLU / alpha only, FULL = 1 everything else
    for src, co in (((64,), 64), ((32,), 48), ((8,), 16)):
        k = (WSTAT, co // 16, _nb(src[0]))
        for g in WRAGGED:
            out += [Case(k + (0,), g, src, co, name) for name in WSTAT_SIMPLE] + [Case(k + (1,), g, src, co, name) for name in WSTAT_FULL]
    # many tiles per workgroup on the narrowest channels
    out += [Case((WSTAT, 1, 1, 0), None, (8,), 16, "bias_relu"), Case((WSTAT, 1, 1, 1), None, (8,), 16, "want_pre")]
    # what the hint does not cover runs the general kernel
    g = (2, 7, 15)
    out += [Case((IG, "bf16", 3, 1, 4), g, (72,), 64, fallback="wstat"),                          # more than 64 input channels
            Case((IG, "bf16", 3, 1, 4), g, (32, 32), 64, fallback="wstat"),                       # two sources
            Case((IG, "bf16", 3, 1, 4), g, (64,), 64, "res_alpha_0.125", fallback="wstat", out_pad=12),  # rows that are not 16-byte aligned
            Case((IG, "bf16", 3, 1, 4), g, (64,), 64, "pixel_shuffle", fallback="wstat"),
            Case((IG, "bf16", 3, 1, 5), g, (64,), 80, fallback="wstat"),                          # cout_tiles 5
            Case((IG, "bf16", 3, 2, 4), g, (64,), 64, fallback="wstat")]                          # mt = 2 asked for
    return _uniq(out)


def exact_cases():
    return _geometry_cases() + _channel_cases() + _cout_cases() + _epilogue_cases() + _probe_cases() + _wstat_cases()


def _real_cases():
    out = []
    for g in [(2, 7, 15), (1, 24, 81)]:
        out += [Case((IG, "bf16", 3, 1, 9), g, (144,), 144, "real_res", family="real"), Case((IG, "bf16", 3, 2, 9), g, (144,), 144, "real_res", family="real"),
                Case((IG, "bf16", 3, 1, 9), g, (144, 144), 144, "real_lrelu", family="real"), Case((IG, "bf16", 3, 2, 1), g, (64,), 3, "real_res", family="real"),
                Case((IG, "bf16", 3, 1, 9), g, (144,), 144, "real_dgrad", family="real"),
                Case((IG, "f32", 3, 1, 5), g, (144,), 144, "real_res", family="real"), Case((IG, "f32", 3, 1, 1), g, (64,), 3, "real_lrelu", family="real"),
                Case((IG, "bf16", 7, 1, 4), g, (32,), 64, "real_res", family="real"), Case((IG, "bf16", 7, 1, 2), g, (64,), 32, "real_lrelu", family="real"),
                Case((IG, "f32", 7, 1, 4), g, (32,), 64, "real_res", family="real"), Case((IG, "f32", 7, 1, 2), g, (64,), 32, "real_dgrad", family="real")]
    for g in [(2, 7, 15), (2, 18, 34)]:
        out += [Case((WSTAT, 4, 2, 1), g, (64,), 64, "real_res", family="real"), Case((WSTAT, 4, 2, 0), g, (64,), 64, "real_lrelu", family="real"),
                Case((WSTAT, 4, 1, 1), g, (8,), 64, "real_dgrad", family="real"), Case((WSTAT, 3, 1, 0), g, (32,), 48, "real_lrelu", family="real")]
    return out


def _gelu_cases():
    out = []
    for k, src, co in [((IG, "bf16", 3, 1, 9), (144,), 144), ((IG, "bf16", 3, 2, 3), (144,), 144), ((IG, "bf16", 7, 1, 4), (32,), 64), ((WSTAT, 4, 2, 1), (64,), 64)]:
        out += [Case(k, (2, 7, 15), src, co, "real_gelu", family="real"), Case(k, (2, 7, 15), src, co, "real_gelu_grad", family="real")]
    return out


def all_cases():
    return exact_cases() + _real_cases() + _gelu_cases()


def exact_args(case):
    """The arguments of conv_ref.assert_exact for a case (taps among them)."""
    e = EPILOGUES[case.epi]
    scales = [e["slope"]] if e.get("act") == CR.ACT_LRELU else []
    scales.append(e.get("alpha", 1.0))
    if e.get("actgrad") == 2:
        scales.append(e["slope"])
    return case.fam, sum(case.src_ch), e.get("bias", True), e.get("res", False), tuple(scales), case.ks ** 2


# ---- operands and expected values -------------------------------------------------------------------------------------------------------
def _mods():
    from vmg_amd import hip, kernels as K
    return hip, K


def _seed(geom, case):
    return (geom[0] * 7919 + geom[1] * 104729 + geom[2] * 1299709 + sum(case.src_ch) * 31 + case.co * 17 + len(case.src_ch) + case.ks) % (2 ** 31 - 1)


def _values(shape, seed, family, f32=False):
    """Operand values: the exact families, or ("real") seeded normal values -- bf16 numbers for the bf16 kernels, any fp32 for the fp32 ones."""
    if family == "real":
        v = torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed))
        return v if f32 else v.bfloat16().float()
    return WR.exact_values(shape, seed, family)


@functools.lru_cache(maxsize=16)
def _operands(geom, ks, src_ch, co, family, o_total, o0, i_total, src_off, dgrad, probe, f32):
    """The CPU side that the epilogues and kernels of a (geometry, channel case) share: sources (wide, where the source is a slice), weight, the
    fp64 sums and, for real-valued cases, the sums of the magnitudes."""
    seed = _seed(geom, Case((IG, "", ks), geom, src_ch, co))
    ci, taps = sum(src_ch), ks * ks
    wide = [_values(geom + (i_total or c,), seed + 11 * s, "real" if probe >= 0 else family, f32) for s, c in enumerate(src_ch)]
    assert not i_total or len(src_ch) == 1
    srcs = [t[..., src_off:src_off + c] if i_total else t for t, c in zip(wide, src_ch)]
    real = family == "real"

    def scaled(w):
        return w if not real else (w / (taps * ci) ** 0.5 if f32 else (w / (taps * ci) ** 0.5).bfloat16().float())
    if dgrad:
        assert len(src_ch) == 1 and not (o_total or i_total or probe >= 0)
        w = scaled(_values((ci, co, ks, ks), seed + 101, family, f32))
        return wide, srcs, w, CR.dgrad_ref(srcs[0], w), (CR.dgrad_ref(srcs[0].abs(), w.abs()) if real else None)
    if probe >= 0:
        w, pi, ptap = CR.one_hot_weight(co, ci, probe, ks)
        acc = CR.conv_ref(srcs, w)
        assert torch.equal(acc, CR.shifted_copy(torch.cat(srcs, -1), pi, ptap, ks).double())  # the probe's reference IS the shifted copy
        return wide, srcs, w, acc, None
    w = scaled(_values((o_total or co, i_total or ci, ks, ks), seed + 101, family, f32))
    kw = dict(src_off=[src_off] if i_total else None, o0=o0, on=co)
    return wide, srcs, w, CR.conv_ref(srcs, w, **kw), (CR.conv_ref([s.abs() for s in srcs], w.abs(), **kw) if real else None)


class _Problem:
    """One convolution with its epilogue: CPU operands, the expected results in the kernel's type (exact) or the fp64 value and bound (real)."""

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
            args = exact_args(case)
            CR.assert_exact(*args[:5], taps=args[5])  # the invariant, before anything runs on the GPU
        values_f32 = f32 and (self.real or case.probe >= 0)
        self.wide, self.srcs, self.w, acc, mag = _operands(geom, case.ks, case.src_ch, case.co, fam, case.o_total, case.o0, case.i_total, case.src_off,
                                                           self.dgrad, case.probe, values_f32)
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
            self.want = self.want_pre_value = None  # (the GELU test computes its own)
            if not self.real:
                _, self.want_pre_value = CR.epilogue_ref(acc, self.bias, act=CR.ACT_GELU, out_dtype=dt)
            return
        out, pre = CR.epilogue_ref(acc, self.bias, aux=self.aux, res=self.res, exact=not self.real, out_dtype=dt, **e)
        if self.pixel_shuffle:
            out = CR.pixel_shuffle_ref(out)
        self.want, self.want_pre_value = out, pre
        if self.real:
            S = mag + (self.bias.abs().double() if self.bias is not None else 0) + (self.res.abs().double() if self.res is not None else 0)
            self.bound = CR.real_bound(out, S, sum(case.src_ch), taps=case.ks ** 2, out_dtype=dt)


def _name(idx, case):
    n, y, x, o = idx
    s = f"image {n}, pixel ({y}, {x}), output channel {o}"
    if case.probe >= 0:
        ks = case.ks
        _, pi, ptap = CR.one_hot_weight(case.co, sum(case.src_ch), case.probe, ks)
        s += f" = the copy of input channel {int(pi[o])} through tap (ky, kx) = ({int(ptap[o]) // ks}, {int(ptap[o]) % ks})"
    return s


def _assert_same(got, want, what, case):
    n, idx, g, w = WR.first_mismatch(got, want)
    if n:
        where = _name(idx, case) if not EPILOGUES[case.epi].get("pixel_shuffle") else f"shuffled element {idx}"
        err, top = float((got.double() - want.double()).abs().max()), float(want.double().abs().max())
        raise AssertionError(f"{what}: {n} of {got.numel()} elements differ from the fp64 reference, the first at {where}: got {g!r}, want "
                             f"{w!r} (largest error {err:g}; 2e-2 of the largest value: {2e-2 * max(1.0, top):g})")
    assert torch.equal(got, want), what


def _full_grid(case):
    """The grid the plan reports for a weights-stationary launch of this channel case that fills the device."""
    hip, K = _mods()
    N, H, W = WSTAT_FILL
    pw = K.pack_conv_weight(torch.zeros(case.co, case.src_ch[0], 3, 3, device="cuda"), torch.bfloat16, cout_tiles=case.kernel[1])
    x = torch.empty(N, H, W, case.src_ch[0], dtype=torch.bfloat16, device="cuda")
    plan = K.conv_forward_plan([x], pw, None, N, H, W, deep=hip.CONV_WSTAT)
    assert plan.family == hip.CONV_FAM_WSTAT, plan
    return plan.grid_x


def _geom(case):
    return case.geom if case.geom is not None else wstat_rows(_full_grid(case))


def _launch(prob):
    """Pack, embed, ask the plan, launch twice.  Returns (out, out_pre or None) as CPU tensors after the checks every case shares: the plan names
    the case's instance, no NaN left inside, nothing changed outside the views, the same bits from the second launch."""
    hip, K = _mods()
    assert (hip.ACT_NONE, hip.ACT_RELU, hip.ACT_LRELU, hip.ACT_GELU) == (CR.ACT_NONE, CR.ACT_RELU, CR.ACT_LRELU, CR.ACT_GELU)
    case, (N, H, W) = prob.case, prob.geom
    dt, ks, tiles, mt, route = request(case)
    deep = dict(general=hip.CONV_GENERAL, wstat=hip.CONV_WSTAT)[route]
    lay = layout(case)
    bits = torch.int16 if dt == torch.bfloat16 else torch.int32
    guard = 12 * W + 40  # pixels: more than a tile with its halo could reach past either end of the image
    dev = "cuda"
    srcs = []
    for t, c, ps in zip(prob.wide, case.src_ch, lay.src_ps):
        v = WR.embed(t.to(dt), ps, guard, device=dev)
        assert v.stride(-2) > t.shape[-1] and torch.equal(v.float().cpu(), t)  # the values are numbers of the kernel's type
        srcs.append(v[..., case.src_off:case.src_off + c] if case.i_total else v)
    w = prob.w.to(dev).contiguous()
    assert tuple(w.shape[2:]) == (ks, ks) and (dt == torch.float32 or torch.equal(w.bfloat16().float(), w))
    pw = K.pack_conv_weight(w, dt, src_ch=list(case.src_ch), src_off=[case.src_off] if case.i_total else None, o0=case.o0, on=case.co,
                            transpose_flip=prob.dgrad, cout_tiles=tiles)
    assert pw.layout == "std" and pw.ks == ks and pw.cout_tiles == tiles and pw.cout == case.co and pw.src_ch == list(case.src_ch)
    emb = lambda t, ps: WR.embed(t.to(dt), ps, guard, device=dev)  # noqa: E731
    res = emb(prob.res, lay.res_ps) if prob.res is not None else None
    aux = emb(prob.aux, lay.aux_ps) if prob.aux is not None else None
    oshape = (N, 2 * H, 2 * W, lay.out_ch) if prob.pixel_shuffle else (N, H, W, lay.out_ch)
    blank = torch.full(oshape, float("nan"), dtype=dt)
    outs = [emb(blank, lay.out_ps)] + ([emb(blank, lay.out_ps)] if prob.want_pre else [])
    assert all(o.stride(-2) > o.shape[-1] for o in outs + [t for t in (res, aux) if t is not None])
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
        if case.kernel[0] == IG:
            assert (plan.grid_x, plan.grid_y) == expected_grid(case, prob.geom), f"{what}: {plan}"
        elif case.geom is None:
            assert_many_tiles(prob.geom, plan.grid_x)  # (the grid of this very launch)
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
            where = _name(first, case) if not prob.pixel_shuffle else f"shuffled element {first}"
            raise AssertionError(f"{what}{(': out', ': out_pre')[k]}: {int(nan.sum())} of {g.numel()} elements are NaN, the first at {where}: "
                                 "something outside the operands was read, or the element was never written")
    return got[0], (got[1] if prob.want_pre else None)


@functools.lru_cache(maxsize=4)
def _problem(geom, case):
    return _Problem(geom, case)


def _prob(case):
    """(the expected values depend on the kernel's dtype and ks only: instances of one dtype share them)"""
    dt = request(case)[0]
    key = case._replace(kernel=(IG, "f32" if dt == torch.float32 else "bf16", case.ks, 1, 1), geom=None, fallback="", out_pad=8)
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


@pytest.mark.parametrize("case", _geometry_cases(), ids=_ids(_geometry_cases()))
def test_geometries(case):
    _run_exact(case)


@pytest.mark.parametrize("case", _channel_cases(), ids=_ids(_channel_cases()))
def test_input_channels(case):
    _run_exact(case)


@pytest.mark.parametrize("case", _cout_cases(), ids=_ids(_cout_cases()))
def test_output_channels_and_pixel_shuffle(case):
    _run_exact(case)


@pytest.mark.parametrize("case", _epilogue_cases(), ids=_ids(_epilogue_cases()))
def test_epilogues(case):
    _run_exact(case)


@pytest.mark.parametrize("case", _probe_cases(), ids=_ids(_probe_cases()))
def test_shift_probes(case):
    _run_exact(case)


@pytest.mark.parametrize("case", _wstat_cases(), ids=_ids(_wstat_cases()))
def test_weights_stationary(case):
    _run_exact(case)


# ------------------------------------------------------------------------------------------------------------------------------------
# real-valued cases: the per-element bound
# ------------------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("case", _gelu_cases(), ids=_ids(_gelu_cases()))
def test_gelu_epilogues_within_the_bound(case):
    """|got - gelu(v) * alpha| <= 2^-8 (|g| + E) + E with E = alpha * (1.13 * e32 + EG), the masked gradient with E = alpha * (1.13 * e32 + |v| * EGRAD)
    (tests/test_linear_kernels_gpu.py: 1.13 bounds sup |gelu'|, EG / EGRAD the device functions' absolute error)."""
    prob = _prob(case)
    out, pre = _launch(prob)
    alpha, ci, taps = prob.kw["alpha"], sum(case.src_ch), case.ks ** 2
    v = prob.acc if prob.bias is None else prob.acc + prob.bias.double()
    S = prob.mag + (prob.bias.abs().double() if prob.bias is not None else 0)
    e32 = CR.sum_bound(S, ci, taps=taps)
    if prob.want_pre:
        _assert_bound(pre, v, CR.real_bound(v, S, ci, taps=taps), case.id + ": out_pre", case)
    if prob.kw.get("actgrad") == 3:
        g = alpha * v * CR.gelu_grad_ref(prob.aux)
        E = alpha * (1.13 * e32 + v.abs() * EGRAD)
    else:
        g = alpha * CR.gelu_ref(v)
        E = alpha * (1.13 * e32 + EG)
    _assert_bound(out, g, 2.0 ** -8 * (g.abs() + E) + E, case.id + ": out", case)
