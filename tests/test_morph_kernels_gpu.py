"""The MorphFC kernels of vmg_amd/csrc/morphfc.hip, every instance and route, element by element against tests/morph_ref.py (fp64, index
arithmetic from the definition).

Fused kernel (vmg_morphfc_fwd, morph_linear_kernel<NK, NCT, EVEN, MASK>).  FUSED is the case table: every (Cp, chunk) pair the product can ask
for -- Cp 144, 112, 64, 32, 16 x chunk 8, 16 -- in the plain form (forward: bias, ReLU, in_scale 1) and the mask form (data gradient: no bias,
no ReLU, the mask holds both signs, +0.0 and -0.0), on both axes, at the geometries that reach each edge: a line of 1 and of 3 positions, a
chunk multiple, remainders 1 and chunk - 1, C < Cp, an odd number of groups at chunk 8 (the last tile's second group is dead), one tile, and
more than 8 * nwg tiles, so that a wave's LDS blocks are used for a second tile (sized from the device's compute units; the last tile partial).
  * exact cases: operands k * 2^-7, |k| <= 255, power-of-two scales: every partial sum in any order is an fp32 number
    (conv_ref.assert_exact), so the output must be the correctly rounded bf16 of the fp64 value, bit for bit, and the token side output the
    reference's token matrix, bit for bit, with zero rows past the last group;
  * permutation probes: a one-hot weight copies one token feature per output feature, exact for any finite input; operands are random bit
    patterns over all normal bf16 numbers and both zeros (0 x Inf or NaN would poison the sum; what the matrix unit does with subnormals is
    no property of this kernel);
  * real-valued cases: seeded normal values, the product's scales (1 / Cp), held per element to conv_ref.real_bound (derived, not measured).
Token kernels (vmg_morph_tokens_gather / _scatter, LDS-tiled and element-wise, bf16 and fp32): permutations, compared as integers over all bit
patterns.  TOKENS is the case table; each case names the route it is meant for and, on the element-wise route, the condition that sends it there.
Autograd level (functional.morph_linear): fused and general path, "small" family, both weight-gradient modes.

Every case asserts the plan's instance / route before it launches; inputs and outputs are contiguous slices of sentinel-filled allocations
(NaN, or a fixed bit pattern for the permutations) with guards before and after; every case launches twice into re-filled outputs: the same
bits both times, nothing outside the views changed, no sentinel left inside (the fused cases a third time without the token side output: the
same output, the token allocation untouched).  tests/test_morph_plan.py checks the tables against the plan
functions without a GPU.

Measured on an MI355X (256 compute units): the whole module, 391 cases, runs in about 5 s; the slowest cases are the first one of each kind
(0.8 s, 0.5 s: library load and first launches) and the loop cases (0.05 .. 0.2 s).  Worst |got - v| / bound of the real-valued cases (the bf16
store's half ulp, 2^-8 |v| just above a power of two, is most of the bound, so values near 1 are expected):
    real-144-8-plain-w-loops 0.986    real-144-16-mask-h 0.968    real-112-16-plain-h 0.970    real-112-8-mask-w 0.985    real-64-8-plain-h 0.982
    real-64-16-mask-w 0.985           real-32-16-plain-h 0.986    real-32-8-mask-w 0.980       real-16-8-plain-h 0.986    real-16-16-mask-w 0.978"""
import collections
import functools
import math

import pytest
import torch

from tests import conv_ref as CR
from tests import morph_ref as MR
from tests import wgrad_ref as WR

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
# ---- the instances, by hand: morph_linear_kernel<NK, NCT, EVEN, MASK>; NK = ceil(Cp / 32), NCT = ceil(Cp / 16), EVEN: S = Cp / chunk is even
NK_NCT = {144: (5, 9), 112: (4, 7), 64: (2, 4), 32: (1, 2), 16: (1, 1)}
S_EVEN = {(144, 8): True, (144, 16): False, (112, 8): True, (112, 16): False, (64, 8): True, (64, 16): True, (32, 8): True, (32, 16): True,
          (16, 8): True, (16, 16): False}
PAIRS = tuple(S_EVEN)
IN_SCALE, OUT_SCALE = 2.0 ** -3, 2.0 ** -7  # the exact cases' scales (the mask form scales on the way in, the plain form on the way out)

Fused = collections.namedtuple("Fused", "id Cp chunk C axis geom form kind tags")  # geom: (B, T, H, W), or None: sized from the CU count (loops)


def instance(case):
    """(NK, NCT, EVEN, MASK) the case is meant for."""
    return NK_NCT[case.Cp] + (S_EVEN[(case.Cp, case.chunk)], case.form == "mask")


def _hw(axis, length, lines):
    return (length, lines) if axis == "h" else (lines, length)


def loop_geometry(chunk, axis, ncu):
    """(B, T, H, W) with just more than 8 * ncu tiles (every workgroup of the ncu-capped grid owns 8 waves, so the first waves own two tiles), lines
    of 2 * chunk + 1 positions (three groups, the third with ONE live position: the wave that took a full group first must see zeros, not that
    group's pixels), and at chunk 8 an odd number of groups (the last tile's second group is dead)."""
    G = 16 // chunk
    lines = -(-(G * 8 * ncu + 1) // 3)
    if G == 2 and lines % 2 == 0:
        lines += 1
    return (1, 1) + _hw(axis, 2 * chunk + 1, lines)


def geometry(case, ncu):
    return case.geom if case.geom is not None else loop_geometry(case.chunk, case.axis, ncu)


def _fused_table():
    t = []
    for Cp, chunk in PAIRS:
        # (name, (B, T), lines, line length, C, tags).  "dead group": chunk 8 and B * T * lines * ceil(length / chunk) odd
        edges = [("len1", (1, 3), 3, 1, Cp, ()), ("len3", (3, 1), 3, 3, Cp, ()), ("multiple", (1, 3), 3, 2 * chunk, Cp, ()),
                 ("rem1", (1, 3), 3, 2 * chunk + 1, Cp, ("dead group",) if chunk == 8 else ()),
                 ("remcm1", (3, 1), 3, 3 * chunk - 1, Cp, ()),
                 ("cpad", (1, 3), 3, 2 * chunk + 1, Cp - 8, ("channel padding",)),
                 ("single", (1, 1), 1, chunk, Cp, ("single tile",) + (("dead group",) if chunk == 8 else ()))]
        if chunk == 8:
            edges.append(("dead17x5", (1, 1), 5, 17, Cp, ("dead group",)))
        for form in ("plain", "mask"):
            for axis in ("h", "w"):
                for name, bt, lines, length, C, tags in edges:
                    t.append(Fused(f"exact-{Cp}-{chunk}-{form}-{axis}-{name}", Cp, chunk, C, axis, bt + _hw(axis, length, lines), form, "exact", tags))
    # more tiles than waves: once per reachable (NK, NCT, EVEN) in the plain form, Cp 144 in both parities in the mask form (there with C < Cp)
    for i, (Cp, chunk) in enumerate([(144, 8), (144, 16), (112, 8), (112, 16), (64, 8), (32, 16), (16, 8), (16, 16)]):
        t.append(Fused(f"exact-{Cp}-{chunk}-plain-{'hw'[i % 2]}-loops", Cp, chunk, Cp, "hw"[i % 2], None, "plain", "exact",
                       ("loops",) + (("dead group",) if chunk == 8 else ())))
    for i, (Cp, chunk) in enumerate([(144, 8), (144, 16)]):
        t.append(Fused(f"exact-{Cp}-{chunk}-mask-{'wh'[i % 2]}-loops", Cp, chunk, Cp - 8, "wh"[i % 2], None, "mask", "exact",
                       ("loops", "channel padding") + (("dead group",) if chunk == 8 else ())))
    # permutation probes: every pair, both axes, two probes
    for Cp, chunk in PAIRS:
        for p, axis in enumerate(("h", "w")):
            t.append(Fused(f"probe{p}-{Cp}-{chunk}-{axis}", Cp, chunk, Cp if p else Cp - 8, axis, (1, 2) + _hw(axis, 2 * chunk + 3, 3), "plain", f"probe{p}",
                           ("channel padding",) if not p else ()))
    # real values: one per Cp in each form, the chunks and axes alternating; Cp 144 plain through a loop case
    t.append(Fused("real-144-8-plain-w-loops", 144, 8, 144, "w", None, "plain", "real", ("loops", "dead group")))
    t.append(Fused("real-144-16-mask-h", 144, 16, 136, "h", (1, 2, 35, 3), "mask", "real", ("channel padding",)))
    for i, Cp in enumerate((112, 64, 32, 16)):
        c1, c2 = (8, 16) if i % 2 else (16, 8)
        t.append(Fused(f"real-{Cp}-{c1}-plain-h", Cp, c1, Cp, "h", (1, 2, 2 * c1 + 3, 5), "plain", "real", ()))
        t.append(Fused(f"real-{Cp}-{c2}-mask-w", Cp, c2, Cp - 8, "w", (2, 1, 3, 2 * c2 + 5), "mask", "real", ("channel padding",)))
    assert len({c.id for c in t}) == len(t)
    return t


FUSED = _fused_table()
_FUSED_BY_ID = {c.id: c for c in FUSED}

# ---- token kernels.  route: 1 = LDS-tiled, 0 = element-wise; cause (element-wise only): "C" (C % vn), "ld" (ld % vn), "lds" (chunk * ld * es > 64 KiB),
# "align" (the feature map starts `off` elements past a 16-byte boundary); vn = 8 (bf16) / 4 (fp32) elements.  sole: no other condition holds.
Tok = collections.namedtuple("Tok", "id dtype axis chunk C Cp ld geom off route cause sole note")
LDS_ROUTE, ELEMENT_ROUTE = 1, 0


def _token_table():
    t = []

    def add(name, dtype, chunk, C, Cp, ld, geom, axes, route, cause=None, sole=False, off=0, note=""):
        for axis in axes:
            B, H, W = geom
            if len(axes) == 1 and axis == "h":
                H, W = W, H
            t.append(Tok(f"{'bf16' if dtype == BF16 else 'fp32'}-{name}-{axis}", dtype, axis, chunk, C, Cp, ld, (B, H, W), off, route, cause, sole, note))
    hw = ("h", "w")
    # LDS route: S = 1, 2, 3; chunk * lvec below and above the 256 threads; ld > Cp (zero features); C < Cp
    add("s1", BF16, 8, 8, 8, 8, (2, 9, 10), hw, LDS_ROUTE, note="S 1, 8 vectors")
    add("s2", BF16, 8, 16, 16, 16, (2, 9, 17), hw, LDS_ROUTE, note="S 2")
    add("s3", BF16, 8, 16, 24, 24, (2, 7, 9), hw, LDS_ROUTE, note="S 3, C < Cp")
    add("wide", BF16, 16, 440, 448, 448, (2, 17, 17), hw, LDS_ROUTE, note="896 vectors > 256 threads")
    add("cp228", BF16, 12, 224, 228, 232, (1, 13, 25), hw, LDS_ROUTE, note="348 vectors, ld > Cp")
    add("s1", F32, 8, 8, 8, 8, (2, 9, 10), hw, LDS_ROUTE, note="S 1")
    add("s2", F32, 4, 8, 8, 8, (2, 5, 9), hw, LDS_ROUTE, note="S 2")
    add("s3", F32, 4, 8, 12, 12, (2, 6, 7), hw, LDS_ROUTE, note="S 3, C < Cp")
    add("wide", F32, 16, 224, 224, 224, (1, 17, 18), hw, LDS_ROUTE, note="896 vectors > 256 threads")
    add("groups", BF16, 3, 8, 9, 16, (1, 130, 400), ("w",), LDS_ROUTE, note="17420 groups > 16384 workgroups")
    add("groups", F32, 3, 8, 9, 12, (1, 130, 400), ("w",), LDS_ROUTE, note="17420 groups > 16384 workgroups")
    # element-wise route, one cause each
    add("c12", BF16, 4, 12, 16, 16, (2, 5, 9), hw, ELEMENT_ROUTE, "C", True)
    add("c6", F32, 4, 6, 8, 8, (2, 5, 9), hw, ELEMENT_ROUTE, "C", True)
    add("ld228", BF16, 12, 224, 228, 228, (1, 13, 25), hw, ELEMENT_ROUTE, "ld", True)
    add("ld9", F32, 3, 8, 9, 9, (2, 4, 7), hw, ELEMENT_ROUTE, "ld", True)
    for ax in hw:  # (two lines of two groups on either axis)
        add("lds", BF16, 112, 448, 448, 448, (1, 2, 113), (ax,), ELEMENT_ROUTE, "lds", True, note="112 * 448 * 2 B = 98 KiB")
        add("lds", F32, 64, 448, 448, 448, (1, 2, 65), (ax,), ELEMENT_ROUTE, "lds", True, note="64 * 448 * 4 B = 112 KiB")
    add("off1", BF16, 8, 16, 16, 16, (2, 9, 17), hw, ELEMENT_ROUTE, "align", True, off=1)
    add("off1", F32, 4, 8, 8, 8, (2, 5, 9), hw, ELEMENT_ROUTE, "align", True, off=1)
    add("blocks", BF16, 4, 12, 12, 12, (1, 450, 400), ("w",), ELEMENT_ROUTE, "C", False, note="8438 blocks > 8192")
    add("blocks", F32, 2, 14, 14, 14, (1, 450, 400), ("w",), ELEMENT_ROUTE, "C", False, note="9844 blocks > 8192")
    assert len({c.id for c in t}) == len(t)
    return t


TOKENS = _token_table()
_TOKENS_BY_ID = {c.id: c for c in TOKENS}

NAN_BITS = {BF16: 0x7FC0, F32: 0x7FC00000}
MARK_BITS = {BF16: -0x5A5B, F32: -0x5A5A5A5B}  # the permutation tests' sentinel: a fixed pattern the random data never holds
_ITYPE = {BF16: torch.int16, F32: torch.int32}


class Guarded:
    """A contiguous tensor of `shape` inside a larger allocation filled with a sentinel bit pattern: `guard` elements before (then `off` elements
    more: an unaligned start) and after it.  The view starts 16-byte aligned when off = 0."""

    def __init__(self, shape, dtype, sentinel, init=None, off=0, guard=8192):
        self.n = int(math.prod(shape))
        self.lo = guard + off
        self.sentinel = sentinel
        self.flat = torch.empty(self.lo + self.n + guard, dtype=dtype, device="cuda")
        self.bits = self.flat.view(_ITYPE[dtype])
        self.bits.fill_(sentinel)
        self.view = self.flat[self.lo:self.lo + self.n].view(tuple(shape))
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (off * self.flat.element_size()) % 16
        if init is not None:
            self.view.copy_(init)
        self.first = self.bits.clone()

    def refill(self):
        self.bits[self.lo:self.lo + self.n] = self.sentinel

    def inside(self):
        return self.bits[self.lo:self.lo + self.n].reshape(self.view.shape)

    def check(self, what, written):
        """Nothing outside the view changed; an input is unchanged altogether, an output holds no sentinel."""
        if written:
            assert torch.equal(self.bits[:self.lo], self.first[:self.lo]) and torch.equal(self.bits[self.lo + self.n:], self.first[self.lo + self.n:]), \
                f"{what}: a guard element was written"
            left = self.inside() == self.sentinel
            assert not bool(left.any()), f"{what}: {int(left.sum())} elements hold the sentinel, the first at {tuple(torch.nonzero(left)[0].tolist())}"
        else:
            assert torch.equal(self.bits, self.first), f"{what}: an input or its guards changed"


def _ncu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _same(got, want, what):
    """got == want element for element (NaN differs from everything), naming the first difference."""
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} for {tuple(want.shape)}"
    n, idx, g, w = WR.first_mismatch(got, want)
    assert n == 0, f"{what}: {n} of {got.numel()} elements differ, the first at {idx}: got {g!r}, want {w!r}"


def _bits(t):
    return t.view(_ITYPE[t.dtype])


def probe_weight(Cp, p):
    """conv_ref.one_hot_linear's probe with a multiplier coprime to Cp (7 divides 112), so that the copied features are all distinct."""
    if Cp % 7:
        w, i = CR.one_hot_linear(Cp, Cp, p)
    else:
        o = torch.arange(Cp)
        i = (5 * o + 31 * p) % Cp
        w = torch.zeros(Cp, Cp)
        w[o, i] = 1.0
    assert len(set(i.tolist())) == Cp
    return w, i


def random_finite_bf16(shape, seed):
    """Random bit patterns over every normal bf16 number and both zeros: sign, exponent field 1 .. 254 and mantissa uniform, one element in 16 a zero."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, tuple(shape), generator=g)
    bits = sign << 15 | torch.randint(1, 255, tuple(shape), generator=g) << 7 | torch.randint(0, 128, tuple(shape), generator=g)
    bits = torch.where(torch.randint(0, 16, tuple(shape), generator=g) == 0, sign << 15, bits)
    return (bits - (bits >= 2 ** 15) * 2 ** 16).to(torch.int16).view(BF16)


def random_bits(shape, dtype, seed):
    """Every bit pattern (NaNs, infinities, -0.0, subnormals) but the permutation sentinel, as a tensor of `dtype`."""
    g = torch.Generator().manual_seed(seed)
    if dtype == BF16:
        b = torch.randint(-2 ** 15, 2 ** 15, tuple(shape), generator=g).to(torch.int16)
    else:
        b = torch.randint(-2 ** 31, 2 ** 31, tuple(shape), generator=g).to(torch.int32)
    b[b == MARK_BITS[dtype]] = 0x1234
    b.reshape(-1)[:4] = torch.tensor([NAN_BITS[dtype], -2 ** (15 if dtype == BF16 else 31), 1, -1], dtype=b.dtype)  # NaN, -0.0, a subnormal, a NaN
    return b.view(dtype)


@functools.lru_cache(maxsize=None)
def _weights_cpu(Cp, kind):
    """(w (Cp, Cp), bias (Cp) or None) as fp32 CPU tensors holding bf16 numbers (the bias any fp32)."""
    if kind == "exact":
        return WR.exact_values((Cp, Cp), 7000 + Cp, "full"), WR.exact_values((Cp,), 7001 + Cp, "full")
    if kind == "real":
        g = torch.Generator().manual_seed(7002 + Cp)
        return (torch.randn(Cp, Cp, generator=g) / Cp ** 0.5).bfloat16().float(), torch.randn(Cp, generator=g) * 0.1
    return probe_weight(Cp, int(kind[-1]))[0], None


@functools.lru_cache(maxsize=None)
def _weights_dev(Cp, kind):
    """Their device copies, kept alive: the pack cache goes by the weight tensor."""
    w, b = _weights_cpu(Cp, kind)
    return w.cuda(), None if b is None else b.cuda()


def _fused_operands(case, shape, seed):
    """x, mask (or None) as bf16 CPU tensors."""
    if case.kind == "exact":
        x = WR.exact_values(shape, seed, "full").bfloat16()
        mask = None
        if case.form == "mask":
            mask = WR.exact_values(shape, seed + 1, "full").bfloat16().reshape(-1)
            mask[3::7] = -0.0
            mask[5::11] = 0.0
            mask = mask.reshape(shape)
        return x, mask
    if case.kind == "real":
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(shape, generator=g).bfloat16()
        return x, (torch.randn(shape, generator=g).bfloat16() if case.form == "mask" else None)
    return random_finite_bf16(shape, seed), None


FusedRef = collections.namedtuple("FusedRef", "shape x mask w bias applied relu in_scale out_scale v S tok want")


def fused_reference(case, ncu):
    """Operands, launch arguments and the fp64 reference of a fused case, with the conditions that must hold before anything is launched: the
    exactness invariant, and non-degeneracy (at least a quarter of the elements cut and a quarter kept by every ReLU / mask, nothing all zero).
    No GPU: tests/test_morph_plan.py runs it too."""
    Cp, chunk, C, axis = case.Cp, case.chunk, case.C, case.axis
    B, T, H, W = geometry(case, ncu)
    shape = (B, T, H, W, C)
    masked, exact, real, probe = case.form == "mask", case.kind == "exact", case.kind == "real", case.kind.startswith("probe")
    x, mask = _fused_operands(case, shape, 100 + sum(map(ord, case.id)))
    w, b = _weights_cpu(Cp, case.kind)
    if masked:
        relu, in_scale, out_scale, bias, applied = False, (1.0 / Cp if real else IN_SCALE), 1.0, None, w.t()
    else:
        relu, in_scale, out_scale, bias, applied = not probe, 1.0, (1.0 if probe else 1.0 / Cp if real else OUT_SCALE), b, w
    if exact:
        CR.assert_exact("full", ci_total=Cp, bias=bias is not None, scales=(in_scale, out_scale), taps=1)
    v, S, tok = MR.branch_ref(x, applied, bias, axis, chunk, Cp, relu, out_scale, mask=mask, in_scale=in_scale)
    v, S = v.reshape(shape), S.reshape(shape)
    want = None if real else CR.round_bf16(v, exact=True)
    if probe:  # the probe's reference IS the copy: output feature o of a token = its feature perm[o]
        perm = probe_weight(Cp, int(case.kind[-1]))[1]
        assert torch.equal(want.float(), MR.untokens_ref(tok[:, perm], axis, chunk, Cp, H, W, C).reshape(shape).float())
    assert bool((v != 0).any()) and bool((tok != 0).any())
    if relu:
        cut = float((v == 0).double().mean())
        assert 0.25 <= cut <= 0.75, f"{case.id}: ReLU cuts {cut:.2f} of the elements"
    if masked:
        keep = float((mask.float() > 0).double().mean())
        assert 0.25 <= keep <= 0.75, f"{case.id}: the mask keeps {keep:.2f} of the elements"
        if exact:
            mb = _bits(mask)
            assert bool((mb == 0).any()) and bool((mb == -2 ** 15).any()) and bool((mask.float() < 0).any()), f"{case.id}: the mask lacks +0.0, -0.0 or a negative"
    return FusedRef(shape, x, mask, w, bias, applied, relu, in_scale, out_scale, v, S, tok, want)


@pytest.mark.parametrize("cid", [c.id for c in FUSED])
def test_fused_kernel(cid):
    from vmg_amd import functional as FH, kernels as K
    case = _FUSED_BY_ID[cid]
    Cp, chunk, C, axis = case.Cp, case.chunk, case.C, case.axis
    ncu = _ncu()
    B, T, H, W = geometry(case, ncu)
    masked, exact, real = case.form == "mask", case.kind == "exact", case.kind == "real"
    # ---- the plan reports the instance the case is meant for, and the geometry reaches the edges the case names
    plan = K.morphfc_plan(axis, chunk, B * T, H, W, C, Cp, masked, ncu)
    assert tuple(plan[:4]) == instance(case), f"the plan says {plan}, the case names {instance(case)}"
    assert plan.nwg == min(ncu, -(-plan.ntiles // 8)) and plan.ntiles == -(-plan.ngroups // (16 // chunk))
    assert ("loops" in case.tags) == (plan.ntiles > 8 * plan.nwg)
    if "loops" in case.tags:
        assert plan.ntiles <= 8 * plan.nwg + 8, "just above: only the first waves take a second tile"
    if "dead group" in case.tags:
        assert chunk == 8 and plan.ngroups % 2 == 1
    if "single tile" in case.tags:
        assert plan.ntiles == 1
    assert ("channel padding" in case.tags) == (C < Cp)
    r = fused_reference(case, ncu)
    shape, relu, in_scale, out_scale, v, S, tok, want = r.shape, r.relu, r.in_scale, r.out_scale, r.v, r.S, r.tok, r.want
    wd, bd = _weights_dev(Cp, case.kind)
    bias_d = bd if r.bias is not None else None
    pw = FH.packed(wd, BF16, "dgrad", None, 0, Cp, tiles=plan.NCT) if masked else FH.packed(wd, BF16, "fwd", [Cp], tiles=plan.NCT)
    x, mask = r.x, r.mask
    # ---- two launches into sentinel-filled outputs
    nan = NAN_BITS[BF16]
    gx, gm = Guarded(shape, BF16, nan, init=x), (Guarded(shape, BF16, nan, init=mask) if masked else None)
    go, gt = Guarded(shape, BF16, nan), Guarded((plan.ntiles * 16, Cp), BF16, nan)
    runs = []
    for launch in range(2):
        go.refill()
        gt.refill()
        y, tk = K.morphfc_forward(gx.view, axis, chunk, Cp, pw, bias_d, relu, in_scale, out_scale, mask=gm.view if masked else None, out=go.view, tok_out=gt.view)
        torch.cuda.synchronize()
        assert y.data_ptr() == go.view.data_ptr() and tk.data_ptr() == gt.view.data_ptr()
        gx.check(f"{cid} launch {launch}: x", False)
        if masked:
            gm.check(f"{cid} launch {launch}: mask", False)
        go.check(f"{cid} launch {launch}: out", True)
        gt.check(f"{cid} launch {launch}: tok_out", True)
        runs.append((go.view.cpu(), gt.view.cpu()))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1])), f"{cid}: two launches, two results"
    # a third launch without the token side output (its stores go to a scratch word): the same output
    go.refill()
    y, tk = K.morphfc_forward(gx.view, axis, chunk, Cp, pw, bias_d, relu, in_scale, out_scale, mask=gm.view if masked else None, out=go.view)
    torch.cuda.synchronize()
    assert tk is None
    go.check(f"{cid} launch without tokens: out", True)
    gt.check(f"{cid} launch without tokens: tok_out", True)
    assert torch.equal(_bits(go.view.cpu()), _bits(runs[0][0])), f"{cid}: the output depends on whether the tokens are written"
    got, gtok = runs[0]
    # ---- the token side output: the reference's operand matrix bit for bit, zero rows past the last group
    rows = tok.shape[0]
    assert rows == plan.ngroups * chunk and gtok.shape[0] >= rows
    _same(gtok[:rows].float(), tok.float(), f"{cid}: token side output")
    assert torch.equal(_bits(gtok[:rows]), _bits(tok)), f"{cid}: token side output differs in the sign of a zero"
    assert not bool(_bits(gtok[rows:]).any()), f"{cid}: rows past the last group are not zero"
    # ---- the output
    if real:
        bound = CR.real_bound(v, S * float(torch.tensor(out_scale, dtype=torch.float32)), ci_total=Cp, taps=1)
        err = (got.double() - v).abs()
        worst = float((err[bound > 0] / bound[bound > 0]).max())  # (the bound is 0 where every operand of the sum is masked: there got must be 0)
        print(f"{cid}: worst |got - v| / bound = {worst:.3f}")
        bad = ~(err <= bound)
        assert not bool(bad.any()), f"{cid}: {int(bad.sum())} elements outside the bound, the first at {tuple(torch.nonzero(bad)[0].tolist())}, worst ratio {worst:.3f}"
    else:
        _same(got.float(), want.float(), f"{cid}: output")
        if exact:
            assert torch.equal(_bits(got), _bits(want)), f"{cid}: output differs in the sign of a zero"


@pytest.mark.parametrize("cid", [c.id for c in TOKENS])
def test_token_kernels(cid):
    from vmg_amd import kernels as K
    case = _TOKENS_BY_ID[cid]
    dtype, axis, chunk, C, Cp, ld = case.dtype, case.axis, case.chunk, case.C, case.Cp, case.ld
    BT, H, W = case.geom
    shape = (1, BT, H, W, C)
    rows = MR.token_rows(axis, chunk, BT, H, W)
    mark = MARK_BITS[dtype]
    x = random_bits(shape, dtype, 300 + sum(map(ord, cid)))
    t = random_bits((rows, ld), dtype, 301 + sum(map(ord, cid)))
    want_tok = torch.zeros((rows, ld), dtype=_ITYPE[dtype])
    want_tok[:, :Cp] = MR.tokens_ref(_bits(x), axis, chunk, Cp)
    want_map = MR.untokens_ref(_bits(t), axis, chunk, Cp, H, W, C).reshape(shape)
    assert bool(want_tok.any()) and bool(want_map.any())
    gx, gt = Guarded(shape, dtype, mark, init=x, off=case.off), Guarded((rows, ld), dtype, mark, init=t)
    go_tok, go_map, go_back = Guarded((rows, ld), dtype, mark), Guarded(shape, dtype, mark, off=case.off), Guarded(shape, dtype, mark, off=case.off)
    # ---- the route, before anything is launched: the same for the three calls (the feature map carries the offset, the token matrices are aligned)
    for a, bb in ((gx.view, go_tok.view), (go_map.view, gt.view), (go_back.view, go_tok.view)):
        aligned = (a.data_ptr() | bb.data_ptr()) % 16 == 0
        assert aligned == (case.off == 0)
        assert K.morph_tokens_route(dtype, chunk, C, ld, aligned) == case.route, f"{cid}: not the route the case is meant for"
    runs = []
    for launch in range(2):
        for g in (go_tok, go_map, go_back):
            g.refill()
        assert K.morph_tokens_gather(gx.view, axis, chunk, Cp, ld, out=go_tok.view).data_ptr() == go_tok.view.data_ptr()
        assert K.morph_tokens_scatter(gt.view, axis, chunk, Cp, shape, out=go_map.view).data_ptr() == go_map.view.data_ptr()
        K.morph_tokens_scatter(go_tok.view, axis, chunk, Cp, shape, out=go_back.view)
        torch.cuda.synchronize()
        gx.check(f"{cid} launch {launch}: x", False)
        gt.check(f"{cid} launch {launch}: tok", False)
        go_tok.check(f"{cid} launch {launch}: gather out", True)
        go_map.check(f"{cid} launch {launch}: scatter out", True)
        go_back.check(f"{cid} launch {launch}: round trip out", True)
        runs.append((go_tok.inside().cpu(), go_map.inside().cpu(), go_back.inside().cpu()))
    for a, bb in zip(*runs):
        assert torch.equal(a, bb), f"{cid}: two launches, two results"
    _same(runs[0][0], want_tok, f"{cid}: gather")
    _same(runs[0][1], want_map, f"{cid}: scatter")
    _same(runs[0][2], _bits(x), f"{cid}: scatter(gather(x))")


# ---- autograd level: functional.morph_linear, fused and general path.  Cp a power of two: the product's 1 / Cp scale rounds nothing.
# (name, dtype, chunk, Cp, C, (B, T, H, W), axis, fused)
AUTOGRAD = [("fused", BF16, 16, 32, 24, (1, 2, 5, 35), "w", True), ("general", BF16, 4, 16, 12, (1, 2, 9, 5), "h", False)]


@pytest.mark.parametrize("mode", ["autograd", "deferred"])
@pytest.mark.parametrize("setting", ["x-grad", "no-x-grad", "no-bias"])
@pytest.mark.parametrize("geo", AUTOGRAD, ids=[a[0] for a in AUTOGRAD])
def test_morph_linear_autograd(geo, setting, mode):
    """y and dx equal the rounded fp64 reference, dW and db equal it exactly ("small" family: k / 4, |k| <= 8; every sum stays exact up to
    2^24 / 64 tokens).  no-x-grad: the weight gradient's token matrices are built without the kernel's side outputs."""
    from vmg_amd import functional as FH, kernels as K
    name, dtype, chunk, Cp, C, (B, T, H, W), axis, fused = geo
    shape = (B, T, H, W, C)
    x, dy = WR.exact_values(shape, 41, "small"), WR.exact_values(shape, 42, "small")
    w = WR.exact_values((Cp, Cp), 43, "small")
    b = WR.exact_values((Cp,), 44, "small") if setting != "no-bias" else None
    rows = MR.token_rows(axis, chunk, B * T, H, W)
    WR.assert_exact("small", rows)
    assert rows <= 2 ** 24 // 64
    # ---- reference, fp64: y = untokens(relu(tok w^T + b) / Cp);  dpre = tok(dy * [y > 0] / Cp);  dx = untokens(dpre w);  dW = dpre^T tok(x);  db = sum dpre
    v, _, tok = MR.branch_ref(x.bfloat16(), w, b, axis, chunk, Cp, True, 1.0 / Cp)
    y_want = CR.round_bf16(v.reshape(shape), exact=True)
    assert 0.25 <= float((v == 0).double().mean()) <= 0.75
    gv, _, dpre = MR.branch_ref(dy.bfloat16(), w.t(), None, axis, chunk, Cp, False, 1.0, mask=y_want, in_scale=1.0 / Cp)
    assert torch.equal(dpre.double(), MR.tokens_ref(torch.where(v.reshape(shape) > 0, dy.double() / Cp, torch.zeros((), dtype=torch.float64)), axis, chunk, Cp))
    dx_want = CR.round_bf16(gv.reshape(shape), exact=True)
    dw_want, db_want = dpre.double().t() @ tok.double(), dpre.double().sum(0)
    assert bool((dx_want != 0).any()) and bool((dw_want != 0).any()) and bool((db_want != 0).any())
    xd = x.cuda().to(dtype).requires_grad_(setting != "no-x-grad")
    wd = torch.nn.Parameter(w.cuda())
    bd = torch.nn.Parameter(b.cuda()) if b is not None else None
    assert K.morph_fused_ok(xd, chunk, Cp) == fused
    FH.set_wgrad_mode(mode)
    try:
        y = FH.morph_linear(xd, wd, bd, axis, chunk, Cp)
        y.backward(dy.cuda().to(dtype))
        if mode == "deferred":
            FH.flush_deferred_wgrads()
    finally:
        FH.set_wgrad_mode("autograd")
    _same(y.detach().cpu().float(), y_want.float(), f"{name} {setting} {mode}: y")
    if setting != "no-x-grad":
        _same(xd.grad.cpu().float(), dx_want.float(), f"{name} {setting} {mode}: dx")
    else:
        assert xd.grad is None
    _same(wd.grad.cpu().double(), dw_want, f"{name} {setting} {mode}: dW")
    if bd is not None:
        _same(bd.grad.cpu().double(), db_want, f"{name} {setting} {mode}: db")


def test_plan_default_is_the_current_device_and_caller_owned_outputs_are_checked():
    from vmg_amd import functional as FH, kernels as K
    from vmg_amd.hip import HipError
    assert K.morphfc_plan("w", 8, 2, 41, 397, 144, 144) == K.morphfc_plan("w", 8, 2, 41, 397, 144, 144, ncu=_ncu())
    x = torch.zeros((1, 2, 5, 17, 16), dtype=BF16, device="cuda")
    pw = FH.packed(_weights_dev(16, "exact")[0], BF16, "fwd", [16], tiles=1)
    rows = 2 * 5 * 3 * 8
    good, gtok = torch.empty_like(x), torch.empty((rows, 16), dtype=BF16, device="cuda")
    y, tok = K.morphfc_forward(x, "w", 8, 16, pw, None, True, 1.0, 1.0, out=good, tok_out=gtok)
    assert y is good and tok is gtok
    y, tok = K.morphfc_forward(x, "w", 8, 16, pw, None, True, 1.0, 1.0)  # the existing calls: fresh outputs, tokens only on request
    assert tok is None and y.shape == x.shape and y.data_ptr() != good.data_ptr()
    wide = torch.empty((1, 2, 5, 17, 32), dtype=BF16, device="cuda")
    for bad in (torch.empty((1, 2, 5, 17, 8), dtype=BF16, device="cuda"), torch.empty_like(x, dtype=F32), wide[..., :16], torch.empty_like(x, device="cpu")):
        with pytest.raises(HipError):
            K.morphfc_forward(x, "w", 8, 16, pw, None, True, 1.0, 1.0, out=bad)
        with pytest.raises(HipError):
            K.morph_tokens_scatter(gtok, "w", 8, 16, x.shape, out=bad)
    for bad in (torch.empty((rows + 16, 16), dtype=BF16, device="cuda"), torch.empty((rows, 16), dtype=F32, device="cuda"),
                torch.empty((rows, 32), dtype=BF16, device="cuda")[:, :16]):
        with pytest.raises(HipError):
            K.morphfc_forward(x, "w", 8, 16, pw, None, True, 1.0, 1.0, tok_out=bad)
        with pytest.raises(HipError):
            K.morph_tokens_gather(x, "w", 8, 16, 16, out=bad)
