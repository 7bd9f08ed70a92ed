"""Every MFMA kernel of csrc/conv_wgrad.hip against the fp64 reference of tests/wgrad_ref.py, bit for bit.

The operands are k * 2^-s with small integer k (tests/wgrad_ref.py: the families "full" and "small"), the initial gradients integers and
the scale a power of two, so the gradient has no rounding in fp32 whatever the order of the additions: the GPU result must EQUAL the
reference (torch.equal, no tolerance), and one dropped, doubled or misplaced pixel, tap or channel changes it.  Operands are views inside
NaN-filled allocations (wgrad_ref.embed) and the slab workspace is filled with NaN before every call: a read outside the image that is not
replaced by zero, of a channel past the 8-rounded count, or of a slab float nobody wrote, poisons the result.  Every case asserts which
kernel ran (vmg_conv_wgrad_last_kernel): the dispatch falls back without an error, and a case that reaches another kernel proves nothing."""
import ctypes
import os
import re

import pytest
import torch

from tests import wgrad_ref as WR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32 = torch.bfloat16, torch.float32
SCALES = (1.0, 0.5, -0.25)


def _mods():
    from vmg_amd import hip, kernels as K
    return hip, K


def _kernel_name(hip, kid):
    kind, a, b, c = kid >> 24, (kid >> 16) & 255, (kid >> 8) & 255, kid & 255
    names = {hip.WGRAD_V1: f"conv_wgrad_kernel<KS={a}, CT={b}, IT={c}>", hip.WGRAD_3: "conv_wgrad3_kernel", hip.WGRAD_3B: "conv_wgrad3b_kernel",
             hip.WGRAD_L2: "linear_wgrad2_kernel", hip.WGRAD_7: f"conv_wgrad7_kernel<CT={a}, KS={b}>"}
    return names.get(kind, f"unknown kernel {kid:#x}")


def _w7_rows():
    """W7Geo<KS>::R of the source: image rows per K unit of conv_wgrad7_kernel, {7: rows, 3: rows}."""
    src = open(os.path.join(ROOT, "vmg_amd", "csrc", "conv_wgrad.hip")).read()
    m = re.search(r"static constexpr int R = KS == 7 \? (\d+) : (\d+);", src)
    assert m, "W7Geo<KS>::R not found in conv_wgrad.hip"
    return {7: int(m.group(1)), 3: int(m.group(2))}


def _c8(c):
    return (c + 7) // 8 * 8


class _Problem:
    """One weight-gradient problem: exact operands (CPU fp32 + embedded device views), integer initial gradients, the expected result."""

    def __init__(self, N, H, W, Ci, Co, ks, P=1, seed=0, dtype=BF16, x_ps=None, dy_ps=None, x_off=0, dy_off=0, bias=True, total=None, o0=0, i0=0,
                 flat=False, probe=None):
        self.dims, self.ks, self.o0, self.i0, self.Ci, self.Co = (N, H, W), ks, o0, i0, Ci, Co
        terms = N * H * W * P
        self.family = family = "full" if terms <= 256 else "small"
        WR.assert_exact(family, terms)  # the invariant, before anything runs on the GPU
        if probe is None:
            xs = [WR.exact_values((N, H, W, Ci), 1000 * seed + p, family) for p in range(P)]
            dys = [WR.exact_values((N, H, W, Co), 1000 * seed + 500 + p, family) for p in range(P)]
        else:  # one-hot probe: a single 1 in the last input channel at the first / last pixel (of the last image), dy all ones
            assert P == 1
            xs, dys = [torch.zeros(N, H, W, Ci)], [torch.ones(N, H, W, Co)]
            xs[0][(0, 0, 0, Ci - 1) if probe == "first" else (N - 1, H - 1, W - 1, Ci - 1)] = 1.0
        self.x_ps = _c8(Ci) + 8 if x_ps is None else x_ps
        self.dy_ps = _c8(Co) + 8 if dy_ps is None else dy_ps
        # guard: at least the rows a K unit and its halo could reach past either end of the image (3 * W + 3 for the 7x7 halo is well inside)
        guard = (8 + ks // 2) * W + 48 + ks // 2
        assert guard >= 3 * W + 3
        self.xs = [WR.embed(x.to(dtype), self.x_ps, guard, offset=x_off, device="cuda") for x in xs]
        self.dys = [WR.embed(d.to(dtype), self.dy_ps, guard, offset=dy_off, device="cuda") for d in dys]
        for a, b in zip(xs + dys, self.xs + self.dys):
            assert torch.equal(a, b.float().cpu())  # the values survive the cast: they are numbers of the operand type
        Ot, It = total or (Co, Ci)
        self.dW0 = WR.exact_init((Ot, It) if flat else (Ot, It, ks, ks), 7000 + seed, family)
        self.db0 = WR.exact_init((Ot,), 8000 + seed, family) if bias else None
        self.scale = SCALES[seed % 3]
        dWr, dbr = WR.wgrad_ref(xs, dys, ks)
        self.ref = dWr
        wW = self.dW0.double().reshape(Ot, It, ks, ks).clone()
        wW[o0:o0 + Co, i0:i0 + Ci] += self.scale * dWr
        self.wantW = wW.float().reshape(self.dW0.shape)
        assert torch.equal(self.wantW.double().reshape(wW.shape), wW)  # the expected value itself is an fp32 number
        self.wantb = None
        if bias:
            wb = self.db0.double().clone()
            wb[o0:o0 + Co] += self.scale * dbr
            self.wantb = wb.float()
            assert torch.equal(self.wantb.double(), wb)


def _assert_same(got, want, what):
    nan = torch.isnan(got)
    if bool(nan.any()):
        first = tuple(int(v) for v in torch.nonzero(nan)[0])
        raise AssertionError(f"{what}: {int(nan.sum())} of {got.numel()} elements are NaN, the first at {first}: something outside the operands "
                             "(guard, channel padding or an unwritten slab float) was read")
    n, idx, g, w = WR.first_mismatch(got, want)
    assert n == 0, f"{what}: {n} of {got.numel()} elements differ from the fp64 reference, the first at {idx}: got {g!r}, want {w!r}"
    assert torch.equal(got, want), what


def _check(prob, outs, what):
    """outs: [(dW, db)] of the two runs (CPU tensors)."""
    (dW, db), (dW2, db2) = outs
    _assert_same(dW, prob.wantW, what + ": dW")
    if prob.db0 is not None:
        _assert_same(db, prob.wantb, what + ": db")
        assert torch.equal(db, db2), what + ": db differs between two runs"
    assert torch.equal(dW, dW2), what + ": dW differs between two runs"
    Ot, It = prob.dW0.shape[:2]
    if (Ot, It) != (prob.Co, prob.Ci):  # a slice of a wider parameter: everything outside keeps the bits of the initial value
        out = torch.ones(Ot, It, dtype=torch.bool)
        out[prob.o0:prob.o0 + prob.Co, prob.i0:prob.i0 + prob.Ci] = False
        assert torch.equal(dW[out], prob.dW0[out]), what + ": dW changed outside the (o0, i0) slice"
        if prob.db0 is not None:
            ob = torch.ones(Ot, dtype=torch.bool)
            ob[prob.o0:prob.o0 + prob.Co] = False
            assert torch.equal(db[ob], prob.db0[ob]), what + ": db changed outside the o0 slice"


def _run(probs, call, kernel, what):
    """Twice from the same initial gradients, the workspace full of NaN: call(list of (dW, db) device tensors, one per problem); then the
    kernel record and each problem against its own reference."""
    hip, K = _mods()
    lib = hip.lib()
    ws = K._workspace("vmg_conv_wgrad_ws_bytes", torch.device("cuda", torch.cuda.current_device()))
    runs = []
    for _ in range(2):
        ws.fill_(255)  # 0xFFFFFFFF as a float: NaN
        grads = [(p.dW0.cuda(), p.db0.cuda() if p.db0 is not None else None) for p in probs]
        call(grads)
        got = lib.vmg_conv_wgrad_last_kernel()
        assert got == kernel, f"{what}: ran {_kernel_name(hip, got)}, the case is about {_kernel_name(hip, kernel)}"
        runs.append([(dW.cpu(), db.cpu() if db is not None else None) for dW, db in grads])
    for i, p in enumerate(probs):
        _check(p, [runs[0][i], runs[1][i]], f"{what} [{_kernel_name(hip, kernel)}]" + (f" problem {i}" if len(probs) > 1 else ""))


def _batched(prob, kernel, what):
    """Through kernels.conv_wgrad_batched (vmg_conv_wgrad_batched_ws: the workspace entry)."""
    hip, K = _mods()
    N, H, W = prob.dims

    def call(grads):
        dW, db = grads[0]
        K.conv_wgrad_batched(prob.xs, prob.dys, dW, db, prob.ks, N, H, W, scale=prob.scale, o0=prob.o0, i0=prob.i0)
    _run([prob], call, kernel, what)


def _single(prob, kernel, what):
    """Through kernels.conv_wgrad (vmg_conv_wgrad: no workspace, the v1 kernel)."""
    hip, K = _mods()
    N, H, W = prob.dims

    def call(grads):
        dW, db = grads[0]
        K.conv_wgrad(prob.xs[0], prob.dys[0], dW, db, prob.ks, N, H, W, scale=prob.scale, o0=prob.o0, i0=prob.i0)
    _run([prob], call, kernel, what)


def _both_3x3_variants(body):
    """body(kernel id) under vmg_conv_wgrad3_variant 0 (conv_wgrad3_kernel) and 1 (conv_wgrad3b_kernel); the previous variant is restored."""
    hip, _ = _mods()
    lib = hip.lib()
    prev = lib.vmg_conv_wgrad3_variant(-1)
    try:
        for variant, kind in ((0, hip.WGRAD_3), (1, hip.WGRAD_3B)):
            lib.vmg_conv_wgrad3_variant(variant)
            body(hip.wgrad_kernel_id(kind))
    finally:
        lib.vmg_conv_wgrad3_variant(prev)
    assert lib.vmg_conv_wgrad3_variant(-1) == prev


def _probe_pattern(ks, H, W, qy, qx):
    """dW[:, ci] of a one-hot x at pixel (qy, qx) under dy = 1: tap (ky, kx) sees the pixel from output pixel (qy - ky + ks//2, qx - kx + ks//2),
    which must lie inside the image -- 1 where the padding allows the tap, 0 elsewhere."""
    pat = torch.zeros(ks, ks)
    for ky in range(ks):
        for kx in range(ks):
            py, px = qy - ky + ks // 2, qx - kx + ks // 2
            pat[ky, kx] = 1.0 if 0 <= py < H and 0 <= px < W else 0.0
    return pat


def _check_probe(prob, probe):
    """The reference of a probe problem is the tap pattern (so that a failure of the case names the tap and the border)."""
    N, H, W = prob.dims
    qy, qx = (0, 0) if probe == "first" else (H - 1, W - 1)
    pat = _probe_pattern(prob.ks, H, W, qy, qx).double()
    want = torch.zeros_like(prob.ref)
    want[:, prob.Ci - 1] = pat
    assert torch.equal(prob.ref, want), "probe reference is not the tap pattern"


# ------------------------------------------------------------------------------------------------------------------------------------
# large-tile 3x3: conv_wgrad3_kernel and conv_wgrad3b_kernel (+ conv_wgrad3_reduce_kernel), Cout > 16 with a workspace
# ------------------------------------------------------------------------------------------------------------------------------------
W3_CASES = [
    # (N, H, W, Cin, Cout, pairs): W = 1 / 31 / 32 / 33 / 65 at H = 2 (65: a third segment of one pixel)
    (1, 2, 1, 48, 144, 1), (1, 2, 31, 48, 144, 1), (1, 2, 32, 48, 144, 1), (1, 2, 33, 48, 144, 1), (1, 2, 65, 48, 144, 1),
    # H = 1 / 5, N = 3
    (1, 1, 33, 48, 144, 1), (1, 5, 33, 48, 144, 1), (3, 2, 33, 48, 144, 1),
    # Cin 8 / 40 / 48 / 56 / 144 (a partial block, the block edge, three blocks) x Cout 24 / 136 / 144 / 152 / 288 (gx 1 / 2, partial last tile)
    (1, 2, 33, 8, 24, 1), (1, 2, 33, 40, 136, 1), (1, 2, 33, 56, 152, 1), (1, 2, 33, 144, 288, 1), (1, 3, 31, 144, 24, 1), (1, 3, 31, 8, 288, 1),
    # S > 1 with U not divisible by S: U = 81 / S = 10, U = 21 / S = 2; U = 27 / S = 3 (divisible)
    (1, 9, 70, 48, 144, 3), (1, 7, 70, 48, 144, 1), (1, 9, 70, 48, 144, 1),
    # 16 pairs: one full launch; 17: a second launch that accumulates onto the first
    (1, 2, 33, 48, 144, 16), (1, 2, 33, 48, 144, 17),
]


@pytest.mark.parametrize("case", W3_CASES, ids=lambda c: "x".join(map(str, c)))
def test_large_tile_3x3_both_variants(case):
    N, H, W, Ci, Co, P = case
    seed = W3_CASES.index(case)
    prob = _Problem(N, H, W, Ci, Co, 3, P, seed=seed, x_ps=None if seed % 2 else Ci, dy_ps=None if seed % 3 else Co)
    _both_3x3_variants(lambda kernel: _batched(prob, kernel, f"3x3 {case}"))


def test_large_tile_3x3_stem_slice_of_padded_input():
    """Cin = 3 as a slice of an 8-channel tensor (the stem conv): channels 3..7 are computed and dropped -- they hold junk here, not zeros."""
    prob = _Problem(2, 3, 33, 3, 144, 3, 2, seed=40, x_ps=8)
    _both_3x3_variants(lambda kernel: _batched(prob, kernel, "3x3 stem"))


def test_large_tile_3x3_without_bias():
    prob = _Problem(1, 2, 33, 48, 144, 3, 2, seed=41, bias=False)
    _both_3x3_variants(lambda kernel: _batched(prob, kernel, "3x3 db=None"))


def test_large_tile_3x3_into_a_slice_of_a_wider_parameter():
    prob = _Problem(1, 2, 33, 48, 144, 3, 2, seed=42, total=(288, 288), o0=136, i0=40)
    _both_3x3_variants(lambda kernel: _batched(prob, kernel, "3x3 slice (136, 40) of (288, 288)"))


@pytest.mark.parametrize("probe", ["first", "last"])
def test_large_tile_3x3_one_hot_probe(probe):
    prob = _Problem(2, 3, 33, 48, 144, 3, seed=43, probe=probe)
    _check_probe(prob, probe)
    _both_3x3_variants(lambda kernel: _batched(prob, kernel, f"3x3 one-hot at the {probe} pixel"))


@pytest.mark.parametrize("nprob", [1, 3, 8, 9])
def test_large_tile_3x3_multi(nprob):
    """vmg_conv_wgrad3_multi: each problem has data, scale and db-or-None of its own and is checked against its own reference (9: 8 + 1
    problems in two launches)."""
    hip, K = _mods()
    N, H, W = 1, 3, 33
    probs = [_Problem(N, H, W, 56, 152, 3, 2, seed=50 + i, bias=(i % 3 != 1)) for i in range(nprob)]

    def call(grads):
        K.conv_wgrad3_multi([(p.xs, p.dys, dW, db, p.scale) for p, (dW, db) in zip(probs, grads)], N, H, W)
    _both_3x3_variants(lambda kernel: _run(probs, call, kernel, f"3x3 multi {nprob}"))


# ------------------------------------------------------------------------------------------------------------------------------------
# large-tile 1x1: linear_wgrad2_kernel (+ linear_wgrad2_reduce_kernel), at least 64 units of 32 pixels
# ------------------------------------------------------------------------------------------------------------------------------------
L2_CASES = [
    # (N, H, W, Cin, Cout, pairs): the last unit full / one pixel / 31 pixels; an image
    (1, 1, 2048, 144, 144, 1), (1, 1, 2049, 144, 144, 1), (1, 1, 2079, 144, 144, 1), (2, 33, 37, 144, 144, 1),
    # gx, gy in {1, 2, 4} with partial last blocks
    (1, 1, 2049, 8, 8, 1), (1, 1, 2049, 136, 152, 1), (1, 1, 2049, 152, 288, 1), (1, 1, 2049, 288, 144, 1), (1, 1, 2049, 144, 576, 1),
    (1, 1, 2049, 576, 136, 1),
    (1, 1, 2049, 144, 144, 3),
]


@pytest.mark.parametrize("case", L2_CASES, ids=lambda c: "x".join(map(str, c)))
def test_large_tile_1x1(case):
    hip, _ = _mods()
    N, H, W, Ci, Co, P = case
    seed = 100 + L2_CASES.index(case)
    prob = _Problem(N, H, W, Ci, Co, 1, P, seed=seed, x_ps=None if seed % 2 else Ci, dy_ps=None if seed % 3 else Co, flat=bool(seed % 2), bias=seed % 5 != 0)
    _batched(prob, hip.wgrad_kernel_id(hip.WGRAD_L2), f"1x1 {case}")


def test_large_tile_1x1_into_a_slice_of_a_wider_parameter():
    hip, _ = _mods()
    prob = _Problem(1, 1, 2049, 136, 152, 1, 1, seed=120, total=(288, 288), o0=136, i0=152)
    _batched(prob, hip.wgrad_kernel_id(hip.WGRAD_L2), "1x1 slice (136, 152) of (288, 288)")


def test_1x1_just_below_the_large_tile_threshold_takes_the_general_kernel():
    """M = 2016: 63 units -- the dispatch returns to the v1 kernel, which must be exact as well."""
    hip, _ = _mods()
    prob = _Problem(1, 1, 2016, 144, 144, 1, 1, seed=121)
    _batched(prob, hip.wgrad_kernel_id(hip.WGRAD_V1, 1, 3, 3), "1x1 M = 2016")


@pytest.mark.parametrize("probe", ["first", "last"])
def test_large_tile_1x1_one_hot_probe(probe):
    hip, _ = _mods()
    prob = _Problem(1, 1, 2049, 144, 152, 1, seed=122, probe=probe)
    _check_probe(prob, probe)
    _batched(prob, hip.wgrad_kernel_id(hip.WGRAD_L2), f"1x1 one-hot at the {probe} pixel")


@pytest.mark.parametrize("nprob", [1, 8, 9])
def test_large_tile_1x1_multi(nprob):
    hip, K = _mods()
    M = 2049
    probs = [_Problem(1, 1, M, 136, 152, 1, 2, seed=130 + i, bias=(i % 3 != 1), flat=True) for i in range(nprob)]

    def call(grads):
        K.linear_wgrad2_multi([(p.xs, p.dys, dW, db, p.scale) for p, (dW, db) in zip(probs, grads)], M)
    _run(probs, call, hip.wgrad_kernel_id(hip.WGRAD_L2), f"1x1 multi {nprob}")


# ------------------------------------------------------------------------------------------------------------------------------------
# conv_wgrad7_kernel (+ conv_wgrad7_reduce_kernel): 7x7 with Cout <= 64 (CT 1 / 2 / 4), 3x3 with Cout <= 16
# ------------------------------------------------------------------------------------------------------------------------------------
W7_CASES = [
    # (ks, H relative to W7Geo<KS>::R or absolute, W, Cin, Cout, pairs, dy dense?): dense dy of 2 / 3 / 17 channels is not a multiple of 8:
    # vec_dy = 0 (the flow head, conv_last)
    (7, "R", 33, 8, 2, 1, False), (7, "R-1", 31, 16, 16, 1, False), (7, "R+1", 33, 24, 17, 1, False), (7, 1, 1, 8, 32, 1, False),
    (7, "R+1", 31, 64, 33, 3, False), (7, "R", 1, 16, 64, 1, False), (7, "R+1", 33, 8, 2, 1, True), (7, "R-1", 33, 24, 17, 3, True),
    (7, 1, 33, 64, 64, 1, False), (7, "R+1", 33, 16, 16, 3, False),
    (3, "R", 33, 8, 2, 1, False), (3, "R-1", 31, 16, 3, 1, True), (3, "R+1", 33, 64, 3, 3, True), (3, "R+1", 1, 24, 16, 1, False),
    (3, 1, 31, 8, 16, 1, False), (3, "R+1", 33, 64, 3, 1, False), (3, "R", 31, 24, 2, 3, True),
]


def _w7_kernel(hip, ks, Co):
    ct = 1 if ks == 3 else {1: 1, 2: 2}.get((Co + 15) // 16, 4)
    return hip.wgrad_kernel_id(hip.WGRAD_7, ct, ks)


def _w7_height(ks, h):
    R = _w7_rows()[ks]
    return {"R": R, "R-1": R - 1, "R+1": R + 1}.get(h, h)


@pytest.mark.parametrize("case", W7_CASES, ids=lambda c: "-".join(map(str, c)))
def test_tap_row_kernel_7x7_and_small_cout_3x3(case):
    hip, _ = _mods()
    ks, h, W, Ci, Co, P, dense = case
    H = _w7_height(ks, h)
    seed = 200 + W7_CASES.index(case)
    prob = _Problem(1 + seed % 2, H, W, Ci, Co, ks, P, seed=seed, x_ps=None if seed % 2 else Ci, dy_ps=Co if dense else None, bias=seed % 5 != 0)
    assert dense == (prob.dy_ps % 8 != 0)
    _batched(prob, _w7_kernel(hip, ks, Co), f"wgrad7 {case} H={H}")


@pytest.mark.parametrize("probe", ["first", "last"])
@pytest.mark.parametrize("ks", [7, 3])
def test_tap_row_kernel_one_hot_probe(ks, probe):
    hip, _ = _mods()
    prob = _Problem(2, _w7_height(ks, "R+1"), 33, 16, 16, ks, seed=230, probe=probe)
    _check_probe(prob, probe)
    _batched(prob, _w7_kernel(hip, ks, 16), f"wgrad7 {ks}x{ks} one-hot at the {probe} pixel")


def test_tap_row_kernel_into_a_slice_of_a_wider_parameter():
    hip, _ = _mods()
    prob = _Problem(1, 5, 33, 16, 17, 7, 2, seed=231, total=(40, 24), o0=20, i0=8)
    _batched(prob, _w7_kernel(hip, 7, 17), "wgrad7 slice (20, 8) of (40, 24)")


# ------------------------------------------------------------------------------------------------------------------------------------
# the general ("v1") kernel conv_wgrad_kernel: every instantiation wgrad_plan picks
# ------------------------------------------------------------------------------------------------------------------------------------
V1_SHAPES = [(1, 3, 33, 8, 16), (1, 3, 33, 40, 56), (1, 3, 33, 144, 48), (2, 1, 70, 24, 24)]


def _v1_kernel(hip, dtype, ks, Ci, Co):
    if ks == 7:
        return hip.wgrad_kernel_id(hip.WGRAD_V1, 7, 1, 1)
    if ks == 3 and dtype == BF16 and Co <= 16:
        return hip.wgrad_kernel_id(hip.WGRAD_V1, 3, 1, 4 if Ci >= 64 else 1)
    return hip.wgrad_kernel_id(hip.WGRAD_V1, 3, 3, 1) if ks == 3 else hip.wgrad_kernel_id(hip.WGRAD_V1, 1, 3, 3)


V1_CASES = [(dtype, ks, shape) for dtype in (BF16, F32) for ks in (3, 1, 7) for shape in V1_SHAPES] + \
           [(BF16, 3, (1, 3, 33, 144, 16)), (BF16, 3, (1, 3, 33, 64, 3))]  # bf16 3x3 with Cout <= 16: Cin >= 64 takes <3, 1, 4>


@pytest.mark.parametrize("case", V1_CASES, ids=lambda c: f"{'bf16' if c[0] == BF16 else 'fp32'}-ks{c[1]}-" + "x".join(map(str, c[2])))
def test_general_kernel_every_instantiation(case):
    """<bf16, 3, 3, 1>, <bf16, 1, 3, 3>, <bf16, 7, 1, 1, 1>, <bf16, 3, 1, 4> (Cout <= 16, Cin >= 64), <bf16, 3, 1, 1> (Cout <= 16, Cin < 64) and
    the three fp32 instantiations through vmg_conv_wgrad: float atomics, exact in any order with these inputs, so two runs are equal too."""
    hip, _ = _mods()
    dtype, ks, shape = case
    N, H, W, Ci, Co = shape
    seed = 300 + V1_CASES.index(case)
    vpl = 8 if dtype == BF16 else 4
    ps = (lambda c: (c + vpl - 1) // vpl * vpl + vpl) if seed % 2 else (lambda c: (c + vpl - 1) // vpl * vpl)
    prob = _Problem(N, H, W, Ci, Co, ks, 1, seed=seed, dtype=dtype, x_ps=ps(Ci), dy_ps=ps(Co), bias=seed % 4 != 0)
    _single(prob, _v1_kernel(hip, dtype, ks, Ci, Co), f"v1 {dtype} ks={ks} {shape}")


@pytest.mark.parametrize("how", ["odd-strides", "unaligned-base"])
@pytest.mark.parametrize("ks", [3, 1, 7])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_general_kernel_element_loads(dtype, ks, how):
    """vec_x = vec_dy = 0: pixel strides that are no multiple of the 16-byte vector, or vector strides behind a base pointer that is one element
    off the 16-byte grid."""
    hip, _ = _mods()
    N, H, W, Ci, Co = 1, 3, 33, 40, 56
    vpl = 8 if dtype == BF16 else 4
    if how == "odd-strides":
        prob = _Problem(N, H, W, Ci, Co, ks, 1, seed=400 + ks, dtype=dtype, x_ps=Ci + 3, dy_ps=Co + 1)
        assert prob.x_ps % vpl and prob.dy_ps % vpl
    else:
        prob = _Problem(N, H, W, Ci, Co, ks, 1, seed=410 + ks, dtype=dtype, x_ps=Ci + vpl, dy_ps=Co + vpl, x_off=1, dy_off=3)
        assert prob.xs[0].data_ptr() % 16 and prob.dys[0].data_ptr() % 16
    _single(prob, _v1_kernel(hip, dtype, ks, Ci, Co), f"v1 {dtype} ks={ks} {how}")


@pytest.mark.parametrize("ks", [3, 1])
def test_general_kernel_with_k_splits(ks):
    """64 or more K units: gridDim.z > 1, several workgroups add their tiles to the same dW elements with float atomics."""
    hip, _ = _mods()
    N, H, W, Ci, Co = (1, 33, 33, 40, 56) if ks == 3 else (1, 1, 2060, 40, 56)
    prob = _Problem(N, H, W, Ci, Co, ks, 1, seed=420 + ks, total=(64, 48), o0=8, i0=8)
    _single(prob, _v1_kernel(hip, BF16, ks, Ci, Co), f"v1 bf16 ks={ks} K splits")


@pytest.mark.parametrize("probe", ["first", "last"])
@pytest.mark.parametrize("ks", [3, 1, 7])
def test_general_kernel_one_hot_probe(ks, probe):
    hip, _ = _mods()
    prob = _Problem(2, 3, 33, 40, 56, ks, seed=430, probe=probe)
    _check_probe(prob, probe)
    _single(prob, _v1_kernel(hip, BF16, ks, 40, 56), f"v1 {ks}x{ks} one-hot at the {probe} pixel")


def test_general_kernel_7x7_slab_form_through_the_workspace_entry():
    """7x7 with more than 64 output channels and a workspace: the v1 kernel stores its K splits as slabs, wgrad_slab_reduce_kernel sums them."""
    hip, _ = _mods()
    prob = _Problem(1, 5, 33, 8, 72, 7, 2, seed=440)
    _batched(prob, hip.wgrad_kernel_id(hip.WGRAD_V1, 7, 1, 1), "v1 7x7 slab form")


def test_general_kernel_fp32_through_the_workspace_entry():
    hip, _ = _mods()
    prob = _Problem(1, 3, 33, 40, 56, 3, 2, seed=441, dtype=F32, x_ps=44, dy_ps=60)
    _batched(prob, hip.wgrad_kernel_id(hip.WGRAD_V1, 3, 3, 1), "v1 fp32 3x3 via the workspace entry")


def test_general_kernel_through_vmg_conv_wgrad_batched():
    """The pairs entry without a workspace (vmg_conv_wgrad_batched), called directly: three pairs in one launch."""
    hip, _ = _mods()
    N, H, W = 1, 3, 33
    prob = _Problem(N, H, W, 40, 56, 3, 3, seed=442)

    def call(grads):
        dW, db = grads[0]
        xa = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in prob.xs])
        da = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in prob.dys])
        hip.check(hip.lib().vmg_conv_wgrad_batched(hip.BF16, 3, 3, xa, da, N, H, W, prob.x_ps, 40, prob.dy_ps, 56, dW.data_ptr(), 40, 0, 0, db.data_ptr(),
                                                   prob.scale, hip.stream_ptr()), "vmg_conv_wgrad_batched")
    _run([prob], call, hip.wgrad_kernel_id(hip.WGRAD_V1, 3, 3, 1), "v1 via vmg_conv_wgrad_batched")
