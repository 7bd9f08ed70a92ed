"""The kernels that move data between the big kernel families, each on its own through its vmg_amd.kernels wrapper: the non-LayerNorm half of
csrc/elementwise.hip (act_bwd, pixel_shuffle both ways, pixel_unshuffle_actgrad, frame_gather, sum_n, cast_clear, pair_steps and
pair_steps_range) and csrc/spynet.hip (avgpool2, upsample2x_ac fwd / bwd, spy_operand fwd / bwd, spy_flow_add, spy_prep), against the plain
CPU references of tests/glue_ref.py (pinned on the CPU by tests/test_glue_ref.py).

Every instance (dtype, mode, nsrc, activation) runs at the sizes where its code changes path: the scalar tail of act_bwd, the scalar
depth<->space kernel (channels no multiple of the vector, or a misaligned tensor), frames split over several blocks with an uneven split
(chunks = min(cdiv(2048, frames), cdiv(fv, 256)) -- the tests recompute it and assert the value they mean to reach), more than 64 step
tensors (pair_steps_range), and past every block cap, where the grid-stride loops wrap (act_bwd sizes its grid by n / 8 in both dtypes, so
fp32 has a case of its own that reaches the 2048-block cap).  The case ids name the instance and the boundary.

Before every call the block the output will be allocated from is filled with NaN (`poison`), so an element the kernel does not write cannot
pass as whatever the allocator left there; outputs the caller passes in (pair_steps) are NaN-filled directly.  Every operand is on the device
BEFORE the poison is laid (an upload of the output's size in between would take the poisoned block and overwrite it), and after the call
`poisoned` asserts that the output's address IS the poisoned block's: the caching allocator answers the same request from the same state with
the same block, and nothing is allocated or freed in between.

All comparisons are of BITS (glue_ref.bits: +0 and -0 differ), except two, which print their worst ratio to a stated bound before asserting:
  * GELU's derivative (act_backward, pixel_unshuffle_actgrad): |got - want| <= EGRAD * |dy * alpha| + r * |want| with EGRAD the bound on the
    device's gelu_erf_grad that tests/test_linear_kernels_gpu.py derived (imported, not copied) and r = 2^-24 (fp32) / 2^-8 (bf16) for the
    rounding to the tensor dtype.  Where the reference formula Phi(x) + x * phi(x) is NaN in fp64 (x = +-inf: inf * 0, as in torch's own
    backward; x = NaN) the kernel's result must be NaN too, and nowhere else.
  * upsample2x_ac: forward |got - want| <= 8 * 2^-24 * S, backward <= 16 * 2^-24 * S, S = |scale| * sum |w_i| |x_i|, from operation counts
    (forward: the (1 - l) subtraction, four products, three additions -- each rounds once; backward: at most 4 x 4 contributing outputs
    summed in two levels, plus their weights).  The reference computes the source coordinate in float32 as the kernel (and torch) does, so
    the index choice is identical and only rounding is left.

Measured on an MI355X (ROCm 7), the worst ratios the tests print:
  * GELU, |got - want| / (EGRAD |dy alpha| + r |want|): act_backward 0.613 (fp32, n = 2 098 179, alpha = 1/3) and 0.996 (bf16, n = 4 196 359,
    alpha = 1); pixel_unshuffle_actgrad 0.446 (fp32, c = 12) and 0.990 (bf16, c = 24).  The bf16 figures sit at 1 by construction: 2^-8 is the
    unit roundoff of bf16, and among millions of values some land half an ulp from a value just above a power of two.
  * upsample2x_ac, err / (2^-24 S), largest at (1, 256, 520, 2) with scale 1/3: forward 3.543 (asserted 8), backward 2.919 (asserted 16);
    (1, 64, 112, 2): 2.957 / 2.332; (2, 5, 3, 2): 2.510 / 1.178; (3, 1, 1, 2): 0.772 / 0.913.
    Before ac_src() in csrc/spynet.hip kept its product from being contracted, the forward measured 1 272.8 at (1, 64, 112, 2) and 31 875.2 at
    (1, 256, 520, 2): the compiler had fused `s - (float)i0` into fma(ratio, dst, -i0), so the weight came from the unrounded product and the
    index from the rounded one -- a coordinate error of up to 2^-24 s that no operation count of the interpolation covers (and a weight
    below 0 wherever the product rounds up to an integer).  The kernel was wrong, not the count; the bounds stand as derived."""
import functools
import gc

import pytest
import torch

from tests import glue_ref as G
from tests import tab_ops_ref as TR
from tests.test_linear_kernels_gpu import EGRAD

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
DT_ID = {F32: "fp32", BF16: "bf16"}
VN = {F32: 4, BF16: 8}           # elements of a 16-byte vector
U = {F32: 2.0 ** -24, BF16: 2.0 ** -8}
ACTS = [(G.ACT_NONE, "none"), (G.ACT_RELU, "relu"), (G.ACT_LRELU, "lrelu"), (G.ACT_GELU, "gelu")]
SLOPE = 0.1
NAN, INF = float("nan"), float("inf")
SPECIALS = [0.0, -0.0, 2.0 ** -130, INF, -INF, NAN]  # (2^-130: a denormal of fp32 AND of bf16)


def cdiv(a, b):
    return -(-a // b)


def chunks_for(frames, fv):
    """Blocks per frame of frame_gather / pair_steps / pair_steps_range (csrc/elementwise.hip)."""
    return max(1, min(cdiv(2048, frames), cdiv(fv, 256)))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, dtype):
    """Seeded normal values, rounded to `dtype`, on the CPU."""
    return torch.randn(tuple(shape), generator=_gen(seed)).to(dtype)


def dev(t, offset=0):
    """The CPU tensor on the device; offset > 0: as a contiguous view `offset` elements into a flat buffer -- not 16-byte aligned."""
    if not offset:
        out = t.cuda()
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device="cuda")
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def poison(*outs):
    """Fill the blocks the next allocations of these (shape, dtype) -- in this order -- come from with NaN (0x7F bytes for uint8), as
    test_tab_ops_gpu.py does for the max-pool backward.  All are held at once, then freed.  Returns their addresses for `poisoned`.  Every
    operand of the call must be on the device already: nothing may be allocated between this and the call."""
    stale = [torch.full(tuple(shape), 0x7F if dtype == torch.uint8 else NAN, dtype=dtype, device="cuda") for shape, dtype in outs]
    ptrs = [t.data_ptr() for t in stale]
    del stale
    return ptrs


def poisoned(ptrs, *outs):
    """The outputs were allocated from the blocks `poison` filled, so an element that is clean now was written by the kernel."""
    return [t.data_ptr() for t in outs] == ptrs


@pytest.fixture(scope="module", autouse=True)
def _module_memory():
    """Garbage of earlier modules is collected before the first poison (a collection between a poison and its call could free a device block
    and change the allocator's answer); the cached CPU operands (about 200 MB) are dropped when the module is done."""
    gc.collect()
    yield
    for cached in (act_operands, _pool, sum_operand):
        cached.cache_clear()


def clean(t):
    return not bool(torch.isnan(t).any())


def same_bits(got, want):
    got = got.cpu()
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(G.bits(got), G.bits(want))


def zero_bits(t):
    return int(G.bits(t).ne(0).sum()) == 0


def plant(ref, positions, rot):
    """SPECIALS at the given flat positions, cyclically, starting at SPECIALS[rot]."""
    flat = ref.view(-1)
    for k, p in enumerate(positions):
        flat[p] = SPECIALS[(k + rot) % len(SPECIALS)]
    return ref


def gelu_check(got, want, mag, dtype, what):
    """|got - want| <= EGRAD * |dy * alpha| + r |want|; NaN exactly where the fp64 formula is NaN.  Prints the worst ratio."""
    got = got.cpu().double()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN at other places than the reference"
    ok = ~nan
    err = (got - want).abs()[ok]
    tol = (EGRAD * mag + U[dtype] * want.abs())[ok]
    ratio = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: worst |got - want| / (EGRAD |dy alpha| + {'2^-24' if dtype == F32 else '2^-8'} |want|) = {ratio:.3f}")
    assert bool((err <= tol).all()), f"{what}: ratio {ratio:.3f}"


# ================================================================================================ act_backward
def act_sizes(dtype):
    vn = VN[dtype]
    sizes = [("n1", 1), ("vn-1_tail_only", vn - 1), ("vn_one_vector", vn), ("vn+1_tail", vn + 1), ("256vn+3_two_blocks_tail", 256 * vn + 3),
             ("gridwrap_tail", 2048 * 256 * vn + 256 * vn + (vn - 1))]
    if dtype == F32:  # vmg_act_bwd sizes its grid by n / 8 for both dtypes: at the size above fp32 wraps with 1025 blocks; this one reaches the cap
        sizes.append(("gridwrap_cap2048_tail", 2048 * 256 * 8 + 256 * 8 + 3))
    return sizes


ACT_CASES = [(d, a, lab, n) for d in DTYPES for a in ACTS for lab, n in act_sizes(d)]


@functools.lru_cache(maxsize=6)
def act_operands(dtype, n):
    return rnd((n,), 100, dtype), rnd((n,), 101, dtype)


def special_positions(n, vn):
    """First, last, last of the vector body, first of the scalar tail -- and their neighbours, so that every special value occurs near each."""
    body = n // vn * vn
    cand = list(range(0, 6)) + list(range(body - 6, body)) + list(range(body, body + vn)) + list(range(n - 6, n))
    return sorted({p for p in cand if 0 <= p < n})


@pytest.mark.parametrize("dtype,act,label,n", ACT_CASES, ids=[f"{DT_ID[d]}-{a[1]}-{lab}" for d, a, lab, n in ACT_CASES])
def test_act_backward(dtype, act, label, n):
    """dy * alpha * act'(ref) for alpha in {1, 1/2, 1/3}: NONE / RELU / LRELU are ((dy * d) * alpha) in fp32 rounded once -- bits; where ref is NaN
    the reference's d is the `else` side (0 / slope).  GELU within the bound of the module docstring.  ref holds +0, -0, a denormal, +-inf and NaN
    at the first and last element, the last of the vector body and the first of the scalar tail (every rotation of the six values where the tensor is small)."""
    from vmg_amd import kernels as K
    vn = VN[dtype]
    dy, ref0 = act_operands(dtype, n)
    pos = special_positions(n, vn)
    if label.startswith("gridwrap"):
        blocks = min(2048, cdiv(n // 8 + 1, 256))  # (vmg_act_bwd sizes its grid by n / 8 for both dtypes: fp32 wraps below the cap already)
        assert n // vn > blocks * 256 and n % vn == vn - 1
        assert (dtype == F32 and label == "gridwrap_tail") or cdiv(n // 8 + 1, 256) > 2048
    dyd = dev(dy)
    for rot in (range(6) if n < 10000 else (0,)):
        ref = plant(ref0.clone(), pos, rot)
        refd = dev(ref)
        for i, alpha in enumerate((1.0, 0.5, 1.0 / 3.0)):
            if n >= 10000:  # another rotation per alpha: over the three, each boundary element sees three of the values
                ref = plant(ref0.clone(), pos, 2 * i)
                refd = dev(ref)
            p = poison(((n,), dtype))
            got = K.act_backward(dyd, refd, act[0], SLOPE, alpha)
            assert got.dtype == dtype and tuple(got.shape) == (n,) and poisoned(p, got)
            what = f"act_backward {DT_ID[dtype]} {act[1]} n = {n} alpha = {alpha:.3g} rot = {rot}"
            if act[0] == G.ACT_GELU:
                want, mag = G.act_backward_ref(dy, ref, act[0], SLOPE, alpha, dtype)
                gelu_check(got, want, mag, dtype, what)
                continue
            want = G.act_backward_ref(dy, ref, act[0], SLOPE, alpha, dtype)
            assert clean(got), what + ": poison (or a NaN from a finite dy) in the output"
            bad = G.bits(got.cpu()) != G.bits(want)
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ, first at {int(bad.nonzero()[0])}"


# ================================================================================================ pixel_shuffle / pixel_unshuffle
PS_C = [1, 3, 4, 8, 12, 24]
PS_SHAPES = [(1, 1, 1), (2, 5, 7), (1, 3, 130)]


def _route(c, dtype):
    return "vector" if c % VN[dtype] == 0 else "scalar"


PS_CASES = [(d, c, s) for d in DTYPES for c in PS_C for s in PS_SHAPES]


def _shuffle_roundtrip(dtype, c, shape, offset=0):
    from vmg_amd import kernels as K
    N, H, W = shape
    x = rnd((N, H, W, 4 * c), 200 + c, dtype)
    y = rnd((N, 2 * H, 2 * W, c), 300 + c, dtype)               # (the inverse also runs on values of its own)
    xd, yd = dev(x, offset), dev(y, offset)
    p = poison(((N, 2 * H, 2 * W, c), dtype))
    up = K.pixel_shuffle(xd, N, H, W)
    assert tuple(up.shape) == (N, 2 * H, 2 * W, c) and poisoned(p, up) and clean(up)
    assert same_bits(up, G.pixel_shuffle_ref(x))
    p = poison(((N, H, W, 4 * c), dtype))
    back = K.pixel_unshuffle(up, N, H, W)
    assert tuple(back.shape) == (N, H, W, 4 * c) and poisoned(p, back) and clean(back)
    assert same_bits(back, x)                                   # unshuffle(shuffle(x)) == x
    p = poison(((N, H, W, 4 * c), dtype))
    down = K.pixel_unshuffle(yd, N, H, W)
    assert poisoned(p, down) and clean(down) and same_bits(down, G.pixel_unshuffle_ref(y))


@pytest.mark.parametrize("dtype,c,shape", PS_CASES, ids=[f"{DT_ID[d]}-c{c}-{_route(c, d)}-{'x'.join(map(str, s))}" for d, c, s in PS_CASES])
def test_pixel_shuffle_and_unshuffle(dtype, c, shape):
    """Depth-to-space takes the 16-byte-vector kernel when c is a multiple of the vector (8 bf16 / 4 fp32: c = 4 and 12 are scalar in bf16 and
    vector in fp32, 1 and 3 scalar in both) and the element kernel otherwise; space-to-depth is always the element kernel."""
    _shuffle_roundtrip(dtype, c, shape)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_pixel_shuffle_misaligned_takes_the_scalar_route(dtype):
    """c = 24 is whole vectors, but the input starts one element into its buffer: the element kernel, the same values."""
    _shuffle_roundtrip(dtype, 24, (2, 5, 7), offset=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_pixel_shuffle_scalar_kernels_past_the_block_cap(dtype):
    """(2, 96, 96) x c = 65: N H W c = 1 198 080 threads' worth against 4096 blocks x 256, in both directions of the element kernel."""
    assert 2 * 96 * 96 * 65 > 4096 * 256 and 65 % VN[dtype]
    _shuffle_roundtrip(dtype, 65, (2, 96, 96))


# ================================================================================================ pixel_unshuffle_actgrad
PUA_CASES = [(d, a, k, s) for d in DTYPES for a in ACTS for k in (1, 3) for s in [(1, 1, 1), (2, 5, 7)]]


@pytest.mark.parametrize("dtype,act,k,shape", PUA_CASES, ids=[f"{DT_ID[d]}-{a[1]}-c{k}vn-{'x'.join(map(str, s))}" for d, a, k, s in PUA_CASES])
def test_pixel_unshuffle_actgrad(dtype, act, k, shape):
    """out[n, y, x, 4c + 2i + j] = dy[n, 2y + i, 2x + j, c] * alpha * act'(ref[same]): pixel_unshuffle_ref(act_backward_ref(...)), bits; GELU
    within its bound.  ref holds the special values at its first and last elements."""
    from vmg_amd import kernels as K
    N, H, W = shape
    c = k * VN[dtype]
    dy = rnd((N, 2 * H, 2 * W, c), 400, dtype)
    ref = rnd((N, 2 * H, 2 * W, c), 401, dtype)
    numel = ref.numel()
    plant(ref, list(range(6)) + list(range(numel - 6, numel)), 0)
    dyd, refd = dev(dy), dev(ref)
    for alpha in (1.0, 1.0 / 3.0):
        p = poison(((N, H, W, 4 * c), dtype))
        got = K.pixel_unshuffle_actgrad(dyd, None if act[0] == G.ACT_NONE else refd, N, H, W, act[0], SLOPE, alpha)
        assert got.dtype == dtype and tuple(got.shape) == (N, H, W, 4 * c) and poisoned(p, got)
        what = f"pixel_unshuffle_actgrad {DT_ID[dtype]} {act[1]} c = {c} {shape} alpha = {alpha:.3g}"
        if act[0] == G.ACT_GELU:
            want, mag = G.act_backward_ref(dy, ref, act[0], SLOPE, alpha, dtype)
            gelu_check(got, G.pixel_unshuffle_ref(want), G.pixel_unshuffle_ref(mag), dtype, what)
        else:
            assert clean(got), what
            assert same_bits(got, G.pixel_unshuffle_ref(G.act_backward_ref(dy, ref, act[0], SLOPE, alpha, dtype))), what


# ================================================================================================ frame_gather
FG_FV = [1, 255, 256, 257, 1000, 2051]
FG_NDST = [1, 3, 10, 2049]
FG_CASES = [(d, fv, nd) for d in DTYPES for fv in FG_FV for nd in FG_NDST]
FG_IDS = [f"{DT_ID[d]}-fv{fv}-ndst{nd}-chunks{chunks_for(nd, fv)}" for d, fv, nd in FG_CASES]


@functools.lru_cache(maxsize=2)
def _pool(dtype):
    """One seeded pool of values per dtype; the frame tests slice their sources from it."""
    return rnd((2049 * 2051 * VN[dtype],), 500, dtype)


def _fg_assert_reach(fv, n_dst):
    """The launch shapes these cases are here for, from the formula of the launch function."""
    ch = chunks_for(n_dst, fv)
    if (fv, n_dst) == (2051, 3):
        assert ch == 9 and len({fv * (k + 1) // ch - fv * k // ch for k in range(ch)}) > 1  # nine chunks of unequal length
    if n_dst == 2049:
        assert ch == 1 and n_dst * ch > 2048
    if fv <= 256:
        assert ch == 1
    if fv == 257 and n_dst <= 10:
        assert ch == 2
    return ch


@pytest.mark.parametrize("dtype,fv,n_dst", FG_CASES, ids=[i + "-nsrc1" for i in FG_IDS])
def test_frame_gather_copy(dtype, fv, n_dst):
    """nsrc = 1: dst frame f = src frame idx[f], for a permutation and for a table with repeats.  (Every index >= 0: that is the caller's
    contract with one column, and nothing here passes another.)"""
    from vmg_amd import kernels as K
    _fg_assert_reach(fv, n_dst)
    fe = fv * VN[dtype]
    g = _gen(510 + n_dst)
    src = _pool(dtype)[:n_dst * fe].view(n_dst, fe)
    srcd = dev(src)
    tables = {"permutation": torch.randperm(n_dst, generator=g), "repeats": torch.randint(0, max(1, n_dst // 2), (n_dst,), generator=g)}
    for name, tab in tables.items():
        idx = tab.to(torch.int32).view(n_dst, 1)
        assert int(idx.min()) >= 0 and int(idx.max()) < n_dst
        idxd = idx.cuda()
        p = poison(((n_dst, fe), dtype))
        got = K.frame_gather(srcd, idxd, n_dst, (fe,))
        assert tuple(got.shape) == (n_dst, fe) and poisoned(p, got) and clean(got), name
        assert same_bits(got, G.frame_gather_ref(src, idx)), name


@pytest.mark.parametrize("dtype,fv,n_dst", FG_CASES, ids=[i + "-nsrc2" for i in FG_IDS])
def test_frame_gather_add(dtype, fv, n_dst):
    """nsrc = 2: 0 + a + b in fp32, one rounding; an index < 0 is no term: pairs, the first entry negative, the second, both (a frame of +0 bits),
    and all four kinds in one table."""
    from vmg_amd import kernels as K
    _fg_assert_reach(fv, n_dst)
    fe = fv * VN[dtype]
    n_src = 5
    g = _gen(520 + n_dst)
    src = _pool(dtype)[:n_src * fe].view(n_src, fe)
    srcd = dev(src)
    pairs = torch.randint(0, n_src, (n_dst, 2), generator=g, dtype=torch.int32)
    neg = torch.full((n_dst,), -1, dtype=torch.int32)
    kind = torch.arange(n_dst) % 4
    tables = {"pairs": pairs, "first_negative": torch.stack([neg, pairs[:, 1]], 1), "second_negative": torch.stack([pairs[:, 0], neg - 6], 1),
              "both_negative": torch.stack([neg, neg], 1),
              "mixed": torch.stack([torch.where((kind == 1) | (kind == 3), neg, pairs[:, 0]), torch.where(kind >= 2, neg, pairs[:, 1])], 1)}
    if n_dst * fv > 1 << 20:  # 67 MB of output: the table that holds all four kinds of row (a row does not depend on the others), and the frames of +0
        tables = {"mixed": tables["mixed"], "both_negative": tables["both_negative"]}
    for name, idx in tables.items():
        idx = idx.contiguous()
        assert int(idx.max()) < n_src
        idxd = idx.cuda()
        p = poison(((n_dst, fe), dtype))
        got = K.frame_gather(srcd, idxd, n_dst, (fe,))
        assert tuple(got.shape) == (n_dst, fe) and poisoned(p, got) and clean(got), name
        assert same_bits(got, G.frame_gather_ref(src, idx)), name
        if name == "both_negative":
            assert zero_bits(got)


# ================================================================================================ sum_n
def sum_sizes(dtype):
    vn = VN[dtype]
    return [("1_vector", vn), ("255_vectors", 255 * vn), ("257_vectors_two_blocks", 257 * vn), ("gridwrap_4096x256+3_vectors", 4096 * 256 * vn + 3 * vn)]


SUM_CASES = [(d, k, lab, n) for d in DTYPES for k in ("2", "3", "4", "2_same_tensor", "3_one_twice") for lab, n in sum_sizes(d)]


@functools.lru_cache(maxsize=8)
def sum_operand(dtype, n, j):
    return rnd((n,), 600 + j, dtype)


@pytest.mark.parametrize("dtype,k,label,n", SUM_CASES, ids=[f"{DT_ID[d]}-src{k}-{lab}" for d, k, lab, n in SUM_CASES])
def test_sum_n(dtype, k, label, n):
    """The fp32 sum of 2..4 tensors in list order from 0, one rounding: a fixed order, so bits in both dtypes."""
    from vmg_amd import kernels as K
    if label.startswith("gridwrap"):
        assert n // VN[dtype] > 4096 * 256
    order = {"2": [0, 1], "3": [0, 1, 2], "4": [0, 1, 2, 3], "2_same_tensor": [0, 0], "3_one_twice": [0, 1, 0]}[k]
    cpu = [sum_operand(dtype, n, j) for j in sorted(set(order))]
    gpu = [dev(t) for t in cpu]
    p = poison(((n,), dtype))
    got = K.sum_n([gpu[j] for j in order])
    assert got.dtype == dtype and poisoned(p, got) and clean(got)
    assert same_bits(got, G.sum_n_ref([cpu[j] for j in order]))


# ================================================================================================ cast_clear
CC_SIZES = [("n4_one_thread", 4), ("n1020_255_threads", 1020), ("n1028_two_blocks", 1028), ("gridwrap_4096x256x4+4", 4096 * 256 * 4 + 4)]
CC_CASES = [(d, add, lab, n) for d in DTYPES for add in (False, True) for lab, n in CC_SIZES]


@pytest.mark.parametrize("dtype,add,label,n", CC_CASES, ids=[f"out_{DT_ID[d]}-{'add' if a else 'noadd'}-{lab}" for d, a, lab, n in CC_CASES])
def test_cast_clear(dtype, add, label, n):
    """(acc [+ add]) rounded once to the output dtype (bf16 AND fp32); the accumulator is all zero bits afterwards."""
    from vmg_amd import kernels as K
    if label.startswith("gridwrap"):
        assert n // 4 > 4096 * 256
    acc = rnd((n,), 700, F32)
    addt = rnd((n,), 701, dtype) if add else None
    accd, addd = dev(acc), dev(addt) if add else None
    p = poison(((n,), dtype))
    got = K.cast_clear(accd, dtype, add=addd)
    assert got.dtype == dtype and poisoned(p, got) and clean(got)
    assert same_bits(got, G.cast_clear_ref(acc, addt, dtype))
    assert zero_bits(accd), "the accumulator is not all +0 afterwards"


# ================================================================================================ pair_steps / pair_steps_range
PS_NT = [(1, 1), (2, 5), (1, 65), (2, 70)]
PS_FV = [60, 257, 2051]
PAIR_CASES = [(d, m, nt, fv) for d in DTYPES for m in (0, 1, 2) for nt in PS_NT for fv in PS_FV]


def _pair_launches(mode, n, t):
    """(frames, ...) per launch: one launch up to 64 steps, else ranges of 64 steps (modes 0, 1) or 32 destination frames (mode 2)."""
    per_frame = n if mode == 2 else 2 * n
    if t <= 64:
        return [per_frame * t]
    per = 32 if mode == 2 else 64
    return [per_frame * min(per, t - j0) for j0 in range(0, t, per)]


def _pair_id(d, m, nt, fv):
    n, t = nt
    ch = [chunks_for(f, fv) for f in _pair_launches(m, n, t)]
    kern = "one_launch" if t <= 64 else f"range_x{len(ch)}"
    return f"{DT_ID[d]}-mode{m}-n{n}t{t}-fv{fv}-{kern}-chunks{'_'.join(map(str, ch))}"


@pytest.mark.parametrize("dtype,mode,nt,fv", PAIR_CASES, ids=[_pair_id(*c) for c in PAIR_CASES])
def test_pair_steps(dtype, mode, nt, fv):
    """The t step tensors (separate allocations) <-> the two sweeps' (n, t) features; mode 2 their fp32 sum with one rounding.  t > 64 takes
    pair_steps_range (mode 2: three ranges of at most 32 destination frames).  Destinations are NaN-filled before the call.  Bits."""
    from vmg_amd import kernels as K
    n, t = nt
    fe = fv * VN[dtype]
    launches = _pair_launches(mode, n, t)
    ch = [chunks_for(f, fv) for f in launches]
    if t > 64:
        assert len(launches) == (3 if mode == 2 else 2)
    if (n, t) == (1, 1):
        assert ch == [{60: 1, 257: 2, 2051: 9}[fv]]     # one or two frames: a frame is split as far as its vectors allow
    if (n, t) == (2, 70) and fv == 2051 and mode != 2:
        assert ch == [8, 9]                              # 256 frames x 8 chunks, then 24 frames x 9
    nan = lambda *shape: torch.full(shape, NAN, dtype=dtype, device="cuda")
    if mode == 1:
        a, b = rnd((n, t, fe), 800, dtype), rnd((n, t, fe), 801, dtype)
        steps = [nan(2 * n, fe) for _ in range(t)]
        K.pair_steps(1, steps, dev(a), dev(b), n, t)
        want = G.pair_steps_ref(1, n, t, a=a, b=b)
        for j in range(t):
            assert clean(steps[j]) and same_bits(steps[j], want[j]), f"step {j}"
        return
    cpu = list(rnd((t, 2 * n, fe), 802, dtype).unbind(0))
    steps = [dev(s.contiguous()) for s in cpu]
    assert len({s.data_ptr() for s in steps}) == t
    if mode == 0:
        a, b = nan(n, t, fe), nan(n, t, fe)
        K.pair_steps(0, steps, a, b, n, t)
        wa, wb = G.pair_steps_ref(0, n, t, steps=cpu)
        assert clean(a) and clean(b) and same_bits(a, wa.contiguous()) and same_bits(b, wb.contiguous())
    else:
        a = nan(n, t, fe)
        K.pair_steps(2, steps, a, None, n, t)
        assert clean(a) and same_bits(a, G.pair_steps_ref(2, n, t, steps=cpu))
    for s, c in zip(steps, cpu):
        assert same_bits(s, c.contiguous())              # the sources are untouched


# ================================================================================================ SPyNet glue
SPY_MEAN, SPY_STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
PREP_SHAPES = [(1, 3, 1, 1), (2, 3, 5, 7), (3, 3, 64, 112), (1, 3, 1024, 1030)]
PIX_SHAPES = [(1, 1, 1), (2, 5, 7), (1, 1024, 1030)]


def _wrap_id(s):
    pix = s[0] * s[-2] * s[-1]
    return "x".join(map(str, s)) + ("-gridwrap" if pix > 4096 * 256 else "-1_pixel" if pix == 1 else "")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("shape", PREP_SHAPES, ids=_wrap_id)
def test_spy_prep(shape, dtype):
    """(img - mean) / std: fp32 subtraction, fp32 division, one round-to-nearest-even, (n, 3, h, w) -> (n, h, w, 8); channels 3..7 are zero BITS."""
    from vmg_amd import kernels as K
    n, _, h, w = shape
    img = torch.rand(shape, generator=_gen(900))
    mean, std = torch.tensor(SPY_MEAN), torch.tensor(SPY_STD)
    imgd, meand, stdd = dev(img), dev(mean), dev(std)
    p = poison(((n, h, w, 8), dtype))
    got = K.spy_prep(imgd, meand, stdd, dtype)
    assert got.dtype == dtype and tuple(got.shape) == (n, h, w, 8) and poisoned(p, got) and clean(got)
    assert zero_bits(got[..., 3:])
    assert same_bits(got, G.spy_prep_ref(img, mean, std, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("shape", PIX_SHAPES, ids=_wrap_id)
def test_spy_operand_forward_backward(shape, dtype):
    """[ref RGB | warped RGB | flow] and the split of its gradient (d warped: zero bits behind the RGB; d flow in fp32).  Bits."""
    from vmg_amd import kernels as K
    ref, warped, up = rnd((*shape, 8), 910, dtype), rnd((*shape, 8), 911, dtype), rnd((*shape, 2), 912, F32)
    dx8 = rnd((*shape, 8), 913, dtype)
    refd, warpedd, upd, dx8d = dev(ref), dev(warped), dev(up), dev(dx8)
    p = poison(((*shape, 8), dtype))
    got = K.spy_operand(refd, warpedd, upd)
    assert poisoned(p, got) and clean(got) and same_bits(got, G.spy_operand_ref(ref, warped, up))
    p = poison(((*shape, 8), dtype), ((*shape, 2), F32))  # both held at once: one pixel of either rounds to the same block size
    dw, du = K.spy_operand_backward(dx8d)
    wdw, wdu = G.spy_operand_bwd_ref(dx8)
    assert poisoned(p, dw, du) and clean(dw) and clean(du) and du.dtype == F32
    assert zero_bits(dw[..., 3:])
    assert same_bits(dw, wdw) and same_bits(du, wdu)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("shape", PIX_SHAPES, ids=_wrap_id)
def test_spy_flow_add(shape, dtype):
    """up (fp32) + res (compute dtype) in fp32: one addition, bits."""
    from vmg_amd import kernels as K
    up, res = rnd((*shape, 2), 920, F32), rnd((*shape, 2), 921, dtype)
    upd, resd = dev(up), dev(res)
    p = poison(((*shape, 2), F32))
    got = K.spy_flow_add(upd, resd)
    assert got.dtype == F32 and poisoned(p, got) and clean(got) and same_bits(got, G.spy_flow_add_ref(up, res))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_avgpool2_past_the_block_cap(dtype):
    """(2, 512, 520, 8): 1 064 960 outputs against 4096 blocks x 256.  Integer inputs: the four-term sum and its quarter are exact."""
    from vmg_amd import kernels as K
    shape = (2, 512, 520, 8)
    assert 2 * 256 * 260 * 8 > 4096 * 256
    x = torch.randint(-4, 5, shape, generator=_gen(930)).float()
    xd = dev(x.to(dtype))
    p = poison(((2, 256, 260, 8), dtype))
    got = K.avgpool2(xd)
    assert got.dtype == dtype and poisoned(p, got) and clean(got)
    assert torch.equal(got.cpu().double(), TR.avgpool2_ref(x)[0])


# ================================================================================================ upsample2x_ac
UP_SHAPES = [(3, 1, 1, 2), (2, 5, 3, 2), (1, 64, 112, 2), (1, 256, 520, 2)]
UP_FWD, UP_BWD = 8, 16  # roundings counted in the module docstring


@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "x".join(map(str, s)) + ("-fwd_gridwrap" if 4 * s[0] * s[1] * s[2] * s[3] > 4096 * 256 else ""))
def test_upsample2x_ac_forward_backward(shape):
    """scale * bilinear x2 (align_corners=True) and its transpose, per element within 8 (forward) / 16 (backward) x 2^-24 x S of the fp64 reference
    whose coordinates are the kernel's; the backward is a gather in a fixed order: two calls give equal bits."""
    from vmg_amd import kernels as K
    n, h, w, c = shape
    x, g = rnd(shape, 940, F32), rnd((n, 2 * h, 2 * w, c), 941, F32)
    xd, gd = dev(x), dev(g)
    u = 2.0 ** -24
    for scale in (2.0, 1.0 / 3.0):
        p = poison(((n, 2 * h, 2 * w, c), F32))
        got = K.upsample2x_ac(xd, scale)
        assert tuple(got.shape) == (n, 2 * h, 2 * w, c) and poisoned(p, got) and clean(got)
        want, S = G.upsample2x_ac_ref(x, scale)
        err = (got.cpu().double() - want).abs()
        ratio = float((err / (u * S).clamp_min(1e-300)).max())
        print(f"upsample2x_ac forward {shape} scale {scale:.3g}: worst err / (2^-24 S) = {ratio:.3f} (asserted {UP_FWD})")
        assert bool((err <= UP_FWD * u * S).all())
        p = poison((shape, F32))
        back = K.upsample2x_ac(gd, scale, backward=True)
        assert tuple(back.shape) == tuple(shape) and poisoned(p, back) and clean(back)
        want, S = G.upsample2x_ac_adjoint_ref(g, scale)
        err = (back.cpu().double() - want).abs()
        ratio = float((err / (u * S).clamp_min(1e-300)).max())
        print(f"upsample2x_ac backward {shape} scale {scale:.3g}: worst err / (2^-24 S) = {ratio:.3f} (asserted {UP_BWD})")
        assert bool((err <= UP_BWD * u * S).all())
        p = poison((shape, F32))
        again = K.upsample2x_ac(gd, scale, backward=True)
        assert poisoned(p, again) and torch.equal(G.bits(again), G.bits(back))


# ================================================================================================ refusals
# Each raises HipError on the host, before any launch, and a following valid call is still correct.
def _raises():
    from vmg_amd.hip import HipError
    return pytest.raises(HipError)


def _misaligned(t):
    """A contiguous view one element (2 or 4 bytes) into a buffer."""
    return dev(t, offset=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_refusals_act_backward_and_actgrad(dtype):
    from vmg_amd import kernels as K
    vn = VN[dtype]
    dy, ref = rnd((4 * vn,), 950, dtype), rnd((4 * vn,), 951, dtype)
    with _raises():
        K.act_backward(_misaligned(dy), _misaligned(ref), G.ACT_RELU, 0.0, 1.0)        # 2-byte (bf16) / 4-byte (fp32) misaligned views
    with _raises():
        K.act_backward(dev(dy), dev(ref.float() if dtype == BF16 else ref.to(BF16)), G.ACT_RELU, 0.0, 1.0)
    assert same_bits(K.act_backward(dev(dy), dev(ref), G.ACT_RELU, 0.0, 1.0), G.act_backward_ref(dy, ref, G.ACT_RELU, 0.0, 1.0, dtype))
    c = vn // 2                                                                      # whole pixels, but no whole vector of channels
    d2, r2 = rnd((1, 2, 2, c), 952, dtype), rnd((1, 2, 2, c), 953, dtype)
    with _raises():
        K.pixel_unshuffle_actgrad(dev(d2), dev(r2), 1, 1, 1, G.ACT_RELU, 0.0, 1.0)
    with _raises():
        K.pixel_unshuffle_actgrad(dev(d2), None, 1, 1, 1, G.ACT_NONE, 0.0, 1.0)
    d3, r3 = rnd((1, 2, 2, vn), 954, dtype), rnd((1, 2, 2, vn), 955, dtype)
    got = K.pixel_unshuffle_actgrad(dev(d3), dev(r3), 1, 1, 1, G.ACT_RELU, 0.0, 1.0)
    assert same_bits(got, G.pixel_unshuffle_ref(G.act_backward_ref(d3, r3, G.ACT_RELU, 0.0, 1.0, dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_refusals_sum_n_and_cast_clear(dtype):
    from vmg_amd import kernels as K
    vn = VN[dtype]
    ts = [rnd((2 * vn,), 960 + j, dtype) for j in range(5)]
    td = [dev(t) for t in ts]
    with _raises():
        K.sum_n(td[:1])
    with _raises():
        K.sum_n(td)
    with _raises():
        K.sum_n([dev(t[:vn + 1].clone()) for t in ts[:2]])                             # no whole vectors
    with _raises():
        K.sum_n([td[0], td[1].float() if dtype == BF16 else td[1].to(BF16)])
    assert same_bits(K.sum_n(td[:3]), G.sum_n_ref(ts[:3]))
    acc, add = rnd((8,), 970, F32), rnd((8,), 971, dtype)
    with _raises():
        K.cast_clear(dev(acc[:6].clone()), dtype)                                      # n % 4 != 0
    with _raises():
        K.cast_clear(dev(acc), dtype, add=dev(add.float() if dtype == BF16 else add.to(BF16)))  # `add` of the other dtype
    accd = dev(acc)
    assert same_bits(K.cast_clear(accd, dtype, add=dev(add)), G.cast_clear_ref(acc, add, dtype)) and zero_bits(accd)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_refusals_frame_gather_and_pair_steps(dtype):
    from vmg_amd import kernels as K
    vn = VN[dtype]
    idx = torch.tensor([[2], [0], [1]], dtype=torch.int32)
    odd = rnd((3, vn + 1), 980, dtype)
    with _raises():
        K.frame_gather(dev(odd), idx.cuda(), 3, (vn + 1,))                             # a frame that is not whole vectors
    with _raises():
        K.frame_gather(dev(odd[:, :vn].contiguous()), idx.long().cuda(), 3, (vn,))     # the table must be int32
    src = rnd((3, 2 * vn), 981, dtype)
    assert same_bits(K.frame_gather(dev(src), idx.cuda(), 3, (2 * vn,)), G.frame_gather_ref(src, idx))
    n, t, fe = 2, 3, 2 * vn
    cpu = list(rnd((t, 2 * n, fe), 982, dtype).unbind(0))
    steps = [dev(s.contiguous()) for s in cpu]
    other = F32 if dtype == BF16 else BF16
    a, b = torch.empty((n, t, fe), dtype=dtype, device="cuda"), torch.empty((n, t, fe), dtype=dtype, device="cuda")
    with _raises():
        K.pair_steps(0, steps[:2] + [steps[2].to(other)], a, b, n, t)                  # a step tensor of the other dtype
    with _raises():
        K.pair_steps(0, steps[:2], a, b, n, t)                                          # t - 1 step tensors
    K.pair_steps(0, steps, a, b, n, t)
    wa, wb = G.pair_steps_ref(0, n, t, steps=cpu)
    assert same_bits(a, wa.contiguous()) and same_bits(b, wb.contiguous())
