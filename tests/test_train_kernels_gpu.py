"""The seven kernels that end a training step -- csrc/optim.hip: adamw_flat_kernel, grad_sumsq_kernel, grad_clip_scale_kernel; csrc/loss.hip:
lap_even_blur_kernel, lap_fwd_kernel, lap_bwd_even_kernel, lap_bwd_kernel -- through the C ABI, every element of every tensor they write
against the fp64 references and the derived bounds of tests/train_ref.py (checked on the CPU by tests/test_train_ref.py).  No asserted
constant is a measured figure; the tests print the worst error / bound ratio (RATIO lines of a run with -s).

  AdamW: one step from a planted state (classes in STATE_CLASSES, laid out in runs of four so that the float4 body and the n % 4 tail both
    see them), n = 1, 3, 4, 5, 1023, 4 * 1024 + 1 and 8192 * 1024 + 4 * 300 + 3 (past the 8192-block cap: the grid stride and the tail in one
    launch), hyper rows read from row 1.. of a device tensor: t = 1 / 10 000, wd = 0 / 0.05, lr = 0 with wd != 0.
  clip: n = 1, 3, 4, 5, 4 * 1023 + 2 (most blocks empty, the tail in the last), 4 * 1024 * 3 + 1, 262 147 and 67 108 864 + 4 * 1024 * 300 + 3 (the
    k == 64 flush and two more trips; built and compared on the device); max_norm far below, far above and one fp32 step either side of
    norm + 1e-6; all-zero, one Inf, one NaN (body and tail).
  loss: (H, W) = (3,3) (3,4) (4,3) (4,4) (5,3) (6,7) (33,18) x planes 1 / 7 x eps 1e-12 / 1e-6 x (gs1, gs2) = (1/n, 0.005/n) (0,1) (1,0); planted
    planes (PLANE_KINDS); 64 x 257 x 256 (past the 16 384-block cap of the full-size kernels) and 256 x 257 x 255 (past it for the quarter-size
    kernels too), evaluated in fp64 on the device.  The backward reference starts from the forward KERNEL's ld.

Worst error / bound ratios, measured on an MI355X (all 1.0 or below is a pass; none of the bounds was adjusted to them):
  AdamW, per state class (p / m / v), every one at n = 8 389 811 (8 million elements sample the worst case best; p at row t1_wd, m and v at t10000):
    fresh 0.674 / 0.707 / 0.934    warm 0.730 / 0.995 / 0.961    still 0.425 / 0 / 0    small_g 0.656 / 0.707 / 0.933
    tiny_g 0.425 / 0.519 / 0.376   big_g 0.606 / 0.761 / 0.829   p_zero 0.677 / 0.707 / 0.934
    (m of a warm state at 0.995: its bound is the three roundings of M + c1 (G - M) and nothing else, so the worst element sits on it.)
  clip: norm 0.250 (n = 3, max_norm 1e6); block partials 0.451 (n = 4094); coefficient and buffer are compared bit for bit.
  loss, the 28 small cases:  a1 0.210 (7x3x4, eps 1e-6)  ld 0.275 (1x33x18, 1e-6)  sum1 0.205 (7x4x3, 1e-12)  sum2 0.044 (1x5x3, 1e-6)
                             u 0.205 (7x4x3, 1e-6, gs (1,0))  dx 0.365 (7x33x18, 1e-6, gs (1/n, 0.005/n))
  loss, past the grid caps:  a1 0.314  u 0.128  dx 0.552  sum1, sum2 0.001 (256x257x255);  ld 0.416 (64x257x256)
The NaN cases of the clip (test_clip_with_one_nan_poisons_everything_as_torch_does) failed on the kernel as it was before this file: it
replaced a NaN coefficient by 1 and returned."""
import math

import numpy as np
import pytest
import torch

from tests import train_ref as R

pytestmark = pytest.mark.gpu

F64, F32, U = R.F64, R.F32, R.U
NAN = float("nan")
B1, B2, EPS = 0.9, 0.99, 1e-8


def _lib():
    from vmg_amd import hip
    return hip, hip.lib()


def _ratio(tag, name, got, want, bound):
    """Every element within its bound; prints the worst error / bound ratio."""
    assert got.shape == want.shape, (tag, name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{tag} {name}: non-finite values (an element the kernel skipped, or a wrong one)"
    r = R.worst_ratio(got, want, bound)
    print(f"RATIO {tag} {name} {r:.3f}")
    if not r <= 1.0:
        err = (got.to(F64) - want).abs()
        bad = (~(err <= bound)).nonzero()
        k = tuple(bad[0].tolist())
        raise AssertionError(f"{tag} {name}: {bad.shape[0]} of {want.numel()} elements out of bound, worst ratio {r:.3f}; first at {k}: "
                             f"got {float(got[k])!r} want {float(want[k])!r} bound {float(bound[k]):.3e}")
    return r


# ================================================================================================ AdamW
STATE_CLASSES = ["fresh", "warm", "still", "small_g", "tiny_g", "big_g", "p_zero"]
BIG_N = 8192 * 1024 + 4 * 300 + 3
ADAMW_N = [1, 3, 4, 5, 1023, 4 * 1024 + 1]
HYPERS = {"t1_wd": dict(t=1, lr=2e-3, wd=0.05), "t1": dict(t=1, lr=2e-3, wd=0.0), "t10000_wd": dict(t=10000, lr=2e-3, wd=0.05),
          "t10000": dict(t=10000, lr=2e-4, wd=0.0), "lr0_wd": dict(t=1, lr=0.0, wd=0.05)}
ADAMW_CASES = [(n, h) for n in ADAMW_N for h in HYPERS] + [(BIG_N, "t1_wd"), (BIG_N, "t10000")]


def adamw_state(n):
    """(p, g, m, v, cls, special) on the CPU, fp32: the class of element i is (i // 4) % 7, the n % 4 tail (and the whole of a tiny buffer) is
    small_g, p_zero, warm, ...; for n >= 64 one NaN and one Inf gradient, each the only non-finite value of its float4."""
    gen = torch.Generator().manual_seed(1000 + n % 9973)
    i = torch.arange(n)
    cls = (i // 4) % 7
    tail = torch.tensor([3, 6, 1, 0, 3, 6, 5, 4, 2] * 2)
    if n < 16:
        cls = tail[:n].clone()
    elif n % 4:
        cls[n - n % 4:] = tail[:n % 4]
    rn = lambda s: torch.randn(n, generator=gen) * s
    p, g = rn(0.1), rn(0.01)
    m, v = torch.zeros(n), torch.zeros(n)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    warm = (cls == 1) | (cls == 5)
    m[warm] = rn(0.01)[warm]
    v[warm] = rn(0.01).square()[warm]
    g[cls == 2] = 0.0
    p[(cls == 2) & (i % 8 == 0)] = -0.0
    expo = 4.0 + 8.0 * torch.rand(n, generator=gen)                       # |g| from 1e-4 down to 1e-12: across eps = 1e-8
    expo[cls == 3] = torch.where(i % 3 == 0, (4.0 + (i // 3) % 9).float(), expo)[cls == 3]  # (the exact decades too)
    g[cls == 3] = (sign * 10.0 ** -expo)[cls == 3]
    g[cls == 4] = (sign * torch.where(i % 2 == 0, 1e-20, 1e-23))[cls == 4]  # g^2: an fp32 denormal, then 0
    g[cls == 5] = (sign * 1e4)[cls == 5]
    p[cls == 6] = (sign * 0.0)[cls == 6]
    special = torch.zeros(n, dtype=torch.bool)
    if n >= 64:
        g[17], g[42] = NAN, float("inf")
        special[17] = special[42] = True
    return p, g, m, v, cls, special


def hyper_tensor():
    """Row 0 is NaN (never read); rows 1.. are HYPERS in order, as FlatAdamW._upload writes them: fl32 of (lr, wd, 1 - b1^t, sqrt(1 - b2^t))."""
    rows = [[NAN] * 4] + [[h["lr"], h["wd"], 1.0 - B1 ** h["t"], math.sqrt(1.0 - B2 ** h["t"])] for h in HYPERS.values()]
    return torch.tensor(rows, dtype=F64).to(F32).cuda()


@pytest.mark.parametrize("n,hname", ADAMW_CASES, ids=lambda v: str(v))
def test_adamw_one_step(n, hname):
    hip, lib = _lib()
    h = HYPERS[hname]
    row = 1 + list(HYPERS).index(hname)
    p, g, m, v, cls, special = adamw_state(n)
    pad = 8  # guard elements behind the segment: a store past n would show
    bufs = []
    for src, guard in ((p, 7.0), (g, 7.0), (m, 7.0), (v, 7.0)):
        b = torch.full((n + pad,), guard, dtype=F32, device="cuda")
        b[:n] = src.cuda()
        bufs.append(b)
    hy = hyper_tensor()
    hip.check(lib.vmg_adamw_flat(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), n, hy.data_ptr() + 16 * row, B1, B2,
                                 EPS, hip.stream_ptr()), "vmg_adamw_flat")
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[n:] == 7.0).all()), "wrote past n"
    assert torch.equal(R.bits(bufs[1][:n].cpu()), R.bits(g)), "the gradient changed"
    dev = "cuda" if n > (1 << 20) else "cpu"  # the reference runs where it is cheap
    pr, mr, vr, k = R.adamw_step_ref(p.to(dev), g.to(dev), m.to(dev), v.to(dev), h["lr"], h["wd"], B1, B2, EPS, h["t"])
    Bp, Bm, Bv = R.adamw_bounds(k)
    got = [b[:n].to(dev) for b in (bufs[0], bufs[2], bufs[3])]
    sp, cl = special.to(dev), cls.to(dev)
    # the NaN and the Inf gradient: their own p, m, v are what IEEE makes of them (NaN; m = v = Inf, p = NaN), nothing else is touched
    for name, gt, rf in zip("pmv", got, (pr, mr, vr)):
        assert torch.equal(~torch.isfinite(gt), sp), f"{name}: non-finite values elsewhere than at the NaN / Inf gradients"
        assert torch.equal(torch.isnan(gt), torch.isnan(rf)) and torch.equal(torch.isinf(gt), torch.isinf(rf)), name
        assert not bool(sp.any()) or bool((gt[sp & torch.isinf(rf)] == rf[sp & torch.isinf(rf)]).all())
    worst = {}
    for ci, cname in enumerate(STATE_CLASSES):
        sel = (cl == ci) & ~sp
        if not bool(sel.any()):
            continue
        for name, gt, rf, bd in zip("pmv", got, (pr, mr, vr), (Bp, Bm, Bv)):
            worst[(cname, name)] = _ratio(f"adamw n={n} {hname} {cname}", name, gt[sel], rf[sel], bd[sel])
    # g = 0 on a fresh state without decay: nothing may move, -0 included
    if h["lr"] * h["wd"] == 0.0:
        still = (cl == 2) & ~sp
        assert torch.equal(R.bits(got[0][still]), R.bits(p.to(dev)[still])), "p of a zero gradient on a zero state changed its bits"
        assert not bool(got[1][still].any()) and not bool(got[2][still].any())
    if h["lr"] == 0.0:  # lr = 0: only the moments move
        fin = ~sp
        same = R.bits(got[0][fin]) == R.bits(p.to(dev)[fin])
        assert bool((same | (p.to(dev)[fin] == 0)).all()), "lr = 0 moved a parameter"


def test_adamw_state_classes_hold_what_they_should():
    """A test of the test (no GPU work): the planted classes are present in the body and in the tail, and cross what they claim to cross."""
    p, g, m, v, cls, special = adamw_state(4 * 1024 + 1)
    assert sorted(set(cls.tolist())) == list(range(7)) and int(special.sum()) == 2 and int(cls[-1]) == 3
    sg = g[cls == 3].abs()
    assert float(sg.min()) < 1e-11 and float(sg.max()) > 5e-5 and bool(((sg > 5e-9) & (sg < 2e-8)).any())
    tg = g[cls == 4].double().abs()
    assert bool(((tg * tg < R.MIN_NORMAL) & (tg * tg > R.DENORM)).any()) and bool((tg * tg < R.DENORM / 2).any())
    assert bool((R.bits(p[cls == 6]) == 0).any()) and bool((R.bits(p[cls == 6]) < 0).any())
    assert sorted(set(adamw_state(5)[4].tolist())) == [0, 1, 3, 6] and int(adamw_state(3)[4][0]) == 3


def test_adamw_refusals_launch_nothing():
    hip, lib = _lib()
    p, g, m, v = (torch.full((64,), float(i + 1), dtype=F32, device="cuda") for i in range(4))
    hy = hyper_tensor()
    s = hip.stream_ptr()
    ptr = lambda t: t.data_ptr()
    args = lambda **kw: [kw.get("p", ptr(p)), kw.get("g", ptr(g)), kw.get("m", ptr(m)), kw.get("v", ptr(v)), kw.get("n", 8), kw.get("h", ptr(hy) + 16),
                         B1, B2, EPS, s]
    for name in "pgmv":
        assert lib.vmg_adamw_flat(*args(**{name: ptr(locals()[name]) + 4})) != 0, name
        assert b"16-byte" in lib.vmg_last_error()
        assert lib.vmg_adamw_flat(*args(**{name: None})) != 0, name
    assert lib.vmg_adamw_flat(*args(h=None)) != 0
    assert lib.vmg_adamw_flat(*args(n=0)) != 0
    assert lib.vmg_adamw_flat(*args(n=-4)) != 0
    torch.cuda.synchronize()
    for i, t in enumerate((p, g, m, v)):
        assert bool((t == float(i + 1)).all())


# ================================================================================================ gradient clip
CLIP_N = [1, 3, 4, 5, 4 * 1023 + 2, 4 * 1024 * 3 + 1, 262147]
CLIP_BIG_N = 67108864 + 4 * 1024 * 300 + 3
_CLIP_INPUT = {}


def clip_input(n):
    if n not in _CLIP_INPUT:
        gen = torch.Generator().manual_seed(77 + n)
        g = torch.randn(n, generator=gen) * 0.02
        if n >= 5:
            g[1], g[2] = -0.0, 0.0
        _CLIP_INPUT[n] = g
    return _CLIP_INPUT[n]


class Clip:
    """One gradient buffer (n + guard elements), the NaN-filled workspace and result of vmg_grad_clip_norm."""

    def __init__(self, n):
        self.hip, self.lib = _lib()
        self.n = n
        self.buf = torch.full((n + 8,), 7.0, dtype=F32, device="cuda")
        self.ws = torch.empty(int(self.lib.vmg_grad_clip_ws_bytes()), dtype=torch.uint8, device="cuda")
        self.out = torch.empty(2, dtype=F32, device="cuda")

    def run(self, g, max_norm):
        """-> (norm_out on the host as np.float32 x 2, the buffer's n elements, still on the device)."""
        self.buf[:self.n] = g.cuda() if g.device.type == "cpu" else g
        self.ws.fill_(0xFF)  # (NaN doubles)
        self.out.fill_(NAN)
        self.hip.check(self.lib.vmg_grad_clip_norm(self.buf.data_ptr(), self.n, float(max_norm), self.ws.data_ptr(), self.out.data_ptr(),
                                                   self.hip.stream_ptr()), "vmg_grad_clip_norm")
        torch.cuda.synchronize()
        assert bool((self.buf[self.n:] == 7.0).all()), "wrote past n"
        return self.out.cpu().numpy().copy(), self.buf[:self.n]


def same_bits(a, b):
    return torch.equal(R.bits(a), R.bits(b))


def check_clip(tag, c, g, max_norm, norm64):
    """Norm within its bound, coefficient = the fp32 formula from norm_out[0] bit for bit, buffer = fl32(g coef) or untouched bit for bit."""
    out, buf = c.run(g, max_norm)
    bound = R.clip_norm_bound(c.n, norm64)
    err = abs(float(out[0]) - norm64)
    print(f"RATIO clip {tag} norm {err / bound if bound else 0.0:.3f}")
    assert err <= bound, (tag, float(out[0]), norm64, bound)
    coef = R.clip_coef_ref(out[0], max_norm)
    assert coef.tobytes() == out[1].tobytes(), (tag, coef, out[1])
    gd = g.cuda() if g.device.type == "cpu" else g
    if coef < 1:
        assert same_bits(buf, gd * torch.tensor(float(coef), dtype=F32, device="cuda")), f"{tag}: the buffer is not fl32(g * coef)"
    else:
        assert same_bits(buf, gd), f"{tag}: a coefficient of 1 changed the buffer"
    return out, buf.clone()


@pytest.mark.parametrize("max_norm", [1e-5, 1e6])
@pytest.mark.parametrize("n", CLIP_N)
def test_clip_norm_coefficient_and_bits(n, max_norm):
    g = clip_input(n)
    norm64 = float(g.double().square().sum().sqrt())
    c = Clip(n)
    out1, buf1 = check_clip(f"n={n} max_norm={max_norm:g}", c, g, max_norm, norm64)
    assert (out1[1] < 1) == (max_norm < 1)
    out2, buf2 = c.run(g, max_norm)
    assert out1.tobytes() == out2.tobytes() and same_bits(buf1, buf2), "two runs differ"


@pytest.mark.parametrize("n", [3, 4 * 1023 + 2, 4 * 1024 * 3 + 1, 262147])
def test_clip_block_partials_and_the_owner_of_the_tail(n):
    """The workspace after a call: 1024 doubles, block b's sum of squares over its per = ceil(n4 / 1024) float4 (an empty range gives 0), and
    the n % 4 tail in the LAST block only -- whoever else added it, or nobody, the partial of that block is out of its bound.  Bound of a
    partial: the summation part of train_ref.clip_norm_bound, (1 + 3 + min(trips, 64)) U relative and DENORM / 2 per square."""
    g = clip_input(n)
    c = Clip(n)
    c.run(g, 1e6)
    got = c.ws.view(torch.float64).cpu()
    n4 = n // 4
    per = -(-n4 // R.CLIP_BLOCKS)
    trips = -(-per // 256)
    sq = g.double().square()
    body = torch.zeros(R.CLIP_BLOCKS * max(per, 1) * 4, dtype=F64)
    body[:4 * n4] = sq[:4 * n4]
    want = body.reshape(R.CLIP_BLOCKS, -1).sum(1)
    want[-1] += sq[4 * n4:].sum()
    assert n % 4 and float(sq[4 * n4:].sum()) > 0 and (n4 >= R.CLIP_BLOCKS or float(want[n4:-1].sum()) == 0)
    bound = ((1 + 3 + min(trips, 64)) * U + 4096 * 2.0 ** -53) * want * R.ORDER2 + 0.5 * 4 * max(per, 1) * R.DENORM
    _ratio(f"clip n={n}", "partials", got, want, bound)


@pytest.mark.parametrize("n", [5, 4 * 1023 + 2, 262147])
def test_clip_at_the_boundary_every_block_decides_the_same(n):
    """max_norm one fp32 step below, at, and one step above norm + 1e-6: the coefficient is below 1 only for the first, and the buffer is then
    scaled as a whole -- or untouched as a whole, as norm_out[1] says."""
    g = clip_input(n)
    c = Clip(n)
    out, _ = c.run(g, 1e6)
    den = np.float32(out[0]) + np.float32(1e-6)
    for k, mx in enumerate((np.nextafter(den, np.float32(-np.inf)), den, np.nextafter(den, np.float32(np.inf)))):
        o, buf = c.run(g, float(mx))
        assert o[0].tobytes() == out[0].tobytes()
        coef = R.clip_coef_ref(o[0], mx)
        assert (coef < 1) == (k == 0) and coef.tobytes() == o[1].tobytes(), (k, coef, o)
        want = g.cuda() * torch.tensor(float(coef), dtype=F32, device="cuda") if coef < 1 else g.cuda()
        assert same_bits(buf, want), f"side {k}: the buffer is neither entirely scaled nor entirely untouched"
        if k == 0 and n > 5:
            assert not same_bits(buf, g.cuda())  # (scaling by 1 - 2^-24 does change most elements: the two outcomes differ)


def test_clip_all_zero_gradient():
    n = 4 * 1023 + 2
    g = torch.zeros(n)
    g[::3] = -0.0
    c = Clip(n)
    out, buf = c.run(g, 1.0)
    assert float(out[0]) == 0.0 and float(out[1]) == 1.0 and same_bits(buf, g.cuda())
    out, buf = c.run(g, 1e-7)
    assert float(out[0]) == 0.0 and out[1].tobytes() == R.clip_coef_ref(0.0, 1e-7).tobytes() and abs(float(out[1]) - 0.1) < 1e-6
    assert same_bits(buf, g.cuda()), "zeros times 0.1 must keep their signs"


@pytest.mark.parametrize("where", ["body", "tail"])
def test_clip_with_one_inf_is_torch_s(where):
    """norm = Inf, coefficient 0: the finite elements become +-0, the Inf becomes NaN (clip_grad_norm_ does the same)."""
    n = 4 * 1023 + 2
    g = clip_input(n).clone()
    k = 7 if where == "body" else n - 1
    g[k] = float("inf")
    out, buf = Clip(n).run(g, 1.0)
    assert float(out[0]) == float("inf") and out[1].tobytes() == np.float32(0).tobytes()
    _, coef, want = R.clip_ref(g, 1.0)
    buf = buf.cpu()
    assert coef == 0 and bool(torch.isnan(buf[k])) and int(torch.isnan(buf).sum()) == 1
    ok = torch.arange(n) != k
    assert same_bits(buf[ok], want[ok]) and not bool(buf[ok].any())


@pytest.mark.parametrize("max_norm", [1e-5, 1e6])
@pytest.mark.parametrize("where", ["body", "tail"])
def test_clip_with_one_nan_poisons_everything_as_torch_does(where, max_norm):
    """torch.nn.utils.clip_grad_norm_ multiplies by clamp(NaN, max=1) = NaN: the norm, the coefficient and every gradient are NaN, whether
    max_norm is above or below the norm of the finite part.  (A coefficient replaced by 1 would let training go on with one poisoned tensor.)"""
    n = 4 * 1023 + 2
    g = clip_input(n).clone()
    g[7 if where == "body" else n - 1] = NAN
    out, buf = Clip(n).run(g, max_norm)
    assert np.isnan(out[0]) and np.isnan(out[1]), out
    assert bool(torch.isnan(buf).all()), f"{int((~torch.isnan(buf)).sum())} of {n} gradients survived a NaN norm"
    assert bool(torch.isnan(R.clip_ref(g, max_norm)[2]).all())


def test_clip_past_the_flush_of_the_fp32_run():
    """n above 4 * 1024 * 16 384: every lane's fp32 run is moved to its double after 64 trips and the lane goes on adding (66 trips).  About
    270 MB: values, fp64 norm and expected bits are made on the device; only scalars come back."""
    n = CLIP_BIG_N
    assert -(-(n // 4) // 1024) > 64 * 256
    gen = torch.Generator(device="cuda").manual_seed(5)
    g = torch.randn(n, generator=gen, device="cuda") * 0.02
    norm64 = float(g.double().square().sum().sqrt())
    c = Clip(n)
    out1, buf1 = check_clip("big max_norm=1", c, g, 1.0, norm64)
    assert out1[1] < 1
    out2, buf2 = c.run(g, 1.0)
    assert out1.tobytes() == out2.tobytes() and same_bits(buf1, buf2), "two runs differ"
    del buf1, buf2
    check_clip("big max_norm=1e6", c, g, 1e6, norm64)


def test_clip_refusals_launch_nothing():
    hip, lib = _lib()
    c = Clip(64)
    c.buf.fill_(3.0)
    c.out.fill_(5.0)
    s = hip.stream_ptr()
    assert lib.vmg_grad_clip_norm(c.buf.data_ptr() + 4, 8, 1.0, c.ws.data_ptr(), c.out.data_ptr(), s) != 0
    assert b"16-byte" in lib.vmg_last_error()
    assert lib.vmg_grad_clip_norm(c.buf.data_ptr(), 0, 1.0, c.ws.data_ptr(), c.out.data_ptr(), s) != 0
    assert lib.vmg_grad_clip_norm(None, 8, 1.0, c.ws.data_ptr(), c.out.data_ptr(), s) != 0
    assert lib.vmg_grad_clip_norm(c.buf.data_ptr(), 8, 0.0, c.ws.data_ptr(), c.out.data_ptr(), s) != 0
    torch.cuda.synchronize()
    assert bool((c.buf == 3.0).all()) and bool((c.out == 5.0).all())


# ================================================================================================ Charbonnier-edge loss
LOSS_HW = [(3, 3), (3, 4), (4, 3), (4, 4), (5, 3), (6, 7), (33, 18)]
PLANE_KINDS = ["random, every fifth pixel x == y", "constant difference", "random", "corner 0,0", "corner 0,W-1", "corner H-1,0", "corner H-1,W-1"]
GRID_CAP = 16384


def loss_inputs(planes, H, W, device="cpu"):
    """x, y (planes, H, W) fp32; plane p is of kind PLANE_KINDS[p % 7].  Values of the planted planes are multiples of 1/64, so their
    differences are exact: a constant plane's d is exactly 0.25 and a corner plane's d is exactly 0 but for one 0.5."""
    gen = torch.Generator(device=device).manual_seed(17 * planes + 3 * H + W)
    x = torch.rand(planes, H, W, generator=gen, device=device) * 0.6 + 0.2
    y = torch.rand(planes, H, W, generator=gen, device=device) * 0.6 + 0.2
    grid = torch.randint(13, 52, (planes, H, W), generator=gen, device=device).float() / 64
    fifth = (torch.arange(H * W, device=device).reshape(H, W) % 5 == 0)
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for p in range(min(planes, 14)):
        kind = p % 7
        if kind == 0:
            x[p] = torch.where(fifth, y[p], x[p])
        elif kind == 1:
            y[p] = grid[p]
            x[p] = grid[p] + 0.25
        elif kind >= 3:
            y[p] = grid[p]
            x[p] = grid[p]
            cy, cx = corners[kind - 3]
            x[p, cy, cx] += 0.5
    return x, y


def run_loss(tag, x, y, eps, gss):
    """Forward and, for every (gs1, gs2) of gss, backward on device tensors x, y; every written tensor against the reference.  The
    reference runs on x's device."""
    hip, lib = _lib()
    planes, H, W = x.shape
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    n = planes * H * W
    nb = int(lib.vmg_charbonnier_edge_blocks(planes, H, W))
    assert nb == min(-(-n // 256), GRID_CAP)
    trips = -(-n // (nb * 256))
    xd, yd = x.cuda(), y.cuda()
    a1 = torch.full((planes, H2, W2), NAN, dtype=F32, device="cuda")
    ld = torch.full((planes, H, W), NAN, dtype=F32, device="cuda")
    partial = torch.full((nb, 2), NAN, dtype=F32, device="cuda")
    eps32 = R.f32(eps)
    s = hip.stream_ptr()
    hip.check(lib.vmg_charbonnier_edge_fwd(xd.data_ptr(), yd.data_ptr(), a1.data_ptr(), ld.data_ptr(), partial.data_ptr(), planes, H, W, eps, s),
              "vmg_charbonnier_edge_fwd")
    torch.cuda.synchronize()
    dev = x.device
    r = R.lap_fwd_ref(x, y, eps32)
    B = R.lap_fwd_bounds(r, trips)
    _ratio(tag, "a1", a1.to(dev), r["a1"], B["a1"])
    _ratio(tag, "ld", ld.to(dev), r["ld"], B["ld"])
    sums = partial.double().sum(0).to(dev)  # as vmg_amd.train sums them
    _ratio(tag, "sum1", sums[0:1], r["sum1"].reshape(1), B["sum1"].reshape(1))
    _ratio(tag, "sum2", sums[1:2], r["sum2"].reshape(1), B["sum2"].reshape(1))
    pyr = r["pyr"]
    del r, B
    ld_in = ld.clone()
    for gs1, gs2 in gss:
        g1, g2 = R.f32(gs1), R.f32(gs2)
        u = torch.full((planes, H2, W2), NAN, dtype=F32, device="cuda")
        dx = torch.full((planes, H, W), NAN, dtype=F32, device="cuda")
        hip.check(lib.vmg_charbonnier_edge_bwd(xd.data_ptr(), yd.data_ptr(), ld.data_ptr(), u.data_ptr(), dx.data_ptr(), planes, H, W, eps, g1, g2, s),
                  "vmg_charbonnier_edge_bwd")
        torch.cuda.synchronize()
        assert torch.equal(R.bits(ld), R.bits(ld_in)), "the backward changed ld"
        b = R.lap_bwd_ref(x, y, ld.to(dev), eps32, g1, g2, pyr)  # from the kernel's own ld
        Bb = R.lap_bwd_bounds(b)
        t2 = f"{tag} gs=({gs1:.3g},{gs2:.3g})"
        _ratio(t2, "u", u.to(dev), b["u"], Bb["u"])
        _ratio(t2, "dx", dx.to(dev), b["dx"], Bb["dx"])
        del b, Bb


@pytest.mark.parametrize("eps", [1e-12, 1e-6])
@pytest.mark.parametrize("planes", [1, 7])
@pytest.mark.parametrize("hw", LOSS_HW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_kernels_per_element(hw, planes, eps):
    H, W = hw
    x, y = loss_inputs(planes, H, W)
    n = planes * H * W
    run_loss(f"loss {planes}x{H}x{W} eps={eps:g}", x, y, eps, [(1.0 / n, 0.005 / n), (0.0, 1.0), (1.0, 0.0)])


def test_loss_inputs_hold_what_they_should():
    """A test of the test (no GPU work)."""
    x, y = loss_inputs(7, 4, 3)
    d = x - y
    assert int((d[0] == 0).sum()) == 3 and bool((d[1] == 0.25).all()) and bool((d[2] != 0).all())
    for k, (cy, cx) in enumerate([(0, 0), (0, 2), (3, 0), (3, 2)]):
        assert float(d[3 + k, cy, cx]) == 0.5 and int((d[3 + k] != 0).sum()) == 1
    # the constant plane's Laplacian is rounding noise in the interior, where w = ld / sqrt(ld^2 + eps) is steepest
    x, y = loss_inputs(7, 33, 18)
    ld = R.lap_fwd_ref(x[1:2], y[1:2], 1e-12)["ld"]
    assert float(ld[0, 4:-4, 4:-4].abs().max()) < 1e-6 and float(ld[0, 0].abs().min()) > 1e-3


@pytest.mark.parametrize("shape", [(64, 257, 256), (256, 257, 255)], ids=lambda s: "x".join(map(str, s)))
def test_loss_kernels_past_the_grid_caps(shape):
    """planes H W just above 16 384 x 256 for the full-size kernels (64 x 257 x 256: two trips of their grid stride), and planes H2 W2 just above it
    for the quarter-size kernels (256 x 257 x 255: 129 x 128 quarter images; four trips of the full-size ones).  Non-square; the reference's
    per-axis matrix products run in fp64 on the device."""
    planes, H, W = shape
    n = planes * H * W
    assert n > GRID_CAP * 256 and (shape[0] == 64 or planes * ((H + 1) // 2) * ((W + 1) // 2) > GRID_CAP * 256)
    x, y = loss_inputs(planes, H, W, device="cuda")
    run_loss(f"loss {planes}x{H}x{W} eps=1e-12", x, y, 1e-12, [(1.0 / n, 0.005 / n)])


def test_loss_through_the_autograd_wrapper():
    """A non-contiguous x and an upstream gradient of 2.5: value and gradient against the oracle at the tolerances of tests/test_optim_gpu.py."""
    from oracle import recipe as Rc
    from oracle import vmg_oracle as O
    from vmg_amd.train import charbonnier_edge_loss_hip
    shape = (1, 2, 3, 33, 18)
    xt = Rc.seeded((1, 2, 3, 18, 33), 311, 0.3) + 0.5
    x, y = xt.transpose(-1, -2), Rc.seeded(shape, 312, 0.3) + 0.5
    assert not x.is_contiguous() and x.shape == shape
    xo = x.clone().requires_grad_(True)
    lo = O.charbonnier_edge_loss(xo, y)
    (2.5 * lo).backward()
    xg = xt.cuda().transpose(-1, -2).requires_grad_(True)
    assert not xg.is_contiguous()
    lg = charbonnier_edge_loss_hip(xg, y.cuda())
    (2.5 * lg).backward()
    lg, lo = float(lg.detach()), float(lo.detach())
    assert abs(lg - lo) <= 2e-6 * max(1.0, abs(lo))
    gmax = float(xo.grad.abs().max())
    assert xg.grad.shape == shape
    assert float((xg.grad.cpu() - xo.grad).abs().max()) <= 2e-5 * gmax + 1e-12


def test_loss_refusals_launch_nothing():
    hip, lib = _lib()
    s = hip.stream_ptr()
    t = [torch.full((2, 4, 4), float(i + 1), dtype=F32, device="cuda") for i in range(5)]
    ptrs = [v.data_ptr() for v in t]
    for H, W in ((2, 4), (4, 2), (2, 2), (1, 16), (0, 4)):
        assert lib.vmg_charbonnier_edge_fwd(*ptrs, 2, H, W, 1e-12, s) != 0, (H, W)
        assert b"H, W >= 3" in lib.vmg_last_error()
        assert lib.vmg_charbonnier_edge_bwd(*ptrs, 2, H, W, 1e-12, 1.0, 1.0, s) != 0, (H, W)
    assert lib.vmg_charbonnier_edge_fwd(None, *ptrs[1:], 2, 4, 4, 1e-12, s) != 0
    assert lib.vmg_charbonnier_edge_bwd(*ptrs[:4], None, 2, 4, 4, 1e-12, 1.0, 1.0, s) != 0
    assert lib.vmg_charbonnier_edge_fwd(*ptrs, 0, 4, 4, 1e-12, s) != 0
    torch.cuda.synchronize()
    for i, v in enumerate(t):
        assert bool((v == float(i + 1)).all())
