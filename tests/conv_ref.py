"""Reference of the OPERATION behind vmg_conv_fwd (include/vmg_hip.h) for ks = 3 and ks = 7 (the weight's own size says which; padding
p = ks // 2, ks * ks taps), spelled the slow obvious way in fp64, and the inputs that make a comparison with it EXACT: torch and numpy only,
nothing of vmg_amd.

    acc[n,y,x,o] = sum_s sum_{ky,kx} sum_i X_s[n, y+ky-p, x+kx-p, i] * W[o0+o, off_s+i, ky, kx]          (zero outside the image)
    v = acc + bias;  out_pre = bf16(v);  v = act(v);  v *= alpha;  v *= mask(aux, actgrad);  v += res;  out = bf16(v)

The kernels multiply bf16 values exactly into fp32 and add in fp32, each in an order of its own (waves that split K, stages walked in a
rotated order, a reduce through LDS).  With every operand k * 2^-s of wgrad_ref.FAMILIES, the bias and the residual of the same kind and
alpha / slope powers of two, every product is an integer multiple of 2^-2s and every later value an integer multiple of a finer power of
two; as long as that integer stays below 2^24 (assert_exact) every partial sum in ANY order and every epilogue intermediate is an fp32
number: the only rounding left is the final one to bf16, and the result must equal round_bf16(fp64 reference) bit for bit.

The data gradient has a spelling of its own (a scatter per tap, dgrad_ref): the transpose_flip packs are then compared with something that
is not the forward reference with a flipped weight.

ks = 1 (every nn.Linear and 1x1 conv) has references of its own -- linear_ref, dlinear_ref, pixel_shuffle_ref, gelu_ref, gelu_grad_ref --
that do not go through conv_ref; assert_exact and real_bound take the tap count (taps = 1; 49 for 7x7), epilogue_ref the output dtype."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.wgrad_ref import FAMILIES

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_GELU = 0, 1, 2, 3  # include/vmg_hip.h VMG_ACT_* (the GPU module asserts that they agree)


def conv_ref(srcs, w, src_off=None, o0=0, on=None, groups=1):
    """3x3 (7x7) convolution with zero padding 1 (3) over the virtual concatenation of srcs[s] (N, H, W, C_s), channels-last, in fp64: a
    gather per tap.  w (O, I, ks, ks), ks = 3 or 7; source s meets the weight's input channels [src_off[s], src_off[s] + C_s) (default: one after the other); the result
    holds output channels [o0, o0 + on).  groups > 1: w is the weight of a grouped convolution (I channels per group) over the
    concatenated sources -- each group of outputs sees its own I input channels only."""
    N, H, W = srcs[0].shape[:3]
    O = w.shape[0]
    on = O - o0 if on is None else on
    ks = _ks(w)
    w = w.double()
    if groups > 1:
        assert src_off is None and o0 == 0 and on == O and O % groups == 0
        x = torch.cat([s.double() for s in srcs], -1)
        I, og = w.shape[1], O // groups
        assert x.shape[-1] == I * groups
        return torch.cat([conv_ref([x[..., g * I:(g + 1) * I]], w[g * og:(g + 1) * og]) for g in range(groups)], -1)
    if src_off is None:
        src_off, a = [], 0
        for s in srcs:
            src_off.append(a)
            a += s.shape[-1]
    acc = torch.zeros(N, H, W, on, dtype=torch.float64)
    for s, off in zip(srcs, src_off):
        C = s.shape[-1]
        assert tuple(s.shape[:3]) == (N, H, W) and off + C <= w.shape[1]
        xpad = F.pad(s.double(), (0, 0, ks // 2, ks // 2, ks // 2, ks // 2))
        for ky in range(ks):
            for kx in range(ks):
                acc += torch.einsum("nhwi,oi->nhwo", xpad[:, ky:ky + H, kx:kx + W], w[o0:o0 + on, off:off + C, ky, kx])
    return acc


def _ks(w):
    """The kernel size of a weight (O, I, ks, ks): 3 or 7."""
    assert w.dim() == 4 and w.shape[2] == w.shape[3] and w.shape[2] in (3, 7), f"weight {tuple(w.shape)}: ks must be 3 or 7"
    return int(w.shape[2])


def dgrad_ref(dy, w, i0=0, inn=None):
    """Data gradient of the 3x3 (7x7) convolution y = conv(x, w), w (O, I, ks, ks), p = ks // 2, as a scatter per tap, in fp64:
    dx[n, y+ky-p, x+kx-p, i] += dy[n, y, x, o] * w[o, i, ky, kx] -- output pixel (y, x) read input pixel (y+ky-p, x+kx-p) through tap (ky, kx).
    dy (N, H, W, O); the result holds input channels [i0, i0 + inn)."""
    N, H, W, O = dy.shape
    assert w.shape[0] == O
    inn = w.shape[1] - i0 if inn is None else inn
    ks = _ks(w)
    p = ks // 2
    w, dy = w.double(), dy.double()
    dxp = torch.zeros(N, H + 2 * p, W + 2 * p, inn, dtype=torch.float64)  # dxp[:, p + y', p + x'] = dx[:, y', x']
    for ky in range(ks):
        for kx in range(ks):
            dxp[:, ky:ky + H, kx:kx + W] += torch.einsum("nhwo,oi->nhwi", dy, w[:, i0:i0 + inn, ky, kx])
    return dxp[:, p:H + p, p:W + p].contiguous()


def linear_ref(srcs, w, src_off=None, o0=0, on=None):
    """ks = 1: one fp64 matmul per source over its K slice of w (O, I).  srcs[s] (..., C_s) channels-last with equal leading shapes; source s
    meets the weight's input channels [src_off[s], src_off[s] + C_s) (default: one after the other); the result holds outputs [o0, o0 + on)."""
    assert w.dim() == 2
    on = w.shape[0] - o0 if on is None else on
    wt = w.double()[o0:o0 + on].t().contiguous()  # (I, on)
    lead = tuple(srcs[0].shape[:-1])
    acc = torch.zeros(lead + (on,), dtype=torch.float64)
    a = 0
    for s, x in enumerate(srcs):
        C = x.shape[-1]
        off = a if src_off is None else src_off[s]
        a += C
        assert tuple(x.shape[:-1]) == lead and off + C <= w.shape[1]
        acc += (x.double().reshape(-1, C) @ wt[off:off + C]).reshape(lead + (on,))
    return acc


def dlinear_ref(dy, w, i0=0, inn=None):
    """Data gradient of y = x @ w.T, w (O, I): dx = dy @ w[:, i0:i0+inn], in fp64 (what a transpose_flip pack of w computes)."""
    assert w.dim() == 2 and dy.shape[-1] == w.shape[0]
    inn = w.shape[1] - i0 if inn is None else inn
    return dy.double() @ w.double()[:, i0:i0 + inn]


def pixel_shuffle_ref(x):
    """(N, H, W, C) -> (N, 2H, 2W, C/4) in torch's PixelShuffle(2) order, by index arithmetic: out[n, 2y+i, 2x+j, c] = x[n, y, x, 4c + 2i + j]."""
    N, H, W, C = x.shape
    assert C % 4 == 0
    out = torch.empty(N, 2 * H, 2 * W, C // 4, dtype=x.dtype)
    for i in range(2):
        for j in range(2):
            out[:, i::2, j::2, :] = x[..., (2 * i + j)::4]
    return out


def gelu_ref(v):
    """GELU, erf form, in fp64: v * Phi(v)."""
    v = v.double()
    return 0.5 * v * (1.0 + torch.erf(v / np.sqrt(2.0)))


def gelu_grad_ref(v):
    """d/dv gelu(v) = Phi(v) + v * phi(v), in fp64."""
    v = v.double()
    return 0.5 * (1.0 + torch.erf(v / np.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / np.sqrt(2.0 * np.pi)


def _is_pow2(v):
    m, _ = np.frexp(abs(float(v)))
    return v != 0 and m == 0.5


def _f32(v64, claim, what):
    """v64 rounded to fp32 (returned as fp64); with `claim`, the assertion that nothing was rounded."""
    r = v64.float().double()
    if claim:
        assert torch.equal(r, v64), f"{what} is not an fp32 number: the case is not exact"
    return r


def round_bf16(v64, exact=True):
    """fp64 -> fp32 -> bf16, both round to nearest even.  exact: the fp64 value must be an fp32 number already (the first step rounds nothing,
    so that the result is THE correctly rounded bf16 of the true value)."""
    v32 = v64.float()
    if exact:
        assert torch.equal(v32.double(), v64), "the fp64 value is not an fp32 number: no exactness can be claimed"
    return v32.bfloat16()


def mask_ref(aux, actgrad, slope):
    """The activation-gradient factor of the epilogue: 1 where aux > 0 (-0.0 and +0.0 are not), else 0 (mode 1) or the slope (mode 2)."""
    assert actgrad in (1, 2)
    lo = 0.0 if actgrad == 1 else float(np.float32(slope))
    return torch.where(aux.double() > 0, torch.ones((), dtype=torch.float64), torch.full((), lo, dtype=torch.float64))


def epilogue_ref(acc, bias=None, act=ACT_NONE, slope=0.0, alpha=1.0, aux=None, actgrad=0, res=None, exact=True, out_dtype=torch.bfloat16):
    """The epilogue in the kernels' order on the fp64 sums `acc`.  exact: every intermediate is asserted to be an fp32 number and the result
    is (out, out_pre) as bf16 tensors.  A LeakyReLU slope that is no power of two is the one step that may round: v * float32(slope),
    rounded to fp32 as the kernel's single multiplication does (assert_exact admits it only where the bf16 rounding follows directly).
    GELU: out is None (only out_pre is exact).  exact=False: no intermediate rounding, (out, out_pre) in fp64.
    out_dtype = torch.float32 (the fp32 kernels): the exact results are the fp64 values themselves, asserted to be fp32 numbers and returned as
    fp32 tensors -- nothing is rounded but a LeakyReLU slope that is no power of two, once, as above."""
    assert out_dtype in (torch.bfloat16, torch.float32)
    final = round_bf16 if out_dtype == torch.bfloat16 else (lambda t: _f32(t, True, "the fp32 output").float())
    slope32, alpha32 = float(np.float32(slope)), float(np.float32(alpha))
    v = acc if bias is None else acc + bias.double()
    v = _f32(v, exact, "acc + bias") if exact else v
    pre = final(v) if exact else v.clone()
    if act == ACT_GELU:
        return None, pre
    if act == ACT_RELU:
        v = torch.clamp(v, min=0.0)
    elif act == ACT_LRELU:
        neg = v * slope32
        v = torch.where(v > 0, v, _f32(neg, _is_pow2(slope32), "v * slope") if exact else neg)
    else:
        assert act == ACT_NONE
    if alpha32 != 1.0:
        v = v * alpha32
        v = _f32(v, True, "v * alpha") if exact else v
    if aux is not None and actgrad:
        v = v * mask_ref(aux, actgrad, slope)
        v = _f32(v, True, "v * mask") if exact else v
    if res is not None:
        v = v + res.double()
        v = _f32(v, True, "v + res") if exact else v
    return (final(v) if exact else v), pre


def assert_exact(family, ci_total, bias=True, res=False, scales=(), taps=9):
    """The invariant, checked before anything runs on the GPU.  Operands k * 2^-s of the family: a partial sum is an integer of at most
    P = kmax^2 * taps * ci_total units of 2^-2s (taps = 9 for 3x3, 49 for 7x7, 1 for ks = 1), the bias adds at most kmax * 2^s of those units.  Every scale (LeakyReLU slope, alpha, the
    slope of mask mode 2) is a power of two 2^-a_j, a_j >= 0: scaling keeps the integer and moves the grid to 2^-(2s+a), a = sum a_j, on
    which the residual is at most kmax * 2^(s+a) units.  Their sum below 2^24 bounds the integer of every intermediate value (conservatively
    for the ones on coarser grids), so each fits fp32's 24-bit significand.  ONE scale may be no power of two if nothing follows it -- no
    other scale but 1, no residual: then the product is rounded once to fp32 and directly to bf16, which the reference does too."""
    kmax, s = FAMILIES[family]
    total = kmax * kmax * taps * ci_total + (kmax * 2 ** s if bias else 0)
    scales = [float(np.float32(c)) for c in scales if float(c) != 1.0]
    odd = [c for c in scales if not _is_pow2(c)]
    if odd:
        assert len(scales) == 1 and not res, f"scale {odd[0]} is no power of two and something follows it: not exact"
        a = 0
    else:
        assert all(0 < c <= 1 for c in scales), f"scales {scales} must be powers of two in (0, 1]"
        a = sum(int(round(-np.log2(c))) for c in scales)
    if res:
        total += kmax * 2 ** (s + a)
    assert total < 2 ** 24, f"family {family!r} is not exact at {ci_total} input channels (shift {a}): {total} >= 2^24"


def one_hot_weight(O, I, t, ks=3):
    """Shift probe t (0 .. ks * ks - 1): output channel o has a single 1, at input channel (7 * o + 31 * t) % I and tap (o + t) % (ks * ks), the
    tap (ky, kx) numbered ky * ks + kx -- output channel o is then a shifted copy of that input channel, exact for ANY input.
    Returns (w (O, I, ks, ks) fp32, input channel per o, tap per o)."""
    assert ks in (3, 7) and 0 <= t < ks * ks
    o = torch.arange(O)
    i = (7 * o + 31 * t) % I
    tap = (o + t) % (ks * ks)
    w = torch.zeros(O, I, ks, ks)
    w[o, i, tap // ks, tap % ks] = 1.0
    return w, i, tap


def shifted_copy(x, i, tap, ks=3):
    """What a shift probe must give, by indexing alone: out[n, y, x, o] = X[n, y + ky - p, x + kx - p, i[o]], p = ks // 2, zero outside the
    image."""
    assert ks in (3, 7)
    N, H, W, _ = x.shape
    p = ks // 2
    xpad = F.pad(x, (0, 0, p, p, p, p))
    out = torch.empty(N, H, W, len(i), dtype=x.dtype)
    for o in range(len(i)):
        ky, kx = int(tap[o]) // ks, int(tap[o]) % ks
        out[..., o] = xpad[:, ky:ky + H, kx:kx + W, int(i[o])]
    return out


def one_hot_linear(O, I, t):
    """Permutation probe t of a ks = 1 weight: output channel o has a single 1, at input channel (7 * o + 31 * t) % I -- output channel o is then a
    copy of that input channel, exact for ANY input.  Returns (w (O, I) fp32, input channel per o)."""
    o = torch.arange(O)
    i = (7 * o + 31 * t) % I
    w = torch.zeros(O, I)
    w[o, i] = 1.0
    return w, i


def sum_bound(S, ci_total, taps=9):
    """e32 of real_bound: the any-order fp32 summation bound of taps * ci_total products, the bias, the two scalings and the residual over
    S = sum |x||w| + |b| + |res| (n terms: n * u * S, u = 2^-24), doubled because the matrix unit's adder may truncate."""
    return 2.0 * (taps * ci_total + 4) * 2.0 ** -24 * S


def real_bound(v, S, ci_total, taps=9, out_dtype=torch.bfloat16):
    """Per-element bound of |got - v| for real-valued operands: v the fp64 result from the operands as the kernel reads them, S = sum |x||w| +
    |b| + |res|, e32 = sum_bound(S, ci_total, taps).  The rounding of the computed value to the output type adds u_out of it -- 2^-8 for bf16
    (2^-9 would do for round to nearest; an ulp is allowed), 2^-23 for fp32: |got - v| <= u_out * (|v| + e32) + e32.  ReLU, LeakyReLU, the
    masks and alpha <= 1 do not enlarge it: they are 1-Lipschitz or do not depend on computed values.  taps: products per input channel
    (9 for 3x3, 49 for 7x7, 1 for ks = 1)."""
    e32 = sum_bound(S, ci_total, taps)
    u_out = 2.0 ** -8 if out_dtype == torch.bfloat16 else 2.0 ** -23
    return u_out * (v.abs() + e32) + e32
