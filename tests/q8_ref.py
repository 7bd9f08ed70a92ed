"""Host reference of the fp8 convolution path (csrc/conv_fp8.hip): Q8 records, the weight quantiser, and the operands that make a
comparison with the fp64 convolution of tests/conv_ref.py EXACT.  torch and numpy only, nothing of vmg_amd.

A Q8 record of a pixel with C channels is [DB = 32 * ceil(C / 32) data bytes: OCP e4m3 values, zero beyond C][16 bytes: one E8M0 scale
byte per 32-channel block, zero beyond the block count]; value = e4m3 * 2^(scale - 127).  The CANONICAL scale byte sb of a block is the one
whose power of two maps the block's largest magnitude into (224, 448]: amax * 2^(127 - sb) in (224, 448], sb clamped to [1, 254] (an all-zero
block has sb = 1).  The data bytes are the values times 2^(127 - sb), rounded to nearest even on the e4m3 grid.

What the exact tests rest on:
  1. an e4m3 value times a power of two is a bf16 number, and the matrix instruction's products are exact;
  2. with ONE nonzero product per output element nothing is added: one-hot weights make the output a shifted copy of the dequantised records,
     one-hot activations (impulse_image) make it the dequantised weight image itself, for ANY operand values;
  3. with small-integer operands every partial sum, the bias in the accumulator included, is an integer; assert_q8_exact checks before any
     launch that S = sum |x||w| + |bias| stays below 2^12 per output element, which the instruction's adder (about 14 bits below its largest
     product) holds without loss however the accumulator input is aligned;
  4. the record quantiser is deterministic given exact fp32 inputs: record outputs are compared byte for byte (zero_sign: the sign of a zero
     is not part of the contract)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_ref as CR

CAP = 2 ** 12  # assert_q8_exact: the largest sum of magnitudes of an exact case (never raised: thin the operands instead)


# ------------------------------------------------------------------------------------------------------------------------------------
# the emulations that tests/test_fp8_gpu.py has used from the start (moved here unchanged: the kernel's own bit formula, torch's e4m3 cast)
# ------------------------------------------------------------------------------------------------------------------------------------
def quant_emul(x):
    """torch emulation of the record quantiser: x (..., C) fp32 -> dequantised fp32 of the same shape."""
    C = x.shape[-1]
    nb = (C + 31) // 32
    xp = F.pad(x, (0, nb * 32 - C)).reshape(*x.shape[:-1], nb, 32)
    amax = xp.abs().amax(-1, keepdim=True)
    bits = amax.view(torch.int32)
    sb = ((bits >> 23) & 255) - 8 + ((bits & 0x7FFFFF) > 0x600000).int()
    sb = sb.clamp(1, 254)
    mult = torch.exp2(127.0 - sb.float())
    q = (xp * mult).to(torch.float8_e4m3fn).float() / mult
    return q.reshape(*x.shape[:-1], nb * 32)[..., :C]


def wquant_emul(w):
    """per-output-channel power-of-two scale, e4m3 values: (O, I, 3, 3) fp32 -> dequantised fp32."""
    amax = w.abs().amax((1, 2, 3), keepdim=True)
    bits = amax.view(torch.int32)
    sb = (((bits >> 23) & 255) - 8 + ((bits & 0x7FFFFF) > 0x600000).int()).clamp(1, 254)
    mult = torch.exp2(127.0 - sb.float())
    return (w * mult).to(torch.float8_e4m3fn).float() / mult


# ------------------------------------------------------------------------------------------------------------------------------------
# e4m3 and the canonical scale, written from their definitions (numpy)
# ------------------------------------------------------------------------------------------------------------------------------------
def _e4m3_table():
    """The 256 values of OCP e4m3 (fn): sign, 4 exponent bits (bias 7), 3 mantissa bits; exponent 0 is subnormal (m * 2^-9); no infinity,
    0x7F / 0xFF are NaN."""
    t = np.empty(256, dtype=np.float64)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        v = m * 2.0 ** -9 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
        if e == 15 and m == 7:
            v = np.nan
        t[b] = -v if b & 0x80 else v
    return t


E4M3 = _e4m3_table()
E4M3_MAX = 448.0


def e4m3_encode(v):
    """float64 array, |v| <= 448 -> uint8 e4m3 codes, round to nearest even on the e4m3 grid (step 2^-9 below 2^-6, else 2^(floor(log2|v|) - 3));
    a zero result carries the sign of v."""
    v = np.asarray(v, dtype=np.float64)
    a = np.abs(v)
    assert not np.isnan(a).any() and (a.size == 0 or float(a.max()) <= E4M3_MAX), "e4m3_encode: value outside [-448, 448]"
    _, ex = np.frexp(a)                                   # a = m * 2^ex, m in [0.5, 1): floor(log2 a) = ex - 1
    step = np.exp2(np.maximum(ex - 1, -6) - 3.0)
    n = np.rint(a / step)                                 # (half to even) -- in [0, 16]: 16 is the next binade's 8
    q = n * step
    _, qx = np.frexp(q)
    e = np.maximum(qx - 1, -7) + 7                        # biased exponent; 0 for subnormals (q < 2^-6)
    m = np.where(e == 0, q * 2.0 ** 9, (q / np.exp2(e - 7.0) - 1.0) * 8.0)
    code = (e.astype(np.int64) << 3 | m.astype(np.int64)) * (q > 0)
    return (code | (np.signbit(v).astype(np.int64) << 7)).astype(np.uint8)


def scale_byte(amax):
    """The canonical E8M0 scale byte of a block maximum (float array >= 0): amax * 2^(127 - sb) in (224, 448], clamped to [1, 254].
    amax = m * 2^e with m in [0.5, 1): 448 = 0.875 * 2^9, so the product lies in (224, 448] with 2^(9 - e) where m <= 0.875 and with 2^(8 - e)
    above it."""
    amax = np.asarray(amax, dtype=np.float64)
    assert not np.isnan(amax).any() and not np.isinf(amax).any() and (amax >= 0).all()
    m, e = np.frexp(amax)
    sb = 127 - np.where(m <= 0.875, 9 - e, 8 - e)
    sb = np.where(amax == 0, 1, sb)
    return np.clip(sb, 1, 254).astype(np.uint8)


def _records(x, sb_of):
    """Block by block (so that nothing is padded to 32 channels in fp64): sb_of(b, |block| max) gives the block's scale bytes."""
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    C = x.shape[-1]
    nb = (C + 31) // 32
    rec = np.zeros(x.shape[:-1] + (nb * 32 + 16,), dtype=np.uint8)
    for b in range(nb):
        xb = x[..., 32 * b:min(C, 32 * b + 32)].astype(np.float64)
        sb = sb_of(b, np.abs(xb).max(-1))
        rec[..., 32 * b:32 * b + xb.shape[-1]] = e4m3_encode(xb * np.exp2(127.0 - sb.astype(np.float64))[..., None])
        rec[..., nb * 32 + b] = sb
    return torch.from_numpy(rec)


def records(x):
    """fp32 (..., C) -> uint8 records (..., 32 * ceil(C / 32) + 16) by the canonical rule."""
    return _records(x, lambda b, amax: scale_byte(amax))


def records_with_scales(x, sb):
    """The same for caller-chosen scale bytes sb (..., nb) uint8: a record is e4m3 * 2^(sb - 127) whatever produced it."""
    sb = sb.detach().cpu().numpy() if isinstance(sb, torch.Tensor) else np.asarray(sb)
    assert sb.dtype == np.uint8 and sb.shape == tuple(x.shape[:-1]) + ((x.shape[-1] + 31) // 32,)
    return _records(x, lambda b, amax: sb[..., b])


def dequant(rec, C):
    """uint8 records (..., rec) -> fp32 (..., C): e4m3 * 2^(scale - 127), formed in fp64: the value is an fp32 number, or -- only where a
    magnitude of at least 255 * 2^120 was rounded up to 256 * 2^120 -- 2^128, which fp32 holds as infinity."""
    r = rec.detach().cpu().numpy()
    nb = (C + 31) // 32
    assert r.dtype == np.uint8 and r.shape[-1] == nb * 32 + 16
    data = E4M3[r[..., :nb * 32]].reshape(r.shape[:-1] + (nb, 32))
    v = data * np.exp2(r[..., nb * 32:nb * 32 + nb].astype(np.float64) - 127.0)[..., None]
    with np.errstate(over="ignore"):
        v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64)[np.abs(v) < 2.0 ** 128], v[np.abs(v) < 2.0 ** 128])
    return torch.from_numpy(v32.reshape(r.shape[:-1] + (nb * 32,))[..., :C].copy())


def zero_sign(rec):
    """Records with the data byte 0x80 (minus zero) replaced by 0x00: a cancelling sum may come out as either zero, so every byte comparison
    goes through this.  The 16 scale bytes at the end are left alone (0x80 there is the scale 2^1)."""
    out = rec.clone()
    data = out[..., :out.shape[-1] - 16]
    data[data == 0x80] = 0
    return out


def wquant_ref(w, transpose_flip=False):
    """The weight image's values, from the statement: e4m3 with one canonical power-of-two scale per output channel of the convolution that
    the pack serves -- output channel o of w (O, I, 3, 3) for the forward pack, INPUT channel i for the data-gradient pack (transpose_flip:
    dx[.., i] sums dy[.., o] * w[o, i, ky, kx] over o and the taps, conv_ref.dgrad_ref).  Returns dequantised fp32 of w's shape."""
    dims = (0, 2, 3) if transpose_flip else (1, 2, 3)
    wd = w.detach().cpu().double().numpy()
    sb = scale_byte(np.abs(wd).max(dims, keepdims=True)).astype(np.float64)
    q = E4M3[e4m3_encode(wd * np.exp2(127.0 - sb))] * np.exp2(sb - 127.0)
    q32 = q.astype(np.float32)
    assert np.array_equal(q32.astype(np.float64), q)
    return torch.from_numpy(q32)


# ------------------------------------------------------------------------------------------------------------------------------------
# the exactness invariant and the operand families
# ------------------------------------------------------------------------------------------------------------------------------------
def magnitude_sum(x, w, bias=None, dgrad=False):
    """S = sum |x||w| + |bias| per output element, in fp64 (the 3x3 magnitude convolution; dgrad: of the data gradient)."""
    S = CR.dgrad_ref(x.abs(), w.abs()) if dgrad else CR.conv_ref([x.abs()], w.abs())
    return S if bias is None else S + bias.abs().double()


def assert_q8_exact(x, w, bias=None, dgrad=False):
    """The invariant, on the CPU before any launch: all operands are integers and max S < 2^12.  Every partial sum of the kernel -- in any
    order, the accumulator (which starts from the bias) included -- is then an integer below 2^12.  Returns max S."""
    for name, t in (("x", x), ("w", w), ("bias", bias)):
        assert t is None or torch.equal(t.double(), t.double().round()), f"{name} holds values that are no integers"
    top = float(magnitude_sum(x, w, bias, dgrad).max())
    assert top < CAP, f"max S = {top:g} is not below 2^12: thin the operands, never raise the cap"
    return top


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def narrow(geom, C, seed, dgrad=False):
    """Dense x in {-2..2}, w in {-1, 0, 1}, bias in {-8..8}: S <= 2 * 9 * 144 + 8 = 2600."""
    N, H, W = geom
    g = _gen(seed)
    x = torch.randint(-2, 3, (N, H, W, C), generator=g).float()
    w = torch.randint(-1, 2, (C, C, 3, 3), generator=g).float()
    bias = torch.randint(-8, 9, (C,), generator=g).float()
    return x, w, bias


def scaled_x(geom, C, seed):
    """x = k * 2^e, k in {-1, 0, 1} at density 1/2, e in {0, 1, 2} drawn per (pixel, 32-channel block); the first channel of each block is
    forced nonzero so that the block's scale byte really varies.  Returns (x, e (N, H, W, nb) int64)."""
    N, H, W = geom
    g = _gen(seed)
    nb = (C + 31) // 32
    k = torch.randint(0, 2, (N, H, W, C), generator=g) * (2 * torch.randint(0, 2, (N, H, W, C), generator=g) - 1)
    first = 2 * torch.randint(0, 2, (N, H, W, nb), generator=g) - 1
    k[..., 0::32] = first
    e = torch.randint(0, 3, (N, H, W, nb), generator=g)
    x = k.float() * torch.exp2(e.repeat_interleave(32, -1)[..., :C].float())
    return x, e


def scaled(geom, C, seed, dgrad=False):
    """scaled_x activations; w = k * 2^f with k in {-1, 0, 1} at density 1/2 and f in {0, 1} drawn per output channel; bias in {-8..8}.
    Both are exact in e4m3 under the canonical scale (a block / channel holds magnitudes 2^a and 2^(a+1) at most)."""
    x, _ = scaled_x(geom, C, seed)
    g = _gen(seed + 1)
    k = torch.randint(0, 2, (C, C, 3, 3), generator=g) * (2 * torch.randint(0, 2, (C, C, 3, 3), generator=g) - 1)
    f = torch.randint(0, 2, (C, 1, 1, 1), generator=g)
    w = k.float() * torch.exp2(f.float())
    bias = torch.randint(-8, 9, (C,), generator=g).float()
    return x, w, bias


FAMILIES = {"narrow": narrow, "scaled": scaled}


# ------------------------------------------------------------------------------------------------------------------------------------
# the weight read-back probe
# ------------------------------------------------------------------------------------------------------------------------------------
IMPULSE_GEOM = (1, 36, 36)


def impulse_image(C):
    """(1, 36, 36, C) fp32: the pixel at (3a + 1, 3b + 1) carries 1.0 in channel 12a + b (where that is below C) and nothing else.  The 3x3
    neighbourhoods of the impulses do not overlap: every output element of a convolution of it has at most ONE nonzero product, and
    out[0, 3a + 2 - ky, 3b + 2 - kx, o] = w[o, 12a + b, ky, kx]."""
    assert C <= 144
    x = torch.zeros(1, 36, 36, C)
    for c in range(C):
        x[0, 3 * (c // 12) + 1, 3 * (c % 12) + 1, c] = 1.0
    return x


def impulse_gather(out, C, dgrad=False):
    """The inverse: the (O, C, 3, 3) weight from the (1, 36, 36, O) output of the forward convolution of impulse_image(C); dgrad: the
    (C, I, 3, 3) weight from the (1, 36, 36, I) data gradient, whose scatter puts w[12a + b, i, ky, kx] at (3a + ky, 3b + kx)."""
    O = out.shape[-1]
    w = torch.empty((C, O, 3, 3) if dgrad else (O, C, 3, 3), dtype=out.dtype)
    for c in range(C):
        a, b = c // 12, c % 12
        for ky in range(3):
            for kx in range(3):
                if dgrad:
                    w[c, :, ky, kx] = out[0, 3 * a + ky, 3 * b + kx]
                else:
                    w[:, c, ky, kx] = out[0, 3 * a + 2 - ky, 3 * b + 2 - kx]
    return w


def first_byte_mismatch(got, want, C):
    """Two record tensors (..., rec) through zero_sign: (number of differing bytes, a description of the first) or (0, None)."""
    g, w = zero_sign(got), zero_sign(want)
    assert g.shape == w.shape and g.dtype == w.dtype == torch.uint8
    bad = g != w
    n = int(bad.sum())
    if n == 0:
        return 0, None
    i = int(torch.nonzero(bad.reshape(-1))[0])
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(g.shape)))
    db = g.shape[-1] - 16
    where = f"channel {idx[-1]}" if idx[-1] < C else (f"padding byte {idx[-1]}" if idx[-1] < db else f"scale byte of block {idx[-1] - db}")
    pix = f"image {idx[0]}, pixel ({idx[1]}, {idx[2]})" if len(idx) == 4 else f"pixel {idx[:-1]}"
    return n, f"{pix}, {where}: got 0x{int(g[idx]):02X}, want 0x{int(w[idx]):02X}"


# ------------------------------------------------------------------------------------------------------------------------------------
# values for the quantiser
# ------------------------------------------------------------------------------------------------------------------------------------
BF16_MAX = float(2.0 ** 127 * (2 - 2.0 ** -7))
# block maxima on and next to the edge of (224, 448] -- a mantissa of exactly 1.75 (3.5, 7, 448) maps to 448 itself, the next bf16 above it to
# just over 224 --, the smallest normal number (the scale byte clamps at 1) and the largest bf16
BOUNDARY_MAXIMA = [3.5, 3.5 + 2.0 ** -6, 7.0, 7.0 + 2.0 ** -5, 448.0, 448.0 + 2.0, 1.0, 2.0 - 2.0 ** -7, 2.0 ** -126, BF16_MAX, 0.0]


def boundary_rows(C, seed=0):
    """(len(BOUNDARY_MAXIMA), C) fp32 of bf16 numbers: in row r every 32-channel block has the largest magnitude BOUNDARY_MAXIMA[r] (at a
    seeded position, with a seeded sign); the other values are seeded fractions of it (zero or the maximum itself for 2^-126: nothing
    subnormal)."""
    g = _gen(seed + 97 * C)
    nb = (C + 31) // 32
    rows = []
    for top in BOUNDARY_MAXIMA:
        frac = torch.rand(C, generator=g) * 2 - 1
        if top == 2.0 ** -126:
            frac = frac.sign() * (frac.abs() > 0.5)
        row = (frac.double() * 0.96 * top).float().bfloat16().float()
        for b in range(nb):
            lo, hi = 32 * b, min(C, 32 * b + 32)
            p = lo + int(torch.randint(0, hi - lo, (1,), generator=g))
            row[p] = top if int(torch.randint(0, 2, (1,), generator=g)) else -top
        assert torch.equal(row.bfloat16().float(), row) and float(row.abs().max()) == top
        rows.append(row)
    return torch.stack(rows)
