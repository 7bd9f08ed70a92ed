"""Reference of the OPERATIONS behind the LayerNorm kernels of csrc/elementwise.hip (layernorm_fwd_kernel, layernorm_bwd_kernel and their
space<->depth forms), spelled the slow obvious way in fp64, with per-element rounding-error bounds derived from the kernels' operation
counts.  Plain module: torch only, nothing of vmg_amd, no fixtures.

Tensors come in their storage dtype (bf16 or fp32, on the CPU): the caller rounds BEFORE calling, so the reference sees the values the
kernel sees.  Two rounding points are declared by the kernel and mirrored here, because they are part of the operation, not of its error:
  * several output gradients are added in fp32 in list order and the sum is rounded to the storage dtype (sum_grads: IEEE adds in a fixed
    order are bit-identical on the CPU); the fp64 formulas are fed the rounded sum;
  * with `add`, dx is rounded to storage and dx + add is rounded again.  The reference returns the unrounded fp64 dx + add and the bound
    accounts for both roundings.

Bounds.  U = 2^-24 (fp32), u = the unit roundoff of the storage dtype (2^-8 bf16, U fp32), xh the fp64 normalised value, g = dy * w, rs the
reciprocal standard deviation, overbars row means.  Each is `operation count x U x magnitude`, first order, with the count written out:
  mean   C - 1 adds and one division: (C - 1) U mean|x| + U |mu| <= Emu = (C + 1) U mean|x|; the test bound adds U |mu| once more.
  rstd   relative Ers = ((C + 8) / 2) U + 0.5 rs^2 Emu^2.  x - mu (1), its square (2 + 1), C - 1 adds, / C (1), + eps (1): (C + 4) U on
         var + eps, halved by the inverse square root; the remaining 2 U is the allowance for rsqrtf.  ASSUMPTION: no HIP math accuracy
         table ships with the ROCm tree this was written against, so the allowance is not taken from one: 2 U relative is 4 half-ulp
         steps, i.e. a result within one to two ulp of the exact one depending on where in its binade it lies.  The mean's error enters
         the two-pass variance only in second order (sum (x - mu - e)^2 = sum (x - mu)^2 + C e^2).
  y      E32 = U (4 |xh w| + |y|) + |xh w| Ers + |w| rs Emu: subtract, two products and the final add (3 U |xh w| + U |y|, one U spare),
         the rstd and the mean error carried through.  fp32: E32.  bf16: u |y| + (1 + u) E32 (the final round-to-nearest).
  dx     Es1 = (C + 2) U mean|g|, Es2 = (C + 6) U mean|g xh| (the sums s1, s2 with their per-term products and xh's two roundings),
         E32 = rs (Es1 + |xh| Es2 + U (3 |g| + 2 |s1| + 6 |xh s2|)) + 2 U |dx|.  fp32: E32.  bf16: u |dx| + (1 + u) E32 -- the factor
         (1 + u) on E32 is re-derived: round-to-nearest of the fp32 value v errs by u |v| <= u (|dx| + E32), as for y.
  dx+add B1 (1 + u') + u' |dx + add| with B1 the bound without add and u' the error of `fp32 add, then round to storage`: U for fp32,
         u + U (1 + u) for bf16 (re-derived: the fp32 sum of two bf16 values is not always exact, so the add rounds twice).
  dw     M products d * xh (3 roundings each with xh's two) summed in any order: (M + 5) U sum|dy xh|.
  db     M exact values summed in any order: (M - 1) U sum|dy|.
  into   caller-owned (dw, db): every add INTO the buffer rounds at the buffer's magnitude, <= |buffer| + sum|terms|.  Re-derived from the
         launch: up to 32 blocks each add with one atomic per channel (`nadd` = blocks roundings); above, one block adds once.
None of these figures is measured on a kernel."""
from collections import namedtuple

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
UB = 2.0 ** -8
EPS = 1e-5
LN_MAXV, LN_SUB = 4, 32
FWD_BLOCK_CAP, BWD_BLOCK_CAP = 1024, 512


def unit(dtype):
    return {F32: U, BF16: UB}[dtype]


def _d(t):
    return None if t is None else t.detach().to(F64)


# ------------------------------------------------------------------------------------------------ the launchers' choices, restated
def ln_vec(dtype, C, vmax=8):
    """Widest vector (in elements) that divides C, at most vmax (the segment length's own ln_vec in the space<->depth forms)."""
    v = next(k for k in ((8, 4, 2, 1) if dtype == BF16 else (4, 2, 1)) if C % k == 0)
    while v > vmax:
        v >>= 1
    return v


def ln_group(nvec):
    """Lanes per row: the G in {64, 32, 16} with the fewest lane slots G * NV, the smaller G on a tie."""
    best, slots = 64, 1 << 30
    for g in (64, 32, 16):
        nv = -(-nvec // g)
        if nv > LN_MAXV:
            continue
        nvp = 4 if nv == 3 else nv
        if g * nvp <= slots:
            slots, best = g * nvp, g
    return best


Inst = namedtuple("Inst", "V G NV nv rpb fwd_blocks bwd_blocks")


def instantiation(dtype, C, M, vmax=8):
    """(V, G, NV, nv, rows per block, forward blocks, backward blocks) of a case; None where the launcher refuses C."""
    V = ln_vec(dtype, C, vmax)
    nvec = C // V
    G = ln_group(nvec)
    if nvec > G * LN_MAXV:
        return None
    nv = -(-nvec // G)
    rpb = 256 // G
    return Inst(V, G, 4 if nv == 3 else nv, nv, rpb, min(FWD_BLOCK_CAP, -(-M // (rpb * 4))), min(BWD_BLOCK_CAP, -(-M // (rpb * 8))))


def case_id(dtype, C, M, vmax=8):
    i = instantiation(dtype, C, M, vmax)
    via = f"via{i.nv}" if i.nv != i.NV else ""
    path = "ws" if i.bwd_blocks > LN_SUB else "atomics"
    return f"{'bf16' if dtype == BF16 else 'fp32'}-C{C}-V{i.V}-G{i.G}-NV{i.NV}{via}-M{M}-blocks{i.fwd_blocks}f{i.bwd_blocks}b-{path}"


# ------------------------------------------------------------------------------------------------ space<->depth row maps
def rows_of(x, mode):
    """The LayerNorm rows of a feature map x (N, Hin, Win, Cin), channel order (neiw neih c) as in ln_src_elem.
    'down': (N, Hin/2, Win/2, 4 Cin), segment neiw*2 + neih of row (h, w) is pixel (2h + neih, 2w + neiw).
    'up':   (N, 2 Hin, 2 Win, Cin/4), row (y, x) is the slice (x%2)*2 + (y%2) of pixel (y/2, x/2)."""
    N, H, W, C = x.shape
    if mode == "down":
        out = x.new_zeros((N, H // 2, W // 2, 4 * C))
        for neiw in (0, 1):
            for neih in (0, 1):
                sg = neiw * 2 + neih
                out[..., sg * C:(sg + 1) * C] = x[:, neih::2, neiw::2, :]
        return out
    c = C // 4
    out = x.new_zeros((N, 2 * H, 2 * W, c))
    for neiw in (0, 1):
        for neih in (0, 1):
            sg = neiw * 2 + neih
            out[:, neih::2, neiw::2, :] = x[..., sg * c:(sg + 1) * c]
    return out


def input_of(rows, mode):
    """The inverse of rows_of: row-shaped values (a gradient) scattered back to the feature map's layout."""
    N, H, W, C = rows.shape
    if mode == "down":
        c = C // 4
        out = rows.new_zeros((N, 2 * H, 2 * W, c))
        for neiw in (0, 1):
            for neih in (0, 1):
                sg = neiw * 2 + neih
                out[:, neih::2, neiw::2, :] = rows[..., sg * c:(sg + 1) * c]
        return out
    out = rows.new_zeros((N, H // 2, W // 2, 4 * C))
    for neiw in (0, 1):
        for neih in (0, 1):
            sg = neiw * 2 + neih
            out[..., sg * C:(sg + 1) * C] = rows[:, neih::2, neiw::2, :]
    return out


# ------------------------------------------------------------------------------------------------ forward
def ln_fwd_ref(x, w, b, eps=EPS):
    """-> (y, mean, rstd) in fp64; x (..., C) rows, w / b (C,)."""
    x, w, b = _d(x), _d(w), _d(b)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    return (x - mu) * rs * w + b, mu.squeeze(-1), rs.squeeze(-1)


Fwd = namedtuple("Fwd", "y mean rstd By Bmean Brstd Emu Ers")


def ln_fwd_bounds(x, w, b, eps=EPS):
    """The forward reference and the per-element / per-row absolute bounds of the module docstring; the storage dtype is x's."""
    u = unit(x.dtype)
    C = x.shape[-1]
    y, mu, rs = ln_fwd_ref(x, w, b, eps)
    xd, wd = _d(x), _d(w)
    Emu = (C + 1) * U * xd.abs().mean(-1)
    Ers = ((C + 8) / 2) * U + 0.5 * rs ** 2 * Emu ** 2
    xhw = ((xd - mu[..., None]) * rs[..., None] * wd).abs()
    E32 = U * (4 * xhw + y.abs()) + xhw * Ers[..., None] + wd.abs() * (rs * Emu)[..., None]
    By = E32 if x.dtype == F32 else u * y.abs() + (1 + u) * E32
    return Fwd(y, mu, rs, By, Emu + U * mu.abs(), rs * Ers, Emu, Ers)


# ------------------------------------------------------------------------------------------------ backward
def sum_grads(dys):
    """The kernel's summed output gradient: fp32 adds in list order, the sum rounded to the storage dtype (one gradient: itself)."""
    if len(dys) == 1:
        return dys[0]
    acc = dys[0].to(F32)
    for t in dys[1:]:
        acc = acc + t.to(F32)
    return acc.to(dys[0].dtype)


def _bwd_terms(dys, x, mean32, rstd32, w):
    dy, xd, wd = _d(sum_grads(list(dys))), _d(x), _d(w)
    mu, rs = _d(mean32).reshape(*x.shape[:-1], 1), _d(rstd32).reshape(*x.shape[:-1], 1)
    xh = (xd - mu) * rs
    g = dy * wd
    s1, s2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    return dy, xh, g, s1, s2, rs


def ln_bwd_ref(dys, x, mean32, rstd32, w, add=None):
    """-> (dx, dw, db) in fp64 for the statistics AS GIVEN (the fp32 values the kernel is handed).  dys: a list of 1..5 gradients."""
    dy, xh, g, s1, s2, rs = _bwd_terms(dys, x, mean32, rstd32, w)
    dx = rs * (g - s1 - xh * s2)
    if add is not None:
        dx = dx + _d(add)
    C = x.shape[-1]
    return dx, (dy * xh).reshape(-1, C).sum(0), dy.reshape(-1, C).sum(0)


Bwd = namedtuple("Bwd", "dx dw db Bdx Bdw Bdb Mdw Mdb")


def ln_bwd_bounds(dys, x, mean32, rstd32, w, add=None):
    """The backward reference and its bounds.  Mdw / Mdb: sum|dy xh| and sum|dy| per channel, what the `into` term multiplies."""
    u = unit(x.dtype)
    C = x.shape[-1]
    M = x.numel() // C
    dy, xh, g, s1, s2, rs = _bwd_terms(dys, x, mean32, rstd32, w)
    dx = rs * (g - s1 - xh * s2)
    Es1 = (C + 2) * U * g.abs().mean(-1, keepdim=True)
    Es2 = (C + 6) * U * (g * xh).abs().mean(-1, keepdim=True)
    E32 = rs * (Es1 + xh.abs() * Es2 + U * (3 * g.abs() + 2 * s1.abs() + 6 * (xh * s2).abs())) + 2 * U * dx.abs()
    B = E32 if x.dtype == F32 else u * dx.abs() + (1 + u) * E32
    if add is not None:
        u2 = U if x.dtype == F32 else u + U * (1 + u)
        dx = dx + _d(add)
        B = B * (1 + u2) + u2 * dx.abs()
    Mdw, Mdb = (dy * xh).abs().reshape(-1, C).sum(0), dy.abs().reshape(-1, C).sum(0)
    return Bwd(dx, (dy * xh).reshape(-1, C).sum(0), dy.reshape(-1, C).sum(0), B, (M + 5) * U * Mdw, (M - 1) * U * Mdb, Mdw, Mdb)


def into_bound(fresh_bound, mag, buf0, k, nadd):
    """Bound of caller-owned dw or db after k calls that each add the gradient to a buffer that held buf0: k times the fresh bound plus,
    per call, `nadd` roundings at the buffer's magnitude (<= |buf0| + k * sum|terms|)."""
    return k * (fresh_bound + nadd * U * (_d(buf0).abs() + k * mag))


def bwd_adds_into_buffer(inst):
    """Roundings at the buffer's magnitude per call: one atomic per block up to LN_SUB blocks, one plain add by the last block above."""
    return inst.bwd_blocks if inst.bwd_blocks <= LN_SUB else 1


# ------------------------------------------------------------------------------------------------ inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_rows(M, C, dtype, seed):
    """(M, C) rows whose kind cycles with the row index -- normal; offset (mean 50, std 1); near constant (1 + 1e-3 n); magnitude 1e3 --
    rounded to dtype.  From 8 rows on, row M // 2 is exactly constant (2.5)."""
    n = torch.randn((M, C), generator=_gen(seed), dtype=F64)
    x = n.clone()
    x[1::4] = 50.0 + n[1::4]
    x[2::4] = 1.0 + 1e-3 * n[2::4]
    x[3::4] = 1e3 * n[3::4]
    if M >= 8:
        x[M // 2] = 2.5
    return x.to(dtype)


def const_row(M):
    return M // 2 if M >= 8 else None


def make_affine(C, seed):
    """fp32 (w, b) that differ between neighbouring channels: a zig-zag of +-0.25 around 1 (w) and +-0.5 (b) plus seeded noise that cannot
    close the gap (|noise| <= 0.1), so that a neighbour's weight is never within a rounding bound of a channel's own."""
    g = _gen(seed)
    zig = torch.tensor([1.0, -1.0]).repeat(C // 2 + 1)[:C]
    w = 1.0 + 0.25 * zig + 0.2 * (torch.rand(C, generator=g) - 0.5)
    b = 0.5 * zig + 0.2 * (torch.rand(C, generator=g) - 0.5)
    return w.to(F32), b.to(F32)


def make_grads(shape, dtype, seed, n=1):
    g = _gen(seed)
    return [torch.randn(tuple(shape), generator=g).to(dtype) for _ in range(n)]


def int_grads(shape, dtype, seed, n=1):
    """Integer gradients in {-4 .. 4} without 0: exact in bf16, and so is any fp32 sum of fewer than 2^22 of them."""
    g = _gen(seed)
    out = []
    for _ in range(n):
        mag = torch.randint(1, 5, tuple(shape), generator=g, dtype=torch.int8)
        sign = torch.randint(0, 2, tuple(shape), generator=g, dtype=torch.int8) * 2 - 1
        out.append((mag * sign).to(dtype))
    return out


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over all elements (0 / 0 counts as 0): <= 1 means every element is within its bound."""
    err = (_d(got) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0
