"""Reference of the OPERATIONS behind the kernels of csrc/tab_ops.hip (group_reduce, group_reduce3, tab_elementwise, maxpool) and of
avgpool2 (csrc/spynet.hip), spelled the slow obvious way in fp64.  Plain module: torch and numpy only, nothing of vmg_amd, no fixtures.

Tensors are (G * R, C)-shaped (any leading shape whose rows split into G equal groups).  Every function converts its inputs to fp64
first: the caller rounds the inputs to the tested dtype BEFORE calling, so that the reference sees the values the kernel sees.

Next to each result the references return a magnitude: the same expression with every term replaced by its absolute value (and
1 - t^2 by 1 + t^2).  Rounding error bounds are multiples of `unit roundoff x magnitude`; the result itself may be small by cancellation."""
import numpy as np
import torch

OP_CA_FWD, OP_CA_BWD, OP_MIX_FWD, OP_MIX_BWD, OP_GATE_FWD, OP_GATE_BWD, OP_AFFINE2, OP_SCALE, OP_GATE_RES_FWD, OP_GATE_RES_BWD = range(10)
OP_NAMES = ("ca_fwd", "ca_bwd", "mix_fwd", "mix_bwd", "gate_fwd", "gate_bwd", "affine2", "scale", "gate_res_fwd", "gate_res_bwd")
# per op: operands read besides p0, coefficients per (group, channel) in coef, whether add (G, C) is read, outputs.  OP_AFFINE2's p1 is optional.
OP_USES = {OP_CA_FWD: (("p1",), 1, False, 1), OP_CA_BWD: ((), 1, True, 2), OP_MIX_FWD: (("p1", "p2"), 3, False, 1), OP_MIX_BWD: ((), 3, True, 3),
           OP_GATE_FWD: (("p1",), 0, False, 1), OP_GATE_BWD: (("p1", "p2"), 0, False, 2), OP_AFFINE2: ((), 2, True, 1), OP_SCALE: ((), 1, False, 1),
           OP_GATE_RES_FWD: (("p1", "p2"), 1, False, 1), OP_GATE_RES_BWD: (("p1", "p2"), 1, False, 2)}


def _d(t):
    return None if t is None else t.detach().to(torch.float64)


def _grc(t, G):
    C = t.shape[-1]
    rows = t.numel() // C
    assert rows % G == 0
    return t.reshape(G, rows // G, C)


# ------------------------------------------------------------------------------------------------ reductions
def group_reduce_ref(a, G, b=None, c3=None, mode=0, scale=1.0):
    """-> (out, mag), fp64 (G, C).  mode 0: out[g, c] = scale * sum_r (a [+ b [+ c3]])[g, r, c]; mode 1: scale * sum_r a * b.
    mag = |scale| * sum_r of the |addends| (|a| + |b| + |c3|, or |a * b|): what a summation error bound multiplies."""
    assert mode in (0, 1) and (mode == 0 or b is not None) and (c3 is None or b is not None)
    a, b, c3 = (None if t is None else _grc(_d(t), G) for t in (a, b, c3))
    if mode == 1:
        assert c3 is None
        term = a * b
        mag = term.abs()
    else:
        term, mag = a, a.abs()
        for t in (b, c3):
            if t is not None:
                term, mag = term + t, mag + t.abs()
    return scale * term.sum(1), abs(scale) * mag.sum(1)


def group_reduce3_ref(a, b0, b1, b2, G, scale=1.0):
    """-> (out, mag), fp64 (G, C, 3): out[g, c, k] = scale * sum_r a * b_k."""
    a = _grc(_d(a), G)
    prods = [a * _grc(_d(t), G) for t in (b0, b1, b2)]
    return scale * torch.stack([p.sum(1) for p in prods], -1), abs(scale) * torch.stack([p.abs().sum(1) for p in prods], -1)


# ------------------------------------------------------------------------------------------------ elementwise
def _round(t, dtype):
    return t if dtype is None or dtype == torch.float64 else t.to(dtype).to(torch.float64)


def tab_elementwise_ref(op, p0, p1=None, p2=None, coef=None, add=None, s=1.0, G=1, dtype=None):
    """-> (outs, mags): lists of fp64 tensors of p0's shape, one per output of the op (include/vmg_hip.h, csrc/tab_ops.hip).
    coef (G, C[, k]) and add (G, C) are broadcast over the R rows of their group.  dtype: the tensor dtype of the kernel under test; only
    the two OP_GATE_RES_* ops use it -- they round one intermediate to it by design (the gate, resp. dout * g: what the two-pass form stored
    between its kernels), and so does this reference, at the same point."""
    shape = p0.shape
    C = shape[-1]
    extra, ncoef, has_add, _ = OP_USES[op]
    assert all({"p1": p1, "p2": p2}[n] is not None for n in extra) and (ncoef == 0 or coef is not None) and (not has_add or add is not None)
    p0, p1, p2 = (None if t is None else _grc(_d(t), G) for t in (p0, p1, p2))
    if ncoef:
        assert coef.numel() == G * C * ncoef
        k = _d(coef).reshape(G, 1, C, ncoef)
        k = [k[..., i] for i in range(ncoef)]
    if has_add:
        assert add.numel() == G * C
        ad = _d(add).reshape(G, 1, C)
    s = float(s)
    if op == OP_CA_FWD:
        outs, mags = [(p0 * k[0] + p1) * s], [((p0 * k[0]).abs() + p1.abs()) * abs(s)]
    elif op == OP_SCALE:
        outs = [p0 * k[0] * s]
        mags = [outs[0].abs()]
    elif op == OP_CA_BWD:
        d = p0 * s
        outs, mags = [d * k[0] + ad, d], [(d * k[0]).abs() + ad.abs(), d.abs()]
    elif op == OP_MIX_FWD:
        terms = [p0 * k[0], p1 * k[1], p2 * k[2]]
        outs, mags = [terms[0] + terms[1] + terms[2]], [terms[0].abs() + terms[1].abs() + terms[2].abs()]
    elif op == OP_MIX_BWD:
        outs, mags = [p0 * k[i] + ad for i in range(3)], [(p0 * k[i]).abs() + ad.abs() for i in range(3)]
    elif op == OP_AFFINE2:
        t, m = p0 * k[0] + ad, (p0 * k[0]).abs() + ad.abs()
        if p1 is not None:
            t, m = t + p1 * k[1], m + (p1 * k[1]).abs()
        outs, mags = [t.clamp_min(0) if s > 0.5 else t], [m]
    elif op == OP_GATE_FWD:
        t = torch.tanh(p1)
        outs, mags = [(p0 + p1) * t], [(p0.abs() + p1.abs()) * t.abs()]
    elif op == OP_GATE_BWD:
        d, x, y = p0, p1, p2
        t = torch.tanh(y)
        outs = [d * t, d * (t + (x + y) * (1 - t * t))]
        mags = [(d * t).abs(), d.abs() * (t.abs() + (x.abs() + y.abs()) * (1 + t * t))]
    elif op == OP_GATE_RES_FWD:
        x, y, res = p0, p1, p2
        gate = _round((x + y) * torch.tanh(y), dtype)
        outs, mags = [(gate * k[0] + res) * s], [((gate * k[0]).abs() + res.abs()) * abs(s)]
    elif op == OP_GATE_RES_BWD:
        x, y = p1, p2
        d = _round(p0 * k[0] * s, dtype)
        t = torch.tanh(y)
        outs = [d * t, d * (t + (x + y) * (1 - t * t))]
        mags = [(d * t).abs(), d.abs() * (t.abs() + (x.abs() + y.abs()) * (1 + t * t))]
    else:
        raise ValueError(op)
    return [o.reshape(shape) for o in outs], [m.reshape(shape) for m in mags]


def gate_res_intermediate(op, p0, p1, p2, coef, s, G):
    """-> (value, mag) fp64 of the intermediate that an OP_GATE_RES_* op rounds to the tensor dtype, before that rounding."""
    p0, p1, p2 = (_grc(_d(t), G) for t in (p0, p1, p2))
    if op == OP_GATE_RES_FWD:
        t = torch.tanh(p1)
        return ((p0 + p1) * t).reshape(-1), ((p0.abs() + p1.abs()) * t.abs()).reshape(-1)
    assert op == OP_GATE_RES_BWD
    v = p0 * _d(coef).reshape(G, 1, -1) * float(s)
    return v.reshape(-1), v.abs().reshape(-1)


def bf16_tie_distance(v):
    """A lower bound of the distance of each fp64 value to the nearest point where round-to-nearest to bf16 changes its result (the midpoint
    of two neighbouring bf16 numbers).  A value computed in fp32 rounds to the same bf16 number as the exact one when its error stays below
    this.  (Below a power of two the spacing halves: both spacings are tried and the smaller distance returned.)"""
    v = v.to(torch.float64)
    r = v.to(torch.bfloat16).to(torch.float64)
    e = torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -120)))
    ulp = torch.pow(2.0, e - 7)
    off = (v - r).abs()
    return torch.minimum((off - ulp / 2).abs(), (off - ulp / 4).abs())


# ------------------------------------------------------------------------------------------------ pooling
def maxpool_ref(x, f, dy=None):
    """Non-overlapping f x f max pooling of (n, h, w, c).  -> (y, idx[, dx]): y fp64 (n, h/f, w/f, c); idx uint8: the position iy * f + ix of
    the FIRST maximum of the window in row-major order (numpy.argmax: a NaN counts as the maximum, the first NaN wins -- as ATen does);
    dx (with dy given): dy at each window's winner, zero elsewhere."""
    n, h, w, c = x.shape
    assert h % f == 0 and w % f == 0 and f >= 1
    ho, wo = h // f, w // f
    win = x.detach().to(torch.float64).numpy().reshape(n, ho, f, wo, f, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, ho, wo, c, f * f)
    idx = np.argmax(win, axis=-1)
    y = np.take_along_axis(win, idx[..., None], -1)[..., 0]
    out = (torch.from_numpy(np.ascontiguousarray(y)), torch.from_numpy(idx.astype(np.uint8)))
    if dy is None:
        return out
    g = dy.detach().to(torch.float64).numpy()
    onehot = (idx[..., None] == np.arange(f * f)) * g[..., None]                                         # (n, ho, wo, c, f*f)
    dx = onehot.reshape(n, ho, wo, c, f, f).transpose(0, 1, 4, 2, 5, 3).reshape(n, h, w, c)
    return out + (torch.from_numpy(np.ascontiguousarray(dx)),)


def avgpool2_ref(x):
    """F.avg_pool2d(x, 2, 2) on channels-last (n, h, w, c): an odd last row / column is dropped.  -> (y, mag) fp64, mag = mean of |x|."""
    n, h, w, c = x.shape
    x = x.detach().to(torch.float64)[:, :h // 2 * 2, :w // 2 * 2].reshape(n, h // 2, 2, w // 2, 2, c)
    return x.sum((2, 4)) * 0.25, x.abs().sum((2, 4)) * 0.25
