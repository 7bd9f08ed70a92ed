"""Reference of the OPERATION behind vmg_win3d_attn_fwd / _bwd (include/vmg_hip.h), spelled the slow obvious way with the oracle's
own window_partition / shift_mask / relative_position_index / window_reverse.  Plain module: no fixtures, imports the oracle only.

The kernels never build a padded volume, a rolled volume, a mask tensor or an index table: they compute all of it per token
(locate(), rel_index() in csrc/win3d.hip).  Nothing of that arithmetic is repeated here, so a mistake in it cannot cancel."""
import torch

from oracle import vmg_oracle as O


def reround(t, dtype):
    """t rounded to `dtype` and brought back.  Autograd rounds the gradient that flows back through this point the same way, which is
    what the kernels do there too: the backward products take dS (the gradient at the probabilities' side) as bf16 operands."""
    return t.to(dtype).to(t.dtype)


def other_slices(i, wt):
    """Token indices of a (wt, 8, 8) window that time slice i's queries attend to: every slice but their own."""
    return [s for s in range(wt * 64) if s // 64 != i]


def win3d_reference(q, kv, bq, bkv, table, heads, wt, shift, *, emulate=None):
    """q (B, D, H, W, C), kv (B, D, H, W, 2C; k then v): outputs of the q / kv Linears on the un-partitioned map; bq (C) / bkv (2C):
    those Linears' biases or None; table ((2 wt - 1) * 225, heads); shift (sd, sh, sw), zeros on an unshifted block.
    -> out (B, D, H, W, C), lse (windows, heads, wt * 64) natural-log logsumexp of every query's logits, in the dtype of q.

    emulate = torch.bfloat16 re-rounds where the kernels document a rounding: the biases that padded tokens hold (bf16 MFMA operands),
    the probabilities before P.V (and with them, in the backward, the gradient arriving there), and the stored output.  It measures a
    rounding floor; it is not a second reference."""
    B, D, H, W, C = q.shape
    d = C // heads
    ws = (wt, 8, 8)
    Dp, Hp, Wp = -(-D // wt) * wt, -(-H // 8) * 8, -(-W // 8) * 8
    rnd = (lambda t: t) if emulate is None else (lambda t: reround(t, emulate))
    shift = tuple(int(s) for s in shift)
    shifted = any(s > 0 for s in shift)

    def windows(x, bias):
        n = x.shape[-1]
        # the reference pads zeros BEFORE the Linears: a padded position comes out of them holding the bias
        vol = x.new_zeros(B, Dp, Hp, Wp, n) if bias is None else rnd(bias.to(x.dtype)).expand(B, Dp, Hp, Wp, n).clone()
        vol[:, :D, :H, :W] = x
        if shifted:
            vol = torch.roll(vol, shifts=(-shift[0], -shift[1], -shift[2]), dims=(1, 2, 3))
        return O.window_partition(vol, ws)  # (B * nW, N, n)

    qw, kvw = windows(q, bq), windows(kv, bkv)
    nwin, N = qw.shape[0], wt * 64
    qh = qw.reshape(nwin, N, heads, d).permute(0, 2, 1, 3)
    kh = kvw[..., :C].reshape(nwin, N, heads, d).permute(0, 2, 1, 3)
    vh = kvw[..., C:].reshape(nwin, N, heads, d).permute(0, 2, 1, 3)
    index = O.relative_position_index(ws)
    bias = table[index.reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)  # (heads, query, key)
    mask = O.shift_mask(Dp, Hp, Wp, ws, shift).to(q.dtype).repeat(B, 1, 1) if shifted else None  # (B * nW, query, key)
    outs, lses = [], []
    for i in range(wt):
        lo, hi, other = 64 * i, 64 * i + 64, other_slices(i, wt)
        logits = (qh[:, :, lo:hi] * d ** -0.5) @ kh[:, :, other].transpose(-2, -1) + bias[None, :, lo:hi][..., other]
        if mask is not None:
            logits = logits + mask[:, None, lo:hi][..., other]
        lses.append(torch.logsumexp(logits, -1))
        p = rnd(torch.softmax(logits, -1))
        outs.append((p @ vh[:, :, other]).transpose(1, 2).reshape(nwin, 64, C))
    o = O.window_reverse(torch.cat(outs, 1).reshape(-1, wt, 8, 8, C), ws, B, Dp, Hp, Wp)
    if shifted:
        o = torch.roll(o, shifts=shift, dims=(1, 2, 3))
    return rnd(o[:, :D, :H, :W].contiguous()), torch.cat(lses, -1)


NAMES = ("out", "lse", "dq", "dkv", "dtable", "dbq", "dbkv")


def reference_all(q, kv, bq, bkv, table, dout, heads, wt, shift, *, dtype=torch.float64, emulate=None):
    """Forward and autograd of win3d_reference on copies of the arguments in `dtype` -> dict of out, lse, dq, dkv, dtable, dbq, dbkv
    (detached, float64).  dbq / dbkv are None when the bias is; a bias no gradient reaches reports exact zeros.  With `emulate`, dq and
    dkv are rounded like the stored output: the kernels write them in the tensors' dtype."""
    leaves = [t.detach().to(dtype).requires_grad_(True) if t is not None else None for t in (q, kv, bq, bkv, table)]
    out, lse = win3d_reference(*leaves, heads, wt, shift, emulate=emulate)
    live = [t for t in leaves if t is not None]
    grads = list(torch.autograd.grad(out, live, dout.to(dtype), allow_unused=True))
    g = [None if t is None else (grads.pop(0), t) for t in leaves]
    g = [None if e is None else (torch.zeros_like(e[1]) if e[0] is None else e[0]) for e in g]
    if emulate is not None:
        g[0], g[1] = reround(g[0], emulate), reround(g[1], emulate)
    res = dict(out=out, lse=lse, dq=g[0], dkv=g[1], dbq=g[2], dbkv=g[3], dtable=g[4])
    return {k: (None if v is None else v.detach().double()) for k, v in res.items()}
