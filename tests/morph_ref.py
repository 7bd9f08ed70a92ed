"""Reference of the MorphFC token layout and of one MorphFC branch (include/vmg_hip.h: vmg_morphfc_fwd, vmg_morph_tokens_gather / _scatter), by
index arithmetic from the definition, in fp64: torch and numpy only, nothing of vmg_amd, and no pad / reshape / permute chain.

A line of the mixed axis (h: a column of H positions, w: a row of W positions) is cut into gpl = ceil(len / chunk) GROUPS of `chunk`
consecutive positions; the channels are padded C -> Cp = chunk * S.  Group g = (bt * lines + line) * gpl + gi becomes `chunk` tokens:

    token row g * chunk + k, feature f = p * S + s   <-   position gi * chunk + p of the line, channel k * S + s          (0 <= p, k < chunk, 0 <= s < S)

with zero for positions past the end of the line and channels >= C.  untokens is the inverse followed by the crop to (H, W, C)."""
import numpy as np
import torch


def _geo(axis, chunk, H, W):
    assert axis in ("h", "w")
    length, lines = (H, W) if axis == "h" else (W, H)
    return length, lines, -(-length // chunk)


def token_rows(axis, chunk, BT, H, W):
    _, lines, gpl = _geo(axis, chunk, H, W)
    return BT * lines * gpl * chunk


def _source_index(axis, chunk, Cp, BT, H, W, C):
    """For every (token row, feature): the flat index into the (BT, H, W, C) feature map it is taken from, and whether it exists at all."""
    assert Cp % chunk == 0 and Cp >= C
    S = Cp // chunk
    length, lines, gpl = _geo(axis, chunk, H, W)
    row = torch.arange(BT * lines * gpl * chunk, dtype=torch.int64)[:, None]
    f = torch.arange(Cp, dtype=torch.int64)[None, :]
    group, k = row // chunk, row % chunk
    gi, r = group % gpl, group // gpl
    line, bt = r % lines, r // lines
    p, s = f // S, f % S
    pos, c = gi * chunk + p, k * S + s
    y, x = (pos, line) if axis == "h" else (line, pos)
    valid = (pos < length) & (c < C)
    src = ((bt * H + y) * W + x) * C + c
    return torch.where(valid, src, torch.zeros((), dtype=torch.int64)), valid


def tokens_ref(x, axis, chunk, Cp):
    """x (..., H, W, C) of any dtype (integer views of bit patterns too) -> the token matrix (rows, Cp) of the same dtype."""
    H, W, C = x.shape[-3:]
    BT = x.numel() // (H * W * C)
    src, valid = _source_index(axis, chunk, Cp, BT, H, W, C)
    return torch.where(valid, x.reshape(-1)[src], torch.zeros((), dtype=x.dtype))


def untokens_ref(t, axis, chunk, Cp, H, W, C):
    """t (rows, >= Cp) -> (BT, H, W, C): element (bt, y, x, c) is feature p * S + s of token row g * chunk + k, where the pixel is position
    gi * chunk + p of its line and c = k * S + s."""
    assert Cp % chunk == 0 and Cp >= C and t.dim() == 2 and t.shape[1] >= Cp
    S = Cp // chunk
    length, lines, gpl = _geo(axis, chunk, H, W)
    BT = t.shape[0] // (lines * gpl * chunk)
    assert BT * lines * gpl * chunk == t.shape[0]
    i = torch.arange(BT * H * W * C, dtype=torch.int64)
    c, pix = i % C, i // C
    xw, r = pix % W, pix // W
    yh, bt = r % H, r // H
    pos, line = (yh, xw) if axis == "h" else (xw, yh)
    gi, p = pos // chunk, pos % chunk
    k, s = c // S, c % S
    row = ((bt * lines + line) * gpl + gi) * chunk + k
    return t[row, p * S + s].reshape(BT, H, W, C)


def prepare_ref(x, mask, in_scale):
    """The data-gradient form's operand: bf16(fp32(x) * in_scale) where mask > 0, else +0 (-0.0, +0.0 and NaN are not positive); the product
    is the fp32 product, rounded once to bf16."""
    assert x.dtype == torch.bfloat16 and mask.dtype == torch.bfloat16 and x.shape == mask.shape
    prod = (x.float() * torch.tensor(in_scale, dtype=torch.float32)).bfloat16()
    return torch.where(mask.float() > 0, prod, torch.zeros((), dtype=torch.bfloat16))


def branch_ref(x, w, bias, axis, chunk, Cp, relu, out_scale, mask=None, in_scale=1.0):
    """The fused kernel's operation in its own order.  x (..., H, W, C) bf16; w (Cp, Cp): the matrix applied to a token (out = tok w^T);
    bias (Cp) or None.  Returns (v, S, tok): v (BT, H, W, C) fp64 = untokens(act(tok w^T + b) * out_scale), S = sum |tok||w| + |b| in the same
    layout (the magnitude sum of the accumulation, unscaled), tok (rows, Cp) bf16: the operand matrix the GEMM multiplies."""
    assert x.dtype == torch.bfloat16
    H, W, C = x.shape[-3:]
    if mask is not None:
        x = prepare_ref(x, mask, in_scale)
    else:
        assert in_scale == 1.0, "the plain form does not scale its operand"
    tok = tokens_ref(x, axis, chunk, Cp)
    t64, w64 = tok.double(), w.double()
    acc, S = t64 @ w64.t(), t64.abs() @ w64.abs().t()
    if bias is not None:
        acc, S = acc + bias.double(), S + bias.double().abs()
    if relu:
        acc = torch.clamp(acc, min=0.0)
    acc = acc * float(np.float32(out_scale))
    return untokens_ref(acc, axis, chunk, Cp, H, W, C), untokens_ref(S, axis, chunk, Cp, H, W, C), tok
