"""Plain CPU references of the glue kernels: the non-LayerNorm half of csrc/elementwise.hip (act_bwd, pixel_shuffle / unshuffle,
pixel_unshuffle_actgrad, frame_gather, sum_n, cast_clear, pair_steps) and csrc/spynet.hip (spy_prep, spy_operand fwd / bwd, spy_flow_add,
upsample2x_ac fwd / bwd).  Each is written from the operation's definition in torch / NumPy -- reshapes, index_select, cat, split, stack --
and not from the kernels' index arithmetic; tests/test_glue_ref.py pins each against an independent torch spelling.

Where the kernel's arithmetic is a fixed sequence of fp32 operations with one rounding to the tensor dtype, the reference performs the
same sequence in float32 (IEEE, so the bits are defined) and the comparison is of bits.  Where it is not (GELU's derivative, the
bilinear up-sampling) the reference is fp64 and returns, next to the value, the magnitude that a rounding-error bound scales with.

All arguments are CPU tensors.  A tensor "of dtype bf16" may be passed as the bf16 tensor itself or as fp32 holding bf16 values."""
import numpy as np
import torch

from tests.conv_ref import gelu_grad_ref

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_GELU = 0, 1, 2, 3  # vmg_amd.hip.ACT_* (include/vmg_hip.h VMG_ACT_*)
F32 = torch.float32


def bits(t):
    """The tensor's bit patterns as integers: equality of these tells +0 from -0 and compares NaNs by payload."""
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ================================================================================================ activation backward
def act_backward_ref(dy, ref, act, slope, alpha, dtype):
    """dy * alpha * act'(ref).  NONE / RELU / LRELU: d = 1, (ref > 0 ? 1 : 0), (ref > 0 ? 1 : slope) -- a NaN ref compares false --
    and the result is ((dy * d) * alpha) in float32, in that order, rounded once to `dtype`: a tensor of `dtype`, exact bits.
    GELU: -> (want, mag) in fp64: want = dy * alpha * (Phi(ref) + ref * phi(ref)), mag = |dy * alpha|.  That formula (conv_ref.gelu_grad_ref,
    torch's own GELU backward) is NaN at ref = +-inf (inf * 0) and at NaN, and `want` says so."""
    dy, ref = dy.to(F32), ref.to(F32)
    if act == ACT_GELU:
        a = np.float64(np.float32(alpha))
        g = dy.double() * a
        return g * gelu_grad_ref(ref), g.abs()
    if act == ACT_NONE:
        d = torch.ones_like(ref)
    else:
        lo = 0.0 if act == ACT_RELU else float(np.float32(slope))
        d = torch.where(ref > 0, torch.ones_like(ref), torch.full_like(ref, lo))
    return ((dy * d) * torch.tensor(alpha, dtype=F32)).to(dtype)


# ================================================================================================ depth <-> space
def pixel_shuffle_ref(x):
    """nn.PixelShuffle(2) on channels-last: (N, H, W, 4c) -> (N, 2H, 2W, c), input channel 4c' + 2i + j -> pixel (2y + i, 2x + j), channel c'."""
    N, H, W, c4 = x.shape
    c = c4 // 4
    return x.reshape(N, H, W, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2 * H, 2 * W, c).contiguous()


def pixel_unshuffle_ref(x):
    """nn.PixelUnshuffle(2) on channels-last: (N, 2H, 2W, c) -> (N, H, W, 4c); the inverse of pixel_shuffle_ref."""
    N, H2, W2, c = x.shape
    return x.reshape(N, H2 // 2, 2, W2 // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(N, H2 // 2, W2 // 2, 4 * c).contiguous()


# ================================================================================================ frame moves
def frame_gather_ref(src, idx):
    """src (n_src, frame elements), idx (n_dst, 1 | 2) int.  One column: dst[f] = src[idx[f, 0]], a copy.  Two columns:
    0 + a + b in float32 in that order, a term whose index is < 0 contributing 0, one rounding to src's dtype."""
    idx = idx.long()
    if idx.shape[1] == 1:
        return src.index_select(0, idx[:, 0])
    acc = torch.zeros((idx.shape[0], src.shape[1]), dtype=F32)
    for k in range(2):
        term = src.index_select(0, idx[:, k].clamp(min=0)).to(F32)
        acc = acc + torch.where((idx[:, k] >= 0)[:, None], term, torch.zeros_like(term))
    return acc.to(src.dtype)


def sum_n_ref(ts):
    """Sequential float32 sum in list order, starting from 0, one rounding to the tensors' dtype."""
    acc = torch.zeros(ts[0].shape, dtype=F32)
    for t in ts:
        acc = acc + t.to(F32)
    return acc.to(ts[0].dtype)


def cast_clear_ref(acc, add, dtype):
    """(acc [+ add]) in float32, one rounding to `dtype`."""
    return (acc if add is None else acc + add.to(F32)).to(dtype)


def pair_steps_ref(mode, n, t, steps=None, a=None, b=None):
    """The t step tensors (2n, *frame) of the lock-step sweeps: rows [0, n) = the backward sweep at frame t-1-j, rows [n, 2n) = the forward
    sweep at frame j.  mode 0: steps -> (back, fwd), both (n, t, *frame) in frame order (split / reversed / stack).  mode 1: back = a,
    fwd = b -> the list of steps.  mode 2: steps -> a[i, f] = steps[t-1-f][i] + steps[f][n+i], float32 sum, one rounding."""
    if mode == 1:
        return [torch.cat([a[:, t - 1 - j], b[:, j]], 0) for j in range(t)]
    halves = [s.split(n, 0) for s in steps]
    back = torch.stack([hv[0] for hv in reversed(halves)], 1)
    fwd = torch.stack([hv[1] for hv in halves], 1)
    if mode == 0:
        return back, fwd
    return (back.to(F32) + fwd.to(F32)).to(steps[0].dtype)


# ================================================================================================ SPyNet glue
def spy_prep_ref(img, mean, std, dtype):
    """(n, 3, h, w) fp32 -> (n, h, w, 8) `dtype`: float32 subtraction, then float32 division, one round-to-nearest-even to `dtype`, in channels
    0..2; channels 3..7 are +0."""
    n, _, h, w = img.shape
    v = (img - mean.reshape(1, 3, 1, 1)) / std.reshape(1, 3, 1, 1)
    out = torch.zeros((n, h, w, 8), dtype=dtype)
    out[..., :3] = v.permute(0, 2, 3, 1).to(dtype)
    return out


def spy_operand_ref(ref, warped, up):
    """[ref RGB | warped RGB | flow cast to the images' dtype]: the level's network input, (..., 8)."""
    return torch.cat([ref[..., :3], warped[..., :3], up.to(ref.dtype)], -1)


def spy_operand_bwd_ref(dx8):
    """-> (d warped (..., 8): channels 3..5 of dx8 in front of five +0, d flow (..., 2) fp32: channels 6, 7)."""
    return torch.cat([dx8[..., 3:6], torch.zeros_like(dx8[..., :5])], -1), dx8[..., 6:8].to(F32)


def spy_flow_add_ref(up, res):
    return up + res.to(F32)


# ================================================================================================ bilinear x2, align_corners=True
def ac_weights(n_in, n_out, coord=np.float32):
    """The (n_out, n_in) interpolation matrix of one axis, fp64.  The source coordinate is computed as torch does for tensors of type `coord`
    (UpSample.h: area_pixel_compute_scale / guard_index_and_lambda): ratio = coord(n_in - 1) / coord(n_out - 1), s = ratio * dst in `coord`,
    i0 = int(s) clamped to the last index, i1 = i0 + 1 where that exists, l1 = s - i0 (exact).  coord = float32 is what a float tensor gets --
    the index choice is then the kernel's, and only rounding is left to bound; coord = float64 is what F.interpolate does on a double tensor."""
    ratio = coord(n_in - 1) / coord(n_out - 1) if n_out > 1 else coord(0)
    dst = np.arange(n_out)
    s = (ratio * dst.astype(coord)).astype(coord)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s.astype(np.float64) - i0
    W = np.zeros((n_out, n_in), dtype=np.float64)
    np.add.at(W, (dst, i0), 1.0 - l1)
    np.add.at(W, (dst, i1), l1)
    return torch.from_numpy(W)


def _apply(Wy, Wx, x, scale):
    """scale * (Wy along axis 1, Wx along axis 2) of x (n, a, b, c) in fp64, and the same with absolute values."""
    s = np.float64(np.float32(scale))
    two = lambda wy, wx, v: torch.einsum("xb,nybc->nyxc", wx, torch.einsum("ya,nabc->nybc", wy, v))  # one axis after the other
    return s * two(Wy, Wx, x.double()), abs(s) * two(Wy.abs(), Wx.abs(), x.double().abs())


def upsample2x_ac_ref(x, scale, coord=np.float32):
    """scale * F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True) on channels-last (n, h, w, c) -> (n, 2h, 2w, c), fp64.
    -> (value, S) with S = |scale| * sum_i |w_i| |x_i| over the (up to four) taps of each output."""
    n, h, w, c = x.shape
    return _apply(ac_weights(h, 2 * h, coord), ac_weights(w, 2 * w, coord), x, scale)


def upsample2x_ac_adjoint_ref(g, scale, coord=np.float32):
    """The transpose of upsample2x_ac_ref: (n, 2h, 2w, c) -> (n, h, w, c), by transposing the SAME two matrices.  -> (value, S)."""
    n, h2, w2, c = g.shape
    return _apply(ac_weights(h2 // 2, h2, coord).t(), ac_weights(w2 // 2, w2, coord).t(), g, scale)
