"""Tensor-level wrappers over the C-ABI (no autograd here; see functional.py).

Every function takes/returns torch device tensors in channels-last layout and enqueues on torch's current
stream.  Shapes are validated on the host before a kernel is launched.
"""
from __future__ import annotations

import collections
import ctypes
import os
import struct
from typing import Optional, Sequence, Tuple

import torch

from . import hip
from .hip import ConvDesc, HipError


def _intarr(v: Sequence[int]):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def cout_tiles_for(cout: int, dtype: torch.dtype = torch.bfloat16, ks: int = 3) -> int:
    """16-channel tiles per workgroup: 9 covers C = 144/288/576 exactly, 7 covers 112/224/448, 8 covers 128/256; otherwise
    the candidate with the least padding.  fp32 (the parity path) has twice the bytes per stage: at most 5 tiles."""
    t = (cout + 15) // 16
    if t <= 1:
        return 1
    if ks == 7:  # SPyNet's 7x7 convs (2 .. 64 output channels): 1, 2 or 4 tiles
        return 2 if t == 2 else 4
    if t <= 4:
        return 4
    best, waste = None, None
    for cand in ((5, 4) if dtype == torch.float32 else (9, 8, 7, 5)):
        w = (t + cand - 1) // cand * cand - t
        if waste is None or w < waste:
            best, waste = cand, w
    return best


class PackedConv:
    """Packed (device) weights of one convolution / linear for one direction (forward or data-gradient)."""

    __slots__ = ("buf", "dtype", "ks", "cout", "src_ch", "cout_tiles", "layout", "call")

    def __init__(self, buf, dtype, ks, cout, src_ch, cout_tiles, layout="std", call=None):
        self.buf, self.dtype, self.ks, self.cout, self.src_ch, self.cout_tiles = buf, dtype, ks, cout, list(src_ch), cout_tiles
        self.layout = layout  # 'std': vmg_conv_pack; 'ws': vmg_convws_pack (the weight-streaming 3x3 kernel, route hip.CONV_WS)
        self.call = call      # (weight data_ptr, O, I, o0, on, src_off, src_ch, transpose_flip): what a plan entry needs to redo this pack


def pack_conv_weight(w: torch.Tensor, dtype: torch.dtype, src_ch: Optional[Sequence[int]] = None,
                     src_off: Optional[Sequence[int]] = None, o0: int = 0, on: Optional[int] = None,
                     transpose_flip: bool = False, out: Optional[torch.Tensor] = None, cout_tiles: Optional[int] = None, groups: int = 1) -> PackedConv:
    """w: fp32 (O, I, KS, KS) or (O, I).  Forward pack: K slices = src_off/src_ch over I, outputs O[o0:o0+on).
    Data-gradient pack (transpose_flip): outputs I[o0:o0+on), K = O[src_off[0]:+src_ch[0]).
    groups > 1: w is the weight of a GROUPED convolution (I = channels per group); the pack is its dense block-diagonal operator over
    groups * I input channels, so that one launch serves all groups."""
    hip.require_cuda(w)
    if w.dtype != torch.float32 or not w.is_contiguous():
        raise HipError("pack_conv_weight expects a contiguous fp32 weight")
    if w.dim() == 2:
        O, I, ks = w.shape[0], w.shape[1], 1
    elif w.dim() == 4 and w.shape[2] == w.shape[3]:
        O, I, ks = w.shape[0], w.shape[1], w.shape[2]
    else:
        raise HipError(f"unsupported weight shape {tuple(w.shape)}")
    kdim, odim = (O, I * groups) if transpose_flip else (I * groups, O)
    if src_ch is None:
        src_ch, src_off = [kdim], [0]
    if src_off is None:
        src_off, acc = [], 0
        for c in src_ch:
            src_off.append(acc)
            acc += c
    if on is None:
        on = odim - o0
    tiles = cout_tiles if cout_tiles else cout_tiles_for(on, dtype, ks)
    flag = (1 if transpose_flip else 0) | ((groups << 8) if groups > 1 else 0)
    code = hip.dtype_code(dtype)
    l = hip.lib()
    nbytes = l.vmg_conv_pack_bytes(code, ks, on, len(src_ch), _intarr(src_ch), tiles)
    if nbytes <= 0:
        raise HipError(f"vmg_conv_pack_bytes rejected channels {list(src_ch)} (must be multiples of 8)")
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    elif out.numel() * out.element_size() < nbytes:
        raise HipError("pack buffer too small")
    hip.check(l.vmg_conv_pack(code, w.data_ptr(), O, I, ks, o0, on, len(src_ch), _intarr(src_off), _intarr(src_ch),
                              flag, tiles, out.data_ptr(), hip.stream_ptr()), "vmg_conv_pack")
    return PackedConv(out, dtype, ks, on, src_ch, tiles, call=(w.data_ptr(), O, I, o0, on, list(src_off), list(src_ch), flag))


WS_128_BLOCKS = os.environ.get("VMG_WS_128", "1") != "0"  # A/B switch of the 128-channel-block weight-streaming route


def ws_eligible(cout: int, ks: int, dtype: torch.dtype, src_ch: Sequence[int]) -> int:
    """cout_tiles (9, 7 or 8) if the weight-streaming kernel covers this conv (bf16, 3x3, output channels in blocks of 144, 112 or 128,
    source channel counts that split into blocks of <= 160 channels that are multiples of 16), else 0."""
    if dtype != torch.bfloat16 or ks != 3:
        return 0
    for c in src_ch:
        parts = 1
        while c // parts > 160 or c % (8 * parts):
            parts += 1
            if parts > c // 8:
                return 0
        if (c // parts) % 16:
            return 0
    if cout % 144 == 0:
        return 9
    if cout % 112 == 0:
        return 7
    if cout % 128 == 0 and WS_128_BLOCKS:
        return 8  # (round 4: `upconv2`, 144 -> 256 before the second PixelShuffle: 128-channel blocks)
    return 0


def pack_conv_weight_ws(w: torch.Tensor, src_ch: Optional[Sequence[int]] = None, src_off: Optional[Sequence[int]] = None, o0: int = 0,
                        on: Optional[int] = None, transpose_flip: bool = False, cout_tiles: int = 9, out: Optional[torch.Tensor] = None,
                        groups: int = 1) -> PackedConv:
    """bf16 pack of a 3x3 weight (O, I, 3, 3) for the weight-streaming kernel (same slicing conventions as pack_conv_weight).
    out: an existing pack buffer of this very pack to rewrite in place."""
    hip.require_cuda(w)
    if w.dtype != torch.float32 or not w.is_contiguous() or w.dim() != 4 or w.shape[2] != 3 or w.shape[3] != 3:
        raise HipError("pack_conv_weight_ws expects a contiguous fp32 (O, I, 3, 3) weight")
    O, I = w.shape[0], w.shape[1]
    kdim, odim = (O, I * groups) if transpose_flip else (I * groups, O)
    if src_ch is None:
        src_ch, src_off = [kdim], [0]
    if src_off is None:
        src_off, acc = [], 0
        for c in src_ch:
            src_off.append(acc)
            acc += c
    if on is None:
        on = odim - o0
    flag = (1 if transpose_flip else 0) | ((groups << 8) if groups > 1 else 0)
    l = hip.lib()
    nbytes = l.vmg_convws_pack_bytes(on, len(src_ch), _intarr(src_ch), cout_tiles)
    if nbytes <= 0:
        raise HipError(f"vmg_convws_pack_bytes rejected channels {list(src_ch)} / cout_tiles {cout_tiles}")
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    elif out.numel() * out.element_size() < nbytes:
        raise HipError("pack buffer too small")
    hip.check(l.vmg_convws_pack(w.data_ptr(), O, I, o0, on, len(src_ch), _intarr(src_off), _intarr(src_ch), flag,
                                cout_tiles, out.data_ptr(), hip.stream_ptr()), "vmg_convws_pack")
    return PackedConv(out, torch.bfloat16, 3, on, src_ch, cout_tiles, layout="ws",
                      call=(w.data_ptr(), O, I, o0, on, list(src_off), list(src_ch), flag))


# vmg_conv_desc as one struct format (checked against the ctypes layout at import): field order of hip.ConvDesc
_CONV_FMT = struct.Struct("=8i4Q4q4iQQQqQQqQqiffiiii4x")
assert _CONV_FMT.size == ctypes.sizeof(ConvDesc), "vmg_conv_desc layout drifted from kernels._CONV_FMT"
_CONV_DESC = ConvDesc()  # reused: vmg_conv_fwd copies what it needs before it returns (single-threaded host side)
_CONV_PACK = _CONV_FMT.pack_into


def _pix_stride(t: torch.Tensor) -> int:
    """Pixel stride (elements) of a channels-last tensor whose leading dims are dense over pixels."""
    st = t.stride()
    if st[-1] != 1:
        raise HipError("channels must be the fastest dimension")
    if t.is_contiguous():  # the common case: one call instead of a size/stride pair per dimension
        return t.shape[-1]
    sh = t.shape
    ps = st[-2]
    # leading dims must be a dense pixel enumeration with that stride
    expect = ps
    for d in range(len(sh) - 2, -1, -1):
        if sh[d] != 1 and st[d] != expect:
            raise HipError(f"tensor of shape {tuple(sh)} / strides {st} is not a dense pixel array")
        expect *= sh[d]
    return ps


def _conv_fill(srcs, pw, bias, N, H, W, act, slope, alpha, res, aux, actgrad, pixel_shuffle, out, out_pre, want_pre, mt, deep):
    """Validates a conv_forward call and fills the shared descriptor; returns (descriptor, out, out_pre)."""
    if len(srcs) != len(pw.src_ch):
        raise HipError(f"conv expects {len(pw.src_ch)} sources, got {len(srcs)}")
    x0 = srcs[0]
    hip.require_cuda(*srcs, bias, res, aux, out)
    dt = x0.dtype
    if dt != pw.dtype:
        raise HipError(f"activation dtype {dt} != packed weight dtype {pw.dtype}")
    M = N * H * W
    nsrc = len(srcs)
    if (pw.layout == "ws") != (deep == hip.CONV_WS):
        deep = hip.CONV_WS if pw.layout == "ws" else hip.CONV_GENERAL  # the packed layout decides the kernel
    sp, sps, sch = [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]
    for i, s in enumerate(srcs):
        if s.dtype != dt or s.shape[-1] != pw.src_ch[i] or s.numel() // s.shape[-1] != M:
            raise HipError(f"source {i}: shape {tuple(s.shape)} / dtype {s.dtype} does not match conv (M={M}, C={pw.src_ch[i]}, {dt})")
        sp[i], sps[i], sch[i] = s.data_ptr(), _pix_stride(s), pw.src_ch[i]
    bias_p = 0
    if bias is not None:
        if bias.dtype != torch.float32 or bias.numel() != pw.cout or not bias.is_contiguous():
            raise HipError("bias must be contiguous fp32 of length Cout")
        bias_p = bias.data_ptr()
    if pixel_shuffle:
        oshape = (N, 2 * H, 2 * W, pw.cout // 4)
    else:
        oshape = (N, H, W, pw.cout)
    if out is None:
        out = torch.empty(oshape, dtype=dt, device=x0.device)
    elif out.dtype != dt or out.numel() // out.shape[-1] != (4 * M if pixel_shuffle else M) or out.shape[-1] != oshape[-1]:
        raise HipError(f"bad output tensor {tuple(out.shape)} for conv output {oshape}")
    out_ps = _pix_stride(out)
    if want_pre and out_pre is None:
        if pixel_shuffle:
            raise HipError("out_pre is not available with pixel_shuffle")
        out_pre = torch.empty(oshape, dtype=dt, device=x0.device)
    pre_p = 0
    if out_pre is not None:
        if _pix_stride(out_pre) != out_ps or out_pre.shape[-1] != pw.cout or out_pre.dtype != dt:
            raise HipError("out_pre must have the layout of out")
        pre_p = out_pre.data_ptr()
    extra = [0, 0, 0, 0]  # res, res_ps, aux, aux_ps
    for k, (name, t) in enumerate((("res", res), ("aux", aux))):
        if t is None:
            continue
        if pixel_shuffle:
            raise HipError(f"{name} is not supported together with pixel_shuffle")
        if t.dtype != dt or t.shape[-1] != pw.cout or t.numel() // t.shape[-1] != M:
            raise HipError(f"{name}: shape {tuple(t.shape)} does not match conv output")
        extra[2 * k], extra[2 * k + 1] = t.data_ptr(), _pix_stride(t)
    # the descriptor is filled with ONE struct.pack_into (30 ctypes attribute stores cost ~9 us per conv, 5 ms per train step)
    d = _CONV_DESC
    _CONV_PACK(d, 0, hip.dtype_code(dt), pw.ks, pw.cout_tiles, N, H, W, pw.cout, nsrc, sp[0], sp[1], sp[2], sp[3], sps[0], sps[1], sps[2], sps[3],
               sch[0], sch[1], sch[2], sch[3], pw.buf.data_ptr(), bias_p, out.data_ptr(), out_ps, pre_p, extra[0], extra[1], extra[2], extra[3],
               act, slope, alpha, actgrad, int(pixel_shuffle), mt, deep)
    return d, out, out_pre


def conv_forward(srcs: Sequence[torch.Tensor], pw: PackedConv, bias: Optional[torch.Tensor], N: int, H: int, W: int,
                 act: int = hip.ACT_NONE, slope: float = 0.0, alpha: float = 1.0, res: Optional[torch.Tensor] = None,
                 aux: Optional[torch.Tensor] = None, actgrad: int = 0, pixel_shuffle: bool = False,
                 out: Optional[torch.Tensor] = None, out_pre: Optional[torch.Tensor] = None, want_pre: bool = False,
                 mt: int = 0, deep: int = hip.CONV_GENERAL) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Runs vmg_conv_fwd.  srcs: channels-last tensors (..., C_s) covering N*H*W pixels each (channel slices of
    wider tensors are fine).  Returns (out, out_pre)."""
    d, out, out_pre = _conv_fill(srcs, pw, bias, N, H, W, act, slope, alpha, res, aux, actgrad, pixel_shuffle, out, out_pre, want_pre, mt, deep)
    hip.check(hip.lib().vmg_conv_fwd(ctypes.byref(d), hip.stream_ptr()), "vmg_conv_fwd")
    return out, out_pre


ConvPlan = collections.namedtuple("ConvPlan", "family dtype ks mt ntb variant vec8 grid_x grid_y tiles_per_wave lds_bytes")


def conv_forward_plan(srcs: Sequence[torch.Tensor], pw: PackedConv, bias: Optional[torch.Tensor], N: int, H: int, W: int,
                      act: int = hip.ACT_NONE, slope: float = 0.0, alpha: float = 1.0, res: Optional[torch.Tensor] = None,
                      aux: Optional[torch.Tensor] = None, actgrad: int = 0, pixel_shuffle: bool = False,
                      out: Optional[torch.Tensor] = None, out_pre: Optional[torch.Tensor] = None, want_pre: bool = False,
                      mt: int = 0, deep: int = hip.CONV_GENERAL, ncu: int = 0) -> ConvPlan:
    """What conv_forward would launch for the same arguments (vmg_conv_fwd_plan; nothing is enqueued): the kernel family
    (hip.CONV_FAM_*), its template arguments, the epilogue flavour, the grid and the LDS size.  ncu = 0: the current device's compute units."""
    d, _, _ = _conv_fill(srcs, pw, bias, N, H, W, act, slope, alpha, res, aux, actgrad, pixel_shuffle, out, out_pre, want_pre, mt, deep)
    plan = (ctypes.c_int * hip.CONV_PLAN_INTS)()
    hip.check(hip.lib().vmg_conv_fwd_plan(ctypes.byref(d), ncu, plan), "vmg_conv_fwd_plan")
    return ConvPlan(*plan)


def _parr(ts):
    return (ctypes.c_void_p * max(1, len(ts)))(*[(t.data_ptr() if t is not None else None) for t in ts])


CHAIN_STATS = {"fwd": {}, "bwd": {}}  # chain calls by the route (hip.CONV_*) their block convolutions took: read by tests


def resblock_chain_forward(srcs: Sequence[torch.Tensor], pw0: PackedConv, b0: torch.Tensor, slope0: float, deep0: int, pw1: Sequence[PackedConv],
                           b1: Sequence[torch.Tensor], pw2: Sequence[PackedConv], b2: Sequence[torch.Tensor], r_scaling: float, deep: int,
                           own_output: bool = False):
    """ResidualBlocksWithInputConv forward as ONE C call (vmg_resblock_chain_fwd).  Returns (ys, ts): nblk + 1 block outputs and nblk
    ReLU outputs, all (N, H, W, C)."""
    x0 = srcs[0]
    hip.require_cuda(*srcs, b0, *b1, *b2)
    N, H, W = x0.shape[0], x0.shape[1], x0.shape[2]
    M = N * H * W
    C, nblk, dt = pw0.cout, len(pw1), x0.dtype
    if len(srcs) != len(pw0.src_ch) or any(s.dtype != dt or s.shape[-1] != c or s.numel() // s.shape[-1] != M for s, c in zip(srcs, pw0.src_ch)):
        raise HipError("resblock_chain: sources do not match conv0's pack")
    if any(p.cout != C or p.src_ch != [C] or p.dtype != dt or p.layout != pw1[0].layout or p.cout_tiles != pw1[0].cout_tiles for p in list(pw1) + list(pw2)) or \
            pw0.dtype != dt or len(pw2) != nblk or len(b1) != nblk or len(b2) != nblk:
        raise HipError("resblock_chain: block packs must be C -> C packs of one layout")
    for b in [b0] + list(b1) + list(b2):
        if b.dtype != torch.float32 or b.numel() != C or not b.is_contiguous():
            raise HipError("resblock_chain: biases must be contiguous fp32 of length C")
    blk = torch.empty((2 * nblk + 1, N, H, W, C), dtype=dt, device=x0.device).unbind(0)  # ONE allocation: 31 torch.empty calls cost 0.1 ms of host time per chain
    ys, ts = list(blk[:nblk + 1]), list(blk[nblk + 1:])
    if own_output:  # the chain's output in its own allocation: the caller drops the intermediates (activation recompute)
        ys[-1] = torch.empty((N, H, W, C), dtype=dt, device=x0.device)
    d = hip.ChainDesc()
    d.dtype, d.N, d.H, d.W, d.C, d.nblk, d.nsrc = hip.dtype_code(dt), N, H, W, C, nblk, len(srcs)
    for i, s in enumerate(srcs):
        d.src[i], d.src_ps[i], d.src_ch[i] = s.data_ptr(), _pix_stride(s), pw0.src_ch[i]
    d.packed0, d.bias0, d.slope0 = pw0.buf.data_ptr(), b0.data_ptr(), slope0
    d.cout_tiles0, d.deep0 = pw0.cout_tiles, hip.CONV_WS if pw0.layout == "ws" else deep0
    keep = [_parr([p.buf for p in pw1]), _parr(list(b1)), _parr([p.buf for p in pw2]), _parr(list(b2)), _parr(ys), _parr(ts)]
    d.packed1, d.bias1, d.packed2, d.bias2, d.y, d.t = keep
    d.r_scaling = r_scaling
    d.cout_tiles = pw1[0].cout_tiles if nblk else pw0.cout_tiles
    d.deep = (hip.CONV_WS if pw1[0].layout == "ws" else deep) if nblk else hip.CONV_GENERAL
    hip.check(hip.lib().vmg_resblock_chain_fwd(ctypes.byref(d), hip.stream_ptr()), "vmg_resblock_chain_fwd")
    CHAIN_STATS["fwd"][d.deep] = CHAIN_STATS["fwd"].get(d.deep, 0) + 1
    return ys, ts


def resblock_chain_backward(g: torch.Tensor, ts: Sequence[torch.Tensor], pd1: Sequence[PackedConv], pd2: Sequence[PackedConv], r_scaling: float,
                            deep: int):
    """Data-gradient sweep of the residual blocks (vmg_resblock_chain_bwd).  g: gradient of the chain output; pd1 / pd2: data-gradient
    packs of conv1 / conv2 per block.  Returns (g_ys, g_ts): g_ys[k] = gradient of y_k (g_ys[nblk] is g), g_ts[k] of conv1_k's pre-activation."""
    hip.require_cuda(g, *ts)
    nblk = len(ts)
    N, H, W, C = g.shape
    g = g.contiguous()
    if nblk == 0:
        return [g], []
    blk = torch.empty((2 * nblk, N, H, W, C), dtype=g.dtype, device=g.device).unbind(0)
    gys, gts = list(blk[:nblk]) + [g], list(blk[nblk:])
    d = hip.ChainDesc()
    d.dtype, d.N, d.H, d.W, d.C, d.nblk, d.nsrc = hip.dtype_code(g.dtype), N, H, W, C, nblk, 1
    keep = [_parr([p.buf for p in pd1]), _parr([p.buf for p in pd2]), _parr(list(ts)), _parr(gys), _parr(gts)]
    d.packed1, d.packed2, d.t, d.g_y, d.g_t = keep
    d.r_scaling = r_scaling
    d.cout_tiles = pd1[0].cout_tiles
    d.deep = hip.CONV_WS if pd1[0].layout == "ws" else deep
    hip.check(hip.lib().vmg_resblock_chain_bwd(ctypes.byref(d), hip.stream_ptr()), "vmg_resblock_chain_bwd")
    CHAIN_STATS["bwd"][d.deep] = CHAIN_STATS["bwd"].get(d.deep, 0) + 1
    return gys, gts


def _wgrad_operands(name: str, xs, dys, dW: torch.Tensor, db: Optional[torch.Tensor], ks: int, M: int, o0: int = 0, i0: int = 0, like=None,
                    whole: bool = False):
    """The operand checks of conv_wgrad, conv_wgrad_batched and the multi wrappers, for one problem: fp32 contiguous gradients; every
    (x, dy) pair of one dtype, channel counts and pixel strides (those of the pair `like`, else of the first pair) over M pixels; dW / db
    matching (ks, Cout + o0, Cin + i0) -- whole: the call covers the whole parameter (3x3: all output channels).
    Returns (Cin, Cout, x_ps, dy_ps, I_total)."""
    hip.require_cuda(dW, db, *xs, *dys)
    if dW.dtype != torch.float32 or not dW.is_contiguous() or (db is not None and (db.dtype != torch.float32 or not db.is_contiguous())):
        raise HipError(f"{name}: parameter gradients must be contiguous fp32")
    x0, d0 = like or (xs[0], dys[0])
    Cin, Cout = x0.shape[-1], d0.shape[-1]
    xps, dps = _pix_stride(x0), _pix_stride(d0)
    for x, d in zip(xs, dys):
        if x.dtype != x0.dtype or d.dtype != x0.dtype or x.shape[-1] != Cin or d.shape[-1] != Cout or x.numel() // Cin != M or \
                d.numel() // Cout != M or _pix_stride(x) != xps or _pix_stride(d) != dps:
            raise HipError(f"{name}: all pairs must share dtype, shape and strides and cover the N*H*W pixels")
    O_total, I_total = dW.shape[0], dW.shape[1]
    kk = 1 if dW.dim() == 2 else dW.shape[2]
    fits = kk == ks and o0 + Cout <= O_total and i0 + Cin <= I_total and (db is None or db.numel() == O_total)
    if whole:  # (3x3: a group of a grouped convolution takes Cin of the weight's I_total input channels)
        fits = fits and O_total == Cout and (dW.dim() == 4 if ks == 3 else (I_total == Cin and dW.numel() == Cout * Cin))
    if not fits:
        raise HipError(f"{name}: gradient tensor {tuple(dW.shape)} does not match conv (ks={ks}, Cout={Cout}+{o0}, Cin={Cin}+{i0})")
    return Cin, Cout, xps, dps, I_total


def conv_wgrad(x: torch.Tensor, dy: torch.Tensor, dW: torch.Tensor, db: Optional[torch.Tensor], ks: int, N: int, H: int,
               W: int, scale: float = 1.0, o0: int = 0, i0: int = 0):
    """dW (fp32, (O_total, I_total, ks, ks) or (O_total, I_total)) += scale * wgrad(x, dy); db += scale * sum(dy).
    x (..., Cin) and dy (..., Cout) are channels-last tensors over the same N*H*W pixels (channel slices allowed)."""
    Cin, Cout, xps, dps, I_total = _wgrad_operands("conv_wgrad", [x], [dy], dW, db, ks, N * H * W, o0, i0)
    hip.check(hip.lib().vmg_conv_wgrad(hip.dtype_code(x.dtype), ks, N, H, W, x.data_ptr(), xps, Cin, dy.data_ptr(), dps, Cout, dW.data_ptr(), I_total, o0, i0,
                                       db.data_ptr() if db is not None else None, scale, hip.stream_ptr()), "vmg_conv_wgrad")


def act_backward(dy: torch.Tensor, ref: torch.Tensor, act: int, slope: float, alpha: float) -> torch.Tensor:
    """dy * alpha * act'(ref); ref = activation output (RELU/LRELU) or pre-activation (GELU)."""
    hip.require_cuda(dy, ref)
    if dy.shape != ref.shape or dy.dtype != ref.dtype or not dy.is_contiguous() or not ref.is_contiguous():
        raise HipError("act_backward: dy / ref must be contiguous tensors of one shape and dtype")
    out = torch.empty_like(dy)
    hip.check(hip.lib().vmg_act_bwd(hip.dtype_code(dy.dtype), dy.data_ptr(), ref.data_ptr(), out.data_ptr(), dy.numel(), act, slope,
                                    alpha, hip.stream_ptr()), "vmg_act_bwd")
    return out


def pixel_shuffle(x: torch.Tensor, N: int, H: int, W: int) -> torch.Tensor:
    """(N,H,W,4c) -> (N,2H,2W,c), torch PixelShuffle(2) order."""
    hip.require_cuda(x)
    c4 = x.shape[-1]
    if c4 % 4 or x.numel() != N * H * W * c4 or not x.is_contiguous():
        raise HipError("pixel_shuffle: bad input")
    out = torch.empty((N, 2 * H, 2 * W, c4 // 4), dtype=x.dtype, device=x.device)
    hip.check(hip.lib().vmg_pixel_shuffle(hip.dtype_code(x.dtype), x.data_ptr(), out.data_ptr(), N, H, W, c4 // 4, 0, hip.stream_ptr()),
              "vmg_pixel_shuffle")
    return out


def frame_gather(src: torch.Tensor, idx: torch.Tensor, n_dst: int, frame_shape) -> torch.Tensor:
    """dst frame f = sum_k src frame idx[f, k] (vmg_frame_gather): src contiguous, its leading dims flattened into frames of prod(frame_shape)
    elements; idx (n_dst, 1 or 2) int32 on the device.  Two columns: an entry < 0 = no term (both < 0: a frame of +0).  One column: a plain
    copy, every entry must be >= 0.  Every entry < number of source frames.  The table is device data, so neither bound is checked here or in
    vmg_frame_gather (it would cost a synchronisation): both are the CALLER's responsibility, and an entry outside them reads out of bounds.
    Returns (n_dst, *frame_shape)."""
    hip.require_cuda(src, idx)
    fe = 1
    for d in frame_shape:
        fe *= int(d)
    if not src.is_contiguous() or src.numel() % fe or idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != n_dst or idx.shape[1] not in (1, 2) or not idx.is_contiguous():
        raise HipError("frame_gather: contiguous src of whole frames and a contiguous int32 (n_dst, 1|2) index table expected")
    dst = torch.empty((n_dst, *frame_shape), dtype=src.dtype, device=src.device)
    hip.check(hip.lib().vmg_frame_gather(hip.dtype_code(src.dtype), src.data_ptr(), dst.data_ptr(), idx.data_ptr(), fe, src.numel() // fe, n_dst, idx.shape[1],
                                         hip.stream_ptr()), "vmg_frame_gather")
    return dst


def sum_n(ts: Sequence[torch.Tensor]) -> torch.Tensor:
    """Sum of 2..4 contiguous tensors of one shape and dtype (bf16 / fp32), fp32 sum, one rounding (vmg_sum_n)."""
    hip.require_cuda(*ts)
    t0 = ts[0]
    vn = 8 if t0.dtype == torch.bfloat16 else 4
    if not 2 <= len(ts) <= 4 or t0.numel() % vn or any(t.shape != t0.shape or t.dtype != t0.dtype or not t.is_contiguous() for t in ts):
        raise HipError("sum_n: 2..4 contiguous tensors of one shape and dtype, whole 16-byte vectors")
    out = torch.empty_like(t0)
    ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    hip.check(hip.lib().vmg_sum_n(hip.dtype_code(t0.dtype), ptrs, len(ts), out.data_ptr(), t0.numel(), hip.stream_ptr()), "vmg_sum_n")
    return out


class DecayList:
    """A list of (weight, Gamma) pairs for vmg_decay_weights with its pointer tables kept between calls: the per-call decay runs at the top of
    every forward, and 48 tensors' worth of argument checks and ctypes conversions there is host time of a host-bound step.  The tables are
    rebuilt (and the tensors checked again) whenever a data pointer has moved (module.to(), an optimizer that re-lays its parameters)."""

    def __init__(self, weights: Sequence[torch.Tensor], gammas: Sequence[torch.Tensor]):
        if not weights or len(weights) != len(gammas):
            raise HipError("decay_weights: two non-empty lists of equal length expected")
        self.weights, self.tensors, self.ptrs, self.args = list(weights), list(weights) + list(gammas), None, None

    def _tables(self, ptrs):
        cnt = len(self.weights)
        hip.require_cuda(*self.tensors)
        for w, g in zip(self.weights, self.tensors[cnt:]):
            if w.dtype != torch.float32 or g.dtype != torch.float32 or w.numel() != g.numel() or w.numel() == 0 or not w.is_contiguous() or not g.is_contiguous():
                raise HipError("decay_weights: dense fp32 weights and Gammas of the same non-zero element counts expected")
        self.args = ((ctypes.c_void_p * cnt)(*ptrs[:cnt]), (ctypes.c_void_p * cnt)(*ptrs[cnt:]), (ctypes.c_int64 * cnt)(*[w.numel() for w in self.weights]), cnt)
        self.ptrs = ptrs

    def run(self, n: int = 1) -> None:
        n = int(n)
        if n < 1:
            raise HipError("decay_weights: n >= 1 expected")
        ptrs = [t.data_ptr() for t in self.tensors]
        if ptrs != self.ptrs:
            self._tables(ptrs)
        hip.check(hip.lib().vmg_decay_weights(*self.args, n, hip.stream_ptr()), "vmg_decay_weights")
        torch.autograd.graph.increment_version(self.weights)


def decay_weights(weights: Sequence[torch.Tensor], gammas: Sequence[torch.Tensor], n: int = 1) -> None:
    """weights[i] <- weights[i] * gammas[i], n times, in place (vmg_decay_weights: each element multiplied n times in a register, the bits of
    n separate `mul_`).  Dense fp32 tensors of pairwise equal element counts; the list may be of any length.  The weights' autograd version
    counters move like after an in-place torch op (the pack cache keys on them)."""
    DecayList(weights, gammas).run(n)


class _AccPool:
    """fp32 scatter accumulators at rest are ZERO (cast_clear leaves them so): a buffer is taken for one scatter, rounded + cleared, given back -- no fill pass per
    use.  A buffer that is not given back (an exception in between) is simply dropped.  One stream: every user runs on the current stream, in order."""

    def __init__(self):
        self.free = {}

    def take(self, shape, device) -> torch.Tensor:
        lst = self.free.get((tuple(shape), str(device)))
        return lst.pop() if lst else torch.zeros(tuple(shape), dtype=torch.float32, device=device)

    def give(self, buf: torch.Tensor) -> None:
        # (never dropped on its own: a captured hipGraph has the addresses of the buffers it used baked into its kernel nodes -- the same reason
        #  PackPlan retires its tables instead of freeing them; clear() is the caller's explicit decision)
        self.free.setdefault((tuple(buf.shape), str(buf.device)), []).append(buf)

    def clear(self) -> None:
        self.free.clear()


ACC_POOL = _AccPool()


def cast_clear(acc: torch.Tensor, dtype: torch.dtype, add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(acc [+ add]) rounded to `dtype` once; acc (contiguous fp32) is ZERO afterwards (vmg_cast_clear)."""
    hip.require_cuda(acc, add)
    if acc.dtype != torch.float32 or not acc.is_contiguous() or acc.numel() % 4 or (add is not None and (add.dtype != dtype or add.shape != acc.shape or not add.is_contiguous())):
        raise HipError("cast_clear: contiguous fp32 accumulator (a multiple of 4 elements); `add` of the output dtype and the same shape")
    out = torch.empty(acc.shape, dtype=dtype, device=acc.device)
    hip.check(hip.lib().vmg_cast_clear(hip.dtype_code(dtype), acc.data_ptr(), add.data_ptr() if add is not None else None, out.data_ptr(), acc.numel(), hip.stream_ptr()),
              "vmg_cast_clear")
    return out


def pair_steps(mode: int, steps: Sequence[torch.Tensor], a: torch.Tensor, b: Optional[torch.Tensor], n: int, t: int) -> None:
    """vmg_pair_steps: the t step tensors of the lock-step recurrence ((2n, *frame) each, separate allocations) <-> a, b = the two sweeps' features
    (n, t, *frame) in frame order.  mode 0: steps -> a, b; mode 1: a, b -> steps; mode 2: a[i, f] = steps[t-1-f][i] + steps[f][n+i] (b unused)."""
    hip.require_cuda(a, b, *steps)
    if len(steps) != t or t < 1 or a.shape[0] != n or a.shape[1] != t or not a.is_contiguous():
        raise HipError("pair_steps: t step tensors and a contiguous (n, t, ...) tensor expected")
    fe = a.numel() // (n * t)
    for st in steps:
        if st.dtype != a.dtype or st.numel() != 2 * n * fe or not st.is_contiguous():
            raise HipError("pair_steps: every step tensor must be contiguous (2n, *frame) of the same dtype")
    if mode != 2 and (b is None or b.shape != a.shape or b.dtype != a.dtype or not b.is_contiguous()):
        raise HipError("pair_steps: the second (n, t, ...) tensor must match the first")
    ptrs = (ctypes.c_void_p * t)(*[st.data_ptr() for st in steps])
    hip.check(hip.lib().vmg_pair_steps(hip.dtype_code(a.dtype), mode, ptrs, a.data_ptr(), b.data_ptr() if b is not None else None, n, t, fe, hip.stream_ptr()),
              "vmg_pair_steps")


def pixel_unshuffle_actgrad(dy: torch.Tensor, ref: Optional[torch.Tensor], N: int, H: int, W: int, act: int, slope: float, alpha: float) -> torch.Tensor:
    """(N,2H,2W,c) gradient (and activation reference) -> (N,H,W,4c) pre-activation gradient of a PixelShuffle conv, one pass."""
    hip.require_cuda(dy, ref)
    c = dy.shape[-1]
    if dy.numel() != 4 * N * H * W * c or not dy.is_contiguous() or (ref is not None and (ref.shape != dy.shape or ref.dtype != dy.dtype or not ref.is_contiguous())):
        raise HipError("pixel_unshuffle_actgrad: bad input")
    out = torch.empty((N, H, W, 4 * c), dtype=dy.dtype, device=dy.device)
    hip.check(hip.lib().vmg_pixel_unshuffle_actgrad(hip.dtype_code(dy.dtype), dy.data_ptr(), ref.data_ptr() if ref is not None else None, out.data_ptr(),
                                                    N, H, W, c, act if ref is not None else hip.ACT_NONE, slope, alpha, hip.stream_ptr()),
              "vmg_pixel_unshuffle_actgrad")
    return out


def pixel_unshuffle(x: torch.Tensor, N: int, H: int, W: int) -> torch.Tensor:
    """(N,2H,2W,c) -> (N,H,W,4c): inverse of pixel_shuffle."""
    hip.require_cuda(x)
    c = x.shape[-1]
    if x.numel() != N * 4 * H * W * c or not x.is_contiguous():
        raise HipError("pixel_unshuffle: bad input")
    out = torch.empty((N, H, W, 4 * c), dtype=x.dtype, device=x.device)
    hip.check(hip.lib().vmg_pixel_shuffle(hip.dtype_code(x.dtype), x.data_ptr(), out.data_ptr(), N, H, W, c, 1, hip.stream_ptr()),
              "vmg_pixel_shuffle")
    return out


def layernorm_forward(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float = 1e-5, want_stats: bool = True):
    hip.require_cuda(x, w, b)
    C = x.shape[-1]
    if not x.is_contiguous() or w.dtype != torch.float32 or b.dtype != torch.float32 or w.numel() != C or b.numel() != C:
        raise HipError("layernorm: x must be contiguous, w/b fp32 of length C")
    M = x.numel() // C
    y = torch.empty_like(x)
    mean = torch.empty(M, dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty(M, dtype=torch.float32, device=x.device) if want_stats else None
    hip.check(hip.lib().vmg_layernorm_fwd(hip.dtype_code(x.dtype), x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(),
                                          mean.data_ptr() if want_stats else None, rstd.data_ptr() if want_stats else None,
                                          M, C, eps, hip.stream_ptr()), "vmg_layernorm_fwd")
    return y, mean, rstd


def _grad_pair(C: int, device, into):
    """(dw, db) accumulators of a LayerNorm backward: fresh zeros, or the caller's fp32 buffers (param.grad) to add into."""
    if into is None:
        return torch.zeros(C, dtype=torch.float32, device=device), torch.zeros(C, dtype=torch.float32, device=device)
    dw, db = into
    for t in (dw, db):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != C or not t.is_cuda:
            raise HipError("LayerNorm gradient buffers must be contiguous fp32 (C,) on the GPU")
    return dw, db


def layernorm_backward(dys, x: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, w: torch.Tensor, into=None, add=None):
    """dys: one gradient, or a list of up to five gradients of the LayerNorm output that the kernel sums on the way in.
    into = (dw, db): the kernel's atomic sums are ADDED to these buffers (param.grad) instead of to fresh zero tensors.
    add: a gradient of x's shape that is summed into dx by the kernel (the skip-connection gradient)."""
    dys = [d.contiguous() for d in dys] if isinstance(dys, (list, tuple)) else [dys.contiguous()]
    hip.require_cuda(x, mean, rstd, w, add, *dys)
    if not 1 <= len(dys) <= 5:
        raise HipError("layernorm_backward: 1..5 output gradients expected")
    for t in dys if add is None else (*dys, add):
        if t.shape != x.shape or t.dtype != x.dtype:
            raise HipError("layernorm_backward: the output gradients and add must have x's shape and dtype")
    if add is not None:
        add = add.contiguous()
    C = x.shape[-1]
    dx = torch.empty_like(x)
    dw, db = _grad_pair(C, x.device, into)
    ws = _layernorm_workspace(x.device)
    hip.check(hip.lib().vmg_layernorm_bwd(hip.dtype_code(x.dtype), len(dys), _ptrs(dys), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), w.data_ptr(),
                                          add.data_ptr() if add is not None else None, dx.data_ptr(), dw.data_ptr(), db.data_ptr(), x.numel() // C, C,
                                          ws.data_ptr() if ws is not None else None, hip.stream_ptr()), "vmg_layernorm_bwd")
    return dx, dw, db


_WS = {}


def _workspace(size_entry: str, device, zero: bool = False) -> torch.Tensor:
    """A kernel family's scratch buffer of lib.<size_entry>() bytes: allocated once per device on first use and kept (the calls that share
    one are stream-ordered on the device's compute stream)."""
    ws = _WS.get((size_entry, device))
    if ws is None:
        nbytes = int(getattr(hip.lib(), size_entry)())
        ws = _WS[size_entry, device] = (torch.zeros if zero else torch.empty)(nbytes, dtype=torch.uint8, device=device)
    return ws


def _layernorm_workspace(device) -> Optional[torch.Tensor]:
    """The zeroed workspace of the LayerNorm backward (the kernel leaves it zero), or None -- the kernel's plain-atomic tail -- while it does
    not exist and the stream is capturing: it must not come from a graph's private pool, and a captured step's warm-up creates it anyway."""
    ws = _WS.get(("vmg_layernorm_bwd_ws_bytes", device))
    if ws is None and not torch.cuda.is_current_stream_capturing():
        ws = _workspace("vmg_layernorm_bwd_ws_bytes", device, zero=True)
    return ws


MORPH_FUSED_CP = (144, 112, 64, 32, 16)


def morph_fused_ok(x: torch.Tensor, chunk: int, Cp: int) -> bool:
    """Shapes the fused MorphFC kernel (vmg_morphfc_fwd) covers: bf16, chunk 8 or 16, Cp instantiated, C a multiple of 8."""
    return x.dtype == torch.bfloat16 and chunk in (8, 16) and Cp in MORPH_FUSED_CP and x.shape[-1] % 8 == 0 and Cp % chunk == 0


MorphfcPlan = collections.namedtuple("MorphfcPlan", "NK NCT EVEN MASK ngroups ntiles nwg lds_bytes")


def morphfc_plan(axis: str, chunk: int, BT: int, H: int, W: int, C: int, Cp: int, has_mask: bool = False, ncu: int = 0) -> MorphfcPlan:
    """What morphfc_forward launches for the geometry (vmg_morphfc_plan, the function the entry point dispatches through; nothing is enqueued):
    the morph_linear_kernel<NK, NCT, EVEN, MASK> instance, groups, 16-token tiles, workgroups and LDS bytes.  ncu = 0: the current device's
    compute units.  Raises HipError with the entry point's message for what the kernel does not serve."""
    if ncu <= 0:
        ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    plan = (ctypes.c_int * hip.MORPHFC_PLAN_INTS)()
    hip.check(hip.lib().vmg_morphfc_plan(0 if axis == "h" else 1, chunk, BT, H, W, C, Cp, 1 if has_mask else 0, ncu, plan), "vmg_morphfc_plan")
    p = MorphfcPlan(*plan)
    return p._replace(EVEN=bool(p.EVEN), MASK=bool(p.MASK))


def morph_tokens_route(dtype: torch.dtype, chunk: int, C: int, ld: int, aligned: bool = True) -> int:
    """The kernel morph_tokens_gather / _scatter run (vmg_morph_tokens_route, which both dispatch through): hip.MORPH_ROUTE_LDS or
    hip.MORPH_ROUTE_ELEMENT.  aligned: both pointers are 16-byte aligned."""
    r = hip.lib().vmg_morph_tokens_route(hip.dtype_code(dtype), chunk, C, ld, 1 if aligned else 0)
    if r < 0:
        hip.check(r, "vmg_morph_tokens_route")
    return r


def _given_out(out: torch.Tensor, like: torch.Tensor, shape, what: str) -> torch.Tensor:
    """A caller-owned output: contiguous, of the stated shape, dtype and device of `like`."""
    hip.require_cuda(out)
    if tuple(out.shape) != tuple(shape) or out.dtype != like.dtype or out.device != like.device or not out.is_contiguous():
        raise HipError(f"{what}: contiguous {like.dtype} {tuple(shape)} on {like.device} expected, got {out.dtype} {tuple(out.shape)} strides {out.stride()}")
    return out


def morphfc_forward(x: torch.Tensor, axis: str, chunk: int, Cp: int, pw: PackedConv, bias: Optional[torch.Tensor], relu: bool, in_scale: float,
                    out_scale: float, mask: Optional[torch.Tensor] = None, want_tokens: bool = False, out: Optional[torch.Tensor] = None,
                    tok_out: Optional[torch.Tensor] = None):
    """x (B,T,H,W,C) contiguous bf16 -> the branch output in the same layout (vmg_morphfc_fwd); mask: the data-gradient form.  want_tokens:
    also returns the token matrix (rows, Cp) the GEMM multiplied (the weight gradient's operand), else None.  out / tok_out: caller-owned
    results (contiguous, x's shape / (vmg_morphfc_token_rows, Cp)); tok_out implies want_tokens."""
    hip.require_cuda(x, bias, mask)
    B, T, H, W, C = x.shape
    if not x.is_contiguous() or (mask is not None and (not mask.is_contiguous() or mask.shape != x.shape or mask.dtype != x.dtype)):
        raise HipError("morphfc: contiguous x (and mask of the same shape) expected")
    if pw.layout != "std" or pw.ks != 1 or pw.cout != Cp or pw.src_ch != [Cp] or pw.cout_tiles != (Cp + 15) // 16 or pw.dtype != torch.bfloat16:
        raise HipError("morphfc: the pack must be a (Cp, Cp) 1x1 pack with all output tiles in one block")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != Cp or not bias.is_contiguous()):
        raise HipError("morphfc: bias must be contiguous fp32 of length Cp")
    out = torch.empty_like(x) if out is None else _given_out(out, x, x.shape, "morphfc: out")
    ax = 0 if axis == "h" else 1
    tok = None
    if want_tokens or tok_out is not None:
        rows = hip.lib().vmg_morphfc_token_rows(ax, chunk, B * T, H, W)
        if rows <= 0:
            raise HipError("morphfc: bad token geometry")
        tok = torch.empty((rows, Cp), dtype=x.dtype, device=x.device) if tok_out is None else _given_out(tok_out, x, (rows, Cp), "morphfc: tok_out")
    hip.check(hip.lib().vmg_morphfc_fwd(ax, chunk, x.data_ptr(), mask.data_ptr() if mask is not None else None, pw.buf.data_ptr(),
                                        bias.data_ptr() if bias is not None else None, out.data_ptr(), tok.data_ptr() if tok is not None else None,
                                        B * T, H, W, C, Cp, pw.cout_tiles, 1 if relu else 0, in_scale, out_scale, hip.stream_ptr()), "vmg_morphfc_fwd")
    return out, tok


def morph_tokens_gather(x: torch.Tensor, axis: str, chunk: int, Cp: int, ld: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (B,T,H,W,C) contiguous -> the MorphFC token matrix (rows, ld) of the reference's pad + rearrange chain (vmg_morph_tokens_gather): row
    (group, k), feature p*S + s = x[position p of the group, channel k*S + s], zeros for padding positions / channels and for features >= Cp.
    out: a caller-owned contiguous (rows, ld) result."""
    hip.require_cuda(x)
    B, T, H, W, C = x.shape
    if not x.is_contiguous():
        raise HipError("morph_tokens_gather: contiguous (B,T,H,W,C) expected")
    ld = Cp if ld is None else ld
    ax = 0 if axis == "h" else 1
    rows = hip.lib().vmg_morph_token_rows(ax, chunk, B * T, H, W)
    tok = torch.empty((rows, ld), dtype=x.dtype, device=x.device) if out is None else _given_out(out, x, (rows, ld), "morph_tokens_gather: out")
    hip.check(hip.lib().vmg_morph_tokens_gather(hip.dtype_code(x.dtype), ax, chunk, x.data_ptr(), tok.data_ptr(), B * T, H, W, C, Cp, ld, hip.stream_ptr()),
              "vmg_morph_tokens_gather")
    return tok


def morph_tokens_scatter(tok: torch.Tensor, axis: str, chunk: int, Cp: int, shape, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The inverse layout + crop: tok (rows, ld >= Cp), row stride ld -> (B,T,H,W,C) (vmg_morph_tokens_scatter).  out: a caller-owned
    contiguous (B,T,H,W,C) result."""
    hip.require_cuda(tok)
    B, T, H, W, C = shape
    ax = 0 if axis == "h" else 1
    rows = hip.lib().vmg_morph_token_rows(ax, chunk, B * T, H, W)
    if tok.dim() != 2 or tok.shape[0] != rows or tok.shape[1] < Cp or tok.stride(1) != 1:
        raise HipError(f"morph_tokens_scatter: token matrix ({rows}, >= {Cp}) expected, got {tuple(tok.shape)}")
    out = torch.empty((B, T, H, W, C), dtype=tok.dtype, device=tok.device) if out is None else _given_out(out, tok, (B, T, H, W, C), "morph_tokens_scatter: out")
    hip.check(hip.lib().vmg_morph_tokens_scatter(hip.dtype_code(tok.dtype), ax, chunk, tok.data_ptr(), out.data_ptr(), B * T, H, W, C, Cp, tok.stride(0),
                                                 hip.stream_ptr()), "vmg_morph_tokens_scatter")
    return out


def _win3d_geom(q, kv, table, heads, wt):
    B, D, H, W, C = q.shape
    if tuple(kv.shape) != (B, D, H, W, 2 * C) or kv.dtype != q.dtype or not q.is_contiguous() or not kv.is_contiguous():
        raise HipError("win3d_attn: contiguous q (B,D,H,W,C) and kv (B,D,H,W,2C) of one dtype expected")
    if table.dtype != torch.float32 or not table.is_contiguous() or tuple(table.shape) != ((2 * wt - 1) * 225, heads):
        raise HipError(f"win3d_attn: the bias table must be contiguous fp32 ((2*{wt}-1)*225, {heads})")
    nwin = B * ((D + wt - 1) // wt) * ((H + 7) // 8) * ((W + 7) // 8)
    return B, D, H, W, C, nwin


def win3d_attn_forward(q, kv, bq, bkv, table, heads: int, wt: int, shift):
    hip.require_cuda(q, kv, bq, bkv, table)
    B, D, H, W, C, nwin = _win3d_geom(q, kv, table, heads, wt)
    out = torch.empty_like(q)
    lse = torch.empty((nwin, heads, wt * 64), dtype=torch.float32, device=q.device)
    pz = lambda t: t.data_ptr() if t is not None else None
    hip.check(hip.lib().vmg_win3d_attn_fwd(hip.dtype_code(q.dtype), q.data_ptr(), kv.data_ptr(), pz(bq), pz(bkv), table.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                           B, D, H, W, C, heads, wt, shift[0], shift[1], shift[2], hip.stream_ptr()), "vmg_win3d_attn_fwd")
    return out, lse


def win3d_attn_backward(q, kv, bq, bkv, table, out, lse, dout, heads: int, wt: int, shift, into=None):
    """into = (dbq, dbkv): existing contiguous fp32 buffers (the biases' .grad) the kernel ADDS its bias gradients to, instead of fresh zeros."""
    B, D, H, W, C, nwin = _win3d_geom(q, kv, table, heads, wt)
    dout = dout.contiguous()
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    dtable = torch.zeros_like(table)
    if into is not None:
        dbq, dbkv = into
        hip.require_cuda(dbq, dbkv)
        if dbq.dtype != torch.float32 or dbkv.dtype != torch.float32 or dbq.numel() != C or dbkv.numel() != 2 * C or not dbq.is_contiguous() or not dbkv.is_contiguous():
            raise HipError("win3d_attn_backward: bias gradient buffers must be contiguous fp32 of C and 2C elements")
    else:
        dbq = torch.zeros(C, dtype=torch.float32, device=q.device) if bq is not None else None
        dbkv = torch.zeros(2 * C, dtype=torch.float32, device=q.device) if bkv is not None else None
    pz = lambda t: t.data_ptr() if t is not None else None
    # per-workgroup table gradients + an ordered reduce launch instead of float atomics from every window onto the same table (kernel doc)
    ws = torch.empty(int(hip.lib().vmg_win3d_attn_bwd_ws_bytes(B, D, H, W, heads, wt)), dtype=torch.uint8, device=q.device)
    hip.check(hip.lib().vmg_win3d_attn_bwd(hip.dtype_code(q.dtype), q.data_ptr(), kv.data_ptr(), pz(bq), pz(bkv), table.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                           dout.data_ptr(), dq.data_ptr(), dkv.data_ptr(), dtable.data_ptr(), pz(dbq), pz(dbkv), ws.data_ptr(), B, D, H, W, C, heads, wt,
                                           shift[0], shift[1], shift[2], hip.stream_ptr()), "vmg_win3d_attn_bwd")
    return dq, dkv, dtable, dbq, dbkv


def maxpool_forward(x: torch.Tensor, f: int):
    """Non-overlapping f x f max pooling of a contiguous channels-last (n,h,w,c) tensor -> (y, idx)."""
    hip.require_cuda(x)
    n, h, w, c = x.shape
    if not x.is_contiguous() or h % f or w % f:
        raise HipError("maxpool: contiguous (n,h,w,c) with h, w multiples of the window expected")
    y = torch.empty((n, h // f, w // f, c), dtype=x.dtype, device=x.device)
    idx = torch.empty((n, h // f, w // f, c), dtype=torch.uint8, device=x.device)
    hip.check(hip.lib().vmg_maxpool_fwd(hip.dtype_code(x.dtype), x.data_ptr(), y.data_ptr(), idx.data_ptr(), n, h, w, c, f, hip.stream_ptr()), "vmg_maxpool_fwd")
    return y, idx


def maxpool_backward(dy: torch.Tensor, idx: torch.Tensor, f: int) -> torch.Tensor:
    hip.require_cuda(dy, idx)
    n, ho, wo, c = dy.shape
    dy = dy.contiguous()
    dx = torch.empty((n, ho * f, wo * f, c), dtype=dy.dtype, device=dy.device)
    hip.check(hip.lib().vmg_maxpool_bwd(hip.dtype_code(dy.dtype), dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), n, ho * f, wo * f, c, f, hip.stream_ptr()),
              "vmg_maxpool_bwd")
    return dx


def avgpool2(x: torch.Tensor) -> torch.Tensor:
    """F.avg_pool2d(x, 2, 2) on a contiguous channels-last (n, h, w, c) tensor."""
    hip.require_cuda(x)
    n, h, w, c = x.shape
    if not x.is_contiguous() or h < 2 or w < 2:
        raise HipError("avgpool2: contiguous (n,h,w,c) with h, w >= 2 expected")
    y = torch.empty((n, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
    hip.check(hip.lib().vmg_avgpool2_nhwc(hip.dtype_code(x.dtype), x.data_ptr(), y.data_ptr(), n, h, w, c, hip.stream_ptr()), "vmg_avgpool2_nhwc")
    return y


def spy_prep(img: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """img (n,3,h,w) fp32 contiguous -> (n,h,w,8) `dtype`: (img - mean) / std in channels 0..2, zeros behind (vmg_spy_prep)."""
    hip.require_cuda(img, mean, std)
    if img.dtype != torch.float32 or img.dim() != 4 or img.shape[1] != 3 or not img.is_contiguous() or mean.numel() != 3 or std.numel() != 3 or \
            mean.dtype != torch.float32 or std.dtype != torch.float32:
        raise HipError("spy_prep: contiguous fp32 (n,3,h,w) image and fp32 mean / std of 3 elements expected")
    n, _, h, w = img.shape
    out = torch.empty((n, h, w, 8), dtype=dtype, device=img.device)
    hip.check(hip.lib().vmg_spy_prep(hip.dtype_code(dtype), img.data_ptr(), mean.contiguous().data_ptr(), std.contiguous().data_ptr(), out.data_ptr(), n, h, w, hip.stream_ptr()),
              "vmg_spy_prep")
    return out


def spy_operand(ref: torch.Tensor, warped: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """[ref RGB | warped RGB | flow] (n,h,w,8) in ref's dtype from ref, warped (n,h,w,8: RGB in channels 0..2) and up (n,h,w,2) fp32 (vmg_spy_operand_fwd)."""
    hip.require_cuda(ref, warped, up)
    if ref.shape[-1] != 8 or warped.shape != ref.shape or warped.dtype != ref.dtype or up.dtype != torch.float32 or tuple(up.shape) != (*ref.shape[:-1], 2) or \
            not (ref.is_contiguous() and warped.is_contiguous() and up.is_contiguous()):
        raise HipError("spy_operand: contiguous (..., 8) images of one dtype and a contiguous fp32 (..., 2) flow expected")
    out = torch.empty_like(ref)
    hip.check(hip.lib().vmg_spy_operand_fwd(hip.dtype_code(ref.dtype), ref.data_ptr(), warped.data_ptr(), up.data_ptr(), out.data_ptr(), ref.numel() // 8,
                                            hip.stream_ptr()), "vmg_spy_operand_fwd")
    return out


def spy_operand_backward(dx8: torch.Tensor):
    """gradient of spy_operand's output -> (d warped (…, 8): channels 3..5 of dx8 in front of zeros, d up (…, 2) fp32: channels 6, 7)."""
    hip.require_cuda(dx8)
    if dx8.shape[-1] != 8 or not dx8.is_contiguous():
        raise HipError("spy_operand_backward: contiguous (..., 8) gradient expected")
    dwarped = torch.empty_like(dx8)
    dup = torch.empty((*dx8.shape[:-1], 2), dtype=torch.float32, device=dx8.device)
    hip.check(hip.lib().vmg_spy_operand_bwd(hip.dtype_code(dx8.dtype), dx8.data_ptr(), dwarped.data_ptr(), dup.data_ptr(), dx8.numel() // 8, hip.stream_ptr()),
              "vmg_spy_operand_bwd")
    return dwarped, dup


def spy_flow_add(up: torch.Tensor, res: torch.Tensor) -> torch.Tensor:
    """up (fp32) + res (any compute dtype) -> fp32, one pass (vmg_spy_flow_add)."""
    hip.require_cuda(up, res)
    if up.dtype != torch.float32 or up.shape != res.shape or not (up.is_contiguous() and res.is_contiguous()):
        raise HipError("spy_flow_add: contiguous tensors of one shape, the first fp32")
    out = torch.empty_like(up)
    hip.check(hip.lib().vmg_spy_flow_add(hip.dtype_code(res.dtype), up.data_ptr(), res.data_ptr(), out.data_ptr(), up.numel(), hip.stream_ptr()), "vmg_spy_flow_add")
    return out


SPY_CHANNELS = (8, 32, 64, 32, 16, 2)  # SPyNetBasicModule: conv i maps SPY_CHANNELS[i] -> SPY_CHANNELS[i + 1]
SPY_FUSED_MAX_PIXELS = 256           # vmg_spy_module_*: h * w <= 256 and the image with its 3-pixel border <= 484 pixels (one LDS tile)
SPY_FUSED_MAX_TILE = 484


def _spy_module_check(name: str, x: torch.Tensor, packs: Sequence[PackedConv], dgrad: bool):
    hip.require_cuda(x)
    if x.dtype != torch.bfloat16 or x.dim() != 4 or x.shape[-1] != 8 or not x.is_contiguous():
        raise HipError(f"{name}: contiguous bf16 (n, h, w, 8) operand expected, got {tuple(x.shape)} {x.dtype}")
    n, h, w, _ = x.shape
    if n < 1 or h * w > SPY_FUSED_MAX_PIXELS or (h + 6) * (w + 6) > SPY_FUSED_MAX_TILE:
        raise HipError(f"{name}: a {h} x {w} level does not fit one workgroup's LDS")
    if len(packs) != 5:
        raise HipError(f"{name}: five packs expected")
    for i, p in enumerate(packs):
        cin, cout = SPY_CHANNELS[i], SPY_CHANNELS[i + 1]
        k, o = ((cout + 7) // 8 * 8, cin) if dgrad else (cin, cout)
        if p.layout != "std" or p.ks != 7 or p.dtype != torch.bfloat16 or p.src_ch != [k] or p.cout != o or p.cout_tiles != cout_tiles_for(o, p.dtype, 7):
            raise HipError(f"{name}: pack {i} is not the 7x7 bf16 {'data-gradient ' if dgrad else ''}pack of a {cin} -> {cout} convolution")
    return n, h, w


def spy_module_forward(x8: torch.Tensor, packs: Sequence[PackedConv], biases: Sequence[torch.Tensor], keep: bool):
    """One SPyNetBasicModule on a coarse level in one launch (vmg_spy_module_fwd): x8 (n,h,w,8) bf16, forward packs and biases of conv0..conv4
    -> (residual (n,h,w,2), [y0..y3] when keep else None)."""
    n, h, w = _spy_module_check("spy_module_forward", x8, packs, False)
    hip.require_cuda(*biases)
    if len(biases) != 5 or any(b.dtype != torch.float32 or b.numel() != SPY_CHANNELS[i + 1] or not b.is_contiguous() for i, b in enumerate(biases)):
        raise HipError("spy_module_forward: five contiguous fp32 biases expected")
    out = torch.empty((n, h, w, 2), dtype=x8.dtype, device=x8.device)
    ys = [torch.empty((n, h, w, c), dtype=x8.dtype, device=x8.device) for c in SPY_CHANNELS[1:5]] if keep else None
    d = hip.SpyModuleDesc()
    d.N, d.H, d.W, d.x, d.out = n, h, w, x8.data_ptr(), out.data_ptr()
    for i in range(5):
        d.packed[i], d.bias[i] = packs[i].buf.data_ptr(), biases[i].data_ptr()
    if keep:
        for i in range(4):
            d.y[i] = ys[i].data_ptr()
    hip.check(hip.lib().vmg_spy_module_fwd(ctypes.byref(d), hip.stream_ptr()), "vmg_spy_module_fwd")
    return out, ys


def spy_module_backward(dpre4: torch.Tensor, packs: Sequence[PackedConv], ys: Sequence[torch.Tensor], want_dx: bool):
    """The data-gradient sweep of spy_module_forward in one launch (vmg_spy_module_bwd): dpre4 (n,h,w,8) bf16 = the residual's gradient zero-padded
    to 8 channels, data-gradient packs of conv0..conv4, ys as kept by the forward -> ([dpre0..dpre3], dx8 (n,h,w,8) or None)."""
    n, h, w = _spy_module_check("spy_module_backward", dpre4, packs, True)
    hip.require_cuda(*ys)
    if len(ys) != 4 or any(y.dtype != dpre4.dtype or tuple(y.shape) != (n, h, w, SPY_CHANNELS[i + 1]) or not y.is_contiguous() for i, y in enumerate(ys)):
        raise HipError("spy_module_backward: y0..y3 as written by spy_module_forward expected")
    dpre = [torch.empty_like(y) for y in ys]
    dx = torch.empty((n, h, w, 8), dtype=dpre4.dtype, device=dpre4.device) if want_dx else None
    d = hip.SpyModuleDesc()
    d.N, d.H, d.W, d.x = n, h, w, dpre4.data_ptr()
    d.out = dx.data_ptr() if want_dx else None
    for i in range(5):
        d.packed[i] = packs[i].buf.data_ptr()
    for i in range(4):
        d.y[i], d.dpre[i] = ys[i].data_ptr(), dpre[i].data_ptr()
    hip.check(hip.lib().vmg_spy_module_bwd(ctypes.byref(d), hip.stream_ptr()), "vmg_spy_module_bwd")
    return dpre, dx


def upsample2x_ac(x: torch.Tensor, scale: float, backward: bool = False) -> torch.Tensor:
    """forward: (n,h,w,c) fp32 -> scale * bilinear x2 (align_corners=True) (n,2h,2w,c); backward: the transpose on (n,2h,2w,c)."""
    hip.require_cuda(x)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 4:
        raise HipError("upsample2x_ac: contiguous fp32 (n,h,w,c) expected")
    n, h, w, c = x.shape
    if not backward:
        y = torch.empty((n, 2 * h, 2 * w, c), dtype=torch.float32, device=x.device)
        hip.check(hip.lib().vmg_upsample2x_ac_fwd(x.data_ptr(), y.data_ptr(), n, h, w, c, scale, hip.stream_ptr()), "vmg_upsample2x_ac_fwd")
        return y
    if h % 2 or w % 2:
        raise HipError("upsample2x_ac backward: even gradient size expected")
    dx = torch.empty((n, h // 2, w // 2, c), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().vmg_upsample2x_ac_bwd(x.data_ptr(), dx.data_ptr(), n, h // 2, w // 2, c, scale, hip.stream_ptr()), "vmg_upsample2x_ac_bwd")
    return dx


def space_depth_ln_forward(x: torch.Tensor, mode: str, w: torch.Tensor, b: torch.Tensor, eps: float = 1e-5):
    """UpdownkeepSampling's rearrangement + LayerNorm in one pass.  x: contiguous (N, Hin, Win, Cin); 'down' -> rows (N, Hin/2, Win/2, 4*Cin),
    'up' -> rows (N, 2*Hin, 2*Win, Cin/4).  Returns (y, mean, rstd)."""
    hip.require_cuda(x, w, b)
    N, Hi, Wi, Ci = x.shape
    if not x.is_contiguous() or w.dtype != torch.float32 or b.dtype != torch.float32:
        raise HipError("space_depth_ln: contiguous x, fp32 w / b expected")
    if mode == "down":
        if Hi % 2 or Wi % 2:
            raise HipError("space_depth_ln (down): even input size expected")
        H, W, cseg, C, m = Hi // 2, Wi // 2, Ci, 4 * Ci, 1
    else:
        if Ci % 4:
            raise HipError("space_depth_ln (up): channels must be a multiple of 4")
        H, W, cseg, C, m = 2 * Hi, 2 * Wi, Ci // 4, Ci // 4, 2
    if w.numel() != C or b.numel() != C:
        raise HipError("space_depth_ln: w / b must have the LayerNorm width")
    y = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
    mean = torch.empty(N * H * W, dtype=torch.float32, device=x.device)
    rstd = torch.empty(N * H * W, dtype=torch.float32, device=x.device)
    hip.check(hip.lib().vmg_space_depth_ln_fwd(hip.dtype_code(x.dtype), m, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                               rstd.data_ptr(), N, H, W, cseg, eps, hip.stream_ptr()), "vmg_space_depth_ln_fwd")
    return y, mean, rstd


def space_depth_ln_backward(dy: torch.Tensor, x: torch.Tensor, mode: str, mean: torch.Tensor, rstd: torch.Tensor, w: torch.Tensor, into=None):
    hip.require_cuda(dy, x, mean, rstd, w)
    N, Hi, Wi, Ci = x.shape
    if mode == "down":
        H, W, cseg, C, m = Hi // 2, Wi // 2, Ci, 4 * Ci, 1
    else:
        H, W, cseg, C, m = 2 * Hi, 2 * Wi, Ci // 4, Ci // 4, 2
    dy = dy.contiguous()
    dx = torch.empty_like(x)
    dw, db = _grad_pair(C, x.device, into)
    ws = _layernorm_workspace(x.device)
    hip.check(hip.lib().vmg_space_depth_ln_bwd(hip.dtype_code(x.dtype), m, dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), w.data_ptr(),
                                               dx.data_ptr(), dw.data_ptr(), db.data_ptr(), N, H, W, cseg, ws.data_ptr() if ws is not None else None,
                                               hip.stream_ptr()), "vmg_space_depth_ln_bwd")
    return dx, dw, db


def conv_wgrad_batched(xs: Sequence[torch.Tensor], dys: Sequence[torch.Tensor], dW: torch.Tensor, db: Optional[torch.Tensor], ks: int,
                       N: int, H: int, W: int, scale: float = 1.0, o0: int = 0, i0: int = 0):
    """dW += scale * sum_p wgrad(xs[p], dys[p]) in as few launches as possible (16 pairs per launch)."""
    if len(xs) != len(dys) or not xs:
        raise HipError("conv_wgrad_batched: need equally many x and dy tensors")
    Cin, Cout, xps, dps, I_total = _wgrad_operands("conv_wgrad_batched", xs, dys, dW, db, ks, N * H * W, o0, i0)
    code = hip.dtype_code(xs[0].dtype)
    l = hip.lib()
    ws = _workspace("vmg_conv_wgrad_ws_bytes", dW.device)
    for s in range(0, len(xs), 16):
        n = min(16, len(xs) - s)
        xa = (ctypes.c_void_p * n)(*[t.data_ptr() for t in xs[s:s + n]])
        da = (ctypes.c_void_p * n)(*[t.data_ptr() for t in dys[s:s + n]])
        hip.check(l.vmg_conv_wgrad_batched_ws(code, ks, n, xa, da, N, H, W, xps, Cin, dps, Cout, dW.data_ptr(), I_total, o0, i0,
                                              db.data_ptr() if db is not None else None, scale, ws.data_ptr(), ws.numel(),
                                              hip.stream_ptr()), "vmg_conv_wgrad_batched_ws")


def conv_wgrad3_multi_ok(x: torch.Tensor, dy: torch.Tensor, ks: int) -> bool:
    """Operands vmg_conv_wgrad3_multi (ks 3) / vmg_linear_wgrad2_multi (ks 1) take: bf16, 16-byte aligned, pixel strides multiples of 8
    channels; 3x3: strides no smaller than the channel counts rounded up to 8; 1x1: channel counts multiples of 8 and at least 2 048 pixels.
    (The conditions of vmg_conv_wgrad_plan for the multi entries, restated here: this runs per parameter on the autograd thread.)"""
    if ks not in (1, 3) or x.dtype != torch.bfloat16 or dy.dtype != torch.bfloat16 or x.data_ptr() % 16 or dy.data_ptr() % 16:
        return False
    try:
        strides = ((_pix_stride(x), x.shape[-1]), (_pix_stride(dy), dy.shape[-1]))
    except HipError:  # (not a dense pixel array: conv_wgrad_batched says so)
        return False
    if ks == 1:
        return all(ps % 8 == 0 and c % 8 == 0 for ps, c in strides) and x.numel() // x.shape[-1] >= 2048
    return all(ps % 8 == 0 and ps >= (c + 7) // 8 * 8 for ps, c in strides)


WGRAD_MULTI_PAIRS = 16  # (x, dy) pairs per problem that one launch of the multi entries sums (csrc/conv_wgrad.hip WG_MAX_PAIRS)


def _wgrad_multi(name: str, probs, dims: Sequence[int]):
    """The body of conv_wgrad3_multi (dims = N, H, W) and linear_wgrad2_multi (dims = M,): checks that the problems share one shape, then
    launches vmg_<name> on them, eight problems and WGRAD_MULTI_PAIRS pairs per launch: the gradients are added to, so a longer list of pairs (a
    weight of the recurrence has one pair per frame of the clip) is summed over several launches."""
    conv3 = len(dims) == 3
    M = dims[0] * dims[1] * dims[2] if conv3 else dims[0]
    xs0, dys0, dW0 = probs[0][:3]
    npairs = len(xs0)
    for xs, dys, dW, db, _ in probs:
        if len(xs) != npairs or len(dys) != npairs or dW.shape != dW0.shape or xs[0].dtype != torch.bfloat16:
            raise HipError(f"{name}: problems must share the shape; operands bf16")
        Cin, Cout, xps, dps, I_total = _wgrad_operands(name, xs, dys, dW, db, 3 if conv3 else 1, M, like=(xs0[0], dys0[0]), whole=True)
    entry = getattr(hip.lib(), "vmg_" + name)
    ws = _workspace("vmg_conv_wgrad_ws_bytes", dW0.device)
    for s in range(0, len(probs), 8):
        grp = probs[s:s + 8]
        n = len(grp)
        wa = (ctypes.c_void_p * n)(*[g[2].data_ptr() for g in grp])
        ba = (ctypes.c_void_p * n)(*[(g[3].data_ptr() if g[3] is not None else None) for g in grp])
        sa = (ctypes.c_float * n)(*[float(g[4]) for g in grp])
        for p0 in range(0, npairs, WGRAD_MULTI_PAIRS):
            p1 = min(npairs, p0 + WGRAD_MULTI_PAIRS)
            xa = (ctypes.c_void_p * (n * (p1 - p0)))(*[t.data_ptr() for g in grp for t in g[0][p0:p1]])
            da = (ctypes.c_void_p * (n * (p1 - p0)))(*[t.data_ptr() for g in grp for t in g[1][p0:p1]])
            hip.check(entry(n, p1 - p0, xa, da, *dims, xps, Cin, dps, Cout, wa, I_total, 0, 0, ba, sa, ws.data_ptr(), ws.numel(), hip.stream_ptr()),
                      "vmg_" + name)


def linear_wgrad2_multi(probs, M: int):
    """probs: list of (xs, dys, dW (O, I[, 1, 1]), db, scale) of ONE shape: dW_i += scale_i * sum_p dys_i[p]^T xs_i[p] over M pixels, eight
    problems per launch (vmg_linear_wgrad2_multi)."""
    _wgrad_multi("linear_wgrad2_multi", probs, (M,))


def conv_wgrad3_multi(probs, N: int, H: int, W: int):
    """probs: list of (xs, dys, dW, db, scale) of ONE shape (same channel counts, strides and number of pairs): dW_i += scale_i * sum_p
    wgrad(xs_i[p], dys_i[p]), eight problems per launch."""
    _wgrad_multi("conv_wgrad3_multi", probs, (N, H, W))


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def warp_bilinear_forward(x: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """x (n,h,w,c) contiguous, flow (n,h,w,2) fp32 contiguous -> bilinear, border padding."""
    hip.require_cuda(x, flow)
    n, h, w, c = x.shape
    if not x.is_contiguous() or flow.dtype != torch.float32 or not flow.is_contiguous() or tuple(flow.shape) != (n, h, w, 2):
        raise HipError("warp: x must be contiguous (n,h,w,c), flow contiguous fp32 (n,h,w,2)")
    out = torch.empty_like(x)
    hip.check(hip.lib().vmg_warp_bilinear_fwd(hip.dtype_code(x.dtype), x.data_ptr(), flow.data_ptr(), out.data_ptr(), n, h, w, c,
                                              hip.stream_ptr()), "vmg_warp_bilinear_fwd")
    return out


def warp_bilinear_backward(x: torch.Tensor, flow: torch.Tensor, dy: torch.Tensor):
    """-> (dx in x's dtype, dflow fp32)."""
    hip.require_cuda(x, flow, dy)
    n, h, w, c = x.shape
    if not x.is_contiguous() or flow.dtype != torch.float32 or not flow.is_contiguous() or tuple(flow.shape) != (n, h, w, 2):
        raise HipError("warp: x must be contiguous (n,h,w,c), flow contiguous fp32 (n,h,w,2)")
    if dy.dtype != x.dtype or tuple(dy.shape) != (n, h, w, c):
        raise HipError(f"warp_bilinear_backward: dy must have x's shape and dtype, got {tuple(dy.shape)} {dy.dtype}")
    dy = dy.contiguous()
    # fp32 sums for bf16 tensors too, rounded once: the accumulator comes from the pool of zeroed buffers and goes back cleared by the rounding pass
    pooled = x.dtype != torch.float32 and (n * h * w * c) % 4 == 0
    dx_acc = ACC_POOL.take((n, h, w, c), x.device) if pooled else torch.zeros((n, h, w, c), dtype=torch.float32, device=x.device)
    dflow = torch.empty((n, h, w, 2), dtype=torch.float32, device=x.device)  # every element is written
    hip.check(hip.lib().vmg_warp_bilinear_bwd(hip.dtype_code(x.dtype), x.data_ptr(), flow.data_ptr(), dy.data_ptr(), dx_acc.data_ptr(),
                                              dflow.data_ptr(), n, h, w, c, hip.stream_ptr()), "vmg_warp_bilinear_bwd")
    if pooled:
        dx = cast_clear(dx_acc, x.dtype)
        ACC_POOL.give(dx_acc)
        return dx, dflow
    return dx_acc.to(x.dtype), dflow


def flow_smooth(x: torch.Tensor, r: int, backward: bool = False) -> torch.Tensor:
    """x (..., H, W) contiguous fp32 planes: forward the r x r block mean of the reflect-padded plane spread back over the block; backward=True: x is the output
    gradient, the result the input gradient (vmg_flow_smooth)."""
    hip.require_cuda(x)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() < 2:
        raise HipError("flow_smooth: contiguous fp32 (..., H, W) expected")
    H, W = x.shape[-2:]
    out = torch.empty_like(x)
    hip.check(hip.lib().vmg_flow_smooth(x.data_ptr(), out.data_ptr(), x.numel() // (H * W), H, W, int(r), 1 if backward else 0, hip.stream_ptr()), "vmg_flow_smooth")
    return out


def warp_nearest_planes(loc: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """loc (n,k2,h,w) fp32 planes advected with nearest sampling / border padding."""
    hip.require_cuda(loc, flow)
    n, k2, h, w = loc.shape
    if loc.dtype != torch.float32 or flow.dtype != torch.float32 or not flow.is_contiguous() or tuple(flow.shape) != (n, h, w, 2):
        raise HipError("warp_nearest_planes: fp32 loc (n,k2,h,w) and flow (n,h,w,2) expected")
    loc = loc.contiguous()
    out = torch.empty_like(loc)
    hip.check(hip.lib().vmg_warp_nearest_planes(loc.data_ptr(), flow.data_ptr(), out.data_ptr(), n, k2, h, w, hip.stream_ptr()),
              "vmg_warp_nearest_planes")
    return out


def _ltam_check_tables(rpe, decay, heads, wh, ww):
    """The kernels index rpe as [heads][wh*ww][wh*ww] and decay as [heads]: a table made for another window would be read out of bounds."""
    wq = wh * ww
    if rpe.dtype != torch.float32 or decay.dtype != torch.float32 or not rpe.is_contiguous():
        raise HipError("ltam: rpe / decay must be fp32")
    if tuple(rpe.shape) != (heads, wq, wq):
        raise HipError(f"ltam: rpe must be (heads, wh*ww, wh*ww) = {(heads, wq, wq)}, got {tuple(rpe.shape)}")
    if decay.numel() != heads or not decay.is_contiguous():
        raise HipError(f"ltam: decay must hold {heads} contiguous values, got {tuple(decay.shape)}")


class LtamTables:
    """The device workspace of the table route (vmg_ltam_fwd_tab / _bwd_tab), one per device and stream: the calls that share a workspace must be
    ordered on one stream (a call's fill kernel overwrites the table the previous call's kernel read).  It grows when t grows.  A superseded buffer
    is retired, not freed: a captured hipGraph has the table's ADDRESS baked into its fill and attention nodes (as PackPlan's entry tables)."""

    def __init__(self):
        self.bufs = {}
        self.retired = []

    def get(self, t: int, device) -> torch.Tensor:
        need = hip.lib().vmg_ltam_tab_bytes(t)
        key = (device.index if device.index is not None else torch.cuda.current_device(), hip.stream_ptr())
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < need:
            if buf is not None:
                self.retired.append(buf)
            buf = self.bufs[key] = torch.empty(max(need, 4096), dtype=torch.uint8, device=device)
        return buf

    def clear(self):
        """The caller's explicit decision: no captured graph that used the table route will be replayed again."""
        self.bufs.clear()
        self.retired.clear()


LTAM_TABLES = LtamTables()


def _ltam_forward(tab, q, keys, vals, loc, rpe, decay, heads, wh, ww, scale):
    hip.require_cuda(q, loc, rpe, decay, *keys, *vals)
    n, h, w, c = q.shape
    t = len(keys)
    ts = [q] + list(keys) + list(vals)
    if any(x.dtype != q.dtype or tuple(x.shape) != (n, h, w, c) or not x.is_contiguous() for x in ts):
        raise HipError("ltam: q / keys / vals must be contiguous (n,h,w,c) tensors of one dtype")
    if loc.dtype != torch.float32 or tuple(loc.shape) != (n, 2 * t, h, w) or not loc.is_contiguous():
        raise HipError(f"ltam: loc must be contiguous fp32 (n,2t,h,w), got {tuple(loc.shape)}")
    _ltam_check_tables(rpe, decay, heads, wh, ww)
    out = torch.empty_like(q)
    lse = torch.empty((n, h, w, heads), dtype=torch.float32, device=q.device)
    if tab:
        if t < 1:
            raise HipError("ltam_forward_tab: at least one key-frame")
        ws = LTAM_TABLES.get(t, q.device)
        hip.check(hip.lib().vmg_ltam_fwd_tab(hip.dtype_code(q.dtype), q.data_ptr(), _ptrs(keys), _ptrs(vals), loc.data_ptr(), rpe.data_ptr(),
                                             decay.data_ptr(), out.data_ptr(), lse.data_ptr(), n, h, w, c, heads, wh, ww, t, scale,
                                             ws.data_ptr(), ws.numel(), hip.stream_ptr()), "vmg_ltam_fwd_tab")
        return out, lse
    hip.check(hip.lib().vmg_ltam_fwd(hip.dtype_code(q.dtype), q.data_ptr(), _ptrs(keys), _ptrs(vals), loc.data_ptr(), rpe.data_ptr(),
                                     decay.data_ptr(), out.data_ptr(), lse.data_ptr(), n, h, w, c, heads, wh, ww, t, scale,
                                     hip.stream_ptr()), "vmg_ltam_fwd")
    return out, lse


def ltam_forward(q, keys, vals, loc, rpe, decay, heads, wh, ww, scale):
    """Key-frame pointers in the kernel arguments: at most 32 key-frames (vmg_ltam_fwd)."""
    return _ltam_forward(False, q, keys, vals, loc, rpe, decay, heads, wh, ww, scale)


def ltam_forward_tab(q, keys, vals, loc, rpe, decay, heads, wh, ww, scale):
    """ltam_forward over any number of key-frames: their pointers in a device table (vmg_ltam_fwd_tab, workspace LTAM_TABLES).  Same checks, same bits."""
    return _ltam_forward(True, q, keys, vals, loc, rpe, decay, heads, wh, ww, scale)


def ltam_backward(q, keys, vals, loc, rpe, decay, out, lse, dout, heads, wh, ww, scale, dk_into=None, dv_into=None, drpe_into=None):
    """Key-frame pointers in the kernel arguments: at most 32 key-frames (vmg_ltam_bwd).  See _ltam_backward."""
    return _ltam_backward(False, q, keys, vals, loc, rpe, decay, out, lse, dout, heads, wh, ww, scale, dk_into, dv_into, drpe_into)


def ltam_backward_tab(q, keys, vals, loc, rpe, decay, out, lse, dout, heads, wh, ww, scale, dk_into=None, dv_into=None, drpe_into=None):
    """ltam_backward over any number of key-frames (vmg_ltam_bwd_tab, workspace LTAM_TABLES): same checks, same dk_into / dv_into / drpe_into semantics."""
    return _ltam_backward(True, q, keys, vals, loc, rpe, decay, out, lse, dout, heads, wh, ww, scale, dk_into, dv_into, drpe_into)


def _ltam_backward(tab, q, keys, vals, loc, rpe, decay, out, lse, dout, heads, wh, ww, scale, dk_into=None, dv_into=None, drpe_into=None):
    """dq, dk[j], dv[j], drpe.  dk / dv are FP32 sums (q's shape) for every tensor dtype: the caller rounds them once.  dk_into / dv_into: per
    key-frame an existing fp32 accumulator to scatter into (the gradient of a frame that several calls attend to is summed by the kernel's
    atomics, see functional.grad_bank), or None for a fresh zeroed one.  drpe_into: an fp32 tensor of rpe's shape to ADD the table gradient into (the
    parameter's .grad in the deferred weight-gradient mode) instead of a fresh zeroed one."""
    hip.require_cuda(q, loc, rpe, decay, out, lse, dout, *keys, *vals)
    n, h, w, c = q.shape
    t = len(keys)
    _ltam_check_tables(rpe, decay, heads, wh, ww)
    for nm, a in (("out", out), ("dout", dout)):
        if a.dtype != q.dtype or tuple(a.shape) != (n, h, w, c):
            raise HipError(f"ltam_backward: {nm} must have q's shape and dtype, got {tuple(a.shape)} {a.dtype}")
    if not out.is_contiguous():
        raise HipError("ltam_backward: out must be contiguous")
    if lse.dtype != torch.float32 or tuple(lse.shape) != (n, h, w, heads) or not lse.is_contiguous():
        raise HipError(f"ltam_backward: lse must be contiguous fp32 (n,h,w,heads), got {tuple(lse.shape)} {lse.dtype}")
    dout = dout.contiguous()
    dq = torch.empty_like(q)
    dk = list(dk_into) if dk_into is not None else [None] * t
    dv = list(dv_into) if dv_into is not None else [None] * t
    for a in dk + dv:
        if a is not None and (a.shape != q.shape or a.dtype != torch.float32 or not a.is_contiguous()):
            raise HipError("ltam_backward: accumulators must be contiguous fp32 tensors of q's shape")
    fresh = [i for i, a in enumerate(dk + dv) if a is None]
    if fresh:  # ONE zero-fill for all new accumulators
        acc = torch.zeros((len(fresh), n, h, w, c), dtype=torch.float32, device=q.device)
        for slot, i in enumerate(fresh):
            if i < t:
                dk[i] = acc[slot]
            else:
                dv[i - t] = acc[slot]
    if drpe_into is not None and (drpe_into.shape != rpe.shape or drpe_into.dtype != torch.float32 or not drpe_into.is_contiguous()):
        raise HipError("ltam_backward: drpe_into must be a contiguous fp32 tensor of the table's shape")
    drpe = drpe_into if drpe_into is not None else torch.zeros_like(rpe)
    if tab:
        if t < 1:
            raise HipError("ltam_backward_tab: at least one key-frame")
        ws = LTAM_TABLES.get(t, q.device)
        hip.check(hip.lib().vmg_ltam_bwd_tab(hip.dtype_code(q.dtype), q.data_ptr(), _ptrs(keys), _ptrs(vals), loc.data_ptr(), rpe.data_ptr(),
                                             decay.data_ptr(), out.data_ptr(), lse.data_ptr(), dout.data_ptr(), dq.data_ptr(), _ptrs(dk), _ptrs(dv),
                                             drpe.data_ptr(), n, h, w, c, heads, wh, ww, t, scale, ws.data_ptr(), ws.numel(), hip.stream_ptr()),
                  "vmg_ltam_bwd_tab")
        return dq, dk, dv, drpe
    hip.check(hip.lib().vmg_ltam_bwd(hip.dtype_code(q.dtype), q.data_ptr(), _ptrs(keys), _ptrs(vals), loc.data_ptr(), rpe.data_ptr(),
                                     decay.data_ptr(), out.data_ptr(), lse.data_ptr(), dout.data_ptr(), dq.data_ptr(), _ptrs(dk), _ptrs(dv),
                                     drpe.data_ptr(), n, h, w, c, heads, wh, ww, t, scale, hip.stream_ptr()), "vmg_ltam_bwd")
    return dq, dk, dv, drpe


# ---- hard trajectory attention, traj_mode 'max' (vmg_ltam_max_*) ----------------------------------------
def _ltam_max_check(nm, q, keys, vals, loc, heads):
    hip.require_cuda(q, loc, *keys, *vals)
    if q.dim() != 4 or len(keys) != len(vals):
        raise HipError(f"{nm}: q (n,h,w,c) and as many keys as vals expected")
    n, h, w, c = q.shape
    t = len(keys)
    ts = [q] + list(keys) + list(vals)
    if any(x.dtype != q.dtype or tuple(x.shape) != (n, h, w, c) or not x.is_contiguous() for x in ts):
        raise HipError(f"{nm}: q / keys / vals must be contiguous (n,h,w,c) tensors of one dtype")
    if loc.dtype != torch.float32 or tuple(loc.shape) != (n, 2 * t, h, w) or not loc.is_contiguous():
        raise HipError(f"{nm}: loc must be contiguous fp32 (n,2t,h,w), got {tuple(loc.shape)} {loc.dtype}")
    return n, h, w, c, t


def _ltam_max_forward(tab, q, keys, vals, loc, heads):
    nm = "ltam_max_forward_tab" if tab else "ltam_max_forward"
    n, h, w, c, t = _ltam_max_check(nm, q, keys, vals, loc, heads)
    if tab and t < 1:
        raise HipError("ltam_max_forward_tab: at least one key-frame")
    out = torch.empty_like(q)
    idx = torch.empty((n, h, w, heads), dtype=torch.int32, device=q.device)
    score = torch.empty((n, h, w, heads), dtype=torch.float32, device=q.device)
    if tab:
        ws = LTAM_TABLES.get(t, q.device)
        hip.check(hip.lib().vmg_ltam_max_fwd_tab(hip.dtype_code(q.dtype), q.data_ptr(), _ptrs(keys), _ptrs(vals), loc.data_ptr(), out.data_ptr(),
                                                 idx.data_ptr(), score.data_ptr(), n, h, w, c, heads, t, ws.data_ptr(), ws.numel(), hip.stream_ptr()),
                  "vmg_ltam_max_fwd_tab")
    else:
        hip.check(hip.lib().vmg_ltam_max_fwd(hip.dtype_code(q.dtype), q.data_ptr(), _ptrs(keys), _ptrs(vals), loc.data_ptr(), out.data_ptr(),
                                             idx.data_ptr(), score.data_ptr(), n, h, w, c, heads, t, hip.stream_ptr()), "vmg_ltam_max_fwd")
    return out, idx, score


def ltam_max_forward(q, keys, vals, loc, heads):
    """Hard trajectory attention (traj_mode 'max'): out (n,h,w,c), idx (n,h,w,heads) int32 -- per pixel and head the FIRST key-frame of maximal
    similarity -- and score (n,h,w,heads) fp32, that similarity.  Key-frame pointers in the kernel arguments: at most 32 (vmg_ltam_max_fwd)."""
    return _ltam_max_forward(False, q, keys, vals, loc, heads)


def ltam_max_forward_tab(q, keys, vals, loc, heads):
    """ltam_max_forward over any number of key-frames: their pointers in a device table (vmg_ltam_max_fwd_tab, workspace LTAM_TABLES).  Same bits."""
    return _ltam_max_forward(True, q, keys, vals, loc, heads)


def _ltam_max_backward(tab, q, keys, vals, loc, idx, dout, heads, dk_into=None, dv_into=None):
    """dq, dk[j], dv[j] for the selection idx (the forward's; never re-decided).  dk / dv: FP32 sums, dk_into / dv_into as _ltam_backward's."""
    nm = "ltam_max_backward_tab" if tab else "ltam_max_backward"
    n, h, w, c, t = _ltam_max_check(nm, q, keys, vals, loc, heads)
    hip.require_cuda(idx, dout)
    if tab and t < 1:
        raise HipError("ltam_max_backward_tab: at least one key-frame")
    if dout.dtype != q.dtype or tuple(dout.shape) != (n, h, w, c):
        raise HipError(f"{nm}: dout must have q's shape and dtype, got {tuple(dout.shape)} {dout.dtype}")
    if idx.dtype != torch.int32 or tuple(idx.shape) != (n, h, w, heads) or not idx.is_contiguous():
        raise HipError(f"{nm}: idx must be contiguous int32 (n,h,w,heads), got {tuple(idx.shape)} {idx.dtype}")
    dout = dout.contiguous()
    dq = torch.empty_like(q)
    dk = list(dk_into) if dk_into is not None else [None] * t
    dv = list(dv_into) if dv_into is not None else [None] * t
    if len(dk) != t or len(dv) != t:
        raise HipError(f"{nm}: one accumulator (or None) per key-frame expected")
    for a in dk + dv:
        if a is not None and (a.shape != q.shape or a.dtype != torch.float32 or not a.is_contiguous() or a.device != q.device):
            raise HipError(f"{nm}: accumulators must be contiguous fp32 tensors of q's shape")
    fresh = [i for i, a in enumerate(dk + dv) if a is None]
    if fresh:  # ONE zero-fill for all new accumulators
        acc = torch.zeros((len(fresh), n, h, w, c), dtype=torch.float32, device=q.device)
        for slot, i in enumerate(fresh):
            if i < t:
                dk[i] = acc[slot]
            else:
                dv[i - t] = acc[slot]
    if tab:
        ws = LTAM_TABLES.get(t, q.device)
        hip.check(hip.lib().vmg_ltam_max_bwd_tab(hip.dtype_code(q.dtype), q.data_ptr(), _ptrs(keys), _ptrs(vals), loc.data_ptr(), idx.data_ptr(),
                                                 dout.data_ptr(), dq.data_ptr(), _ptrs(dk), _ptrs(dv), n, h, w, c, heads, t, ws.data_ptr(), ws.numel(),
                                                 hip.stream_ptr()), "vmg_ltam_max_bwd_tab")
    else:
        hip.check(hip.lib().vmg_ltam_max_bwd(hip.dtype_code(q.dtype), q.data_ptr(), _ptrs(keys), _ptrs(vals), loc.data_ptr(), idx.data_ptr(),
                                             dout.data_ptr(), dq.data_ptr(), _ptrs(dk), _ptrs(dv), n, h, w, c, heads, t, hip.stream_ptr()),
                  "vmg_ltam_max_bwd")
    return dq, dk, dv


def ltam_max_backward(q, keys, vals, loc, idx, dout, heads, dk_into=None, dv_into=None):
    """Key-frame pointers in the kernel arguments: at most 32 key-frames (vmg_ltam_max_bwd).  See _ltam_max_backward."""
    return _ltam_max_backward(False, q, keys, vals, loc, idx, dout, heads, dk_into, dv_into)


def ltam_max_backward_tab(q, keys, vals, loc, idx, dout, heads, dk_into=None, dv_into=None):
    """ltam_max_backward over any number of key-frames (vmg_ltam_max_bwd_tab, workspace LTAM_TABLES): same checks, same dk_into / dv_into semantics."""
    return _ltam_max_backward(True, q, keys, vals, loc, idx, dout, heads, dk_into, dv_into)


OP_CA_FWD, OP_CA_BWD, OP_MIX_FWD, OP_MIX_BWD, OP_GATE_FWD, OP_GATE_BWD, OP_AFFINE2, OP_SCALE, OP_GATE_RES_FWD, OP_GATE_RES_BWD = range(10)


def group_reduce(a: torch.Tensor, G: int, b: Optional[torch.Tensor] = None, c3: Optional[torch.Tensor] = None, mode: int = 0,
                 scale: float = 1.0) -> torch.Tensor:
    """a (and b, c3): contiguous (G*R, C)-shaped data; returns fp32 (G, C): scale * sum_r of (a+b+c3) or of a*b."""
    hip.require_cuda(a, b, c3)
    C = a.shape[-1]
    rows = a.numel() // C
    if rows % G or not a.is_contiguous() or any(t is not None and (t.shape != a.shape or t.dtype != a.dtype or not t.is_contiguous()) for t in (b, c3)):
        raise HipError("group_reduce: contiguous tensors of one shape / dtype covering G groups expected")
    out = torch.empty((G, C), dtype=torch.float32, device=a.device)
    ws = _workspace("vmg_group_reduce_ws_bytes", a.device)
    hip.check(hip.lib().vmg_group_reduce(hip.dtype_code(a.dtype), a.data_ptr(), b.data_ptr() if b is not None else None,
                                         c3.data_ptr() if c3 is not None else None, out.data_ptr(), G, rows // G, C, mode, scale,
                                         ws.data_ptr(), ws.numel(), hip.stream_ptr()), "vmg_group_reduce")
    return out


def group_reduce3(a: torch.Tensor, b0: torch.Tensor, b1: torch.Tensor, b2: torch.Tensor, G: int, scale: float = 1.0) -> torch.Tensor:
    """fp32 (G, C, 3): scale * sum_r a * {b0, b1, b2} over the rows of each group, one pass over a."""
    hip.require_cuda(a, b0, b1, b2)
    C = a.shape[-1]
    rows = a.numel() // C
    if rows % G or any(t.shape != a.shape or t.dtype != a.dtype or not t.is_contiguous() for t in (a, b0, b1, b2)):
        raise HipError("group_reduce3: contiguous tensors of one shape / dtype covering G groups expected")
    out = torch.empty((G, C, 3), dtype=torch.float32, device=a.device)
    ws = _workspace("vmg_group_reduce_ws_bytes", a.device)
    hip.check(hip.lib().vmg_group_reduce3(hip.dtype_code(a.dtype), a.data_ptr(), b0.data_ptr(), b1.data_ptr(), b2.data_ptr(), out.data_ptr(), G,
                                          rows // G, C, scale, ws.data_ptr(), ws.numel(), hip.stream_ptr()), "vmg_group_reduce3")
    return out


# per op: coefficients per (group, channel) in `coef` (0: no coef), whether `add` (G, C) is read, outputs
_TAB_EW = {OP_CA_FWD: (1, False, 1), OP_CA_BWD: (1, True, 2), OP_MIX_FWD: (3, False, 1), OP_MIX_BWD: (3, True, 3), OP_GATE_FWD: (0, False, 1),
           OP_GATE_BWD: (0, False, 2), OP_AFFINE2: (2, True, 1), OP_SCALE: (1, False, 1), OP_GATE_RES_FWD: (1, False, 1), OP_GATE_RES_BWD: (1, False, 2)}


def tab_elementwise(op: int, p0, p1=None, p2=None, coef=None, add=None, s: float = 1.0, G: int = 1, nout: int = 1):
    hip.require_cuda(p0, p1, p2, coef, add)
    if op not in _TAB_EW:
        raise HipError(f"tab_elementwise: unknown op {op}")
    ncoef, has_add, op_nout = _TAB_EW[op]
    C = p0.shape[-1]
    rows = p0.numel() // C
    if G <= 0 or rows % G:
        raise HipError(f"tab_elementwise: {rows} rows do not split into G = {G} groups")
    if nout != op_nout:
        raise HipError(f"tab_elementwise: op {op} writes {op_nout} outputs, not {nout}")
    if ncoef and (coef is None or coef.numel() != G * C * ncoef):
        raise HipError(f"tab_elementwise: op {op} needs coef of G*C*{ncoef} = {G * C * ncoef} elements")
    if has_add and (add is None or add.numel() != G * C):
        raise HipError(f"tab_elementwise: op {op} needs add of G*C = {G * C} elements")
    for t in (p0, p1, p2):
        if t is not None and (not t.is_contiguous() or t.shape != p0.shape or t.dtype != p0.dtype):
            raise HipError("tab_elementwise: contiguous operands of one shape / dtype expected")
    for t in (coef, add):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise HipError("tab_elementwise: coefficients must be contiguous fp32")
    outs = [torch.empty_like(p0) for _ in range(nout)]
    ptr = lambda t: t.data_ptr() if t is not None else None
    o = outs + [None] * (3 - nout)
    hip.check(hip.lib().vmg_tab_elementwise(hip.dtype_code(p0.dtype), op, ptr(p0), ptr(p1), ptr(p2), ptr(coef), ptr(add), s, ptr(o[0]),
                                            ptr(o[1]), ptr(o[2]), rows, rows // G, C, hip.stream_ptr()), "vmg_tab_elementwise")
    return outs[0] if nout == 1 else outs


def _gate_args(who, act, tensors, coef, G):
    """Shared checks of the gate family: returns (activation code, rows, C)."""
    hip.require_cuda(*tensors, coef)
    p0 = tensors[0]
    if act not in hip.GATE_ACTS:
        raise HipError(f"{who}: activation {act!r} is not one of {sorted(hip.GATE_ACTS)}")
    if p0.dtype not in (torch.float32, torch.bfloat16) or any(not t.is_contiguous() or t.shape != p0.shape or t.dtype != p0.dtype for t in tensors):
        raise HipError(f"{who}: contiguous fp32 / bf16 operands of one shape and dtype expected")
    C = p0.shape[-1]
    rows = p0.numel() // C
    if coef is not None and (G <= 0 or rows % G or coef.dtype != torch.float32 or not coef.is_contiguous() or coef.numel() != G * C):
        raise HipError(f"{who}: coef must be contiguous fp32 of G * C = {G * C} elements, G = {G} dividing the {rows} rows")
    return hip.GATE_ACTS[act], rows, C


def gate_forward(a: torch.Tensor, y: torch.Tensor, act: str = "tanh", asym: bool = False, res: Optional[torch.Tensor] = None,
                 coef: Optional[torch.Tensor] = None, G: int = 1) -> torch.Tensor:
    """(a + y) * act(y), or silu(a) * gelu(y) with asym (vmg_gate_fwd); with res and coef (G, C) fp32: res + gate * coef (vmg_gate_res_fwd)."""
    if (res is None) != (coef is None):
        raise HipError("gate_forward: res and coef come together")
    code, rows, C = _gate_args("gate_forward", act, [a, y] + ([res] if res is not None else []), coef, G)
    out = torch.empty_like(a)
    if res is None:
        hip.check(hip.lib().vmg_gate_fwd(hip.dtype_code(a.dtype), int(asym), code, a.data_ptr(), y.data_ptr(), out.data_ptr(), rows, C,
                                         hip.stream_ptr()), "vmg_gate_fwd")
    else:
        hip.check(hip.lib().vmg_gate_res_fwd(hip.dtype_code(a.dtype), int(asym), code, a.data_ptr(), y.data_ptr(), res.data_ptr(), coef.data_ptr(),
                                             out.data_ptr(), rows, G, C, hip.stream_ptr()), "vmg_gate_res_fwd")
    return out


def gate_backward(d: torch.Tensor, a: torch.Tensor, y: torch.Tensor, act: str = "tanh", asym: bool = False, coef: Optional[torch.Tensor] = None,
                  G: int = 1):
    """(da, dy) of gate_forward for the output gradient d (vmg_gate_bwd); with coef the gradient is d * coef first (vmg_gate_res_bwd)."""
    code, rows, C = _gate_args("gate_backward", act, [d, a, y], coef, G)
    da, dy = torch.empty_like(a), torch.empty_like(a)
    if coef is None:
        hip.check(hip.lib().vmg_gate_bwd(hip.dtype_code(a.dtype), int(asym), code, d.data_ptr(), a.data_ptr(), y.data_ptr(), da.data_ptr(),
                                         dy.data_ptr(), rows, C, hip.stream_ptr()), "vmg_gate_bwd")
    else:
        hip.check(hip.lib().vmg_gate_res_bwd(hip.dtype_code(a.dtype), int(asym), code, d.data_ptr(), a.data_ptr(), y.data_ptr(), coef.data_ptr(),
                                             da.data_ptr(), dy.data_ptr(), rows, G, C, hip.stream_ptr()), "vmg_gate_res_bwd")
    return da, dy


def se_mlp_forward(m: torch.Tensor, w1: torch.Tensor, b1, w2: torch.Tensor, b2, act1: int, mode: int):
    """Squeeze-excite MLP on pooled rows m (G, C) fp32: returns (pre (G, Hd), out (G, Co)); mode 0 sigmoid, mode 1 softmax over triples."""
    hip.require_cuda(m, w1, w2)
    G, C = m.shape
    Hd, Co = w1.shape[0], w2.shape[0]
    for t in (m, w1, w2, b1, b2):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise HipError("se_mlp: contiguous fp32 tensors only")
    pre = torch.empty(G, Hd, dtype=torch.float32, device=m.device)
    out = torch.empty(G, Co, dtype=torch.float32, device=m.device)
    hip.check(hip.lib().vmg_se_mlp_fwd(m.data_ptr(), w1.data_ptr(), b1.data_ptr() if b1 is not None else None, w2.data_ptr(),
                                       b2.data_ptr() if b2 is not None else None, pre.data_ptr(), out.data_ptr(), G, C, Hd, Co, act1, mode,
                                       hip.stream_ptr()), "vmg_se_mlp_fwd")
    return pre, out


def se_mlp_backward(dout: torch.Tensor, out: torch.Tensor, m: torch.Tensor, pre: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, act1: int,
                    mode: int, dm_scale: float, into=None):
    """-> dm (G, C) * dm_scale, dw1, db1, dw2, db2 (fresh tensors); into = (gw1, gb1, gw2, gb2): the parameter gradients are ADDED to these
    contiguous fp32 buffers (param.grad) and returned as such."""
    hip.require_cuda(dout, out, m, pre, w1, w2)
    G, C = m.shape
    Hd, Co = w1.shape[0], w2.shape[0]
    for t in (dout, out, m, pre, w1, w2):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise HipError("se_mlp: contiguous fp32 tensors only")
    dev = m.device
    sizes = (G * C, G * (Co + Hd)) if into is not None else (G * C, G * (Co + Hd), Hd * C, Hd, Co * Hd, Co)
    buf = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
    o = 0
    parts = []
    for n in sizes:
        parts.append(buf[o:o + n])
        o += n
    if into is not None:
        dm, ws = parts
        dw1, db1, dw2, db2 = into
        for t, n in zip(into, (Hd * C, Hd, Co * Hd, Co)):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n or not t.is_cuda:
                raise HipError("se_mlp: gradient buffers must be contiguous fp32 of the parameters' sizes")
    else:
        dm, ws, dw1, db1, dw2, db2 = parts
    hip.check(hip.lib().vmg_se_mlp_bwd(dout.data_ptr(), out.data_ptr(), m.data_ptr(), pre.data_ptr(), w1.data_ptr(), w2.data_ptr(), dm.data_ptr(),
                                       dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), ws.data_ptr(), G, C, Hd, Co, act1, mode,
                                       float(dm_scale), 1 if into is not None else 0, hip.stream_ptr()), "vmg_se_mlp_bwd")
    if into is not None:
        return dm.view(G, C), dw1, db1, dw2, db2
    return dm.view(G, C), dw1.view(Hd, C), db1, dw2.view(Co, Hd), db2


# ---- the patch-shift FFN (csrc/shift_ffn.hip)
SHIFT_ROUTES = {hip.SHIFT_VECTOR: "vector", hip.SHIFT_ELEMENT: "element"}


def patch_shift_route(Cs: int, dtype: torch.dtype, aligned: bool = True) -> str:
    """The kernel a patch shift of Cs channels runs on (vmg_patch_shift_plan, the function the entries themselves call; no device needed):
    'vector' when the chunk width ceil(Cs / 9) and Cs are multiples of the 16-byte vector and the pointers are 16-byte aligned, else 'element'."""
    r = hip.lib().vmg_patch_shift_plan(hip.dtype_code(dtype), int(Cs), int(bool(aligned)))
    if r not in SHIFT_ROUTES:
        raise HipError(f"patch_shift_route: no route for Cs = {Cs}, {dtype}")
    return SHIFT_ROUTES[r]


def _shift_args(who, x, others):
    hip.require_cuda(x, *others)
    if x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous():
        raise HipError(f"{who}: a contiguous fp32 / bf16 (N, H, W, Cs) tensor expected")
    if any(t.shape != x.shape or t.dtype != x.dtype or not t.is_contiguous() for t in others):
        raise HipError(f"{who}: contiguous operands of one shape / dtype expected")
    if min(x.shape) < 1:
        raise HipError(f"{who}: empty tensor")


def patch_shift_forward(x: torch.Tensor, sign: int, gelu: bool = False) -> torch.Tensor:
    """PatchShift2D (sign +1) / its inverse (-1) of x (N, H, W, Cs), with gelu: of gelu(x) (vmg_patch_shift_fwd)."""
    _shift_args("patch_shift_forward", x, [])
    N, H, W, Cs = x.shape
    y = torch.empty_like(x)
    hip.check(hip.lib().vmg_patch_shift_fwd(hip.dtype_code(x.dtype), int(sign), hip.ACT_GELU if gelu else hip.ACT_NONE, x.data_ptr(), y.data_ptr(), N, H, W, Cs,
                                            hip.stream_ptr()), "vmg_patch_shift_fwd")
    return y


def patch_shift_backward(dy: torch.Tensor, sign: int, x: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The input gradient of patch_shift_forward(x, sign, gelu): x given = the GELU form (vmg_patch_shift_bwd)."""
    _shift_args("patch_shift_backward", dy, [x] if x is not None else [])
    N, H, W, Cs = dy.shape
    dx = torch.empty_like(dy)
    hip.check(hip.lib().vmg_patch_shift_bwd(hip.dtype_code(dy.dtype), int(sign), hip.ACT_GELU if x is not None else hip.ACT_NONE, dy.data_ptr(),
                                            x.data_ptr() if x is not None else None, dx.data_ptr(), N, H, W, Cs, hip.stream_ptr()), "vmg_patch_shift_bwd")
    return dx


def group_reduce2(a: torch.Tensor, b0: torch.Tensor, b1: torch.Tensor, G: int, scale: float = 1.0) -> torch.Tensor:
    """fp32 (G, C, 2): scale * sum_r a * {b0, b1} over the rows of each group, one pass over a."""
    hip.require_cuda(a, b0, b1)
    C = a.shape[-1]
    rows = a.numel() // C
    if G <= 0 or rows % G or any(t.shape != a.shape or t.dtype != a.dtype or not t.is_contiguous() for t in (a, b0, b1)):
        raise HipError("group_reduce2: contiguous tensors of one shape / dtype covering G groups expected")
    out = torch.empty((G, C, 2), dtype=torch.float32, device=a.device)
    ws = _workspace("vmg_group_reduce_ws_bytes", a.device)
    hip.check(hip.lib().vmg_group_reduce2(hip.dtype_code(a.dtype), a.data_ptr(), b0.data_ptr(), b1.data_ptr(), out.data_ptr(), G, rows // G, C, scale,
                                          ws.data_ptr(), ws.numel(), hip.stream_ptr()), "vmg_group_reduce2")
    return out


def mix2_forward(h: torch.Tensor, w: torch.Tensor, coef: torch.Tensor, G: int) -> torch.Tensor:
    """h * coef[g, c, 0] + w * coef[g, c, 1], coef (G, C, 2) fp32 (vmg_mix2_fwd)."""
    hip.require_cuda(h, w, coef)
    C = h.shape[-1]
    rows = h.numel() // C
    if G <= 0 or rows % G or w.shape != h.shape or w.dtype != h.dtype or not (h.is_contiguous() and w.is_contiguous()):
        raise HipError("mix2_forward: contiguous operands of one shape / dtype covering G groups expected")
    if coef.dtype != torch.float32 or not coef.is_contiguous() or coef.numel() != G * C * 2:
        raise HipError(f"mix2_forward: coef must be contiguous fp32 of G*C*2 = {G * C * 2} elements")
    y = torch.empty_like(h)
    hip.check(hip.lib().vmg_mix2_fwd(hip.dtype_code(h.dtype), h.data_ptr(), w.data_ptr(), coef.data_ptr(), y.data_ptr(), rows, rows // G, C,
                                     hip.stream_ptr()), "vmg_mix2_fwd")
    return y


def mix2_backward(dy: torch.Tensor, coef: torch.Tensor, add: torch.Tensor, G: int):
    """(dy * coef[g, c, 0] + add[g, c], dy * coef[g, c, 1] + add[g, c]) in one launch (vmg_mix2_bwd)."""
    hip.require_cuda(dy, coef, add)
    C = dy.shape[-1]
    rows = dy.numel() // C
    if G <= 0 or rows % G or not dy.is_contiguous():
        raise HipError("mix2_backward: a contiguous gradient covering G groups expected")
    for t, n in ((coef, G * C * 2), (add, G * C)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise HipError("mix2_backward: coef (G, C, 2) and add (G, C) must be contiguous fp32")
    dh, dw = torch.empty_like(dy), torch.empty_like(dy)
    hip.check(hip.lib().vmg_mix2_bwd(hip.dtype_code(dy.dtype), dy.data_ptr(), coef.data_ptr(), add.data_ptr(), dh.data_ptr(), dw.data_ptr(), rows,
                                     rows // G, C, hip.stream_ptr()), "vmg_mix2_bwd")
    return dh, dw


def se_mlp2_forward(m: torch.Tensor, w1: torch.Tensor, b1, w2: torch.Tensor, b2):
    """The re-weighting MLP of Mlp_cnn_shift on pooled rows m (G, C) fp32: returns (pre (G, Hd), a (G, 2C) = (G, C, 2): softmax over each channel's two logits)."""
    hip.require_cuda(m, w1, w2, b1, b2)
    G, C = m.shape
    Hd = w1.shape[0]
    for t in (m, w1, w2, b1, b2):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise HipError("se_mlp2: contiguous fp32 tensors only")
    if tuple(w1.shape) != (Hd, C) or tuple(w2.shape) != (2 * C, Hd):
        raise HipError(f"se_mlp2: W1 ({Hd}, {C}) and W2 ({2 * C}, {Hd}) expected")
    pre = torch.empty(G, Hd, dtype=torch.float32, device=m.device)
    out = torch.empty(G, 2 * C, dtype=torch.float32, device=m.device)
    hip.check(hip.lib().vmg_se_mlp2_fwd(m.data_ptr(), w1.data_ptr(), b1.data_ptr() if b1 is not None else None, w2.data_ptr(),
                                        b2.data_ptr() if b2 is not None else None, pre.data_ptr(), out.data_ptr(), G, C, Hd, hip.stream_ptr()), "vmg_se_mlp2_fwd")
    return pre, out


def se_mlp2_backward(dout: torch.Tensor, out: torch.Tensor, m: torch.Tensor, pre: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, dm_scale: float, into=None):
    """-> dm (G, C) * dm_scale, dw1, db1, dw2, db2 (fresh tensors); into = (gw1, gb1, gw2, gb2): the parameter gradients are ADDED to these
    contiguous fp32 buffers (param.grad) and returned as such -- se_mlp_backward's contract."""
    hip.require_cuda(dout, out, m, pre, w1, w2)
    G, C = m.shape
    Hd, Co = w1.shape[0], 2 * C
    for t in (dout, out, m, pre, w1, w2):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise HipError("se_mlp2: contiguous fp32 tensors only")
    if dout.numel() != G * Co or out.numel() != G * Co or tuple(w2.shape) != (Co, Hd):
        raise HipError("se_mlp2: dout and out (G, 2C), W2 (2C, Hd) expected")
    sizes = (G * C, G * (Co + Hd)) if into is not None else (G * C, G * (Co + Hd), Hd * C, Hd, Co * Hd, Co)
    buf = torch.empty(sum(sizes), dtype=torch.float32, device=m.device)
    o = 0
    parts = []
    for n in sizes:
        parts.append(buf[o:o + n])
        o += n
    if into is not None:
        dm, ws = parts
        dw1, db1, dw2, db2 = into
        for t, n in zip(into, (Hd * C, Hd, Co * Hd, Co)):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n or not t.is_cuda:
                raise HipError("se_mlp2: gradient buffers must be contiguous fp32 of the parameters' sizes")
    else:
        dm, ws, dw1, db1, dw2, db2 = parts
    hip.check(hip.lib().vmg_se_mlp2_bwd(dout.data_ptr(), out.data_ptr(), m.data_ptr(), pre.data_ptr(), w1.data_ptr(), w2.data_ptr(), dm.data_ptr(),
                                        dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), ws.data_ptr(), G, C, Hd, float(dm_scale),
                                        1 if into is not None else 0, hip.stream_ptr()), "vmg_se_mlp2_bwd")
    if into is not None:
        return dm.view(G, C), dw1, db1, dw2, db2
    return dm.view(G, C), dw1.view(Hd, C), db1, dw2.view(Co, Hd), db2


# ---- the depthwise 3x3 convolution of the MBConv mixer (csrc/dwconv.hip)
DWCONV_ROUTES = {hip.DWCONV_VECTOR: "vector", hip.DWCONV_ELEMENT: "element"}
DWCONV_ACTS = {None: 0, "relu6": 1}
DwconvPlan = collections.namedtuple("DwconvPlan", "route tile_h tile_w chan_block grid lds_bytes partials wgrad_grid")


def dwconv3_plan(N: int, H: int, W: int, C: int, dtype: torch.dtype, aligned: bool = True) -> DwconvPlan:
    """What the depthwise 3x3 entries launch for the geometry (vmg_dwconv3_plan, the function they dispatch through; no device needed): route
    ('vector' / 'element'), the workgroup's pixel tile and channel block, the grid and LDS bytes of the forward / data gradient, the
    first-stage partial count and grid of the weight gradient.  aligned: every activation pointer is 16-byte aligned.  Raises HipError with
    the entries' message for what they refuse (N * H * W * C >= 2^31)."""
    plan = (ctypes.c_int * hip.DWCONV_PLAN_INTS)()
    hip.check(hip.lib().vmg_dwconv3_plan(hip.dtype_code(dtype), int(N), int(H), int(W), int(C), int(bool(aligned)), plan), "vmg_dwconv3_plan")
    p = DwconvPlan(*plan)
    return p._replace(route=DWCONV_ROUTES[p.route])


def dwconv3_route(C: int, dtype: torch.dtype, aligned: bool = True) -> str:
    """The kernel a depthwise 3x3 of C channels runs on: 'vector' when C is a multiple of the 16-byte vector (8 bf16 / 4 fp32) and the
    pointers are 16-byte aligned, else 'element' (from the plan; the route does not depend on N, H, W)."""
    return dwconv3_plan(1, 1, 1, C, dtype, aligned).route


def _dwconv_args(who, x, others, weight, bias, src_act, act):
    hip.require_cuda(x, weight, bias, *others)
    if x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous():
        raise HipError(f"{who}: a contiguous fp32 / bf16 (N, H, W, C) tensor expected")
    if any(t.shape != x.shape or t.dtype != x.dtype or not t.is_contiguous() for t in others):
        raise HipError(f"{who}: contiguous operands of one shape / dtype expected")
    if min(x.shape) < 1:
        raise HipError(f"{who}: empty tensor")
    C = x.shape[-1]
    if weight.dtype != torch.float32 or not weight.is_contiguous() or tuple(weight.shape) != (C, 1, 3, 3):
        raise HipError(f"{who}: a contiguous fp32 weight ({C}, 1, 3, 3) expected")
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or tuple(bias.shape) != (C,)):
        raise HipError(f"{who}: a contiguous fp32 bias ({C},) expected")
    if src_act not in DWCONV_ACTS or act not in DWCONV_ACTS:
        raise HipError(f"{who}: src_act and act are None or 'relu6', got {src_act!r}, {act!r}")
    return DWCONV_ACTS[src_act], DWCONV_ACTS[act]


def dwconv3_forward(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, src_act=None, act=None) -> torch.Tensor:
    """act(depthwise conv3x3(src_act(x)) + bias) of x (N, H, W, C), stride 1, zero padding 1 (vmg_dwconv3_fwd)."""
    sa, oa = _dwconv_args("dwconv3_forward", x, [], weight, bias, src_act, act)
    N, H, W, C = x.shape
    y = torch.empty_like(x)
    hip.check(hip.lib().vmg_dwconv3_fwd(hip.dtype_code(x.dtype), sa, oa, x.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(), N, H, W, C,
                                        hip.stream_ptr()), "vmg_dwconv3_fwd")
    return y


def dwconv3_backward_data(dy: torch.Tensor, y: Optional[torch.Tensor], x: Optional[torch.Tensor], weight: torch.Tensor, src_act=None, act=None) -> torch.Tensor:
    """The input gradient of dwconv3_forward in one launch (vmg_dwconv3_bwd_data): y, the stored output, is read with act; x with src_act."""
    others = [t for t, on in ((y, act), (x, src_act)) if on is not None]
    if any(t is None for t in others):
        raise HipError("dwconv3_backward_data: y is needed with act, x with src_act")
    sa, oa = _dwconv_args("dwconv3_backward_data", dy, others, weight, None, src_act, act)
    N, H, W, C = dy.shape
    dx = torch.empty_like(dy)
    hip.check(hip.lib().vmg_dwconv3_bwd_data(hip.dtype_code(dy.dtype), sa, oa, dy.data_ptr(), y.data_ptr() if oa else None, x.data_ptr() if sa else None,
                                             weight.data_ptr(), dx.data_ptr(), N, H, W, C, hip.stream_ptr()), "vmg_dwconv3_bwd_data")
    return dx


def dwconv3_backward_weight(dy: torch.Tensor, y: Optional[torch.Tensor], x: torch.Tensor, src_act=None, act=None, into=None):
    """(dW (C, 1, 3, 3), db (C,)) fp32 of dwconv3_forward (vmg_dwconv3_bwd_weight: two ordered launches, no atomics, a workspace of
    vmg_dwconv3_wgrad_ws_bytes).  into = (gW, gb): the sums are ADDED to these contiguous fp32 buffers (param.grad) and returned as such."""
    if act is not None and y is None:
        raise HipError("dwconv3_backward_weight: y is needed with act")
    C = dy.shape[-1]
    if into is not None:
        dW, db = into
        if any(t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda for t in into) or dW.numel() != 9 * C or db.numel() != C:
            raise HipError("dwconv3_backward_weight: gradient buffers must be contiguous fp32 of the parameters' sizes")
    else:
        dW = torch.empty((C, 1, 3, 3), dtype=torch.float32, device=dy.device)
        db = torch.empty(C, dtype=torch.float32, device=dy.device)
    sa, oa = _dwconv_args("dwconv3_backward_weight", dy, [x] + ([y] if act is not None else []), dW.view(C, 1, 3, 3), db, src_act, act)
    N, H, W, _ = dy.shape
    code = hip.dtype_code(dy.dtype)
    nbytes = int(hip.lib().vmg_dwconv3_wgrad_ws_bytes(code, N, H, W, C))
    if nbytes < 0:
        raise HipError(f"vmg_dwconv3_wgrad_ws_bytes: {hip.lib().vmg_last_error().decode()}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dy.device)
    hip.check(hip.lib().vmg_dwconv3_bwd_weight(code, sa, oa, dy.data_ptr(), y.data_ptr() if oa else None, x.data_ptr(), dW.data_ptr(), db.data_ptr(), N, H, W, C,
                                               1 if into is not None else 0, ws.data_ptr(), nbytes, hip.stream_ptr()), "vmg_dwconv3_bwd_weight")
    return dW, db


class PackPlan:
    """One-launch repacking of many weights (vmg_pack_entry / vmg_pack_run): the entry array lives on the device and is rebuilt only
    when the set of packs (or a weight's / pack buffer's address) changes."""

    def __init__(self):
        self.sig, self.dev, self.n, self.blocks = None, None, 0, 0
        # superseded entry tables are never freed: a captured hipGraph (train.TrainStep.capture, infer.GraphedModel) has the table's ADDRESS
        # baked into its vmg_pack_run node, and a later plan rebuild (an eager call at another shape creates new packs) must not hand that
        # memory back to the allocator while the graph can still be replayed.  A table is ~100 B per pack; plans are rebuilt a handful of times.
        self.retired = []

    def run(self, packs: Sequence[PackedConv], reuse: bool = False):
        """reuse: the caller guarantees that `packs` is the list of the previous call unless it has reset self.sig to None."""
        l = hip.lib()
        if reuse and self.sig is not None:
            hip.check(l.vmg_pack_run(self.dev.data_ptr(), self.n, self.blocks, hip.stream_ptr()), "vmg_pack_run")
            return
        packs = [p for p in packs if p.call is not None]
        if not packs:
            return
        sig = tuple((p.call[0], p.buf.data_ptr()) for p in packs)
        if sig != self.sig:
            esz = l.vmg_pack_entry_bytes()
            host = (ctypes.c_char * (esz * len(packs)))()
            base = ctypes.addressof(host)
            blk = 0
            owner = []  # entry index of every block: the kernel's blocks look their entry up here (appended to the entry array)
            for i, p in enumerate(packs):
                wptr, O, I, o0, on, soff, sch, tf = p.call
                nb = l.vmg_pack_entry(base + i * esz, 1 if p.layout == "ws" else 0, hip.dtype_code(p.dtype), wptr, O, I, p.ks, o0, on, len(sch),
                                      _intarr(soff), _intarr(sch), tf, p.cout_tiles, p.buf.data_ptr(), blk)
                if nb <= 0:
                    hip.check(nb if nb < 0 else -1, "vmg_pack_entry")
                blk += nb
                owner.extend([i] * nb)
            if self.dev is not None:
                self.retired.append(self.dev)
            table = struct.pack("<%di" % len(owner), *owner)
            self.dev = torch.frombuffer(bytearray(bytes(host) + table), dtype=torch.uint8).to(packs[0].buf.device)
            self.sig, self.n, self.blocks = sig, len(packs), blk
        hip.check(l.vmg_pack_run(self.dev.data_ptr(), self.n, self.blocks, hip.stream_ptr()), "vmg_pack_run")


# ---- fp8 (e4m3, block-scaled) convolution: Q8 records, packed weights, the kernel (csrc/conv_fp8.hip) ------------------------------------
def q8_record_bytes(C: int) -> int:
    return (C + 31) // 32 * 32 + 16


def q8_quantize(x: torch.Tensor) -> torch.Tensor:
    """bf16 channels-last (..., C) -> Q8 records uint8 (..., q8_record_bytes(C)) (vmg_q8_quantize)."""
    hip.require_cuda(x)
    C = x.shape[-1]
    if x.dtype != torch.bfloat16 or x.stride(-1) != 1:
        raise HipError("q8_quantize: bf16 channels-last tensor expected")
    ps = _pix_stride(x)
    M = x.numel() // C
    out = torch.empty(tuple(x.shape[:-1]) + (q8_record_bytes(C),), dtype=torch.uint8, device=x.device)
    hip.check(hip.lib().vmg_q8_quantize(x.data_ptr(), ps, out.data_ptr(), M, C, hip.stream_ptr()), "vmg_q8_quantize")
    return out


def q8_dequantize(rec: torch.Tensor, C: int) -> torch.Tensor:
    """Records -> fp32 (..., C) with torch ops (tests and tools; the product path never dequantises)."""
    nb = (C + 31) // 32
    data = rec[..., :nb * 32].contiguous().view(torch.float8_e4m3fn).float().reshape(*rec.shape[:-1], nb, 32)
    scale = torch.exp2(rec[..., nb * 32:nb * 32 + nb].float() - 127.0)
    return (data * scale[..., None]).reshape(*rec.shape[:-1], nb * 32)[..., :C]


class PackedQ8:
    __slots__ = ("buf", "cout", "cin", "call")

    def __init__(self, buf, cout, cin, call):
        self.buf, self.cout, self.cin, self.call = buf, cout, cin, call


def pack_conv_weight_q8(w: torch.Tensor, transpose_flip: bool = False, out: Optional[torch.Tensor] = None) -> PackedQ8:
    """fp32 (O, I, 3, 3) -> the fp8 convolution's weight image (vmg_convq8_pack): e4m3 with one power-of-two scale per output channel."""
    hip.require_cuda(w)
    if w.dtype != torch.float32 or not w.is_contiguous() or w.dim() != 4 or w.shape[2] != 3 or w.shape[3] != 3:
        raise HipError("pack_conv_weight_q8 expects a contiguous fp32 (O, I, 3, 3) weight")
    O, I = w.shape[0], w.shape[1]
    cout, cin = (I, O) if transpose_flip else (O, I)
    nbytes = hip.lib().vmg_convq8_pack_bytes(cout, cin)
    if nbytes <= 0:
        raise HipError(f"vmg_convq8_pack_bytes: {hip.lib().vmg_last_error().decode()}")
    buf = out if (out is not None and out.numel() >= int(nbytes)) else torch.empty(int(nbytes), dtype=torch.uint8, device=w.device)
    hip.check(hip.lib().vmg_convq8_pack(w.data_ptr(), O, I, 1 if transpose_flip else 0, buf.data_ptr(), hip.stream_ptr()), "vmg_convq8_pack")
    return PackedQ8(buf, cout, cin, (w.data_ptr(), O, I, 1 if transpose_flip else 0))


def q8_eligible(cout: int, cin: int) -> bool:
    return cout == cin and cout in (144, 112)


_Q8_DESC = hip.ConvQ8Desc()


def conv_q8_forward(src: torch.Tensor, pw: PackedQ8, bias: Optional[torch.Tensor], N: int, H: int, W: int, act: int = hip.ACT_NONE,
                    slope: float = 0.0, alpha: float = 1.0, res: Optional[torch.Tensor] = None, want_bf16: bool = True, want_q8: bool = True,
                    out: Optional[torch.Tensor] = None, outq: Optional[torch.Tensor] = None):
    """[res +] alpha * act(conv3x3(src records) + bias) -> (bf16 (N,H,W,Cout) or None, records (N,H,W,rec) or None) (vmg_convq8_fwd).
    out / outq: the caller's bf16 rows / contiguous record buffer, used instead of a fresh allocation."""
    hip.require_cuda(src, bias, res, out, outq)
    rec_in, rec_out = q8_record_bytes(pw.cin), q8_record_bytes(pw.cout)
    if src.dtype != torch.uint8 or not src.is_contiguous() or src.shape[-1] != rec_in or src.numel() != N * H * W * rec_in:
        raise HipError(f"conv_q8: contiguous uint8 records (N*H*W, {rec_in}) expected, got {tuple(src.shape)}")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != pw.cout or not bias.is_contiguous()):
        raise HipError("conv_q8: bias must be contiguous fp32 of length Cout")
    if res is not None and (res.dtype != torch.bfloat16 or res.shape[-1] != pw.cout or res.numel() // pw.cout != N * H * W):
        raise HipError("conv_q8: the residual must be a bf16 tensor of the output's shape")
    if outq is not None and (outq.dtype != torch.uint8 or not outq.is_contiguous() or outq.shape[-1] != rec_out or outq.numel() != N * H * W * rec_out):
        raise HipError(f"conv_q8: outq must be contiguous uint8 records (N*H*W, {rec_out}), got {tuple(outq.shape)}")
    o = oq = None
    if want_bf16:
        o = out if out is not None else torch.empty((N, H, W, pw.cout), dtype=torch.bfloat16, device=src.device)
    if want_q8:
        oq = outq if outq is not None else torch.empty((N, H, W, rec_out), dtype=torch.uint8, device=src.device)
    d = _Q8_DESC
    d.N, d.H, d.W, d.Cin, d.Cout = N, H, W, pw.cin, pw.cout
    d.src, d.packed, d.bias = src.data_ptr(), pw.buf.data_ptr(), bias.data_ptr() if bias is not None else None
    d.out, d.out_ps = (o.data_ptr(), _pix_stride(o)) if o is not None else (None, 0)
    d.outq = oq.data_ptr() if oq is not None else None
    d.res, d.res_ps = (res.data_ptr(), _pix_stride(res)) if res is not None else (None, 0)
    d.act, d.slope, d.alpha = act, slope, alpha
    hip.check(hip.lib().vmg_convq8_fwd(ctypes.byref(d), hip.stream_ptr()), "vmg_convq8_fwd")
    return o, oq


def resblock_chain_forward_q8(y0: torch.Tensor, pw1, b1, pw2, b2, r_scaling: float, keep_t: bool):
    """The fp8 part of a residual chain as ONE C call (vmg_resblock_chain_fwd_q8): y0 (N,H,W,C) bf16 -> (ys, ts); ts entries are None when not kept."""
    hip.require_cuda(y0, *b1, *b2)
    N, H, W, C = y0.shape
    nblk = len(pw1)
    if y0.dtype != torch.bfloat16 or not y0.is_contiguous() or len(pw2) != nblk or any(p.cout != C or p.cin != C for p in list(pw1) + list(pw2)):
        raise HipError("resblock_chain_forward_q8: contiguous bf16 y0 and C -> C fp8 packs expected")
    for b in list(b1) + list(b2):
        if b.dtype != torch.float32 or b.numel() != C or not b.is_contiguous():
            raise HipError("resblock_chain_forward_q8: biases must be contiguous fp32 of length C")
    rec = q8_record_bytes(C)
    q = q8_quantize(y0)
    qb = torch.empty((N, H, W, rec), dtype=torch.uint8, device=y0.device)
    blk = torch.empty((nblk * (2 if keep_t else 1), N, H, W, C), dtype=torch.bfloat16, device=y0.device).unbind(0)
    ys = [y0] + list(blk[:nblk])
    ts = list(blk[nblk:]) if keep_t else [None] * nblk
    d = hip.ChainQ8Desc()
    d.N, d.H, d.W, d.C, d.nblk = N, H, W, C, nblk
    d.q0, d.qa, d.qb = q.data_ptr(), q.data_ptr(), qb.data_ptr()
    keep = [_parr([p.buf for p in pw1]), _parr(list(b1)), _parr([p.buf for p in pw2]), _parr(list(b2)), _parr(ys), _parr(ts) if keep_t else None]
    d.packed1, d.bias1, d.packed2, d.bias2, d.y = keep[:5]
    if keep_t:
        d.t = keep[5]
    d.r_scaling = r_scaling
    hip.check(hip.lib().vmg_resblock_chain_fwd_q8(ctypes.byref(d), hip.stream_ptr()), "vmg_resblock_chain_fwd_q8")
    return ys, ts


def gaussian_window(ksize: int = 11, sigma: float = 1.5):
    """cv2.getGaussianKernel(ksize, sigma) for the sizes that have no fixed table: exp(-x^2 / (2 sigma^2)) in float64, scaled by the
    reciprocal of the sum (utils/metrics.py:56)."""
    import math
    t = [math.exp(-0.5 / (sigma * sigma) * (i - (ksize - 1) * 0.5) ** 2) for i in range(ksize)]
    s = 1.0 / sum(t)
    return [v * s for v in t]


def frame_metrics_sums(a: torch.Tensor, b: torch.Tensor, ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """vmg_frame_metrics on two uint8 (T, 3, H, W) VIEWS of any strides (planar or interleaved storage, crops, frame subsets): returns the
    device tensors sse_rgb (T) int64 and sums (T, 5) float64 = [SSE of Y, SSIM map sums of R, G, B, Y].  Nothing is synchronised."""
    hip.require_cuda(a, b, ws)
    if a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise HipError(f"frame_metrics: uint8 frames expected, got {a.dtype} and {b.dtype}")
    if a.dim() != 4 or a.shape[1] != 3 or a.shape != b.shape:
        raise HipError(f"frame_metrics: two (T, 3, H, W) views of one shape expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    T, _, H, W = a.shape
    lib = hip.lib()
    need = int(lib.vmg_frame_metrics_ws_bytes(T, H, W))
    if ws is None and need > 0:
        ws = torch.empty(need, dtype=torch.uint8, device=a.device)
    sse = torch.empty(T, dtype=torch.int64, device=a.device)
    sums = torch.empty((T, 5), dtype=torch.float64, device=a.device)
    sa, sb = (ctypes.c_int64 * 4)(*a.stride()), (ctypes.c_int64 * 4)(*b.stride())
    win = (ctypes.c_double * 11)(*gaussian_window(11, 1.5))
    hip.check(lib.vmg_frame_metrics(a.data_ptr(), sa, b.data_ptr(), sb, T, H, W, win, ws.data_ptr() if ws is not None else None,
                                    ws.numel() if ws is not None else 0, sse.data_ptr(), sums.data_ptr(), hip.stream_ptr()), "vmg_frame_metrics")
    return sse, sums


LR_OUT_TYPES = {torch.uint8: 0, torch.float32: 1, torch.bfloat16: 2, torch.float64: 3}  # VMG_LR_* of include/vmg_hip.h


def bicubic_down(view: torch.Tensor, s: int, out_dtype: torch.dtype = torch.uint8) -> torch.Tensor:
    """vmg_bicubic_down on a uint8 (T, 3, H, W) VIEW of any strides (planar or interleaved storage, crops, frame subsets): the contiguous
    planar (T, 3, H/s, W/s) result as out_dtype (uint8, float32, bfloat16: the stored byte, / 255 for the float types; float64: unrounded,
    0..255).  One launch, no workspace, nothing is synchronised."""
    hip.require_cuda(view)
    if view.dtype != torch.uint8:
        raise HipError(f"bicubic_down: uint8 frames expected, got {view.dtype}")
    if view.dim() != 4 or view.shape[1] != 3:
        raise HipError(f"bicubic_down: a (T, 3, H, W) view expected, got {tuple(view.shape)}")
    if out_dtype not in LR_OUT_TYPES:
        raise HipError(f"bicubic_down: out_dtype must be uint8, float32, bfloat16 or float64, got {out_dtype}")
    s = int(s)
    T, _, H, W = view.shape
    out = torch.empty((T, 3, H // s if s > 0 else 0, W // s if s > 0 else 0), dtype=out_dtype, device=view.device)
    strides = (ctypes.c_int64 * 4)(*view.stride())
    hip.check(hip.lib().vmg_bicubic_down(view.data_ptr(), strides, T, H, W, s, LR_OUT_TYPES[out_dtype], out.data_ptr(), hip.stream_ptr()),
              "vmg_bicubic_down")
    return out


CROP_OUT_TYPES = {torch.uint8: 0, torch.float32: 1, torch.bfloat16: 2}  # VMG_CROP_* of include/vmg_hip.h


def crop_batch(frames: torch.Tensor, strides: Sequence[int], desc: torch.Tensor, H: int, W: int, ch: int, cw: int, channel_reverse: bool,
               out: torch.Tensor) -> torch.Tensor:
    """vmg_crop_batch: frames = device int64 (N) absolute addresses of uint8 H x W x 3 frames that share the byte strides (row, pixel,
    channel); desc = device int32 (N, 3) {y0, x0, hflip | vflip << 1 | rot << 2}; out = contiguous (N, 3, ch, cw) or any contiguous tensor
    of that many uint8 / float32 / bfloat16 elements, written in place.  The kernel trusts the descriptors (vmg_amd.batches checks them
    on the host).  One launch, no workspace, nothing is synchronised."""
    hip.require_cuda(frames, desc, out)
    if frames.dtype != torch.int64 or frames.dim() != 1 or not frames.is_contiguous():
        raise HipError(f"crop_batch: a contiguous int64 (N) table of frame addresses expected, got {frames.dtype} {tuple(frames.shape)}")
    N = frames.shape[0]
    if desc.dtype != torch.int32 or tuple(desc.shape) != (N, 3) or not desc.is_contiguous():
        raise HipError(f"crop_batch: a contiguous int32 ({N}, 3) descriptor table expected, got {desc.dtype} {tuple(desc.shape)}")
    if out.dtype not in CROP_OUT_TYPES:
        raise HipError(f"crop_batch: the output must be uint8, float32 or bfloat16, got {out.dtype}")
    if not out.is_contiguous() or out.numel() != N * 3 * ch * cw:
        raise HipError(f"crop_batch: a contiguous output of {N} x 3 x {ch} x {cw} elements expected, got {tuple(out.shape)}")
    st = (ctypes.c_int64 * 3)(*[int(s) for s in strides])
    hip.check(hip.lib().vmg_crop_batch(frames.data_ptr(), st, desc.data_ptr(), N, int(H), int(W), int(ch), int(cw), int(bool(channel_reverse)),
                                       CROP_OUT_TYPES[out.dtype], out.data_ptr(), hip.stream_ptr()), "vmg_crop_batch")
    return out


HR_TYPES = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2}  # VMG_HR_* of include/vmg_hip.h


def _frame_stride(t: torch.Tensor, what: str) -> int:
    """Element stride between the frames of a (n, ...) VIEW whose frames are dense runs (a window cut from a longer clip is one)."""
    if not t[0].is_contiguous():
        raise HipError(f"{what}: every frame must be a dense run of elements, got strides {tuple(t.stride())} for {tuple(t.shape)}")
    return int(t.stride(0)) if t.shape[0] > 1 else 0


def frame_sqerr_ws_bytes(n: int, C: int, h: int, w: int) -> int:
    return int(hip.lib().vmg_frame_sqerr_ws_bytes(int(n), int(C), int(h), int(w)))


def frame_sqerr(out: torch.Tensor, hr: torch.Tensor, ws: Optional[torch.Tensor] = None, err: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vmg_frame_sqerr: err[f] = float64 mean of (clamp(out[f], 0, 1) - clamp(hr[f], 0, 1))^2.  out: (n, C, h, w) fp32 / bf16 view with dense frames;
    hr: the same shape in fp32 / bf16, or (n, h, w, 3) uint8 read as byte / 255.  ws: at least frame_sqerr_ws_bytes(n, C, h, w) bytes; err: (>= n)
    float64, the first n entries are written and returned.  Two launches, nothing is synchronised."""
    hip.require_cuda(out, hr, ws, err)
    if out.dim() != 4 or out.dtype not in (torch.float32, torch.bfloat16):
        raise HipError(f"frame_sqerr: out must be (n, C, h, w) fp32 or bf16, got {out.dtype} {tuple(out.shape)}")
    n, C, h, w = out.shape
    if hr.dtype not in HR_TYPES:
        raise HipError(f"frame_sqerr: hr must be fp32, bf16 or uint8, got {hr.dtype}")
    want = (n, h, w, 3) if hr.dtype == torch.uint8 else (n, C, h, w)
    if tuple(hr.shape) != want or (hr.dtype == torch.uint8 and C != 3):
        raise HipError(f"frame_sqerr: hr must be {want} for out {tuple(out.shape)}, got {tuple(hr.shape)}")
    need = frame_sqerr_ws_bytes(n, C, h, w)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=out.device)
    if err is None:
        err = torch.empty(n, dtype=torch.float64, device=out.device)
    if err.dtype != torch.float64 or not err.is_contiguous() or err.numel() < n:
        raise HipError("frame_sqerr: err must be a contiguous float64 tensor of at least n entries")
    if not ws.is_contiguous():
        raise HipError("frame_sqerr: the workspace must be contiguous")
    hip.check(hip.lib().vmg_frame_sqerr(hip.dtype_code(out.dtype), out.data_ptr(), _frame_stride(out, "frame_sqerr"), HR_TYPES[hr.dtype], hr.data_ptr(),
                                        _frame_stride(hr, "frame_sqerr"), n, C, h, w, ws.data_ptr(), ws.numel() * ws.element_size(), err.data_ptr(),
                                        hip.stream_ptr()), "vmg_frame_sqerr")
    return err[:n]


def best_window_select(out: torch.Tensor, err: torch.Tensor, t0: int, window: int, cap: float, canvas: torch.Tensor, best_in: torch.Tensor,
                       choice_in: torch.Tensor, best_out: torch.Tensor, choice_out: torch.Tensor, table: Optional[torch.Tensor] = None) -> None:
    """vmg_best_window_select: the n frames of `out` ((n, C, h, w) fp32 / bf16, dense frames) are frames t0 .. t0 + n - 1 of the (T, C, h, w) fp32
    canvas.  A frame whose float32 score (from err, `cap` where err == 0) beats best_in strictly -- every frame when window == 0 -- is copied into
    its slot; best / choice (T fp32 / int32 each) move from *_in to *_out.  table: None or (T, n_windows) fp32.  One launch, no synchronisation."""
    hip.require_cuda(out, err, canvas, best_in, choice_in, best_out, choice_out, table)
    if out.dim() != 4 or canvas.dim() != 4 or out.shape[1:] != canvas.shape[1:]:
        raise HipError(f"best_window_select: frames {tuple(out.shape)} do not fit the canvas {tuple(canvas.shape)}")
    if canvas.dtype != torch.float32 or not canvas.is_contiguous():
        raise HipError("best_window_select: the canvas must be contiguous fp32")
    n, T = out.shape[0], canvas.shape[0]
    if err.dtype != torch.float64 or not err.is_contiguous() or err.numel() < n:
        raise HipError("best_window_select: err must be a contiguous float64 tensor of at least n entries")
    for name, t, dt in (("best_in", best_in, torch.float32), ("best_out", best_out, torch.float32), ("choice_in", choice_in, torch.int32),
                        ("choice_out", choice_out, torch.int32)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() != T:
            raise HipError(f"best_window_select: {name} must be a contiguous {dt} tensor of {T} entries")
    if table is not None and (table.dtype != torch.float32 or not table.is_contiguous() or table.dim() != 2 or table.shape[0] != T):
        raise HipError(f"best_window_select: the table must be a contiguous fp32 ({T}, n_windows) tensor")
    n_windows = int(table.shape[1]) if table is not None else int(window) + 1
    hip.check(hip.lib().vmg_best_window_select(hip.dtype_code(out.dtype), out.data_ptr(), _frame_stride(out, "best_window_select"), err.data_ptr(), n,
                                               out[0].numel(), T, int(t0), int(window), float(cap), canvas.data_ptr(), best_in.data_ptr(),
                                               choice_in.data_ptr(), best_out.data_ptr(), choice_out.data_ptr(),
                                               table.data_ptr() if table is not None else None, n_windows, hip.stream_ptr()), "vmg_best_window_select")


FRAME_TYPES = {torch.uint8: 0, torch.float32: 1, torch.bfloat16: 2}  # VMG_FRAME_* of include/vmg_hip.h


def convert_frames(src: torch.Tensor, dst: torch.Tensor, hflip: bool = False, vflip: bool = False, rot90: bool = False) -> torch.Tensor:
    """vmg_convert_frames on two (T, 3, h, w) VIEWS of any strides (planar or interleaved storage, frame subsets, crops): dst = Tester.augment
    of src (flip width, flip height, swap the axes) converted uint8 -> fp32 / bf16 (byte / 255), fp32 / bf16 -> uint8 (clamp, * 255, round
    half to even) or uint8 -> uint8.  dst is (T, 3, w, h) with rot90.  One launch, no workspace, nothing is synchronised."""
    hip.require_cuda(src, dst)
    if src.dtype not in FRAME_TYPES or dst.dtype not in FRAME_TYPES:
        raise HipError(f"convert_frames: uint8, float32 and bfloat16 are the element types, got {src.dtype} -> {dst.dtype}")
    if src.dim() != 4 or src.shape[1] != 3:
        raise HipError(f"convert_frames: a (T, 3, H, W) source view expected, got {tuple(src.shape)}")
    T, _, H, W = src.shape
    want = (T, 3, W, H) if rot90 else (T, 3, H, W)
    if tuple(dst.shape) != want:
        raise HipError(f"convert_frames: the destination view must be {want}, got {tuple(dst.shape)}")
    flags = int(bool(hflip)) | int(bool(vflip)) << 1 | int(bool(rot90)) << 2
    ss, ds = (ctypes.c_int64 * 4)(*src.stride()), (ctypes.c_int64 * 4)(*dst.stride())
    hip.check(hip.lib().vmg_convert_frames(FRAME_TYPES[src.dtype], src.data_ptr(), ss, FRAME_TYPES[dst.dtype], dst.data_ptr(), ds, T, H, W, flags,
                                           hip.stream_ptr()), "vmg_convert_frames")
    return dst


def grad_pack_bf16(g: torch.Tensor, out: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """vmg_grad_pack_bf16: out = bfloat16(g * scale) over two flat contiguous buffers of one length (fp32 in, bf16 out), round to nearest
    even.  The payload of the staged data-parallel exchange (train.GradBucketReducer.exchange); one launch, nothing is synchronised."""
    hip.require_cuda(g, out)
    if g.dtype != torch.float32 or out.dtype != torch.bfloat16 or g.dim() != 1 or out.shape != g.shape or not (g.is_contiguous() and out.is_contiguous()):
        raise HipError("grad_pack_bf16: a flat fp32 buffer and a flat bfloat16 buffer of the same length expected")
    hip.check(hip.lib().vmg_grad_pack_bf16(g.data_ptr(), out.data_ptr(), g.numel(), float(scale), hip.stream_ptr()), "vmg_grad_pack_bf16")
    return out


def grad_unpack_bf16(payload: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """vmg_grad_unpack_bf16: g = float(payload), the inverse walk of grad_pack_bf16."""
    hip.require_cuda(payload, g)
    if g.dtype != torch.float32 or payload.dtype != torch.bfloat16 or g.dim() != 1 or payload.shape != g.shape or not (g.is_contiguous() and payload.is_contiguous()):
        raise HipError("grad_unpack_bf16: a flat bfloat16 buffer and a flat fp32 buffer of the same length expected")
    hip.check(hip.lib().vmg_grad_unpack_bf16(payload.data_ptr(), g.data_ptr(), g.numel(), hip.stream_ptr()), "vmg_grad_unpack_bf16")
    return g
