"""Helpers of the MBConv mixer tests (test infrastructure): the depthwise 3x3 convolution with its two ReLU6 and its three gradients restated
with shifted slices (any float dtype; the tests use fp64), the inverted-residual block and the mixer built on it, the fixture
tools/gen_mbconv_golden.py recorded from the reference, and the product model built with mixer_type entries 'mbconv'."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "mbconv.npz")
MODULES = [(16, 2), (20, 1), (112, 1)]  # (C, blocks) of the recorded Multi_MBConv cases
TINY_MODELS = ["mbconv_mbconv", "mbconv_mlps"]


def fixture():
    z = np.load(GOLD)
    return z, json.loads(str(z["meta"]))


# ------------------------------------------------------------------------------------------------ the depthwise convolution, restated
def relu6(v):
    return v.clamp(0, 6)


def relu6_grad(v):
    """torch's: 1 only where 0 < v < 6, strictly."""
    return ((v > 0) & (v < 6)).to(v.dtype)


def _act(v, act):
    return relu6(v) if act == "relu6" else v


def _act_grad(v, act):
    return relu6_grad(v) if act == "relu6" else torch.ones_like(v)


def _taps(H, W):
    """(ky, kx, destination rows, destination columns, source rows, source columns) of the in-image part of every tap: destination pixel (y, x)
    reads source pixel (y + ky - 1, x + kx - 1)."""
    for ky in range(3):
        for kx in range(3):
            y0, y1 = max(0, 1 - ky), min(H, H + 1 - ky)
            x0, x1 = max(0, 1 - kx), min(W, W + 1 - kx)
            if y0 < y1 and x0 < x1:
                yield ky, kx, slice(y0, y1), slice(x0, x1), slice(y0 + ky - 1, y1 + ky - 1), slice(x0 + kx - 1, x1 + kx - 1)


def dwconv3(e, w, b, src_act=None, act=None, pre=False):
    """a = act( sum_k w[c, ky, kx] * src_act(e)[y + ky - 1, x + kx - 1, c] + b[c] ) on (..., H, W, C), zero padding; w (C, 1, 3, 3).  pre: the
    pre-activation sum instead."""
    H, W = e.shape[-3:-1]
    s = _act(e, src_act)
    out = torch.zeros_like(e)
    for ky, kx, dy, dx, sy, sx in _taps(H, W):
        out[..., dy, dx, :] += w[:, 0, ky, kx] * s[..., sy, sx, :]
    out = out + b
    return out if pre else _act(out, act)


def dwconv3_grads(e, w, a, da, src_act=None, act=None):
    """(de, dW, db) of dwconv3 for the output gradient da; the output's ReLU6 derivative is taken from a, the (stored) output."""
    H, W = e.shape[-3:-1]
    g = da * _act_grad(a, act)
    s = _act(e, src_act)
    de = torch.zeros_like(e)
    dW = torch.zeros_like(w)
    lead = tuple(range(e.dim() - 1))
    for ky, kx, dy, dx, sy, sx in _taps(H, W):
        de[..., sy, sx, :] += w[:, 0, ky, kx] * g[..., dy, dx, :]
        dW[:, 0, ky, kx] = (g[..., dy, dx, :] * s[..., sy, sx, :]).sum(lead)
    return de * _act_grad(e, src_act), dW, g.sum(lead)


def abs_term_sums(e, w, b, a, da, src_act=None, act=None):
    """The sums of the MAGNITUDES of the added terms of the forward, the data gradient, dW and db: what the rounding-error bounds scale with."""
    H, W = e.shape[-3:-1]
    g = (da * _act_grad(a, act)).abs()
    s = _act(e, src_act).abs()
    fwd, dat, dW = torch.zeros_like(e), torch.zeros_like(e), torch.zeros_like(w)
    lead = tuple(range(e.dim() - 1))
    for ky, kx, dy, dx, sy, sx in _taps(H, W):
        k = w[:, 0, ky, kx].abs()
        fwd[..., dy, dx, :] += k * s[..., sy, sx, :]
        dat[..., sy, sx, :] += k * g[..., dy, dx, :]
        dW[:, 0, ky, kx] = (g[..., dy, dx, :] * s[..., sy, sx, :]).sum(lead)
    return fwd + b.abs(), dat, dW, g.sum(lead)


# ------------------------------------------------------------------------------------------------ block and mixer (autograd does their gradients)
def block_keys(prefix=""):
    return [f"{prefix}bottleneck.{i}.0.{leaf}" for i in range(3) for leaf in ("weight", "bias")]


def mixer_keys(blocks: int):
    return [k for i in range(blocks) for k in block_keys(f"main.0.{i}.")]


def mixer_shapes(C: int, blocks: int) -> dict:
    M = 4 * C
    one = {"bottleneck.0.0.weight": [M, C, 1, 1], "bottleneck.0.0.bias": [M], "bottleneck.1.0.weight": [M, 1, 3, 3], "bottleneck.1.0.bias": [M],
           "bottleneck.2.0.weight": [C, M, 1, 1], "bottleneck.2.0.bias": [C]}
    return {f"main.0.{i}.{k}": v for i in range(blocks) for k, v in one.items()}


def inverted_residual(sd, p, x):
    """InvertedResidual.forward on x (..., H, W, C): conv1x1 + ReLU6, depthwise conv3x3 + ReLU6, conv1x1, + x."""
    e = F.linear(x, sd[f"{p}bottleneck.0.0.weight"][:, :, 0, 0], sd[f"{p}bottleneck.0.0.bias"])
    a = dwconv3(e, sd[f"{p}bottleneck.1.0.weight"], sd[f"{p}bottleneck.1.0.bias"], "relu6", "relu6")
    return F.linear(a, sd[f"{p}bottleneck.2.0.weight"][:, :, 0, 0], sd[f"{p}bottleneck.2.0.bias"]) + x


def multi_mbconv(sd, p, x):
    """Multi_MBConv.forward: the blocks under {p}main.0. in index order."""
    i = 0
    while f"{p}main.0.{i}.bottleneck.0.0.weight" in sd:
        x = inverted_residual(sd, f"{p}main.0.{i}.", x)
        i += 1
    return x


def module_case(meta, C: int, blocks: int):
    """(state dict, x, dout) of a recorded module case: all rebuilt from the recorded shapes and seeds."""
    from oracle import recipe as R
    m = meta["modules"][f"{C}_{blocks}"]
    return R.recipe_state_dict(m["shapes"], 0), R.seeded(m["x_shape"], m["seed"]), R.seeded(m["x_shape"], m["seed"] + 1)


# ------------------------------------------------------------------------------------------------ product models
def tiny_cfg(T=None):
    from oracle import cases as C
    _, meta = fixture()
    return C.cfg_tiny_few(T or meta["tiny"]["T"])


def vmg_kwargs(cfg, mixer_type, mixer_n, compute_dtype=torch.float32, **extra):
    kw = dict(embed_dim=list(cfg.embed_dim), depths=list(cfg.depths), num_heads=list(cfg.num_heads), num_frames=cfg.num_frames,
              window_sizes=[list(w) for w in cfg.window_sizes], mdsc=cfg.mdsc, if_concat=False, mlp_ratio=cfg.mlp_ratio,
              n_groups=cfg.n_groups, spynet_pretrained=None, image_size=list(cfg.image_size), is_train=cfg.is_train,
              traj_win=list(cfg.traj_win), traj_keyframes_n=list(cfg.traj_keyframes_n), traj_heads=list(cfg.traj_heads),
              temporal_type=list(cfg.temporal_type), temporal_empty=cfg.temporal_empty, traj_res_n=list(cfg.traj_res_n),
              spatial_type=list(cfg.spatial_type), flow_smooth=cfg.flow_smooth, smooth_region_range=cfg.smooth_region_range,
              ffn_type=cfg.ffn_type, mixer_type=list(mixer_type), mixer_n=list(mixer_n), r_scaling=cfg.r_scaling, chunk_ratios=list(cfg.chunk_ratios),
              twins=list(cfg.twins), traj_scale=cfg.traj_scale, m_scaling=cfg.m_scaling, if_local_fuse=cfg.if_local_fuse,
              channel_mixer=cfg.channel_mixer, compute_dtype=compute_dtype)
    kw.update(extra)
    return kw


def build_product(cfg, mixer_type, mixer_n, compute_dtype=torch.float32, device="cuda", **extra):
    """vmg_amd.VMG for cfg with the given mixers and a random-init SPyNet attached."""
    import vmg_amd
    m = vmg_amd.VMG(**vmg_kwargs(cfg, mixer_type, mixer_n, compute_dtype, **extra))
    m.spynet = vmg_amd.SPyNet(None)
    return m.to(device) if device else m


def tiny_state_dict(meta, name, cfg):
    """Recipe state dict of a recorded tiny model from its recorded shapes."""
    from oracle import recipe as R
    chunk_of, window_of = R.vmg_chunk_lookup(cfg)
    return R.recipe_state_dict(meta["tiny_models"][name]["shapes"], 0, chunk_of=chunk_of, window_of=window_of)


def expected_route(C: int, dtype, aligned: bool = True) -> str:
    """The issue's rule: 16-byte vectors where C is a multiple of 8 bf16 / 4 fp32 elements and the pointers are 16-byte aligned."""
    return "vector" if aligned and C % (8 if dtype == torch.bfloat16 else 4) == 0 else "element"
