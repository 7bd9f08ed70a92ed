"""Helpers of the patch-shift FFN tests (test infrastructure): PatchShift2D in closed form, Mlp_cnn_shift restated with it (any float dtype; the
tests use fp64), the same in the oracle's FFN signature, the fixture tools/gen_shift_ffn_golden.py recorded from the reference, and the product
model built with ffn_type='ffn_cnn_shift'."""
import dataclasses
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "shift_ffn.npz")
FFN = "ffn_cnn_shift"
# (N, H, W, Cs) of the shift cases (the issue's table) and the module cases (C, exp_r)
SHIFT_SHAPES = [(1, 1, 1, 9), (2, 1, 5, 4), (2, 5, 1, 10), (3, 2, 2, 16), (2, 3, 7, 19), (2, 9, 11, 32), (2, 4, 4, 144), (1, 6, 5, 288), (1, 3, 3, 112),
                (1, 3, 3, 672)]
MODULES = [(16, 2), (19, 2), (112, 6)]
KEY_ORDER = ["fc.weight", "fc.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "reweight.fc1.weight", "reweight.fc1.bias",
             "reweight.fc2.weight", "reweight.fc2.bias", "proj.weight", "proj.bias"]


def fixture():
    z = np.load(GOLD)
    return z, json.loads(str(z["meta"]))


def shape_name(shape) -> str:
    return "x".join(str(int(s)) for s in shape)


def expected_route(Cs: int, dtype) -> str:
    """The route the issue's rule gives: the vector path needs the chunk width ceil(Cs / 9) and Cs to be multiples of 8 bf16 / 4 fp32 elements."""
    vec = 8 if dtype == torch.bfloat16 else 4
    g = -(-Cs // 9)
    return "vector" if g % vec == 0 and Cs % vec == 0 else "element"


# ------------------------------------------------------------------------------------------------ the closed forms
def patch_shift(x: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """PatchShift2D on (..., H, W, Cs): out[..., y, x, c] = in[..., y - s (1 - i // 3), x - s (1 - i % 3), c] with i = c // ceil(Cs / 9), zero outside the
    frame; s = +1, or -1 with inverse.  Plain slicing: every value is a copy."""
    H, W, Cs = x.shape[-3:]
    g = -(-Cs // 9)
    s = -1 if inverse else 1
    out = torch.zeros_like(x)
    for i in range(9):
        c0, c1 = i * g, min((i + 1) * g, Cs)
        if c0 >= Cs:
            break
        dy, dx = s * (1 - i // 3), s * (1 - i % 3)
        ys0, ys1 = max(0, -dy), min(H, H - dy)  # source rows ys, destination rows ys + dy
        xs0, xs1 = max(0, -dx), min(W, W - dx)
        if ys0 < ys1 and xs0 < xs1:
            out[..., ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx, c0:c1] = x[..., ys0:ys1, xs0:xs1, c0:c1]
    return out


def gelu_and_derivative(x: torch.Tensor):
    phi = 0.5 * (1 + torch.erf(x / math.sqrt(2.0)))
    return x * phi, phi + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def mlp_cnn_shift(sd, p, x):
    """Mlp_cnn_shift.forward on x (B, T, H, W, C) in the oracle's FFN signature (oracle.vmg_oracle.mlp_vanilla's), in the dtype of x and sd."""
    B, C = x.shape[0], x.shape[-1]
    lin = lambda name, t: F.linear(t, sd[f"{p}{name}.weight"], sd[f"{p}{name}.bias"])
    x1 = F.gelu(lin("fc", x))
    h = patch_shift(F.gelu(lin("fc1", patch_shift(x1))), inverse=True)
    w = F.gelu(lin("fc2", x1))
    a = lin("reweight.fc2", F.gelu(lin("reweight.fc1", (h + w).mean((1, 2, 3)))))
    a = a.reshape(B, C, 2).softmax(-1)[:, None, None, None]
    return lin("proj", h * a[..., 0] + w * a[..., 1])


def reweight_mix2(h, w, fc1w, fc1b, fc2w, fc2b):
    """The two-branch re-weighting alone on (G, R, C) tensors."""
    G, _, C = h.shape
    a = F.linear(F.gelu(F.linear((h + w).mean(1), fc1w, fc1b)), fc2w, fc2b).reshape(G, C, 2).softmax(-1)[:, None]
    return h * a[..., 0] + w * a[..., 1]


def module_shapes(C: int, r) -> dict:
    hid = int(C * r)
    return {"fc.weight": [hid, C], "fc.bias": [hid], "fc1.weight": [C, hid], "fc1.bias": [C], "fc2.weight": [C, hid], "fc2.bias": [C],
            "reweight.fc1.weight": [C // 4, C], "reweight.fc1.bias": [C // 4], "reweight.fc2.weight": [2 * C, C // 4], "reweight.fc2.bias": [2 * C],
            "proj.weight": [C, C], "proj.bias": [C]}


def module_state_dict(shapes: dict):
    from oracle import recipe as R
    return R.recipe_state_dict(shapes, 0)


def module_case(meta, C: int, r):
    """(state dict, x, dout) of a recorded module case: all rebuilt from the recorded shapes and seeds."""
    from oracle import recipe as R
    m = meta["modules"][f"{C}_{r}"]
    return module_state_dict(m["shapes"]), R.seeded(m["x_shape"], m["seed"]), R.seeded(m["x_shape"], m["seed"] + 1)


# ------------------------------------------------------------------------------------------------ product models
def shift_cfg(T=None):
    from oracle import cases as C
    _, meta = fixture()
    return dataclasses.replace(C.cfg_tiny_few(T or meta["tiny"]["T"]), ffn_type=FFN)


def vmg_kwargs(cfg, compute_dtype=torch.float32, **extra):
    ne = cfg.num_enc_layers
    kw = dict(embed_dim=list(cfg.embed_dim), depths=list(cfg.depths), num_heads=list(cfg.num_heads), num_frames=cfg.num_frames,
              window_sizes=[list(w) for w in cfg.window_sizes], mdsc=cfg.mdsc, if_concat=False, mlp_ratio=cfg.mlp_ratio,
              n_groups=cfg.n_groups, spynet_pretrained=None, image_size=list(cfg.image_size), is_train=cfg.is_train,
              traj_win=list(cfg.traj_win), traj_keyframes_n=list(cfg.traj_keyframes_n), traj_heads=list(cfg.traj_heads),
              temporal_type=list(cfg.temporal_type), temporal_empty=cfg.temporal_empty, traj_res_n=list(cfg.traj_res_n),
              spatial_type=list(cfg.spatial_type), flow_smooth=cfg.flow_smooth, smooth_region_range=cfg.smooth_region_range,
              ffn_type=cfg.ffn_type, mixer_type=["mlps"] * ne, mixer_n=[None] * ne, r_scaling=cfg.r_scaling, chunk_ratios=list(cfg.chunk_ratios),
              twins=list(cfg.twins), traj_scale=cfg.traj_scale, m_scaling=cfg.m_scaling, if_local_fuse=cfg.if_local_fuse,
              channel_mixer=cfg.channel_mixer, compute_dtype=compute_dtype)
    kw.update(extra)
    return kw


def build_product_shift(cfg, compute_dtype=torch.float32, device="cuda", **extra):
    """vmg_amd.VMG for cfg (ffn_type as cfg says: shift_cfg() gives 'ffn_cnn_shift') with a random-init SPyNet attached."""
    import vmg_amd
    m = vmg_amd.VMG(**vmg_kwargs(cfg, compute_dtype, **extra))
    m.spynet = vmg_amd.SPyNet(None)
    return m.to(device) if device else m


def tiny_state_dict(meta, cfg, traj_max=False):
    """Recipe state dict of the tiny model from the recorded shapes (ffn_type 'ffn_cnn_shift')."""
    from oracle import recipe as R
    chunk_of, window_of = R.vmg_chunk_lookup(cfg)
    sd = R.recipe_state_dict(meta["tiny_shapes"], 0, chunk_of=chunk_of, window_of=window_of)
    if traj_max:  # (that mode's attention has neither position table nor decay buffer: tests/test_traj_max_gpu.py)
        sd = {k: v for k, v in sd.items() if not k.endswith(("relative_pos_encoding", "decay_v"))}
    return sd
