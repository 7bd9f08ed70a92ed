"""Helpers of the traj_mode 'max' tests (test infrastructure): the product model built in that mode, and the oracle's attention step in that mode."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import ltam_max_ref as MR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ltam_max.npz")


def fixture():
    z = np.load(GOLD)
    return z, json.loads(str(z["meta"]))


def build_product_max(cfg, compute_dtype=torch.float32, device="cuda", **extra):
    """tests.util.build_product with traj_mode='max' (and any further VMG keyword)."""
    import vmg_amd
    ne = cfg.num_enc_layers
    m = vmg_amd.VMG(embed_dim=list(cfg.embed_dim), depths=list(cfg.depths), num_heads=list(cfg.num_heads), num_frames=cfg.num_frames,
                    window_sizes=[list(w) for w in cfg.window_sizes], mdsc=cfg.mdsc, if_concat=False, mlp_ratio=cfg.mlp_ratio,
                    n_groups=cfg.n_groups, spynet_pretrained=None, image_size=list(cfg.image_size), is_train=cfg.is_train,
                    traj_win=list(cfg.traj_win), traj_keyframes_n=list(cfg.traj_keyframes_n), traj_heads=list(cfg.traj_heads),
                    temporal_type=list(cfg.temporal_type), temporal_empty=cfg.temporal_empty, traj_res_n=list(cfg.traj_res_n),
                    spatial_type=list(cfg.spatial_type), flow_smooth=cfg.flow_smooth, smooth_region_range=cfg.smooth_region_range,
                    symm_act="tanh", ffn_type=cfg.ffn_type, mixer_type=["mlps"] * ne, mixer_n=[None] * ne, r_scaling=cfg.r_scaling,
                    chunk_ratios=list(cfg.chunk_ratios), twins=list(cfg.twins), traj_scale=cfg.traj_scale, m_scaling=cfg.m_scaling,
                    if_local_fuse=cfg.if_local_fuse, channel_mixer=cfg.channel_mixer, compute_dtype=compute_dtype, traj_mode="max", **extra)
    m.spynet = vmg_amd.SPyNet(None)
    return m.to(device) if device else m


def ltam_max_oracle(sd, p, q, keys, anchor, vals, loc, heads, twins, scale_on=True):
    """oracle.vmg_oracle.ltam_wins' signature, mode 'max': tests/ltam_max_ref.torch_forward (differentiable, in the inputs' dtype), the output
    projection and the anchor.  monkeypatch.setattr(oracle.vmg_oracle, "ltam_wins", ltam_max_oracle) turns O.trajectory / O.vmg_forward into the
    max-mode oracle: they look the name up at call time."""
    att, _ = MR.torch_forward(q, list(keys.unbind(1)), list(vals.unbind(1)), loc, heads)
    return F.linear(att, sd[f"{p}proj.weight"], sd[f"{p}proj.bias"]) + anchor


def tiny_state_dict(meta):
    """The recipe weights of the recorded tiny max-mode model (its state-dict shapes are in the fixture)."""
    from oracle import cases as C
    from oracle import recipe as R
    cfg = C.cfg_tiny_few(meta["tiny"]["T"])
    chunk_of, window_of = R.vmg_chunk_lookup(cfg)
    return R.recipe_state_dict(meta["tiny_shapes"], 0, chunk_of=chunk_of, window_of=window_of)
