"""Helpers of the mixer-gate tests (test infrastructure): the oracle's token mixer restated with the gate as a parameter, the fp64 formulas of the
gate kernels, the fixture, and the product model built with a gate configuration.

GATES names the seven configurations as tools/gen_mixer_gate_golden.py does: name -> (gating, if_symm, symm_act)."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "mixer_gates.npz")
TANH_TREE = os.path.join(HERE, "golden", "mixer_gate_tanh_tree.json")
GATES = {"tanh": (True, True, "tanh"), "sigmoid": (True, True, "sigmoid"), "relu": (True, True, "relu"), "gelu": (True, True, "gelu"),
         "swish": (True, True, "swish"), "asym": (True, False, "tanh"), "none": (False, True, "tanh")}
NEW_GATES = [g for g in GATES if g != "tanh"]
SYMM_ACTS = ["tanh", "sigmoid", "relu", "gelu", "swish"]


def fixture():
    z = np.load(GOLD)
    return z, json.loads(str(z["meta"]))


# ------------------------------------------------------------------------------------------------ formulas (any float dtype; the kernel tests use fp64)
def act_and_derivative(y: torch.Tensor, act: str):
    """(a(y), a'(y)) of a symmetric-gate activation by the config's name (models/vmg.py:265-274)."""
    if act == "tanh":
        t = torch.tanh(y)
        return t, 1 - t * t
    if act == "sigmoid":  # the reference's sigmoid_symm
        s = torch.sigmoid(y)
        return s - 0.5, s * (1 - s)
    if act == "relu":
        return y.clamp_min(0), (y > 0).to(y.dtype)
    if act == "gelu":
        phi = 0.5 * (1 + torch.erf(y / math.sqrt(2.0)))
        return y * phi, phi + y * torch.exp(-0.5 * y * y) / math.sqrt(2 * math.pi)
    if act == "swish":
        s = torch.sigmoid(y)
        return y * s, s * (1 + y * (1 - s))
    raise KeyError(act)


def gate_formulas(a: torch.Tensor, y: torch.Tensor, d: torch.Tensor, act: str, asym: bool):
    """(gate, da, dy) in the inputs' dtype: symmetric (a + y) * act(y); asymmetric silu(a) * gelu(y)."""
    if asym:
        sa, dsa = act_and_derivative(a, "swish")
        gy, dgy = act_and_derivative(y, "gelu")
        return sa * gy, d * gy * dsa, d * sa * dgy
    v, dv = act_and_derivative(y, act)
    return (a + y) * v, d * v, d * (v + (a + y) * dv)


def apply_gate(sd, p, x, y, gate: str):
    """The gate of configuration `gate` on the mixer input x and the projection output y (models/function.py:796-802), torch ops."""
    gating, symm, act = GATES[gate]
    if not gating:
        return y
    if not symm:
        return F.silu(F.linear(x, sd[f"{p}gating_fc.weight"], sd[f"{p}gating_fc.bias"])) * F.gelu(y)
    return (x + y) * act_and_derivative(y, act)[0]


# ------------------------------------------------------------------------------------------------ the oracle's mixer with the gate as a parameter
def morphfc_decay_gated(gate: str):
    """oracle.vmg_oracle.morphfc_decay's signature with the output gate of configuration `gate`: the same op sequence up to the projection (the
    oracle's own helpers), then apply_gate.  monkeypatch.setattr(oracle.vmg_oracle, "morphfc_decay", morphfc_decay_gated(g)) turns O.tab /
    O.vmg_forward into that configuration's oracle: they look the name up at call time."""
    from oracle import vmg_oracle as O

    def morphfc_decay(sd, p, x, chunk_h, chunk_w, mutate=True, call_index=1):
        B, T, H, W, C = x.shape
        Ch = int(math.ceil(C / chunk_h)) * chunk_h
        Cw = int(math.ceil(C / chunk_w)) * chunk_w

        def decayed(name, gname):
            if mutate:
                sd[name].mul_(sd[gname])
                return sd[name]
            wv = sd[name]
            for _ in range(call_index):
                wv = wv * sd[gname]
            return wv

        wh = decayed(f"{p}mlp_h.0.weight", f"{p}gamma_h")
        th = F.relu(F.linear(O.morph_tokens(x, "h", chunk_h, Ch), wh, sd[f"{p}mlp_h.0.bias"])) / Ch
        h = O.morph_untokens(th, "h", chunk_h, Ch, H, W, C)
        ww = decayed(f"{p}mlp_w.0.weight", f"{p}gamma_w")
        tw = F.relu(F.linear(O.morph_tokens(x, "w", chunk_w, Cw), ww, sd[f"{p}mlp_w.0.bias"])) / Cw
        w = O.morph_untokens(tw, "w", chunk_w, Cw, H, W, C)
        if f"{p}mlp_c.0.weight" in sd:
            c = F.relu(F.linear(x, sd[f"{p}mlp_c.0.weight"], sd[f"{p}mlp_c.0.bias"])) / C
        else:
            c = O.rcab(sd, f"{p}mlp_c.", x) / C
        a = (h + w + c).mean((1, 2, 3))
        a = F.linear(a, sd[f"{p}reweight.fc1.weight"], sd[f"{p}reweight.fc1.bias"])
        a = F.linear(F.gelu(a), sd[f"{p}reweight.fc2.weight"], sd[f"{p}reweight.fc2.bias"])
        a = a.reshape(B, C, 3).softmax(-1)[:, None, None, None]
        y = h * a[..., 0] + w * a[..., 1] + c * a[..., 2]
        y = F.linear(y, sd[f"{p}proj.weight"], sd[f"{p}proj.bias"])
        return apply_gate(sd, p, x, y, gate)

    return morphfc_decay


# ------------------------------------------------------------------------------------------------ product models
def vmg_kwargs(cfg, gate: str, compute_dtype=torch.float32, **extra):
    """The keywords of tests.util.build_product with the gate configuration `gate`."""
    ne = cfg.num_enc_layers
    gating, symm, act = GATES[gate]
    return dict(embed_dim=list(cfg.embed_dim), depths=list(cfg.depths), num_heads=list(cfg.num_heads), num_frames=cfg.num_frames,
                window_sizes=[list(w) for w in cfg.window_sizes], mdsc=cfg.mdsc, if_concat=False, mlp_ratio=cfg.mlp_ratio,
                n_groups=cfg.n_groups, spynet_pretrained=None, image_size=list(cfg.image_size), is_train=cfg.is_train,
                traj_win=list(cfg.traj_win), traj_keyframes_n=list(cfg.traj_keyframes_n), traj_heads=list(cfg.traj_heads),
                temporal_type=list(cfg.temporal_type), temporal_empty=cfg.temporal_empty, traj_res_n=list(cfg.traj_res_n),
                spatial_type=list(cfg.spatial_type), flow_smooth=cfg.flow_smooth, smooth_region_range=cfg.smooth_region_range,
                gating=gating, symm=symm, symm_act=act, ffn_type=cfg.ffn_type, mixer_type=["mlps"] * ne, mixer_n=[None] * ne,
                r_scaling=cfg.r_scaling, chunk_ratios=list(cfg.chunk_ratios), twins=list(cfg.twins), traj_scale=cfg.traj_scale,
                m_scaling=cfg.m_scaling, if_local_fuse=cfg.if_local_fuse, channel_mixer=cfg.channel_mixer, compute_dtype=compute_dtype, **extra)


def build_product_gated(cfg, gate: str, compute_dtype=torch.float32, device="cuda", **extra):
    import vmg_amd
    m = vmg_amd.VMG(**vmg_kwargs(cfg, gate, compute_dtype, **extra))
    m.spynet = vmg_amd.SPyNet(None)
    return m.to(device) if device else m


def tiny_shapes(meta, gate: str):
    """State-dict shapes of the tiny few-levels model in configuration `gate`: recorded from the reference for 'gelu' and 'asym'; the other
    symmetric activations and 'none' have gelu's keys (no gate has parameters but the asymmetric one)."""
    return meta["tiny_shapes"]["asym" if gate == "asym" else "gelu"]


def tiny_state_dict(meta, gate: str, T=None):
    from oracle import cases as C
    from oracle import recipe as R
    cfg = C.cfg_tiny_few(T or meta["tiny"]["T"])
    chunk_of, window_of = R.vmg_chunk_lookup(cfg)
    return R.recipe_state_dict(tiny_shapes(meta, gate), 0, chunk_of=chunk_of, window_of=window_of), cfg
