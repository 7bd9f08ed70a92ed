"""Writes tests/golden/mbconv.npz: what the REFERENCE computes for its MBConv spatial mixer (models/CNNs.py InvertedResidual :159-185 and
Multi_MBConv :187-201, models/vmg.py with mixer_type entries 'mbconv'; imported unmodified at run time with oracle/_standins on the path).
Build container only; TEST INFRASTRUCTURE.  Only data is recorded: seeds, shapes, state-dict key lists and output numbers.  Inputs are seeded
(oracle/recipe.py) and weights come by recipe from the state-dict shapes the reference's modules report, so the tests rebuild both.

  (a) Multi_MBConv(embed_dim=C, expansion_factor=4, stride=1, num_blocks=n) at (C, n) of MODULES on a seeded (2, 2, 5, 6, C) input: the output,
      the input gradient for a seeded dout, and every parameter gradient.  Stored whole (the largest has 50 176 elements).
  (b) the tiny few-levels VMG (oracle/cases.py cfg_tiny_few, T = 3, 64 x 64) with each (mixer_type, mixer_n) of TINY_MODELS: output (strided
      subsample + float64 checksums of oracle/cases.py), state-dict shapes and key list.  The script builds the reference VMG itself:
      oracle/gen_golden._vmg_from_cfg passes 'mlps' for every stage.

    VMG_REFERENCE=<path of the reference checkout> python tools/gen_mbconv_golden.py
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cases as C  # noqa: E402
from oracle import recipe as R  # noqa: E402

REF = os.environ.get("VMG_REFERENCE", "")
MODULES = [(16, 2), (20, 1), (112, 1)]
MODULE_X = [2, 2, 5, 6]
MODULE_SEED = 610
TINY = dict(T=3, seed=150)
TINY_MODELS = {"mbconv_mbconv": (["mbconv", "mbconv"], [2, 2]), "mbconv_mlps": (["mbconv", "mlps"], [1, None])}


def import_reference():
    if not os.path.isdir(REF):
        raise SystemExit("reference not present: the fixture can only be regenerated in the build container")
    sys.path.insert(0, os.path.join(ROOT, "oracle", "_standins"))
    sys.path.insert(1, REF)
    warnings.filterwarnings("ignore")
    import models.CNNs as Cn  # noqa
    import models.vmg as V  # noqa
    return Cn, V


def load_recipe(m, **lookups):
    shapes = {k: list(v.shape) for k, v in m.state_dict().items()}
    sd = R.recipe_state_dict(shapes, 0, **lookups)
    own = m.state_dict()
    for k in sd:
        if R.is_buffer(k):  # keep the reference's own bits (gen_golden.py checks the closed forms)
            sd[k] = own[k].clone()
    m.load_state_dict(sd, strict=True)
    m.eval()
    return shapes


def reference_vmg(V, cfg, mixer_type, mixer_n):
    """The reference's VMG for an oracle config, as oracle/gen_golden._vmg_from_cfg builds it but for mixer_type / mixer_n."""
    ne = cfg.num_enc_layers
    m = V.VMG(embed_dim=list(cfg.embed_dim), depths=list(cfg.depths), num_heads=list(cfg.num_heads), num_frames=cfg.num_frames,
              window_sizes=[list(w) for w in cfg.window_sizes], mdsc=cfg.mdsc, if_concat=False, mlp_ratio=cfg.mlp_ratio, n_groups=cfg.n_groups,
              spynet_pretrained=None, image_size=list(cfg.image_size), is_train=cfg.is_train, ltam=True, traj_win=list(cfg.traj_win),
              traj_keyframes_n=list(cfg.traj_keyframes_n), traj_heads=list(cfg.traj_heads), temporal_type=list(cfg.temporal_type),
              temporal_empty=cfg.temporal_empty, traj_res_n=list(cfg.traj_res_n), spatial_type=list(cfg.spatial_type), flow_smooth=cfg.flow_smooth,
              smooth_region_range=cfg.smooth_region_range, retention_decay=True, non_linear=True, gating=True, symm=True, symm_act="tanh",
              relu_scale=True, relu_scale_norm=False, ffn_type=cfg.ffn_type, mixer_type=list(mixer_type), mixer_n=list(mixer_n),
              r_scaling=cfg.r_scaling, chunk_ratios=list(cfg.chunk_ratios), traj_mode="wins", twins=list(cfg.twins), traj_scale=cfg.traj_scale,
              traj_refine=None, m_scaling=cfg.m_scaling, if_local_fuse=cfg.if_local_fuse, channel_mixer=cfg.channel_mixer,
              deform_groups=[8] * ne, max_residual_scale=[1] * ne)
    m.spynet = V.SPyNet(None)  # a random-init SPyNet attached after construction, as the oracle does
    return m


def main():
    Cn, V = import_reference()
    torch.manual_seed(0)
    data, meta = {}, {"modules": {}, "tiny": TINY, "tiny_models": {}}
    for j, (c, n) in enumerate(MODULES):
        m = Cn.Multi_MBConv(embed_dim=c, expansion_factor=4, stride=1, num_blocks=n)
        shapes = load_recipe(m)
        seed = MODULE_SEED + 10 * j
        xs = MODULE_X + [c]
        x, dout = R.seeded(xs, seed).requires_grad_(True), R.seeded(xs, seed + 1)
        out = m(x)
        out.backward(dout)
        key = f"{c}_{n}"
        meta["modules"][key] = dict(C=c, blocks=n, shapes=shapes, keys=list(m.state_dict().keys()), x_shape=xs, seed=seed)
        data[f"module/{key}/out"], data[f"module/{key}/dx"] = out.detach().numpy().copy(), x.grad.numpy().copy()
        for k, p in m.named_parameters():
            data[f"module/{key}/grad/{k}"] = p.grad.numpy().copy()
        print("module", key, float(out.abs().max()), float(x.grad.abs().max()))

    cfg = C.cfg_tiny_few(TINY["T"])
    chunk_of, window_of = R.vmg_chunk_lookup(cfg)
    for name, (mt, mn) in TINY_MODELS.items():
        m = reference_vmg(V, cfg, mt, mn)
        rec = dict(mixer_type=mt, mixer_n=mn)
        rec["shapes"] = load_recipe(m, chunk_of=chunk_of, window_of=window_of)
        rec["keys"] = list(m.state_dict().keys())
        rec["mixer_classes"] = [type(t.spatial_mixing).__name__ for t in m.modules() if hasattr(t, "spatial_mixing")]
        with torch.no_grad():
            o = m(R.synthetic_clip(1, TINY["T"], 64, 64, TINY["seed"])).float()
        data[f"tiny/{name}/out/sub"] = C.subsample(o)
        data[f"tiny/{name}/out/sums"] = np.array(C.checksums(o), dtype=np.float64)
        data[f"tiny/{name}/out/shape"] = np.array(o.shape, dtype=np.int64)
        meta["tiny_models"][name] = rec
        print("tiny", name, tuple(o.shape), len(rec["keys"]), "state-dict entries", rec["mixer_classes"])

    meta["source"] = "InvertedResidual, Multi_MBConv (models/CNNs.py) and VMG (models/vmg.py) of the reference, imported unmodified"
    data["meta"] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "mbconv.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
