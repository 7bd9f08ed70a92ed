"""Writes tests/golden/shift_ffn.npz: what the REFERENCE computes for its patch-shift FFN (models/function.py PatchShift2D :197-236 and
Mlp_cnn_shift :239-279, models/vmg.py with ffn_type='ffn_cnn_shift'; imported unmodified at run time with oracle/_standins on the path).
Build container only; TEST INFRASTRUCTURE.  Only data is recorded: seeds, shapes, state-dict key lists and output numbers.  Inputs are seeded
(oracle/recipe.py) and weights come by recipe from the state-dict shapes the reference's modules report, so the tests rebuild both.

  (a) PatchShift2D(inv=False) and (inv=True) on a seeded tensor of each small shape (N, H, W, Cs) of SHIFT_SHAPES, fed as (1, N, H, W, Cs).  Stored whole.
  (b) Mlp_cnn_shift(in_features=C, exp_r=r) at (C, r) of MODULES on a seeded (2, 2, 5, 6, C) input: the output, the input gradient for a seeded
      dout, and every parameter gradient.  Stored whole, but for the three hidden-width weight gradients of (112, 6) (75 264 elements each): of
      those every BIG_STRIDE-th element of the flattened tensor and its float64 checksums (sum, sum of magnitudes), which keeps the file small.
  (c) the tiny few-levels VMG (oracle/cases.py cfg_tiny_few, T = 3, 64 x 64) with ffn_type='ffn_cnn_shift': output (strided subsample + float64
      checksums of oracle/cases.py), state-dict shapes and key list.

    VMG_REFERENCE=<path of the reference checkout> python tools/gen_shift_ffn_golden.py
"""
import dataclasses
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
SHIFT_SHAPES = [(1, 1, 1, 9), (2, 1, 5, 4), (2, 5, 1, 10), (3, 2, 2, 16), (2, 3, 7, 19), (2, 9, 11, 32), (2, 4, 4, 144), (1, 6, 5, 288), (1, 3, 3, 112),
                (1, 3, 3, 672)]
SHIFT_SEED = 510
MODULES = [(16, 2), (19, 2), (112, 6)]
MODULE_X = [2, 2, 5, 6]
MODULE_SEED = 520
TINY = dict(T=3, seed=140)
BIG, BIG_STRIDE = 60000, 5  # a tensor of more than BIG elements is recorded as flat[::BIG_STRIDE] + checksums


def import_reference():
    if not os.path.isdir(REF):
        raise SystemExit("reference not present: the fixture can only be regenerated in the build container")
    sys.path.insert(0, os.path.join(ROOT, "oracle", "_standins"))
    sys.path.insert(1, REF)
    warnings.filterwarnings("ignore")
    import models.function as Fn  # noqa
    import models.vmg as V  # noqa
    return Fn, V


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


def main():
    Fn, V = import_reference()
    torch.manual_seed(0)
    data, meta = {}, {"shift_shapes": [list(s) for s in SHIFT_SHAPES], "shift_seed": SHIFT_SEED, "modules": {}, "tiny": TINY, "big": BIG,
                      "big_stride": BIG_STRIDE}
    for i, shp in enumerate(SHIFT_SHAPES):
        name = "x".join(map(str, shp))
        x = R.seeded(shp, SHIFT_SEED + i)
        for inv in (False, True):
            y = Fn.PatchShift2D(inv=inv)(x[None])[0]
            data[f"shift/{name}/{'inv' if inv else 'fwd'}"] = y.numpy().copy()
        print("shift", name, float(x.abs().max()))

    for j, (c, r) in enumerate(MODULES):
        m = Fn.Mlp_cnn_shift(in_features=c, exp_r=r)
        shapes = load_recipe(m)
        seed = MODULE_SEED + 10 * j
        xs = MODULE_X + [c]
        x, dout = R.seeded(xs, seed).requires_grad_(True), R.seeded(xs, seed + 1)
        out = m(x)
        out.backward(dout)
        key = f"{c}_{r}"
        meta["modules"][key] = dict(C=c, r=r, shapes=shapes, keys=list(m.state_dict().keys()), x_shape=xs, seed=seed)
        data[f"module/{key}/out"], data[f"module/{key}/dx"] = out.detach().numpy().copy(), x.grad.numpy().copy()
        for k, p in m.named_parameters():
            if p.grad.numel() > BIG:
                data[f"module/{key}/grad/{k}/sub"] = p.grad.reshape(-1)[::BIG_STRIDE].numpy().copy()
                data[f"module/{key}/grad/{k}/sums"] = np.array(C.checksums(p.grad), dtype=np.float64)
            else:
                data[f"module/{key}/grad/{k}"] = p.grad.numpy().copy()
        print("module", key, float(out.abs().max()), float(x.grad.abs().max()))

    from oracle import gen_golden as G
    cfg = dataclasses.replace(C.cfg_tiny_few(TINY["T"]), ffn_type="ffn_cnn_shift")
    chunk_of, window_of = R.vmg_chunk_lookup(cfg)
    m = G._vmg_from_cfg(V, cfg)
    meta["tiny_shapes"] = load_recipe(m, chunk_of=chunk_of, window_of=window_of)
    meta["tiny_keys"] = list(m.state_dict().keys())
    meta["tiny_ffn_class"] = sorted({type(t.channel_mixing).__name__ for t in m.modules() if hasattr(t, "channel_mixing")})
    with torch.no_grad():
        o = m(R.synthetic_clip(1, TINY["T"], 64, 64, TINY["seed"])).float()
    data["tiny/out/sub"] = C.subsample(o)
    data["tiny/out/sums"] = np.array(C.checksums(o), dtype=np.float64)
    data["tiny/out/shape"] = np.array(o.shape, dtype=np.int64)
    print("tiny", tuple(o.shape), len(meta["tiny_keys"]), "state-dict entries", meta["tiny_ffn_class"])

    meta["source"] = "PatchShift2D, Mlp_cnn_shift (models/function.py) and VMG (models/vmg.py) of the reference, imported unmodified"
    data["meta"] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "shift_ffn.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
