"""Writes tests/golden/ltam_max.npz: what the REFERENCE computes in traj_mode 'max' (models/trajectory.py, models/vmg.py, imported
unmodified at run time with oracle/_standins on the path).  Build container only; TEST INFRASTRUCTURE.  Only data is recorded: seeds,
shapes, state-dict key lists and output numbers.  Inputs are seeded (oracle/recipe.py seeded / synthetic_clip, oracle/cases.py
int_locations) and weights come by recipe from the state-dict shapes the reference's modules report, so the tests rebuild both.

  (a) LTAM_multi_head(mode='max') at (n, t, h, w, c) = (2, 3, 9, 7, 32) and (1, 2, 16, 16, 144), locations incl. out-of-range ones: the output and,
      by autograd, the gradients w.r.t. q, keys, vals and anchor for a seeded dout.  The small case is stored whole, the large one as the strided
      subsample + float64 checksums of oracle/cases.py.
  (b) Trajectory_multi_head(embed_dim=32, mode='max', num_blocks=2, frame_stride=2) on a (2, 5, 32, 15, 13) input, flows as in trajectory_c32.
  (c) the tiny few-levels VMG (oracle/cases.py cfg_tiny_few, T = 3, 64 x 64) with traj_mode='max': output and state-dict key list.

    VMG_REFERENCE=<path of the reference checkout> python tools/gen_ltam_max_golden.py
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
LTAM_CASES = [dict(name="ltam_9x7_c32", n=2, t=3, h=9, w=7, c=32, seed=200, whole=True),
              dict(name="ltam_16x16_c144", n=1, t=2, h=16, w=16, c=144, seed=210, whole=False)]
TRAJ = dict(name="trajectory_max_c32", n=2, T=5, h=15, w=13, c=32, seed=225)
TINY = dict(name="vmg_tiny_few_max", T=3, seed=140)


def ltam_inputs(g):
    """The seeded inputs of an (a) case: what tests/ rebuild."""
    n, t, h, w, c, s = g["n"], g["t"], g["h"], g["w"], g["c"], g["seed"]
    return dict(q=R.seeded((n, h, w, c), s), keys=R.seeded((n, t, h, w, c), s + 1), anchor=R.seeded((n, h, w, c), s + 2),
                vals=R.seeded((n, t, h, w, c), s + 3), loc=C.int_locations(n, t, h, w, s + 4), dout=R.seeded((n, h, w, c), s + 5))


def traj_inputs(g):
    n, T, h, w, c, s = g["n"], g["T"], g["h"], g["w"], g["c"], g["seed"]
    return dict(x=R.seeded((n, T, h, w, c), s), ff=R.seeded((n, T - 1, 2, h, w), s + 1, 1.5), fb=R.seeded((n, T - 1, 2, h, w), s + 2, 1.5))


def import_reference():
    if not os.path.isdir(REF):
        raise SystemExit("reference not present: the fixture can only be regenerated in the build container")
    sys.path.insert(0, os.path.join(ROOT, "oracle", "_standins"))
    sys.path.insert(1, REF)
    warnings.filterwarnings("ignore")
    import models.trajectory as Tj  # noqa
    import models.vmg as V  # noqa
    return Tj, V


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


def put(data, name, t, whole):
    t = t.detach().float()
    if whole:
        data[name] = t.numpy().copy()
    else:
        data[name + "/sub"] = C.subsample(t)
        data[name + "/sums"] = np.array(C.checksums(t), dtype=np.float64)
        data[name + "/shape"] = np.array(t.shape, dtype=np.int64)


class _MaxVMG:
    """models.vmg with VMG(...) constructed in traj_mode 'max' (oracle/gen_golden.py's constructor call names 'wins')."""

    def __init__(self, V):
        self.V = V
        self.SPyNet = V.SPyNet

    def VMG(self, **kw):
        kw["traj_mode"] = "max"
        return self.V.VMG(**kw)


def main():
    Tj, V = import_reference()
    torch.manual_seed(0)
    data, meta = {}, {"ltam": LTAM_CASES, "trajectory": TRAJ, "tiny": TINY}
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    nt = lambda t: t.permute(0, 1, 4, 2, 3).contiguous()
    for g in LTAM_CASES:
        m = Tj.LTAM_multi_head(embed_dim=g["c"], stride=4, dim=g["c"], mode="max", head=4, en_field=False, if_scale=True, if_ia=False, twins=[2, 2])
        shapes = load_recipe(m)
        assert sorted(shapes) == ["proj.bias", "proj.weight"], shapes
        inp = ltam_inputs(g)
        leaves = {k: inp[k].clone().requires_grad_(True) for k in ("q", "keys", "vals", "anchor")}
        o = m(nchw(leaves["q"]), nt(leaves["keys"]), nchw(leaves["anchor"]), nt(leaves["vals"]), None, None, inp["loc"], g["t"])
        o = o.permute(0, 2, 3, 1)
        o.backward(inp["dout"])
        put(data, g["name"] + "/out", o, g["whole"])
        for k, v in leaves.items():
            put(data, g["name"] + "/d" + k, v.grad, g["whole"])
        print(g["name"], tuple(o.shape), float(o.abs().max()))
    g = TRAJ
    m = Tj.Trajectory_multi_head(embed_dim=g["c"], mode="max", num_blocks=2, frame_stride=2, traj_win=16, head=4, en_field=False, head_scale=True,
                                 feature_refine=None, r_scaling=0.1, twins=[2, 2], ltam=True)
    meta["trajectory_shapes"] = load_recipe(m)
    inp = traj_inputs(g)
    with torch.no_grad():
        o = m(inp["x"].permute(0, 1, 4, 2, 3).contiguous(), inp["ff"], inp["fb"]).permute(0, 1, 3, 4, 2).contiguous()
    put(data, g["name"] + "/out", o, False)
    print(g["name"], tuple(o.shape), float(o.abs().max()))

    from oracle import gen_golden as G
    cfg = C.cfg_tiny_few(TINY["T"])
    chunk_of, window_of = R.vmg_chunk_lookup(cfg)
    m = G._vmg_from_cfg(_MaxVMG(V), cfg)
    meta["tiny_shapes"] = load_recipe(m, chunk_of=chunk_of, window_of=window_of)
    meta["tiny_keys"] = list(m.state_dict().keys())
    with torch.no_grad():
        o = m(R.synthetic_clip(1, TINY["T"], 64, 64, TINY["seed"]))
    put(data, TINY["name"] + "/out", o, False)
    print(TINY["name"], tuple(o.shape), len(meta["tiny_keys"]), "state-dict entries")

    meta["source"] = "LTAM_multi_head / Trajectory_multi_head (models/trajectory.py) and VMG (models/vmg.py) of the reference, mode 'max', imported unmodified"
    data["meta"] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "ltam_max.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
