"""Writes tests/golden/mixer_gates.npz: what the REFERENCE computes for every output gate its token mixer can be configured with
(models/function.py:596-805 Enhanced_MorphFCs_decay, models/vmg.py:265-274; imported unmodified at run time with oracle/_standins on the path).
Build container only; TEST INFRASTRUCTURE.  Only data is recorded: seeds, shapes, state-dict key lists and output numbers.  Inputs are seeded
(oracle/recipe.py) and weights come by recipe from the state-dict shapes the reference's modules report, so the tests rebuild both.

  (a) Enhanced_MorphFCs_decay(dim=16, chunk_h=chunk_w=8, qkv_bias=True, channel_mixer='rcab') in each of the seven gate configurations (GATES) on a
      seeded (2, 2, 10, 12, 16) input: the outputs of calls 1 and 2 (the weight decay is stateful) and, by autograd through call 1, the input
      gradient for a seeded dout.  Stored whole.
  (b) the tiny few-levels VMG (oracle/cases.py cfg_tiny_few, T = 3, 64 x 64) with symm_act='gelu' and with if_symm=False: output (strided subsample
      + float64 checksums of oracle/cases.py), state-dict shapes and key list.

    VMG_REFERENCE=<path of the reference checkout> python tools/gen_mixer_gate_golden.py
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
# name -> (gating, if_symm, symm_act as the YAML spells it)
GATES = {"tanh": (True, True, "tanh"), "sigmoid": (True, True, "sigmoid"), "relu": (True, True, "relu"), "gelu": (True, True, "gelu"),
         "swish": (True, True, "swish"), "asym": (True, False, "tanh"), "none": (False, True, "tanh")}
MIXER = dict(dim=16, chunk=8, shape=[2, 2, 10, 12, 16], seed=410)
TINY = dict(T=3, seed=140, variants=["gelu", "asym"])


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


class _GatedVMG:
    """models.vmg with VMG(...) constructed with one gate configuration (oracle/gen_golden.py's constructor call names the tanh gate)."""

    def __init__(self, V, gate):
        self.V, self.gate = V, gate
        self.SPyNet = V.SPyNet

    def VMG(self, **kw):
        kw["gating"], kw["symm"], kw["symm_act"] = GATES[self.gate]
        return self.V.VMG(**kw)


def main():
    Fn, V = import_reference()
    torch.manual_seed(0)
    data, meta = {}, {"gates": GATES, "mixer": MIXER, "tiny": TINY}
    acts = {"tanh": torch.nn.Tanh, "sigmoid": Fn.sigmoid_symm, "relu": torch.nn.ReLU, "gelu": torch.nn.GELU, "swish": torch.nn.SiLU}  # models/vmg.py:265-274
    x0, dout = R.seeded(MIXER["shape"], MIXER["seed"]), R.seeded(MIXER["shape"], MIXER["seed"] + 1)
    meta["mixer_shapes"], meta["mixer_keys"] = {}, {}
    for name, (gating, symm, act) in GATES.items():
        m = Fn.Enhanced_MorphFCs_decay(dim=MIXER["dim"], chunk_h=MIXER["chunk"], chunk_w=MIXER["chunk"], qkv_bias=True, non_linear=True, gating=gating,
                                       symm=symm, symm_act=acts[act], relu_scale=True, channel_mixer="rcab")
        meta["mixer_shapes"][name] = load_recipe(m, chunk_of=lambda k: MIXER["chunk"])
        meta["mixer_keys"][name] = list(m.state_dict().keys())
        x = x0.clone().requires_grad_(True)
        o1 = m(x)
        o1.backward(dout)
        with torch.no_grad():
            o2 = m(x0.clone())
        data[f"mixer/{name}/out1"], data[f"mixer/{name}/out2"] = o1.detach().numpy().copy(), o2.numpy().copy()
        data[f"mixer/{name}/dx"] = x.grad.numpy().copy()
        print("mixer", name, float(o1.abs().max()), float((o1 - o2).abs().max()), float(x.grad.abs().max()))

    from oracle import gen_golden as G
    cfg = C.cfg_tiny_few(TINY["T"])
    chunk_of, window_of = R.vmg_chunk_lookup(cfg)
    meta["tiny_shapes"], meta["tiny_keys"] = {}, {}
    for name in TINY["variants"]:
        m = G._vmg_from_cfg(_GatedVMG(V, name), cfg)
        meta["tiny_shapes"][name] = load_recipe(m, chunk_of=chunk_of, window_of=window_of)
        meta["tiny_keys"][name] = list(m.state_dict().keys())
        with torch.no_grad():
            o = m(R.synthetic_clip(1, TINY["T"], 64, 64, TINY["seed"])).float()
        data[f"tiny/{name}/out/sub"] = C.subsample(o)
        data[f"tiny/{name}/out/sums"] = np.array(C.checksums(o), dtype=np.float64)
        data[f"tiny/{name}/out/shape"] = np.array(o.shape, dtype=np.int64)
        print("tiny", name, tuple(o.shape), len(meta["tiny_keys"][name]), "state-dict entries")

    meta["source"] = "Enhanced_MorphFCs_decay (models/function.py) and VMG (models/vmg.py) of the reference, imported unmodified"
    data["meta"] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "mixer_gates.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
