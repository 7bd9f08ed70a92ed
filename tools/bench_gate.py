"""The mixer's gate kernels (vmg_gate_fwd / _bwd / _res_fwd / _res_bwd) for every form and activation, next to the tanh ops of vmg_tab_elementwise
(OP_GATE_* / OP_GATE_RES_*) and next to a device copy that moves the same bytes, in ONE process, at the bench shape of stage 0: 4 x 7 frames of
64 x 64 pixels, 144 channels, bf16.  Stream events around `reps` launches after a warm-up, `rounds` rounds with all candidates ALTERNATING inside
a round; reported: the median over the rounds in us, the rate over the bytes the kernel has to move, and the spread (max - min) / median of the
tanh ops' timing in the same run, which is what a difference has to exceed.  Bytes per call in tensors of the shape (T = rows * C * 2 bytes):
forward 2 in + 1 out = 3T, forward with residual 3 + 1 = 4T, backward 3 + 2 = 5T (the (G, C) coefficient is noise).  The asymmetric kernels move
the same bytes as the symmetric ones; that configuration's extra tensor is gating_fc's output, written by the Linear before the gate reads it.
Writes profiles/gate_bench.json.

    python tools/bench_gate.py [reps] [rounds]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vmg_amd import kernels as K

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
if not torch.cuda.is_available():
    raise SystemExit("bench_gate.py measures on the GPU; none is visible")
torch.manual_seed(0)
B, T, H, W, C = 4, 7, 64, 64, 144
dt = torch.bfloat16
shape = (B, T, H, W, C)
a, y, res, d = (torch.randn(shape, device="cuda").to(dt) for _ in range(4))
coef = torch.full((B, C), 1.0 / 0.9, device="cuda")
coef[1] = 0.0  # (a dropped sample)
tensor_bytes = a.numel() * a.element_size()
KINDS = {"fwd": 3, "res_fwd": 4, "bwd": 5, "res_bwd": 5}  # tensors moved per call


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def gate_fns(act, asym):
    return {"fwd": lambda: K.gate_forward(a, y, act, asym), "res_fwd": lambda: K.gate_forward(a, y, act, asym, res=res, coef=coef, G=B),
            "bwd": lambda: K.gate_backward(d, a, y, act, asym), "res_bwd": lambda: K.gate_backward(d, a, y, act, asym, coef=coef, G=B)}


cands = {"tanh_ops": {"fwd": lambda: K.tab_elementwise(K.OP_GATE_FWD, a, y),
                      "res_fwd": lambda: K.tab_elementwise(K.OP_GATE_RES_FWD, a, y, res, coef=coef, s=1.0, G=B),
                      "bwd": lambda: K.tab_elementwise(K.OP_GATE_BWD, d, a, y, nout=2),
                      "res_bwd": lambda: K.tab_elementwise(K.OP_GATE_RES_BWD, d, a, y, coef=coef, s=1.0, G=B, nout=2)}}
for act in ("tanh", "sigmoid", "relu", "gelu", "swish"):
    cands["symm_" + act] = gate_fns(act, False)
cands["asym"] = gate_fns("gelu", True)
copies = {}
for n in sorted(set(KINDS.values())):  # a copy reads and writes half of the n tensors each
    src = torch.randn(a.numel() * n // 2, device="cuda").to(dt)
    dst = torch.empty_like(src)
    copies[n] = (lambda s_, d_: (lambda: d_.copy_(s_)))(src, dst)
cands["copy"] = {k: copies[n] for k, n in KINDS.items()}

for fns in cands.values():  # warm-up of everything the timed window uses
    for fn in fns.values():
        for _ in range(3):
            fn()
torch.cuda.synchronize()
ts = {name: {k: [] for k in fns} for name, fns in cands.items()}
for _ in range(rounds):
    for k in KINDS:
        for name, fns in cands.items():
            ts[name][k].append(timed(fns[k]))

rows = []
for name, per in ts.items():
    row = {"kernel": name}
    for k, v in per.items():
        med = statistics.median(v)
        row[k + "_us"] = round(med, 1)
        row[k + "_TBps"] = round(KINDS[k] * tensor_bytes / med / 1e6, 2)
        row[k + "_spread"] = round((max(v) - min(v)) / med, 4)
    rows.append(row)
    print("%-13s" % name + "  ".join("%s %6.1f us %5.2f TB/s (spread %4.1f %%)" % (k, row[k + "_us"], row[k + "_TBps"], 100 * row[k + "_spread"]) for k in KINDS), flush=True)

out = {"shape": list(shape), "dtype": "bf16", "tensor_bytes": tensor_bytes, "tensors_per_call": KINDS, "reps": reps, "rounds": rounds,
       "device": torch.cuda.get_device_name(0), "rows": rows}
path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gate_bench.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", path)
