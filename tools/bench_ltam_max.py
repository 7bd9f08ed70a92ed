"""Hard trajectory attention (vmg_ltam_max_fwd / _bwd, traj_mode 'max') next to the window pair (vmg_ltam_fwd / _bwd) in ONE process, at the bench
batch's shape (8 x 64 x 64 pixels, 144 channels, 4 heads, bf16) for t = 1..6 and t = 17 key-frames.  Stream events around `reps` launches after a
warm-up, `rounds` rounds per kernel and t with the four kernels ALTERNATING inside a round; reported: the median over the rounds and the spread
(max - min) / median of the 'wins' timing in that same run, which is what a difference has to exceed.  The backward times include zeroing the fp32
accumulators, as in the step.  Writes profiles/ltam_max_bench.json.

    python tools/bench_ltam_max.py [reps] [rounds]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vmg_amd import kernels as K

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
torch.manual_seed(0)
n, h, w, c, heads = 8, 64, 64, 144, 4
dt = torch.bfloat16


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


rows = []
for t in (1, 2, 3, 4, 5, 6, 17):
    q = torch.randn(n, h, w, c, device="cuda").to(dt)
    keys = [torch.randn(n, h, w, c, device="cuda").to(dt) for _ in range(t)]
    vals = [torch.randn(n, h, w, c, device="cuda").to(dt) for _ in range(t)]
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    loc = (torch.stack([xs, ys], 0).repeat(t, 1, 1)[None].repeat(n, 1, 1, 1) + 3.0 * torch.randn(n, 2 * t, h, w, device="cuda")).contiguous()
    rpe, decay = torch.randn(heads, 4, 4, device="cuda"), torch.rand(heads, device="cuda")
    scale = (c // heads) ** -0.5
    dout = torch.randn(n, h, w, c, device="cuda").to(dt)
    out, lse = K.ltam_forward(q, keys, vals, loc, rpe, decay, heads, 2, 2, scale)
    _, idx, _ = K.ltam_max_forward(q, keys, vals, loc, heads)
    fns = {
        "wins_fwd": lambda: K.ltam_forward(q, keys, vals, loc, rpe, decay, heads, 2, 2, scale),
        "max_fwd": lambda: K.ltam_max_forward(q, keys, vals, loc, heads),
        "wins_bwd": lambda: K.ltam_backward(q, keys, vals, loc, rpe, decay, out, lse, dout, heads, 2, 2, scale),
        "max_bwd": lambda: K.ltam_max_backward(q, keys, vals, loc, idx, dout, heads),
    }
    for fn in fns.values():  # warm-up of every shape the timed window uses
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    row = {"t": t}
    for k, v in ts.items():
        row[k + "_us"] = round(statistics.median(v), 1)
        row[k + "_spread"] = round((max(v) - min(v)) / statistics.median(v), 4)
    used = int(torch.unique(idx).numel())
    row["key_frames_selected"] = used
    rows.append(row)
    print("t = %2d : forward wins %7.1f us (spread %4.1f %%)  max %7.1f us   backward wins %7.1f us (spread %4.1f %%)  max %7.1f us" % (
        t, row["wins_fwd_us"], 100 * row["wins_fwd_spread"], row["max_fwd_us"], row["wins_bwd_us"], 100 * row["wins_bwd_spread"], row["max_bwd_us"]), flush=True)

res = {"shape": [n, h, w, c], "dtype": "bf16", "heads": heads, "reps": reps, "rounds": rounds, "device": torch.cuda.get_device_name(0), "rows": rows}
path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ltam_max_bench.json")
with open(path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", path)
