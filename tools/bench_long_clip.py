"""Long clips in one call: the few_levels network on a (1, T, 3, 128, 128) tile, bf16, no_grad, at T = 32, 64, 100 and 200 (key-frame stride 3: 11, 22,
34 and 67 key-frames; beyond 64 frames vmg_pair_steps takes several launches, beyond 32 key-frames the attention takes its table route).  Per T: the
stream-event time of one call after a warm-up call (median, min, max of `reps`), LR-frames/s from it and the peak of max_memory_allocated over the call.
Then the trajectory attention alone at the tile's lock-step shape (2 x 128 x 128 pixels, 144 channels, 2 x 2 windows, bf16) at t = 17 and t = 32
key-frames, argument route (vmg_ltam_fwd / _bwd) against table route (vmg_ltam_fwd_tab / _bwd_tab: + one fill launch), alternated call by call in the
same process: microseconds per call, forward and backward, after the two routes' outputs were compared for equality.
Prints one JSON line; --out PATH also writes it there.
    python tools/bench_long_clip.py [--frames 32,64,100,200] [--reps 3] [--attn-reps 30] [--out profiles/long_clip_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--frames", default="32,64,100,200")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--attn-reps", type=int, default=30)
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_long_clip needs the GPU"
import vmg_amd
from vmg_amd import functional as FH
from vmg_amd import kernels as K
from vmg_amd.data import REDS_FEW_LEVELS, synthetic_clip

dev = torch.device("cuda", 0)
torch.manual_seed(0)
res = {"what": "long_clip", "tile": [128, 128], "dtype": "bf16", "network": "few_levels", "reps": args.reps, "attn_reps": args.attn_reps, "clips": {}, "attention": {}}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    del r
    return e0.elapsed_time(e1)


stride = REDS_FEW_LEVELS["traj_keyframes_n"][0]
for T in [int(v) for v in args.frames.split(",")]:
    m = vmg_amd.VMG(num_frames=T, image_size=[128, 128], is_train=False, spynet_pretrained=None, compute_dtype=torch.bfloat16, **REDS_FEW_LEVELS)
    m.spynet = vmg_amd.SPyNet(None)
    m = m.to(dev).eval()
    x = synthetic_clip(1, T, 128, 128, seed=7, device=dev)
    with torch.no_grad():
        out = m(x)  # warm-up: weight packs, code objects
        finite = bool(torch.isfinite(out.float()).all())
        del out
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms = [event_ms(lambda: m(x)) for _ in range(args.reps)]
        peak = torch.cuda.max_memory_allocated()
    med = statistics.median(ms)
    res["clips"][str(T)] = {"ms_per_call_median": round(med, 2), "ms_min_max": [round(min(ms), 2), round(max(ms), 2)], "lr_frames_per_s": round(T / med * 1e3, 2),
                            "peak_GB": round(peak / 1e9, 3), "key_frames": (T - 1) // stride + 1, "ltam_route_of_the_last_step": FH.ltam_route((T - 2) // stride + 1),
                            "finite": finite}
    print("T = %d: %s" % (T, res["clips"][str(T)]), file=sys.stderr, flush=True)
    del m, x
    torch.cuda.empty_cache()

n, h, w, c, heads = 2, 128, 128, 144, 4
dt = torch.bfloat16
for t in (17, 32):
    q = torch.randn(n, h, w, c, device=dev).to(dt)
    keys = [torch.randn(n, h, w, c, device=dev).to(dt) for _ in range(t)]
    vals = [torch.randn(n, h, w, c, device=dev).to(dt) for _ in range(t)]
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    loc = (torch.stack([xs, ys], 0).repeat(t, 1, 1)[None].repeat(n, 1, 1, 1) + 3.0 * torch.randn(n, 2 * t, h, w, device=dev)).contiguous()
    rpe = torch.randn(heads, 4, 4, device=dev)
    decay = 1.0 - 0.1 * torch.rand(heads, device=dev)
    scale = (c // heads) ** -0.5
    dout = torch.randn(n, h, w, c, device=dev).to(dt)
    out, lse = K.ltam_forward(q, keys, vals, loc, rpe, decay, heads, 2, 2, scale)
    out_t, lse_t = K.ltam_forward_tab(q, keys, vals, loc, rpe, decay, heads, 2, 2, scale)
    assert torch.equal(out, out_t) and torch.equal(lse, lse_t), "the two routes' forward results differ"
    acc = [torch.zeros(n, h, w, c, device=dev) for _ in range(2 * t)]  # (accumulators handed in: the timed calls launch nothing but the route's kernels)
    drpe = torch.zeros_like(rpe)
    fns = {
        "fwd_args": lambda: K.ltam_forward(q, keys, vals, loc, rpe, decay, heads, 2, 2, scale),
        "fwd_table": lambda: K.ltam_forward_tab(q, keys, vals, loc, rpe, decay, heads, 2, 2, scale),
        "bwd_args": lambda: K.ltam_backward(q, keys, vals, loc, rpe, decay, out, lse, dout, heads, 2, 2, scale, dk_into=acc[:t], dv_into=acc[t:], drpe_into=drpe),
        "bwd_table": lambda: K.ltam_backward_tab(q, keys, vals, loc, rpe, decay, out, lse, dout, heads, 2, 2, scale, dk_into=acc[:t], dv_into=acc[t:], drpe_into=drpe),
    }
    for _ in range(3):
        for fn in fns.values():
            fn()
    us = {k: [] for k in fns}
    for _ in range(args.attn_reps):
        for k, fn in fns.items():
            us[k].append(event_ms(fn) * 1e3)
    ent = {k + "_us_median": round(statistics.median(v), 1) for k, v in us.items()}
    ent.update({k + "_us_min_max": [round(min(v), 1), round(max(v), 1)] for k, v in us.items()})
    ent["fwd_table_over_args"] = round(statistics.median(us["fwd_table"]) / statistics.median(us["fwd_args"]), 4)
    ent["bwd_table_over_args"] = round(statistics.median(us["bwd_table"]) / statistics.median(us["bwd_args"]), 4)
    res["attention"][str(t)] = ent

line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
