"""Frame scoring (vmg_amd.metrics.frame_metrics) on 100 frame pairs of 720 x 1280, planar output against interleaved ground truth:
stream-event time of the two kernels per call, median of `reps` calls after warm-up, and the wall time of the whole call (kernels +
the one host copy + the logarithms).  With --numpy N the float64 numpy restatement (tests/metrics_ref.py) scores N of the same frames
on 16 threads for comparison.  Prints one JSON line; --out PATH also writes it there.
    python tools/bench_metrics.py [--frames 100] [--reps 9] [--numpy 16] [--out profiles/metrics.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vmg_amd import kernels as K
from vmg_amd.metrics import frame_metrics

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--numpy", type=int, default=0, help="frames scored by the numpy restatement (0: skip)")
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_metrics needs the GPU"
T, H, W = args.frames, 720, 1280
g = torch.Generator(device="cuda").manual_seed(0)
gt = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)  # decoded images: interleaved
noise = torch.randint(-4, 5, (T, H, W, 3), dtype=torch.int16, device="cuda", generator=g)
out = (gt.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8).permute(0, 3, 1, 2).contiguous()  # network output: planar
del noise
a, b = out, gt.permute(0, 3, 1, 2)
ws = torch.empty(int(K.hip.lib().vmg_frame_metrics_ws_bytes(T, H, W)), dtype=torch.uint8, device="cuda")

for _ in range(3):
    K.frame_metrics_sums(a, b, ws)
torch.cuda.synchronize()
dev_ms, wall_ms = [], []
for _ in range(args.reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    K.frame_metrics_sums(a, b, ws)
    e1.record()
    torch.cuda.synchronize()
    dev_ms.append(e0.elapsed_time(e1))
for _ in range(args.reps):
    t0 = time.perf_counter()
    m = frame_metrics(out, gt)
    wall_ms.append((time.perf_counter() - t0) * 1e3)

res = {
    "what": "frame_metrics", "frames": T, "H": H, "W": W, "reps": args.reps,
    "kernels_us_per_frame_median": statistics.median(dev_ms) * 1e3 / T,
    "kernels_us_per_frame_min_max": [min(dev_ms) * 1e3 / T, max(dev_ms) * 1e3 / T],
    "call_wall_us_per_frame_median": statistics.median(wall_ms) * 1e3 / T,
    "psnr_mean": float(m.psnr.mean()), "ssim_mean": float(m.ssim.mean()),
}

if args.numpy > 0:
    from concurrent.futures import ThreadPoolExecutor
    from tests import metrics_ref as R
    n = min(args.numpy, T)
    o_np, g_np = out[:n].permute(0, 2, 3, 1).cpu().numpy(), gt[:n].cpu().numpy()
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        rows = list(ex.map(lambda i: R.frame_scores(o_np[i], g_np[i]), range(n)))
    dt = time.perf_counter() - t0
    res["numpy_16_threads_frames"] = n
    res["numpy_16_threads_us_per_frame"] = dt * 1e6 / n
    res["max_abs_ssim_difference_vs_numpy"] = max(abs(float(m.ssim[i]) - rows[i][2]) for i in range(n))

line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
