"""LR synthesis (vmg_amd.degrade.bicubic_lr, vmg_bicubic_down) on a batch of 100 HR frames of 720 x 1280 -> 180 x 320: stream-event time
of the kernel per call and wall time of the whole degrade.lr_clip call (synchronised), each the median of `reps` calls after warm-up, in
microseconds per frame, for interleaved and planar storage.  Next to it the bandwidth floor: a plain device copy (Tensor.copy_) of as
many bytes as the kernel reads once and writes (HR + LR bytes).  GB/s counts those bytes once for the kernel and once for the copy.
Prints one JSON line; --out PATH also writes it there.
    python tools/bench_lr.py [--frames 100] [--reps 9] [--scale 4] [--out profiles/lr.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vmg_amd import degrade
from vmg_amd import kernels as K

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scale", type=int, default=4)
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_lr needs the GPU"
T, H, W, s = args.frames, 720, 1280, args.scale
g = torch.Generator(device="cuda").manual_seed(0)
hr = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)  # decoded images: interleaved
views = {"interleaved": hr.permute(0, 3, 1, 2), "planar": hr.permute(0, 3, 1, 2).contiguous()}


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


res = {"what": "bicubic_lr", "frames": T, "H": H, "W": W, "scale": s, "reps": args.reps}
for out_dtype, tag in ((torch.uint8, "u8"), (torch.float32, "f32")):
    esize = torch.empty((), dtype=out_dtype).element_size()
    nbytes = T * 3 * H * W + T * 3 * (H // s) * (W // s) * esize
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    copy_ms = event_ms(lambda: dst.copy_(src), args.reps)
    del src, dst
    copy_us = statistics.median(copy_ms) * 1e3 / T
    res[f"copy_same_bytes_{tag}_us_per_frame"] = copy_us
    res[f"copy_same_bytes_{tag}_GBps"] = nbytes / T / copy_us / 1e3
    for layout, view in views.items():
        ms = event_ms(lambda: K.bicubic_down(view, s, out_dtype), args.reps)
        us = statistics.median(ms) * 1e3 / T
        res[f"kernel_{layout}_{tag}_us_per_frame_median"] = us
        res[f"kernel_{layout}_{tag}_us_per_frame_min_max"] = [min(ms) * 1e3 / T, max(ms) * 1e3 / T]
        res[f"kernel_{layout}_{tag}_GBps"] = nbytes / T / us / 1e3
        res[f"kernel_{layout}_{tag}_over_copy"] = us / copy_us

wall = []
for _ in range(args.reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    clip = degrade.lr_clip(hr, s)
    torch.cuda.synchronize()
    wall.append((time.perf_counter() - t0) * 1e3)
res["lr_clip_call_wall_us_per_frame_median"] = statistics.median(wall) * 1e3 / T
res["lr_clip_shape"] = list(clip.shape)

# a small batch: the launch is what is left
one = hr[:1]
ms = event_ms(lambda: K.bicubic_down(one.permute(0, 3, 1, 2), s, torch.uint8), args.reps)
res["kernel_one_frame_interleaved_u8_us"] = statistics.median(ms) * 1e3

line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
