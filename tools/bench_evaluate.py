"""The conversions around the network in infer.evaluate (vmg_convert_frames) at the REDS4 shape: 100 x 180 x 320 x 3 uint8 frames in
(frames_to_clip -> (1, 100, 3, 180, 320) fp32) and a (100, 3, 720, 1280) fp32 clip out (clip_to_frames -> (100, 720, 1280, 3) uint8), with no
flags and with hflip + vflip + rot90.  Per job: stream-event time of one call in microseconds (median, min, max of `reps` calls after
warm-up) and the rise of max_memory_allocated over one call, for three ways of doing it, alternated call by call in the same run:
    new     the one launch of vmg_convert_frames
    parent  what infer.evaluate_reds does for the same job: the 256-entry table gathered through permute().long() (+ _augment) on the way in,
            (_augment +) to_uint8_device(...).permute(0, 2, 3, 1).contiguous() on the way out
    copy    a plain device copy (Tensor.copy_) of as many bytes as the job reads once and writes once: the bandwidth floor
The results of new and parent are compared for equality before anything is timed.  Prints one JSON line; --out PATH also writes it there.
    python tools/bench_evaluate.py [--frames 100] [--reps 9] [--out profiles/evaluate_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vmg_amd import infer

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--height", type=int, default=180)
ap.add_argument("--width", type=int, default=320)
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_evaluate needs the GPU"
T, H, W = args.frames, args.height, args.width
g = torch.Generator(device="cuda").manual_seed(0)
lr = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
sr = torch.rand((T, 3, 4 * H, 4 * W), device="cuda", generator=g) * 1.2 - 0.1  # the network's frames: mostly inside [0, 1], some beyond


def parent_in(flags):
    x = infer._u8_to_unit(lr.device)[lr.permute(0, 3, 1, 2).long()].unsqueeze(0)
    return infer._augment(x, *flags) if any(flags) else x.contiguous()


def parent_out(flags):
    o = infer._augment(sr, *flags) if any(flags) else sr
    return infer.to_uint8_device(o).permute(0, 2, 3, 1).contiguous()


def timed(fns, reps):
    """Event times in microseconds of each callable, the callables alternated call by call."""
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3)
    return us


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return peak


res = {"what": "evaluate_conversions", "frames": T, "lr": [H, W], "sr": [4 * H, 4 * W], "reps": args.reps}
jobs = {
    "in": (lambda fl: infer.frames_to_clip(lr, torch.float32, *fl), parent_in, lr.numel() * (1 + 4)),
    "out": (lambda fl: infer.clip_to_frames(sr, *fl), parent_out, sr.numel() * (4 + 1)),
}
for job, (new, parent, nbytes) in jobs.items():
    src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    for tag, flags in (("plain", (False, False, False)), ("flipped_rotated", (True, True, True))):
        a, b = new(flags), parent(flags)
        assert a.shape == b.shape and torch.equal(a, b), f"{job} {tag}: the new path and the parent's differ"
        del a, b
        # the copy moves nbytes / 2 bytes from one buffer to another: nbytes of traffic, like the job
        us = timed({"new": lambda: new(flags), "parent": lambda: parent(flags), "copy": lambda: dst.copy_(src)}, args.reps)
        key = f"{job}_{tag}"
        for k, v in us.items():
            res[f"{key}_{k}_us_median"] = statistics.median(v)
            res[f"{key}_{k}_us_min_max"] = [min(v), max(v)]
        res[f"{key}_bytes_read_plus_written"] = nbytes
        res[f"{key}_new_GBps"] = nbytes / res[f"{key}_new_us_median"] / 1e3
        res[f"{key}_new_over_parent"] = res[f"{key}_new_us_median"] / res[f"{key}_parent_us_median"]
        res[f"{key}_new_over_copy"] = res[f"{key}_new_us_median"] / res[f"{key}_copy_us_median"]
        res[f"{key}_new_peak_bytes"] = peak_bytes(lambda: new(flags))
        res[f"{key}_parent_peak_bytes"] = peak_bytes(lambda: parent(flags))
    del src, dst

line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
