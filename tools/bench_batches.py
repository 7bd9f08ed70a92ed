"""Batch assembly (vmg_amd.batches.assemble, vmg_crop_batch) out of resident 180 x 320 / 720 x 1280 frames: stream-event time of the two
launches (tables already on the device) and wall time of the whole assemble call (plan checks, table upload, both launches; synchronised),
each the median of `reps` calls after warm-up with the min and max next to it, in microseconds per batch.  Shapes: the bench batch B = 4,
T = 7, 64 x 64 / 256 x 256, and the reference config's B = 8, T = 16; output fp32 and bf16; flags all off, all on (hflip + vflip + transpose)
and mixed; interleaved and planar stores.  Next to each the bandwidth floor: a plain device copy (Tensor.copy_) of as many bytes as the
kernels read once plus write.  GB/s counts those bytes once for the kernels and once for the copy.
Prints one JSON line; --out PATH also writes it there.
    python tools/bench_batches.py [--reps 21] [--clips 4] [--frames 20] [--out profiles/batches.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vmg_amd import batches
from vmg_amd import kernels as K

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--clips", type=int, default=4)
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_batches needs the GPU"
s, H, W, c = 4, 180, 320, 64
g = torch.Generator(device="cuda").manual_seed(0)
hr = torch.randint(0, 256, (args.clips, args.frames, s * H, s * W, 3), dtype=torch.uint8, device="cuda", generator=g)
lr = torch.randint(0, 256, (args.clips, args.frames, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
stores = {"interleaved": batches.FrameStore(hr, lr, s),
          "planar": batches.FrameStore(hr.permute(0, 1, 4, 2, 3).contiguous(), lr.permute(0, 1, 4, 2, 3).contiguous(), s)}


def event_us(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return us


def wall_us(fn, reps):
    for _ in range(5):
        fn()
    us = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return us


def plan(B, T, flags):
    rng = np.random.default_rng(B * 100 + T)
    start = rng.integers(0, args.frames - T + 1, B)
    f = {"off": np.zeros(B, int), "on": np.full(B, 7), "mixed": np.arange(B) % 8}[flags]
    return batches.BatchPlan(clip=rng.integers(0, args.clips, B), frames=start[:, None] + np.arange(T)[None, :], y0=rng.integers(0, H - c + 1, B),
                             x0=rng.integers(0, W - c + 1, B), hflip=(f & 1) != 0, vflip=(f & 2) != 0, rot=(f & 4) != 0, crop=c)


def tables(store, p):
    """The device tables assemble uploads, made once: the event time is of the two launches alone."""
    B, T = p.frames.shape
    out = []
    for side, m in ((store.lr, 1), (store.hr, s)):
        ptr = (side.base[p.clip][:, None] + p.frames * side.fstride[p.clip][:, None]).reshape(-1)
        fl = p.hflip.astype(np.int32) + 2 * p.vflip + 4 * p.rot
        desc = np.stack([np.repeat(a, T) for a in (m * p.y0, m * p.x0, fl)], axis=1).astype(np.int32)
        out.append((torch.from_numpy(ptr).cuda(), torch.from_numpy(desc).cuda()))
    return out


res = {"what": "assemble", "lr_frame": [H, W], "scale": s, "crop": [c, s * c], "reps": args.reps, "unit": "us per batch"}
for B, T in ((4, 7), (8, 16)):
    if T > args.frames:
        continue
    for dt, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        es = torch.empty((), dtype=dt).element_size()
        px = B * T * 3 * (c * c + s * c * s * c)
        nbytes = px + px * es                      # every source byte of the crops once, every output element once
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        cp = event_us(lambda: dst.copy_(src), args.reps)
        del src, dst
        key = f"B{B}_T{T}_{tag}"
        res[f"{key}_bytes"] = nbytes
        res[f"{key}_copy_same_bytes_us"] = [statistics.median(cp), min(cp), max(cp)]
        lrs = torch.empty((B, T, 3, c, c), dtype=dt, device="cuda")
        hrs = torch.empty((B, T, 3, s * c, s * c), dtype=dt, device="cuda")
        for layout, store in stores.items():
            for flags in ("off", "on", "mixed"):
                p = plan(B, T, flags)
                (pl, dl), (ph, dh) = tables(store, p)

                def launches():
                    K.crop_batch(pl, store.lr.strides, dl, H, W, c, c, True, lrs)
                    K.crop_batch(ph, store.hr.strides, dh, s * H, s * W, s * c, s * c, True, hrs)

                ev = event_us(launches, args.reps)
                wl = wall_us(lambda: batches.assemble(store, p, dt, out=(lrs, hrs)), args.reps)
                k = f"{key}_{layout}_{flags}"
                res[f"{k}_launches_us"] = [statistics.median(ev), min(ev), max(ev)]
                res[f"{k}_GBps"] = nbytes / statistics.median(ev) / 1e3
                res[f"{k}_over_copy"] = statistics.median(ev) / statistics.median(cp)
                res[f"{k}_assemble_wall_us"] = [statistics.median(wl), min(wl), max(wl)]

line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
