"""Best window per frame, streamed vs the literal restatement: time per sequence and peak device memory of infer.best_window_clips (float HR
and uint8 HR) against infer.test_clips_max, on window outputs REPLAYED from device memory (no network in the timed region).

    python tools/bench_best_window.py [--frames 100 --window 50 --overlap 25 --height 720 --width 1280 --reps 5 --out FILE.json]

The default is the REDS4 evaluation shape: 100 frames, windows of 50 with 25 shared frames (3 windows), 720 x 1280 outputs.  Times are host
clocks around a call that ends in a device synchronise; memory is torch.cuda.max_memory_allocated above what was allocated before the call
(inputs, HR and the replayed outputs are excluded, the function's own canvases and scratch are counted).  Needs the GPU."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vmg_amd import infer  # noqa: E402


class Replay:
    def __init__(self, outs):
        self.outs, self.i = outs, 0

    def __call__(self, x):
        o = self.outs[self.i % len(self.outs)]
        self.i += 1
        return o


def measure(fn, reps):
    fn()  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times, peak = [], 0
    for _ in range(reps):
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
        del out
    times.sort()
    return {"ms_median": times[len(times) // 2], "ms_min": times[0], "ms_max": times[-1], "peak_bytes": peak}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--overlap", type=int, default=25)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_best_window: needs the GPU (there is no CPU path and no CPU timing is reported)")
    T, nf, of, hh, ww = a.frames, a.window, a.overlap, a.height, a.width
    if hh % 4 or ww % 4:
        sys.exit("bench_best_window: height and width must be multiples of the scale 4")
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    ts = infer.tile_starts(T, nf, of)
    hr_u8 = torch.randint(0, 256, (T, hh, ww, 3), generator=g, dtype=torch.uint8, device=dev)
    hr_f = (hr_u8.permute(0, 3, 1, 2).float() / torch.full((), 255.0, device=dev)).unsqueeze(0).contiguous()
    # window k = HR + noise whose size differs from window to window and from frame to frame: every frame has a clear winner
    outs = []
    for k, t in enumerate(ts):
        amp = 0.02 + 0.01 * ((torch.arange(nf, device=dev) * 7 + 3 * k) % 5).float()
        outs.append((hr_f[:, t:t + nf] + amp[None, :, None, None, None] * torch.randn((1, nf, 3, hh, ww), generator=g, device=dev)).contiguous())
    x = torch.zeros(1, T, 3, hh // 4, ww // 4, device=dev)

    runs = {
        "best_window_clips_float_hr": lambda: infer.best_window_clips(Replay(outs), x, hr_f, nf, of),
        "best_window_clips_uint8_hr": lambda: infer.best_window_clips(Replay(outs), x, hr_u8, nf, of),
        "test_clips_max": lambda: infer.test_clips_max(Replay(outs), x, hr_f, nf, of),
    }
    same = bool(torch.equal(runs["best_window_clips_float_hr"](), runs["test_clips_max"]())) and \
        bool(torch.equal(runs["best_window_clips_uint8_hr"](), runs["test_clips_max"]()))
    res = {"what": "best window per frame, per sequence, outputs replayed from device memory", "frames": T, "window": nf, "overlap": of, "windows": len(ts),
           "output": [3, hh, ww], "reps": a.reps, "device": torch.cuda.get_device_name(0), "frames_equal_test_clips_max": same,
           "canvas_bytes": T * 3 * hh * ww * 4, "window_output_bytes": nf * 3 * hh * ww * 4}
    for name, fn in runs.items():
        res[name] = measure(fn, a.reps)
    res["time_ratio_test_clips_max_over_streamed"] = res["test_clips_max"]["ms_median"] / res["best_window_clips_float_hr"]["ms_median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
