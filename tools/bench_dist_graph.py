"""The data-parallel train step on the per-GPU shard of BASELINE configs[2] (bench.py's `train_full`: full VMG-REDS, C = 112, one clip of
1 x 7 x 3 x 64 x 64, bf16), four ways in ONE process with ONE RCCL rank (every collective issued, nothing crosses xGMI):

  (a) eager_dist    the eager distributed step (bucketed all-reduce launched from the gradient hooks during backward)
  (b) graph2_fp32   TrainStep.capture with a reducer: graph A -> eager exchange of the fp32 flat gradient buffer -> graph B
  (c) graph2_bf16   the same with exchange_dtype = torch.bfloat16 (pack, all-reduce of the half-size payload, unpack)
  (d) graph1_single the one-graph step without a reducer: the ceiling

    python tools/bench_dist_graph.py [--steps 6] [--windows 5] [--warmup 3] [--timeout 900] [--out profiles/dist_graph_bench.json]

Each variant: `warmup` untimed steps, then `windows` windows of `steps` steps, a host clock around each window with a device synchronise at both
ends; ms/step is the median over the windows, with the smallest and largest window next to it.  The variants run one after the other (a step
object cannot go back to eager once captured), so box drift between them is inside the spread, not cancelled.  The exchange's own time in (b) and
(c) comes from a pair of HIP events recorded on the compute stream around GradBucketReducer.exchange() in every timed step (median).
The measurement runs in a child process under a time limit; the parent never opens the GPU.  Prints one JSON line."""
import argparse
import gc
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _measure(args):
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC for RCCL (tests/test_distributed_gpu.py)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if "MASTER_PORT" not in os.environ:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(s.getsockname()[1])
    import torch
    import torch.distributed as dist
    import bench
    from vmg_amd.data import synthetic_clip, synthetic_target
    from vmg_amd.train import TrainStep
    from vmg_amd.wgrad import DEFERRED
    if not torch.cuda.is_available():
        raise SystemExit("bench_dist_graph: no GPU (there is no CPU path to time)")
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=device)
    wl = bench.WORKLOADS["train_full"]
    B, Tn, S = wl["batch"], wl["frames"], wl["size"]
    lrs = synthetic_clip(B, Tn, S, S, seed=1234, device=device)
    hrs = synthetic_target(lrs, seed=4321)

    def make(**kw):
        return TrainStep(bench.build_model(device, wl), lr=2e-4, betas=(0.9, 0.99), aux=True, aux_ratio=0.005, **kw)

    def timed(ts, events=None):
        for _ in range(args.warmup):
            ts(lrs, hrs)
        per = []
        for _ in range(args.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ts(lrs, hrs)
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) / args.steps * 1e3)
        ms = statistics.median(per)
        out = {"ms_per_step": round(ms, 3), "ms_min": round(min(per), 3), "ms_max": round(max(per), 3), "lr_frames_per_s": round(B * Tn / ms * 1e3, 2),
               "timed_steps": args.steps * args.windows}
        if events:
            ex = [a.elapsed_time(b) for a, b in events[-args.steps * args.windows:]]
            out.update(exchange_ms=round(statistics.median(ex), 4), exchange_ms_min=round(min(ex), 4), exchange_ms_max=round(max(ex), 4))
        return out

    def time_exchange(ts):
        events, inner = [], ts.reducer.exchange

        def exchange(payload=None):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            inner(payload)
            b.record()
            events.append((a, b))
        ts.reducer.exchange = exchange
        return events

    res = {}
    # (a) then (b) on the same step object: the eager distributed step, then the same step captured
    ts = make(distributed=True, single_rank_collectives=True)
    res["eager_dist"] = timed(ts)
    res["flat_gradient_mbytes"] = round(ts.opt.n * 4 / 1e6, 2)
    res["buckets"] = len(ts.reducer.buckets)
    ts.capture(lrs, hrs, warmup=max(1, args.warmup))
    res["graph2_fp32"] = timed(ts, time_exchange(ts))
    del ts
    gc.collect()
    torch.cuda.empty_cache()
    # (c) bf16 payload
    ts = make(distributed=True, single_rank_collectives=True, exchange_dtype=torch.bfloat16)
    ts.capture(lrs, hrs, warmup=max(1, args.warmup))
    res["graph2_bf16"] = timed(ts, time_exchange(ts))
    del ts
    gc.collect()
    torch.cuda.empty_cache()
    # (d) the one-graph step without a reducer (the last reducer's completion callback is unhooked first: this step has none)
    DEFERRED.callbacks[:] = []
    ts = make()
    ts.capture(lrs, hrs, warmup=max(1, args.warmup))
    res["graph1_single"] = timed(ts)
    del ts
    a, b, d = res["eager_dist"]["ms_per_step"], res["graph2_fp32"]["ms_per_step"], res["graph1_single"]["ms_per_step"]
    res["speed_graph2_fp32_over_eager_dist"] = round(a / b, 4)
    res["speed_graph2_fp32_over_graph1_single"] = round(d / b, 4)
    res["workload"] = wl["name"]
    res["setup"] = "one process, ONE RCCL rank (world_size 1, every collective issued): the exchange is a local RCCL call, nothing crosses xGMI"
    res["device"] = torch.cuda.get_device_name(0)
    dist.barrier()
    dist.destroy_process_group()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=6, help="timed steps per window")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per variant (steps x windows >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900, help="seconds the measuring child process may take")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps * args.windows < 20:
        ap.error("at least 20 timed steps per variant (steps x windows)")
    if args.child:
        return _measure(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    p = subprocess.Popen(cmd)
    try:
        rc = p.wait(timeout=args.timeout)
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
        raise SystemExit(f"bench_dist_graph: the measurement did not finish in {args.timeout} s and was stopped")
    raise SystemExit(rc)


if __name__ == "__main__":
    main()
