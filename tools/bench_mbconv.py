"""The depthwise 3x3 kernels of the MBConv mixer (csrc/dwconv.hip: vmg_dwconv3_fwd / _bwd_data / _bwd_weight) next to a device copy that moves the
same bytes, and the whole mixer (Multi_MBConv, two blocks, forward + backward) next to Enhanced_MorphFCs_decay at the same shape, in ONE process, at
the bench shape of stage 0 -- 4 x 7 frames of 64 x 64 pixels, bf16 -- for C = 144 (mid width 576) and C = 112 (mid width 448), both on the vector
path, and the per-element path at the odd mid width 575.  Stream events around `reps` launches after a warm-up, `rounds` rounds with all candidates
ALTERNATING inside a round; reported: the median over the rounds in us, the rate over the bytes the kernel has to move, the median of the copy of
the same bytes, and the spread (max - min) / median.  Bytes per call in tensors of the kernel's shape: forward e in + a out = 2; data gradient da,
a, e in + de out = 4; weight gradient da, a, e in = 3 (the 9 C weights and the partial sums are noise).  Writes profiles/mbconv_bench.json.

    python tools/bench_mbconv.py [reps] [rounds]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vmg_amd import kernels as K
from vmg_amd.model import Enhanced_MorphFCs_decay, Multi_MBConv

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
if not torch.cuda.is_available():
    raise SystemExit("bench_mbconv.py measures on the GPU; none is visible")
torch.manual_seed(0)
B, T, H, W = 4, 7, 64, 64
dt = torch.bfloat16
R6 = "relu6"


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def copy_of(nbytes):
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda").zero_()
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


def measure(cands):
    """cands: name -> (fn, bytes moved or 0, launches per timing).  Returns rows with medians."""
    for fn, _, _ in cands.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in cands}
    for _ in range(rounds):
        for k, (fn, _, n) in cands.items():
            ts[k].append(timed(fn, n))
    rows = []
    for k, v in ts.items():
        med = statistics.median(v)
        row = {"kernel": k, "us": round(med, 1), "spread": round((max(v) - min(v)) / med, 4)}
        if cands[k][1]:
            row["bytes"] = cands[k][1]
            row["TBps"] = round(cands[k][1] / med / 1e6, 2)
        rows.append(row)
        print("  %-26s %8.1f us %s (spread %4.1f %%)" % (k, row["us"], "%5.2f TB/s" % row["TBps"] if "TBps" in row else "          ", 100 * row["spread"]), flush=True)
    return rows


def kernel_cands(M):
    """The three launches at mid width M with both ReLU6 on, and copies of 2, 3 and 4 tensors."""
    N = B * T
    e = (3 * torch.randn(N, H, W, M, device="cuda")).to(dt)
    da = torch.randn(N, H, W, M, device="cuda").to(dt)
    w, b = torch.randn(M, 1, 3, 3, device="cuda") / 3, torch.randn(M, device="cuda")
    a = K.dwconv3_forward(e, w, b, R6, R6)
    tb = e.numel() * 2
    return tb, {
        "dwconv3_fwd": (lambda: K.dwconv3_forward(e, w, b, R6, R6), 2 * tb, reps), "copy_2T": (copy_of(2 * tb), 2 * tb, reps),
        "dwconv3_bwd_data": (lambda: K.dwconv3_backward_data(da, a, e, w, R6, R6), 4 * tb, reps), "copy_4T": (copy_of(4 * tb), 4 * tb, reps),
        "dwconv3_bwd_weight": (lambda: K.dwconv3_backward_weight(da, a, e, R6, R6), 3 * tb, reps), "copy_3T": (copy_of(3 * tb), 3 * tb, reps),
    }


out = {"frames": [B, T, H, W], "dtype": "bf16", "reps": reps, "rounds": rounds, "device": torch.cuda.get_device_name(0), "configs": []}
for C in (144, 112):
    M = 4 * C
    tb, cands = kernel_cands(M)
    plan = K.dwconv3_plan(B * T, H, W, M, dt)
    print(f"C = {C}, mid = {M}: {plan}", flush=True)
    x5 = torch.randn(B, T, H, W, C, device="cuda").to(dt).requires_grad_(True)
    d5 = torch.randn(B, T, H, W, C, device="cuda").to(dt)
    chunk = H // 8  # chunk_ratios[0] = 1/8 of the 64 x 64 stage, as the few-levels configuration has it
    mixers = (("mbconv_2_fwd_bwd", Multi_MBConv(C, num_blocks=2).cuda()),
              ("morphfc_fwd_bwd", Enhanced_MorphFCs_decay(C, chunk, chunk, True, "rcab").cuda()))
    for name, mod in mixers:
        def step(mod=mod):
            x5.grad = None
            mod(x5).backward(d5)
        cands[name] = (step, 0, max(1, reps // 5))
    rows = measure(cands)
    out["configs"].append({"C": C, "mid": M, "plan": plan._asdict(), "tensor_bytes": tb, "rows": rows})
    del cands, x5, d5, mixers
    torch.cuda.empty_cache()

M = 575  # the per-element path: an odd width next to 576
tb, cands = kernel_cands(M)
plan = K.dwconv3_plan(B * T, H, W, M, dt)
print(f"mid = {M}: {plan}", flush=True)
out["configs"].append({"C": None, "mid": M, "plan": plan._asdict(), "tensor_bytes": tb, "rows": measure(cands)})

path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mbconv_bench.json")
if os.path.exists(path):  # the bench.py series of the commit and its parent (entered by hand: this tool does not run bench.py) stay with the file
    with open(path) as f:
        prev = json.load(f)
    if "bench_py" in prev:
        out["bench_py"] = prev["bench_py"]
with open(path, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", path)
