"""The kernels of the patch-shift FFN (csrc/shift_ffn.hip: vmg_patch_shift_fwd / _bwd, vmg_group_reduce2, vmg_se_mlp2_fwd / _bwd, vmg_mix2_fwd / _bwd)
next to a device copy that moves the same bytes, and the whole FFN (Mlp_cnn_shift, forward + backward) next to Mlp_cnn at the same shape, in ONE
process, at the bench shape of stage 0 -- 4 x 7 frames of 64 x 64 pixels, bf16 -- for C = 144, hidden 288 (chunk widths 32 and 16: the vector path)
and C = 112, hidden 672 (chunk widths 75 and 13: the per-element path).  Stream events around `reps` launches after a warm-up, `rounds` rounds with
all candidates ALTERNATING inside a round; reported: the median over the rounds in us, the rate over the bytes the kernel has to move, the median of
the copy of the same bytes, and the spread (max - min) / median.  Bytes per call in tensors of the kernel's shape: shift 1 in + 1 out = 2, the GELU
shift's backward 2 + 1 = 3, group_reduce2 3 in, mix2 forward 2 + 1 = 3, mix2 backward 1 + 2 = 3 (the (G, C) coefficients are noise; the SE MLP
moves kilobytes and is reported as a time only).  Writes profiles/shift_ffn_bench.json.

    python tools/bench_shift_ffn.py [reps] [rounds]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vmg_amd import kernels as K
from vmg_amd.model import Mlp_cnn, Mlp_cnn_shift

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
if not torch.cuda.is_available():
    raise SystemExit("bench_shift_ffn.py measures on the GPU; none is visible")
torch.manual_seed(0)
B, T, H, W = 4, 7, 64, 64
dt = torch.bfloat16


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
        print("  %-22s %8.1f us %s (spread %4.1f %%)" % (k, row["us"], "%5.2f TB/s" % row["TBps"] if "TBps" in row else "          ", 100 * row["spread"]), flush=True)
    return rows


out = {"frames": [B, T, H, W], "dtype": "bf16", "reps": reps, "rounds": rounds, "device": torch.cuda.get_device_name(0), "configs": []}
for C, r in ((144, 2), (112, 6)):
    hid = int(C * r)
    N = B * T
    xh = torch.randn(N, H, W, hid, device="cuda").to(dt)
    u, d, h, w = (torch.randn(N, H, W, C, device="cuda").to(dt) for _ in range(4))
    tb_h, tb_c = xh.numel() * 2, u.numel() * 2
    coef = torch.softmax(torch.randn(B, C, 2, device="cuda"), -1).contiguous()
    dm = torch.randn(B, C, device="cuda") * 1e-3
    m = torch.randn(B, C, device="cuda")
    w1, b1, w2, b2 = (torch.randn(s, device="cuda") * 0.1 for s in ((C // 4, C), (C // 4,), (2 * C, C // 4), (2 * C,)))
    pre, a = K.se_mlp2_forward(m, w1, b1, w2, b2)
    da = torch.randn(B, 2 * C, device="cuda")
    print(f"C = {C}, hidden = {hid}: routes {K.patch_shift_route(hid, dt)} (hidden), {K.patch_shift_route(C, dt)} (C)", flush=True)
    cands = {
        "shift_fwd_hidden": (lambda: K.patch_shift_forward(xh, 1), 2 * tb_h, reps), "copy_2T_hidden": (copy_of(2 * tb_h), 2 * tb_h, reps),
        "shift_bwd_hidden": (lambda: K.patch_shift_backward(xh, 1), 2 * tb_h, reps),
        "shift_inv_gelu_fwd": (lambda: K.patch_shift_forward(u, -1, True), 2 * tb_c, reps), "copy_2T": (copy_of(2 * tb_c), 2 * tb_c, reps),
        "shift_inv_gelu_bwd": (lambda: K.patch_shift_backward(d, -1, u), 3 * tb_c, reps), "copy_3T": (copy_of(3 * tb_c), 3 * tb_c, reps),
        "group_reduce2": (lambda: K.group_reduce2(d, h, w, B), 3 * tb_c, reps),
        "mix2_fwd": (lambda: K.mix2_forward(h, w, coef, B), 3 * tb_c, reps),
        "mix2_bwd": (lambda: K.mix2_backward(d, coef, dm, B), 3 * tb_c, reps),
        "se_mlp2_fwd": (lambda: K.se_mlp2_forward(m, w1, b1, w2, b2), 0, reps),
        "se_mlp2_bwd": (lambda: K.se_mlp2_backward(da, a, m, pre, w1, w2, 1.0 / (T * H * W)), 0, reps),
    }
    x5 = torch.randn(B, T, H, W, C, device="cuda").to(dt).requires_grad_(True)
    d5 = torch.randn(B, T, H, W, C, device="cuda").to(dt)
    for name, mod in (("ffn_cnn_shift_fwd_bwd", Mlp_cnn_shift(C, exp_r=r).cuda()), ("ffn_cnn_fwd_bwd", Mlp_cnn(C, exp_r=r, n_groups=1).cuda())):
        def step(mod=mod):
            x5.grad = None
            mod(x5).backward(d5)
        cands[name] = (step, 0, max(1, reps // 5))
    rows = measure(cands)
    out["configs"].append({"C": C, "hidden": hid, "routes": {"hidden": K.patch_shift_route(hid, dt), "C": K.patch_shift_route(C, dt)},
                           "tensor_bytes": {"hidden": tb_h, "C": tb_c}, "rows": rows})
    del cands, xh, u, d, h, w, x5, d5
    torch.cuda.empty_cache()

path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "shift_ffn_bench.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", path)
