"""Train-step time of the few_levels network (bench.py's flagship workload: 4 x 7 x 3 x 64 x 64 bf16, forward + loss + backward + AdamW, eager) with
traj_mode='max' next to traj_mode='wins', in ONE process: two models, `rounds` rounds of `steps` steps each, alternating, a device synchronise around
every round; medians and the spread of the 'wins' rounds.  A one-off beside bench.py, which times 'wins' only.

    python tools/bench_step_max.py [steps] [rounds]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import vmg_amd
from vmg_amd.data import REDS_FEW_LEVELS, synthetic_clip, synthetic_target
from vmg_amd.train import TrainStep

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
B, T, S = 4, 7, 64


def build(mode):
    torch.manual_seed(0)
    m = vmg_amd.VMG(num_frames=T, image_size=[S, S], is_train=True, spynet_pretrained=None, compute_dtype=torch.bfloat16, **dict(REDS_FEW_LEVELS, traj_mode=mode))
    m.spynet = vmg_amd.SPyNet(None)
    m = m.cuda().train()
    return TrainStep(m, lr=2e-4, betas=(0.9, 0.99), aux=True, aux_ratio=0.005)


x = synthetic_clip(B, T, S, S, seed=1234, device="cuda")
y = synthetic_target(x)
ts = {mode: build(mode) for mode in ("wins", "max")}
for t in ts.values():  # warm-up of both models
    for _ in range(3):
        loss = t(x, y)
torch.cuda.synchronize()
ms = {mode: [] for mode in ts}
for _ in range(rounds):
    for mode, t in ts.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = t(x, y)
        torch.cuda.synchronize()
        ms[mode].append((time.perf_counter() - t0) / steps * 1e3)
        assert torch.isfinite(loss)
res = {mode: {"ms_per_step": round(statistics.median(v), 2), "spread": round((max(v) - min(v)) / statistics.median(v), 4),
              "lr_frames_per_s": round(B * T / statistics.median(v) * 1e3, 1)} for mode, v in ms.items()}
print(json.dumps({"workload": "few_levels train step 4x7x3x64x64 bf16, eager", "steps": steps, "rounds": rounds, **res}))
