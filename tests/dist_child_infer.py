"""Child process of tests/test_call_index_gpu.py: one rank of a sharded sliding-window run of the tiny VMG (infer.test_clips_sharded).

    python tests/dist_child_infer.py <geometry> <dtype> <outdir>     (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment)

All ranks use GPU 0 and talk over gloo.  Every rank loads the same weights; geometry 'spatial' = the (1, 5, 3, 72, 64) clip of the oracle
case infer_vmg_clips through temporal windows 3 / 1 and tiles 64 / 8 (four calls), 'odd' = seven frames through windows 3 / 1 without tiles
(three calls).  Writes the frames (rank 0) or None, the model's call count and its mixer weights to <outdir>/rank<r>.pt."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    geometry, dtype, outdir = sys.argv[1], getattr(torch, sys.argv[2]), sys.argv[3]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import cases as C
    from oracle import recipe as R
    from tests.util import build_product
    from vmg_amd import infer
    case = C.CASES["infer_vmg_clips"]
    shapes, _ = C.load_fixture(os.path.join(ROOT, "tests", "golden", "infer_vmg_clips.npz"))
    m = build_product(case["cfg"], dtype)
    m.load_state_dict(C.case_state_dict(case, shapes), strict=True)
    m.eval()
    if geometry == "spatial":
        x, args = case["inputs"]()["x"], (3, 1, [64, 64], 8, 4)
    else:
        x, args = R.synthetic_clip(1, 7, 72, 64, 94), (3, 1, None, None, 4)
    x = x.cuda().to(dtype)
    out = infer.test_clips_sharded(m, x, *args)
    plan = infer.plan_calls(x.shape[1], x.shape[3], x.shape[4], *args[:4])
    weights = {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if k.endswith("mlp_h.0.weight") or k.endswith("mlp_w.0.weight")}
    torch.save({"out": None if out is None else out.cpu(), "forward_calls": m.forward_calls, "plan_len": len(plan), "weights": weights},
               os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
