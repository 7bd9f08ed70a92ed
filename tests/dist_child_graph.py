"""Child process of tests/test_dist_graph_gpu.py: one data-parallel rank of the tiny VMG whose train step is replayed from two graphs
around the eager gradient exchange (TrainStep.capture with a reducer).

    python tests/dist_child_graph.py <mode> <outdir>     (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment)

All ranks use GPU 0.  Backend: VMG_DIST_BACKEND = 'gloo' (two ranks on a one-GPU box) or 'nccl' (= RCCL; ONE rank, every collective issued).
mode 'graph' : refusals first, then capture(x, y, warmup=2) and 3 replayed steps; per step the state the step started from (weights, moments,
               rates), the exchanged gradients and the weights at that moment (grad_hook) and the order in which exchange() issued the buckets; a checkpoint after replay 2.
mode 'resume': a fresh step loads that checkpoint, captures and replays once.
mode 'bf16'  : exchange_dtype = torch.bfloat16 (RCCL only); the flat gradient buffer is cloned right before and right after exchange().
Writes <outdir>/<mode>_rank<r>.pt."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCHEDULE = dict(T_period=[40], eta_min=1e-7, flow_fix=1, pre_lr_ratio=0.125, warmup_iter=-1)
LR, GRAD_CLIP = 1e-4, 0.05


def _cpu(d):
    return {k: v.detach().cpu().clone() for k, v in d.items()}


def _moments(step, m):
    off_of = {id(p): o for p, o in zip(step.opt.params, step.opt.offsets)}
    mm, vv = {}, {}
    for n, p in m.named_parameters():
        o = off_of[id(p)]
        mm[n] = step.opt.m[o:o + p.numel()].view_as(p).cpu().clone()
        vv[n] = step.opt.v[o:o + p.numel()].view_as(p).cpu().clone()
    return mm, vv


def _raises(fn, exc):
    try:
        fn()
    except exc as e:
        return str(e) or type(e).__name__
    return ""


def main():
    mode, outdir = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    backend = os.environ.get("VMG_DIST_BACKEND", "gloo")
    if backend == "nccl":
        assert world == 1, "one RCCL rank per device"
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import cases as C
    from oracle import recipe as R
    from tests.util import build_product
    from vmg_amd.train import TrainStep
    name = "vmg_tiny_few"
    case = C.CASES[name]
    cfg = case["cfg"]
    shapes, _ = C.load_fixture(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
    sd = C.case_state_dict(case, shapes, seed=rank)  # different weights per rank on purpose: the wrap must broadcast rank 0's
    m = build_product(cfg, torch.float32)
    m.load_state_dict(sd)
    m.train()
    x = R.synthetic_clip(1, cfg.num_frames, 64, 64, 60 + rank).cuda()
    y = R.synthetic_target(x.cpu()).cuda()
    res = {"backend": dist.get_backend(), "refused": {}}
    kw = dict(lr=LR, distributed=True, bucket_bytes=16 << 10, single_rank_collectives=world == 1, schedule=dict(SCHEDULE), grad_clip=GRAD_CLIP)

    if mode == "graph" and backend == "gloo":
        p0 = next(m.parameters()).data_ptr()
        res["refused"]["bf16_on_gloo"] = _raises(lambda: TrainStep(m, exchange_dtype=torch.bfloat16, **kw), ValueError)
        assert next(m.parameters()).data_ptr() == p0  # refused before the parameters were re-homed
    ckpt = os.path.join(outdir, f"ckpt_rank{rank}.pt")
    if mode == "resume":
        saved = torch.load(ckpt)
        m.load_state_dict(saved["model"])
    step = TrainStep(m, exchange_dtype=torch.bfloat16 if mode == "bf16" else torch.float32, **kw)
    if mode == "resume":
        step.load_state_dict(saved["train"])
        res["loaded"] = {"iter": step.iter, "t": step.opt.t, "lrs": [g["lr"] for g in step.opt.param_groups]}
    res["spy_initial"] = torch.cat([p.detach().reshape(-1) for p in m.spynet.parameters()]).cpu().clone()
    red = step.reducer

    # every all-reduce this rank issues while `rec["on"]`: which bucket's slice (of the flat gradient buffer or of the bf16 payload) it carries
    rec = {"on": False, "order": []}
    real = dist.all_reduce

    def logged(t, *a, **k):
        if rec["on"]:
            hit = [i for i, f in enumerate(red.flat) if f.data_ptr() == t.data_ptr() and f.numel() == t.numel()]
            if step._payload is not None:
                hit += [i for i, (lo, hi) in enumerate(red.bounds) if step._payload.data_ptr() + 2 * lo == t.data_ptr() and hi - lo == t.numel()]
            rec["order"].append(hit[0] if len(hit) == 1 else -1)
        return real(t, *a, **k)
    dist.all_reduce = logged

    log = []

    def hook(ts):
        log[-1]["grads"] = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
        # the weights the optimizer is about to update: the step's starting weights, except the MorphFC mixer weights, which this step's forward
        # has multiplied by their Gamma in place (the retention decay)
        log[-1]["params"] = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    step.grad_hook = hook

    if mode == "graph":
        res["refused"]["replayer"] = _raises(lambda: step.capture(x, y, warmup=2, replayer=True), RuntimeError)
        assert step.iter == 0 and step.opt.t == 0 and step.graph is None
    if mode == "bf16":
        res["refused"]["bf16_eager"] = _raises(lambda: step(x, y), RuntimeError)
        assert step.iter == 0 and step.opt.t == 0
    step.grad_hook = None
    step.capture(x, y, warmup=2)
    step.grad_hook = hook
    res["warmup_steps"] = step.iter
    res["buckets"] = len(red.buckets)
    assert red.active and not red.enabled and step.graph is not None and step.graph_update is not None

    if mode == "bf16":
        seen = {}
        exchange = red.exchange

        def wrapped(payload=None):
            seen["before"] = step.opt.g.clone()
            exchange(payload)
            seen["after"] = step.opt.g.clone()
            seen["payload"] = payload
        red.exchange = wrapped

    n_replays = {"graph": 3, "resume": 1, "bf16": 2}[mode]
    for it in range(n_replays):
        mm, vv = _moments(step, m)
        log.append({"state": _cpu(m.state_dict()), "m": mm, "v": vv, "t": step.opt.t, "iter": step.iter,
                    "lrs": [g["lr"] for g in step.opt.param_groups]})
        rec["on"], rec["order"] = True, []
        loss = step(x, y)
        rec["on"] = False
        torch.cuda.synchronize()
        log[-1]["order"] = list(rec["order"])
        log[-1]["loss"] = float(loss)
        log[-1]["grad_norm"] = step.grad_norm.cpu().clone()
        log[-1]["reducer_reset"] = red.pending == [len(b) for b in red.buckets] and red.works == [] and len(red._seen) == 0
        if mode == "bf16":
            log[-1]["g_before"], log[-1]["g_after"] = seen["before"].cpu(), seen["after"].cpu()
            log[-1]["payload_is_the_steps"] = seen["payload"] is step._payload and seen["payload"].data_ptr() == step._payload.data_ptr()
        if mode == "graph" and it == 1:  # "after replay 2"
            train = step.state_dict()
            train["opt"]["m"] = [t.cpu() for t in train["opt"]["m"]]
            train["opt"]["v"] = [t.cpu() for t in train["opt"]["v"]]
            torch.save({"model": _cpu(m.state_dict()), "train": train}, ckpt)
            res["saved"] = {"iter": step.iter, "t": step.opt.t, "lrs": [g["lr"] for g in step.opt.param_groups]}
    mm, vv = _moments(step, m)
    res["final"] = {"state": _cpu(m.state_dict()), "m": mm, "v": vv, "t": step.opt.t, "iter": step.iter,
                    "lrs": [g["lr"] for g in step.opt.param_groups]}
    res["finite"] = all(bool(torch.isfinite(v).all()) for v in res["final"]["state"].values() if v.is_floating_point())

    if mode == "graph":
        res["refused"]["grad_acc"] = _raises(lambda: step(x, y, grad_acc=2), RuntimeError)
        assert step.iter == res["final"]["iter"]
        # the weight packs follow the replayed optimizer: the trained module and a fresh one loaded with its weights give the same eval output
        # (every forward call multiplies the MorphFC mixer weights by their Gamma in place, so the weights are taken BEFORE the trained module's call)
        with torch.no_grad():
            now = {k: v.detach().clone() for k, v in m.state_dict().items()}
            out_a = m.eval()(x).float().cpu()
            fresh = build_product(cfg, torch.float32)
            fresh.load_state_dict(now)
            out_b = fresh.eval()(x).float().cpu()
        res["eval_trained"], res["eval_fresh"] = out_a, out_b
    dist.all_reduce = real
    torch.save({"log": log, **res}, os.path.join(outdir, f"{mode}_rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
