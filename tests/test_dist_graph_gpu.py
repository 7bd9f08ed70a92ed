"""The data-parallel train step replayed from two graphs around the eager gradient exchange (TrainStep.capture with a reducer):
graph A (forward, loss, backward, deferred weight gradients) -> GradBucketReducer.exchange() -> grad_hook -> graph B (clip, AdamW, repack, clear).

Fresh child processes (tests/dist_child_graph.py) on GPU 0: two ranks over gloo, and one rank on RCCL with every collective issued.  Each run
is made once (module-scoped fixtures) and looked at by several tests.  The helpers follow tests/test_distributed_gpu.py."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = "vmg_tiny_few"
REPLAYS = 3


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _local_grads(state, clip_seed):
    """Single-process gradients of one rank's sample on the weights a step started from."""
    from oracle import cases as C
    from oracle import recipe as R
    from tests.util import build_product
    from vmg_amd.train import charbonnier_edge_loss_hip
    cfg = C.CASES[CASE]["cfg"]
    m = build_product(cfg, torch.float32)
    m.load_state_dict(state)
    m.train()
    x = R.synthetic_clip(1, cfg.num_frames, 64, 64, clip_seed).cuda()
    y = R.synthetic_target(x.cpu()).cuda()
    loss = charbonnier_edge_loss_hip(m(x).float(), y.float())
    loss.backward()
    return {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}


def _run_children(mode, outdir, world, backend="gloo"):
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   VMG_DIST_BACKEND=backend)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (dmabuf IPC for RCCL, as in tests/test_distributed_gpu.py)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_child_graph.py"), mode, str(outdir)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out[-3000:]
    return [torch.load(os.path.join(outdir, f"{mode}_rank{r}.pt")) for r in range(world)]


def _check_exchange(res, world, tol=2e-3):
    """tests/test_distributed_gpu.py::_check_exchange over the replayed steps: identical replicas, and the exchanged gradients equal the average of
    the single-process local gradients on the step's starting weights -- relative to the tensor's scale, floored at 1e-3 of the model's largest."""
    for it in range(len(res[0]["log"])):
        s0 = res[0]["log"][it]["state"]
        for r in range(1, world):
            for key in ("state", "m", "v"):
                a, b = res[0]["log"][it][key], res[r]["log"][it][key]
                for k in a:
                    assert torch.equal(a[k], b[k]), f"step {it}: {key}[{k}] differs between the ranks"
        want = None
        for rank in range(world):
            g = _local_grads(s0, 60 + rank)
            want = g if want is None else {n: want[n] + g[n] for n in g}
        gmax = max(float(v.abs().max()) for v in want.values()) / world
        for n in want:
            ref = want[n] / world
            for r in range(world):
                got = res[r]["log"][it]["grads"][n]
                scale = max(float(ref.abs().max()), 1e-3 * gmax)
                err = float((got - ref).abs().max()) / scale
                assert err <= tol, f"replayed step {it} rank {r}: {n} relative error {err:.2e}"


def _check_order(res):
    for r, one in enumerate(res):
        assert one["buckets"] >= 3
        for it, rec in enumerate(one["log"]):
            assert rec["order"] == list(range(one["buckets"])), f"rank {r} step {it}: buckets were issued as {rec['order']}"
            assert rec["reducer_reset"]


def _host_lrs(n_steps):
    """Group rates after n_steps optimizer steps, from a host-only LRSchedule over two dummy groups (SPyNet lr 0, the rest)."""
    from tests.dist_child_graph import LR, SCHEDULE
    from vmg_amd.train import LRSchedule
    groups = [{"lr": 0.0}, {"lr": LR}]
    sch = LRSchedule(groups, **SCHEDULE)
    for i in range(n_steps):
        sch.step(i)
    return [g["lr"] for g in groups]


def _check_bookkeeping(one):
    """iter, the learning rates and SPyNet's freeze follow the schedule through the warm-up steps and the replays."""
    from tests.dist_child_graph import SCHEDULE
    k = one["warmup_steps"]
    assert 2 <= k <= 8
    recs = one["log"] + [one["final"]]
    assert one["final"]["iter"] == k + REPLAYS and one["final"]["t"] == k + REPLAYS
    spy_keys = [n for n in recs[0]["grads"] if n.startswith("spynet.")]  # (named_parameters order = the order of m.spynet.parameters())
    assert spy_keys
    spy = lambda st: torch.cat([st[n].reshape(-1) for n in spy_keys])
    moved_once = False
    for j, rec in enumerate(recs):
        assert rec["iter"] == k + j and rec["t"] == k + j
        assert rec["lrs"] == _host_lrs(k + j), (j, rec["lrs"])
        if j == len(recs) - 1:
            break
        # optimizer step number i (0-based) runs with the rates schedule.step(i - 1) left: SPyNet's is 0 while i - 1 <= flow_fix
        frozen = (k + j) - 1 <= SCHEDULE["flow_fix"]
        assert (rec["lrs"][0] == 0.0) == frozen
        same = torch.equal(spy(rec["state"]), spy(recs[j + 1]["state"]))
        assert same == frozen, f"step {k + j}: SPyNet {'did not move' if same else 'moved'} at lr {rec['lrs'][0]:.3e}"
        moved_once |= not same
        rest = [n for n in rec["grads"] if not n.startswith("spynet.")]
        assert any(not torch.equal(rec["state"][n], recs[j + 1]["state"][n]) for n in rest)
    assert moved_once
    # the warm-up steps 0 .. k - 1 are frozen ones while i - 1 <= flow_fix
    assert (spy(recs[0]["state"]).numel() == one["spy_initial"].numel())
    assert torch.equal(spy(recs[0]["state"]), one["spy_initial"]) == (k - 2 <= SCHEDULE["flow_fix"])


def _check_adamw(one):
    """Each replayed step against torch.optim.AdamW + clip_grad_norm_ on the logged weights, moments and exchanged gradients; the bound
    is the one of tests/test_optim_gpu.py::test_flat_adamw_matches_torch_adamw (2e-6 of max(1, |p|max): fused multiply-adds round differently)."""
    from tests.dist_child_graph import GRAD_CLIP
    recs = one["log"] + [one["final"]]
    for j, rec in enumerate(one["log"]):
        names = list(rec["grads"])
        # the update starts from the weights as they stood between the graphs (logged by the grad_hook): the starting state, except that the forward
        # multiplies the MorphFC mixers' mlp_h / mlp_w weights by their Gamma in place at every call
        decayed = [n for n in names if not torch.equal(rec["params"][n], rec["state"][n])]
        assert decayed and all(n.endswith((".mlp_h.0.weight", ".mlp_w.0.weight")) for n in decayed), decayed
        ps = {n: torch.nn.Parameter(rec["params"][n].clone()) for n in names}
        for n in names:
            ps[n].grad = rec["grads"][n].clone()
        spy = [ps[n] for n in names if n.startswith("spynet.")]
        rest = [ps[n] for n in names if not n.startswith("spynet.")]
        opt = torch.optim.AdamW([{"params": spy, "lr": rec["lrs"][0]}, {"params": rest, "lr": rec["lrs"][1]}], betas=(0.9, 0.99), weight_decay=0.0,
                                foreach=False)
        for n in names:
            opt.state[ps[n]] = {"step": torch.tensor(float(rec["t"])), "exp_avg": rec["m"][n].clone(), "exp_avg_sq": rec["v"][n].clone()}
        norm = torch.nn.utils.clip_grad_norm_(list(ps.values()), GRAD_CLIP, norm_type=2)
        got_norm = float(rec["grad_norm"][0])
        assert abs(got_norm - float(norm)) <= 1e-5 * float(norm), (got_norm, float(norm))
        opt.step()
        for n in names:
            after = recs[j + 1]["state"][n]
            err = float((after - ps[n].detach()).abs().max())
            assert err <= 2e-6 * max(1.0, float(ps[n].detach().abs().max())), f"step {j}: {n}: {err:.3e}"


@pytest.fixture(scope="module")
def gloo_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("gloo2")
    return d, _run_children("graph", d, 2)


@pytest.fixture(scope="module")
def rccl_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("rccl1")
    return d, _run_children("graph", d, 1, backend="nccl")


def test_two_ranks_over_gloo_exchange_between_the_graphs(gloo_run):
    _, res = gloo_run
    assert len(res[0]["log"]) == REPLAYS and res[0]["backend"] == "gloo"
    _check_order(res)
    _check_exchange(res, 2)
    for key in ("state", "m", "v"):
        for k in res[0]["final"][key]:
            assert torch.equal(res[0]["final"][key][k], res[1]["final"][key][k]), f"final {key}[{k}] differs between the ranks"


def test_single_rank_on_rccl_exchanges_between_the_graphs(rccl_run):
    _, res = rccl_run
    assert len(res[0]["log"]) == REPLAYS and res[0]["backend"] == "nccl"
    _check_order(res)
    _check_exchange(res, 1)


@pytest.mark.parametrize("which", ["gloo", "rccl"])
def test_update_phase_ran_and_the_bookkeeping_followed(which, request):
    _, res = request.getfixturevalue(f"{which}_run")
    for one in res:
        assert one["finite"]
        _check_bookkeeping(one)
    _check_adamw(res[0])
    # the weight packs are current after the replays
    assert torch.equal(res[0]["eval_trained"], res[0]["eval_fresh"])


def test_refusals(gloo_run, rccl_run):
    for res in (gloo_run[1], rccl_run[1]):
        for one in res:
            assert "replayer" in one["refused"]["replayer"]
            assert "accumulation" in one["refused"]["grad_acc"]
    for one in gloo_run[1]:
        assert "gloo" in one["refused"]["bf16_on_gloo"]


def test_state_dict_resumes_under_the_two_graph_replay(gloo_run):
    """The checkpoint written after replay 2 loads into a fresh step in a second pair of children; capture's warm-up steps and one replay continue
    iter and the learning-rate sequence."""
    d, res = gloo_run
    saved = res[0]["saved"]
    k = res[0]["warmup_steps"]
    assert saved["iter"] == k + 2 and saved["lrs"] == _host_lrs(k + 2)
    again = _run_children("resume", d, 2)
    for one in again:
        assert one["loaded"] == saved
        w = one["warmup_steps"] - saved["iter"]
        assert 2 <= w <= 8
        rec, fin = one["log"][0], one["final"]
        assert rec["iter"] == saved["iter"] + w and rec["lrs"] == _host_lrs(saved["iter"] + w)
        assert fin["iter"] == saved["iter"] + w + 1 and fin["t"] == fin["iter"] and fin["lrs"] == _host_lrs(fin["iter"])
        assert one["finite"] and rec["order"] == list(range(one["buckets"]))
    for k_ in again[0]["final"]["state"]:
        assert torch.equal(again[0]["final"]["state"][k_], again[1]["final"]["state"][k_])


def test_bf16_payload_on_one_rccl_rank(tmp_path):
    """exchange_dtype = torch.bfloat16 on ONE RCCL rank (scale 1 / world = 1, the sum over one rank is the value itself): after exchange() the flat
    gradient buffer is bit-equal to bfloat16(g_before) widened again.  g_before is a clone taken right before exchange() in the same step (the child
    wraps the reducer's method), so the check does not lean on the model being bit-stable from run to run.  The steps after it run finite."""
    res = _run_children("bf16", tmp_path, 1, backend="nccl")[0]
    assert "capture" in res["refused"]["bf16_eager"]
    assert res["buckets"] >= 3 and res["finite"]
    for it, rec in enumerate(res["log"]):
        assert rec["payload_is_the_steps"]
        assert rec["order"] == list(range(res["buckets"])), rec["order"]
        assert float(rec["g_before"].abs().max()) > 0
        want = rec["g_before"].to(torch.bfloat16).float()
        assert torch.equal(rec["g_after"].view(torch.int32), want.view(torch.int32)), f"step {it}"
        assert rec["loss"] == rec["loss"] and abs(rec["loss"]) < float("inf")
