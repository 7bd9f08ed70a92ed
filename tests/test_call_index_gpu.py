"""Inference at any call index (forward call k of a freshly loaded model runs on W * Gamma^k).

  * vmg_decay_weights through the C-ABI: n decays in one launch == n successive in-place multiplies, BIT FOR BIT (no tolerance: the
    kernel multiplies n times in a register, it never forms a power), on awkward sizes / alignments and with planted zeros, a negative
    zero, the smallest normal and a denormal; captured in a graph and replayed.
  * VMG.forward_calls / advance_calls / set_forward_calls: k calls == advance_calls(k - 1) + one call, bit for bit (outputs and mixer
    weights; a stale weight pack would give call 1's output), and against the oracle's call_index within the whole-model tolerances of
    tests/test_model_gpu.py (fp32: max |diff| <= 2e-3 on [0,1]-scale outputs; bf16: PSNR >= 40 dB against the fp32 oracle).
  * infer.plan_calls / run_calls / blend: shards of a sequence's calls computed on separate models, in any execution order, fold to the
    bits of the sequential test_clips; infer.test_clips_sharded over two gloo ranks on one card likewise."""
import ctypes
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ------------------------------------------------------------------------------------------------ the kernel
def _decay_lists(seed=7):
    """[(weight, gamma)] on the host: 144^2 aligned; 228^2 with BOTH one element past a 16-byte boundary (vector body behind 3 leading
    scalars); 7, 1 and 3 elements; 4099 elements with only the weight off the boundary (no common boundary: element by element)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n, woff, goff in [(144 * 144, 0, 0), (228 * 228, 1, 1), (7, 0, 0), (1, 0, 0), (4099, 1, 0), (3, 0, 0), (4 * 1000 + 2, 0, 0)]:
        w = torch.randn(n, generator=g) * 0.05
        gam = 1.0 - 0.5 * torch.rand(n, generator=g)  # (0.5, 1]
        planted = [0.0, -0.0, 1.17549435e-38, 1e-40, -1e-40, 2.5e-38, -1.17549435e-38]  # zeros, the smallest normal, denormals (and what decays INTO them)
        for j, v in enumerate(planted[:n]):
            w[(j * 611) % n if n > len(planted) else j] = v
        out.append((w, gam, woff, goff))
    return out


def _to_device(lists):
    ws, gs, keep = [], [], []
    for w, gam, woff, goff in lists:
        wb = torch.zeros(w.numel() + woff + 8, device="cuda")
        gb = torch.zeros(w.numel() + goff + 8, device="cuda")
        wv, gv = wb[woff:woff + w.numel()], gb[goff:goff + w.numel()]
        wv.copy_(w)
        gv.copy_(gam)
        assert wv.data_ptr() % 16 == 4 * woff and gv.data_ptr() % 16 == 4 * goff
        ws.append(wv)
        gs.append(gv)
        keep += [wb, gb]
    return ws, gs, keep


def _call_decay(ws, gs, n):
    from vmg_amd import hip
    cnt = len(ws)
    wp = (ctypes.c_void_p * cnt)(*[w.data_ptr() for w in ws])
    gp = (ctypes.c_void_p * cnt)(*[g.data_ptr() for g in gs])
    ne = (ctypes.c_int64 * cnt)(*[w.numel() for w in ws])
    hip.check(hip.lib().vmg_decay_weights(wp, gp, ne, cnt, n, hip.stream_ptr()), "vmg_decay_weights")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _assert_same_bits(ws, keep, lists, n):
    for i, (w, gam, woff, goff) in enumerate(lists):
        want = w.clone()
        for _ in range(n):
            want.mul_(gam)
        assert (want != 0).any() or w.numel() < 3
        assert torch.equal(_bits(ws[i]), _bits(want)), f"n = {n}, tensor {i} ({w.numel()} elements): {int((_bits(ws[i]) != _bits(want)).sum())} elements differ"
        wb = keep[2 * i]  # nothing outside the tensor was touched
        assert float(wb[:woff].abs().sum()) == 0.0 and float(wb[woff + w.numel():].abs().sum()) == 0.0


@pytest.mark.parametrize("n", [1, 2, 5, 17, 100])
def test_decay_weights_is_n_successive_multiplies_bit_for_bit(n):
    lists = _decay_lists()
    ws, gs, keep = _to_device(lists)
    _call_decay(ws, gs, n)
    torch.cuda.synchronize()
    _assert_same_bits(ws, keep, lists, n)


def test_decay_weights_list_longer_than_one_launch():
    """Forty tensors (the kernel's argument table holds fewer): every one decayed, through the Python wrapper, versions bumped."""
    from vmg_amd import kernels as K
    g = torch.Generator().manual_seed(11)
    host = [(torch.randn(97 + 13 * i, generator=g) * 0.05, 1.0 - 0.5 * torch.rand(97 + 13 * i, generator=g)) for i in range(40)]
    ws, gs = [w.cuda() for w, _ in host], [gm.cuda() for _, gm in host]
    v0 = [w._version for w in ws]
    K.decay_weights(ws, gs, 3)
    for (w, gm), d, v in zip(host, ws, v0):
        want = w.clone()
        for _ in range(3):
            want.mul_(gm)
        assert torch.equal(_bits(d), _bits(want)) and d._version > v
    with pytest.raises(K.HipError):
        K.decay_weights(ws, gs, 0)


@pytest.mark.parametrize("n", [1, 5])
def test_decay_weights_captured_and_replayed(n):
    lists = _decay_lists(seed=9)
    ws, gs, keep = _to_device(lists)
    scratch_w, scratch_g, _ = _to_device(lists)
    _call_decay(scratch_w, scratch_g, n)  # (first use outside the capture: the code object is loaded)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _call_decay(ws, gs, n)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    _assert_same_bits(ws, keep, lists, 3 * n)


# ------------------------------------------------------------------------------------------------ the model
def _fresh(name, dtype, fixture=None):
    from oracle import cases as C
    from tests.util import build_product
    case = C.CASES[name]
    shapes, _ = C.load_fixture(os.path.join(GOLD, f"{fixture or name}.npz"))
    sd = C.case_state_dict(case, shapes)
    m = build_product(case["cfg"], dtype)
    m.load_state_dict(sd, strict=True)
    m.eval()
    return m, sd, case


def _mixer_weights(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items() if k.endswith("mlp_h.0.weight") or k.endswith("mlp_w.0.weight")}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["vmg_tiny_few", "vmg_tiny_multi"])
def test_advance_calls_then_one_call_equals_k_calls(name, dtype):
    k = 4
    a, sd, case = _fresh(name, dtype)
    x = case["inputs"]()["x"].cuda()
    with torch.no_grad():
        outs = [a(x).float().cpu() for _ in range(k)]
    b, _, _ = _fresh(name, dtype)
    keys = list(b.state_dict().keys())
    b.advance_calls(k - 1)
    assert b.forward_calls == k - 1
    with torch.no_grad():
        got = b(x).float().cpu()
    assert a.forward_calls == k and b.forward_calls == k
    assert float((outs[0] - outs[-1]).abs().max()) > 0  # (not vacuous: call k differs from call 1)
    assert torch.equal(got, outs[-1])
    wa, wb = _mixer_weights(a), _mixer_weights(b)
    assert wa and wa.keys() == wb.keys()
    for key in wa:
        assert torch.equal(wa[key], wb[key]), key
    assert list(b.state_dict().keys()) == keys and list(a.state_dict().keys()) == keys
    # the packs follow a later advance as well (they are cached by now): calls 5, 6 on A == advance by one, call 6 on B
    with torch.no_grad():
        a(x)
        want6 = a(x).float().cpu()
        b.advance_calls(1)
        got6 = b(x).float().cpu()
    assert torch.equal(got6, want6) and a.forward_calls == b.forward_calls == k + 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["vmg_tiny_few", "vmg_tiny_multi"])
def test_call_index_matches_the_oracle(name, dtype):
    from oracle import vmg_oracle as O
    from tests.util import psnr
    k = 3
    m, sd, case = _fresh(name, dtype)
    x = case["inputs"]()["x"]
    m.set_forward_calls(k - 1)
    with torch.no_grad():
        got = m(x.cuda()).float().cpu()
        want = O.vmg_forward({key: v.clone() for key, v in sd.items()}, case["cfg"], x, mutate=False, call_index=k)
        first = O.vmg_forward({key: v.clone() for key, v in sd.items()}, case["cfg"], x, mutate=False, call_index=1)
    err, p = float((got - want).abs().max()), psnr(got, want)
    print(f"{name} {dtype} call {k}: max |hip - oracle| = {err:.3e}, PSNR = {p:.2f} dB; oracle call {k} vs call 1: {float((want - first).abs().max()):.3e}")
    assert float((want - first).abs().max()) > 0
    if dtype == torch.float32:
        assert err <= 2e-3
    else:
        assert p >= 40.0


def test_counter_resets_on_load_and_never_goes_back():
    m, sd, case = _fresh("vmg_tiny_few", torch.float32)
    keys = list(m.state_dict().keys())
    x = case["inputs"]()["x"].cuda()
    assert m.forward_calls == 0
    with torch.no_grad():
        m(x)
    m.advance_calls(2)
    m.advance_calls(0)
    assert m.forward_calls == 3
    with pytest.raises(ValueError):
        m.advance_calls(-1)
    with pytest.raises(ValueError):
        m.set_forward_calls(2)
    m.set_forward_calls(3)
    assert m.forward_calls == 3 and list(m.state_dict().keys()) == keys
    assert not any("forward_calls" in n for n, _ in list(m.named_buffers()) + list(m.named_parameters()))
    m.load_state_dict(sd, strict=True)
    assert m.forward_calls == 0 and list(m.state_dict().keys()) == keys
    for key, v in _mixer_weights(m).items():
        assert torch.equal(v.cpu(), sd[key]), key


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graphed_model_starts_at_the_given_call(dtype):
    from vmg_amd import infer
    e, sd, case = _fresh("vmg_tiny_few", dtype)
    x = case["inputs"]()["x"].cuda()
    with torch.no_grad():
        outs = [e(x).float().cpu() for _ in range(4)]
    m, _, _ = _fresh("vmg_tiny_few", dtype)
    net = infer.GraphedModel(m)
    net.set_forward_calls(2)
    got3 = net(x).float().cpu()  # (captures: the warm-up calls must neither count nor stay in the weights)
    assert net.forward_calls == 3 and m.forward_calls == 3
    assert torch.equal(got3, outs[2])
    got4 = net(x).float().cpu()
    assert net.forward_calls == 4 and torch.equal(got4, outs[3])
    assert float((outs[2] - outs[0]).abs().max()) > 0
    we, wm = _mixer_weights(e), _mixer_weights(m)
    for key in we:
        assert torch.equal(we[key], wm[key]), key


# ------------------------------------------------------------------------------------------------ plan / run / blend
CLIPS = dict(num_frames=3, overlap_frames=1, test_spatial=[64, 64], overlap_spatial=8)  # on (1, 5, 3, 72, 64): four stateful calls


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_shards_on_separate_models_blend_to_the_sequential_bits(dtype):
    from vmg_amd import infer
    seq, sd, case = _fresh("infer_vmg_clips", dtype)
    x = case["inputs"]()["x"].cuda()
    F = infer.test_clips(seq, x, 3, 1, [64, 64], 8, 4)
    assert seq.forward_calls == 4
    plan = infer.plan_calls(5, 72, 64, **CLIPS)
    assert len(plan) == 4 and [(c.index, c.t, c.origin) for c in plan] == [(1, 0, (0, 0)), (2, 0, (8, 0)), (3, 2, (0, 0)), (4, 2, (8, 0))]
    for order in ("plan", "reversed"):
        ma, mb = _fresh("infer_vmg_clips", dtype)[0], _fresh("infer_vmg_clips", dtype)[0]
        if order == "plan":
            first = infer.run_calls(ma, x, plan, range(1, 3))
            second = infer.run_calls(mb, x, plan, plan[2:4], first_call=3)
        else:
            second = infer.run_calls(mb, x, plan, range(3, 5), first_call=3)
            first = infer.run_calls(ma, x, plan, range(1, 3), first_call=1)
        assert ma.forward_calls == 2 and mb.forward_calls == 4
        got = infer.blend(plan, first + second, x.dtype)
        assert got.dtype == F.dtype and torch.equal(got, F), order
        assert not torch.equal(first[0], second[0])
    fresh = _fresh("infer_vmg_clips", dtype)[0]
    with pytest.raises(ValueError):
        infer.run_calls(fresh, x, plan, range(3, 5))  # a model in front of call 1 asked for call 3 without first_call
    with pytest.raises(ValueError):
        infer.blend(plan, first, x.dtype)
    # a second sequence continues from the count the first one left, as a single process does
    again = infer.test_clips(seq, x, 3, 1, [64, 64], 8, 4)
    assert seq.forward_calls == 8 and not torch.equal(again, F)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("geometry,dtype", [("spatial", "float32"), ("odd", "float32"), ("spatial", "bfloat16")])
def test_two_rank_sharded_sequence_equals_the_single_process(geometry, dtype, tmp_path):
    """Two fresh child processes on GPU 0 over gloo (tests/dist_child_infer.py): rank 0's frames == test_clips of one process, rank 1
    returns None, both models end at the plan's length with the single process's weights.  'odd': three temporal windows, no tiles."""
    from oracle import recipe as R
    from vmg_amd import infer
    world, port, procs = 2, _free_port(), []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_child_infer.py"), geometry, dtype, str(tmp_path)], env=env,
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
    res = [torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(world)]

    td = getattr(torch, dtype)
    m, sd, case = _fresh("infer_vmg_clips", td)
    if geometry == "spatial":
        x, args, ncalls = case["inputs"]()["x"], (3, 1, [64, 64], 8, 4), 4
    else:
        x, args, ncalls = R.synthetic_clip(1, 7, 72, 64, 94), (3, 1, None, None, 4), 3
    x = x.cuda().to(td)
    want = infer.test_clips(m, x, *args)
    assert m.forward_calls == ncalls
    assert res[1]["out"] is None and res[0]["out"] is not None
    assert res[0]["out"].dtype == want.dtype and torch.equal(res[0]["out"], want.cpu())
    wm = _mixer_weights(m)
    for r in range(world):
        assert res[r]["forward_calls"] == ncalls and res[r]["plan_len"] == ncalls
        for key in wm:
            assert torch.equal(res[r]["weights"][key], wm[key].cpu()), (r, key)
