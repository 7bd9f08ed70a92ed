"""traj_mode 'max' through the product modules and the whole model, against the reference's recorded numbers (tests/golden/ltam_max.npz) and the oracle
recurrence with its attention step replaced by the max-mode one (tests/traj_max_util.ltam_max_oracle, monkeypatched over oracle.vmg_oracle.ltam_wins:
O.trajectory and O.vmg_forward look the name up at call time).  Tolerances are those the 'wins' tests of tests/test_modules_gpu.py,
tests/test_grad_gpu.py and tests/test_long_clip_gpu.py use."""
import numpy as np
import pytest
import torch

from tests import traj_max_util as MU

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
# bf16 PSNR of the tiny few-levels model against the fp32 oracle on the MI355X: 'wins' 48.6 dB (tests/test_long_clip_gpu.py); 'max', T = 67: see
# test_tiny_model_on_a_67_frame_clip_bf16 -- measured 47.83 dB (0.8 dB below 'wins'), the floor is that minus 3 dB
PSNR_BF16_MAX_T67 = 47.83


@pytest.fixture()
def max_oracle(monkeypatch):
    from oracle import vmg_oracle as O
    monkeypatch.setattr(O, "ltam_wins", MU.ltam_max_oracle)
    return O


def _recorded(z, name):
    return dict(sub=z[name + "/sub"], sums=z[name + "/sums"], shape=tuple(z[name + "/shape"]))


def _ltam_inputs(g):
    from oracle import cases as C
    from oracle import recipe as R
    n, t, h, w, c, s = g["n"], g["t"], g["h"], g["w"], g["c"], g["seed"]
    return dict(q=R.seeded((n, h, w, c), s), keys=R.seeded((n, t, h, w, c), s + 1), anchor=R.seeded((n, h, w, c), s + 2),
                vals=R.seeded((n, t, h, w, c), s + 3), loc=C.int_locations(n, t, h, w, s + 4), dout=R.seeded((n, h, w, c), s + 5))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", [0, 1], ids=["9x7-c32", "16x16-c144"])
def test_ltam_fixture_through_the_product_module(which, dtype):
    """(a) LTAM_multi_head(mode='max') incl. the output projection and the anchor add against the reference's recorded numbers: the output in both
    dtypes at the tolerances of test_modules_gpu.test_ltam_fixture_through_the_product_module (2e-4 / 3e-2 of the scale), and in fp32 also the
    gradients w.r.t. q, keys, vals and anchor (2e-4 of each tensor's scale)."""
    from oracle import cases as C
    from oracle import recipe as R
    from vmg_amd.model import LTAM_multi_head
    z, meta = MU.fixture()
    g = meta["ltam"][which]
    inp = _ltam_inputs(g)
    c = g["c"]
    m = LTAM_multi_head(c, 4, True, (2, 2), mode="max").cuda()
    m.load_state_dict(R.recipe_state_dict({"proj.weight": [c, c], "proj.bias": [c]}, 0), strict=True)
    dev = lambda t: t.cuda().to(dtype).contiguous().requires_grad_(True)
    q, anchor = dev(inp["q"]), dev(inp["anchor"])
    keys, vals = [dev(k) for k in inp["keys"].unbind(1)], [dev(v) for v in inp["vals"].unbind(1)]
    got = m(q, keys, anchor, vals, inp["loc"].cuda())
    got.backward(inp["dout"].cuda().to(dtype))
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    tensors = {"out": got, "dq": q.grad, "dkeys": torch.stack([k.grad for k in keys], 1), "dvals": torch.stack([v.grad for v in vals], 1), "danchor": anchor.grad}
    for nm, t in tensors.items():
        if dtype != torch.float32 and nm != "out":
            continue
        t = t.detach().float().cpu()
        if g["whole"]:
            want = torch.from_numpy(z[f"{g['name']}/{nm}"])
            err, scale = (t.reshape(want.shape) - want).abs(), max(1.0, float(want.abs().max()))
        else:
            r = _recorded(z, f"{g['name']}/{nm}")
            assert tuple(t.shape) == r["shape"]
            err, scale = torch.from_numpy(np.abs(C.subsample(t) - r["sub"])), max(1.0, float(np.abs(r["sub"]).max()))
        print(f"{g['name']} {nm} {dtype}: max err {float(err.max()):.3e} (scale {scale:.3g}), share over the tolerance {float((err > tol * scale).double().mean()):.2e}")
        assert float(err.max()) <= tol * scale, nm


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_trajectory_fixture_through_the_product_module(dtype, max_oracle):
    """(b) Trajectory_multi_head(mode='max') on 5 frames of 15 x 13 (odd map, partial tiles, stride 2: two key-frames to choose from at steps 3 and 4)
    against the patched oracle and the reference's recorded output; tolerances of test_modules_gpu.test_trajectory_fixture_through_the_product_module."""
    from oracle import cases as C
    from oracle import recipe as R
    from vmg_amd.model import Trajectory_multi_head
    O = max_oracle
    z, meta = MU.fixture()
    g = meta["trajectory"]
    n, T, h, w, c, s = g["n"], g["T"], g["h"], g["w"], g["c"], g["seed"]
    x, ff, fb = R.seeded((n, T, h, w, c), s), R.seeded((n, T - 1, 2, h, w), s + 1, 1.5), R.seeded((n, T - 1, 2, h, w), s + 2, 1.5)
    sd = R.recipe_state_dict(meta["trajectory_shapes"], 0)
    assert not any("relative_pos_encoding" in k or "decay_v" in k for k in sd)
    m = Trajectory_multi_head(c, 2, 2, 4, True, 0.1, (2, 2), mode="max").cuda()
    m.load_state_dict(sd, strict=True)
    m.eval()
    with torch.no_grad():
        got = m(x.cuda().to(dtype), ff.cuda(), fb.cuda()).float().cpu()
        want = O.trajectory({k: v.clone() for k, v in sd.items()}, "", x, ff, fb, O.VMGConfig(traj_keyframes_n=(2, None), traj_heads=(4, None), r_scaling=0.1), 0, 2)
    tol = 2e-4 if dtype == torch.float32 else 4e-2
    scale = max(1.0, float(want.abs().max()))
    err = float((got.reshape(want.shape) - want).abs().max())
    ref = _recorded(z, g["name"] + "/out")
    err_ref = float(np.abs(C.subsample(got) - ref["sub"]).max())
    print(f"trajectory max ({dtype}): max |hip - oracle| = {err:.3e}, |hip - reference| = {err_ref:.3e} (scale {scale:.3g})")
    assert err <= tol * scale and err_ref <= tol * scale


@pytest.mark.parametrize("shape", [(1, 7, 15, 13), (1, 67, 9, 7)], ids=["T7-15x13", "T67-9x7"])
def test_trajectory_module_gradients_match_the_patched_oracle(shape, max_oracle):
    """fp32: loss and the gradients of every parameter and of the input at stride 2.  T = 7: up to three key-frames to choose from; T = 67: 34
    key-frames, the last steps run the table route.  Bounds of tests/test_long_clip_gpu.py::test_trajectory_module_backward_on_a_long_clip."""
    from oracle import recipe as R
    from vmg_amd.model import Trajectory_multi_head
    O = max_oracle
    _, meta = MU.fixture()
    (n, T, h, w), c = shape, 32
    x, ff, fb = R.seeded((n, T, h, w, c), 325), R.seeded((n, T - 1, 2, h, w), 326, 1.5), R.seeded((n, T - 1, 2, h, w), 327, 1.5)
    tgt = R.seeded((n, T, h, w, c), 328)
    sd = R.recipe_state_dict(meta["trajectory_shapes"], 0)
    m = Trajectory_multi_head(c, 2, 2, 4, True, 0.1, (2, 2), mode="max").cuda()
    m.load_state_dict(sd, strict=True)
    m.train()
    xd = x.cuda().requires_grad_(True)
    loss = ((m(xd, ff.cuda(), fb.cuda()).float() - tgt.cuda()) ** 2).mean()
    loss.backward()
    params = dict(m.named_parameters())
    osd = {k: v.clone().requires_grad_(k in params) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    want = O.trajectory(osd, "", xo, ff, fb, O.VMGConfig(traj_keyframes_n=(2, None), traj_heads=(4, None), r_scaling=0.1), 0, 2)
    oloss = ((want - tgt) ** 2).mean()
    oloss.backward()
    assert abs(loss.item() - oloss.item()) <= 1e-4 * abs(oloss.item())
    grads = {k: (p.grad, osd[k].grad) for k, p in params.items()}
    grads["x"] = (xd.grad, xo.grad)
    assert len(grads) == len(sd) + 1
    gmax = max(float(wg.abs().max()) for _, wg in grads.values())
    for k, (gg, wg) in grads.items():
        assert gg is not None and wg is not None, k
        scale = max(float(wg.abs().max()), 1e-3 * gmax)
        err = float((gg.float().cpu().reshape(wg.shape) - wg).abs().max()) / scale
        print(f"grad {k}: relative error {err:.3e}")
        assert err <= 5e-3, f"{k}: relative gradient error {err:.3e}"


def _tiny(dtype, T=None, **extra):
    from oracle import cases as C
    _, meta = MU.fixture()
    sd = MU.tiny_state_dict(meta)
    cfg = C.cfg_tiny_few(T or meta["tiny"]["T"])
    m = MU.build_product_max(cfg, dtype, **extra)
    m.load_state_dict(sd, strict=True)
    return m, sd, cfg, meta


def test_tiny_model_against_the_reference_fixture_fp32(max_oracle):
    """(c) the tiny few-levels model with traj_mode='max', call 1: the reference's recorded output and the patched oracle, at the tolerance the tiny
    'wins' model is held to (2e-3, tests/test_infer_gpu.py / test_call_index_gpu.py)."""
    from oracle import cases as C
    from oracle import recipe as R
    O = max_oracle
    z, _ = MU.fixture()
    m, sd, cfg, meta = _tiny(torch.float32)
    m.eval()
    x = R.synthetic_clip(1, meta["tiny"]["T"], 64, 64, meta["tiny"]["seed"])
    with torch.no_grad():
        got = m(x.cuda()).float().cpu()
        want = O.vmg_forward({k: v.clone() for k, v in sd.items()}, cfg, x)
    ref = _recorded(z, meta["tiny"]["name"] + "/out")
    assert tuple(got.shape) == ref["shape"]
    e1, e2 = float(np.abs(C.subsample(got) - ref["sub"]).max()), float((got - want).abs().max())
    print(f"tiny max fp32: |hip - reference| = {e1:.3e}, |hip - oracle| = {e2:.3e}")
    assert e1 <= 2e-3 and e2 <= 2e-3


@pytest.mark.parametrize("mode", ["autograd", "deferred"])
def test_tiny_model_parameter_gradients_match_the_patched_oracle(mode, max_oracle):
    """As tests/test_grad_gpu.py::test_parameter_gradients_match_oracle_autograd does for 'wins', T = 5 (two key-frames at the last steps), both
    weight-gradient modes."""
    from oracle import recipe as R
    from tests.test_grad_gpu import _oracle_grads
    from vmg_amd import functional as FH
    x = R.synthetic_clip(1, 5, 64, 64, 141)
    tgt = R.synthetic_target(x)
    FH.set_wgrad_mode(mode)
    try:
        m, sd, cfg, _ = _tiny(torch.float32, T=5)
        m.train()
        out = m(x.cuda())
        loss = (out - tgt.cuda()).square().mean()
        loss.backward()
    finally:
        FH.set_wgrad_mode("autograd")
    osd, oloss = _oracle_grads(sd, cfg, x, tgt)
    assert abs(float(loss) - oloss) <= 1e-5 * max(1.0, abs(oloss))
    gmax = max(float(v.grad.abs().max()) for v in osd.values() if v.grad is not None)
    worst = 0.0
    for k, p in m.named_parameters():
        want = osd[k].grad
        assert p.grad is not None and want is not None, k
        scale = max(float(want.abs().max()), 1e-3 * gmax)
        err = float((p.grad.cpu() - want).abs().max()) / scale
        worst = max(worst, err)
        assert err <= 5e-3, f"{k}: relative gradient error {err:.3e}"
    print(f"tiny max {mode}: worst relative gradient error {worst:.2e}")


_long = {}


def _long_oracle(O):
    from oracle import recipe as R
    if "out" not in _long:
        _, sd, cfg, _ = _tiny(torch.float32, T=67)
        _long["x"] = R.synthetic_clip(1, 67, 64, 64, 47)
        with torch.no_grad():
            _long["out"] = O.vmg_forward({k: v.clone() for k, v in sd.items()}, cfg, _long["x"], mutate=False, call_index=1)
    return _long["x"], _long["out"]


def test_tiny_model_on_a_67_frame_clip_fp32_forward_and_backward(max_oracle):
    """T = 67 at stride 2: 34 key-frames, so the last steps run the table route inside the model.  Forward against the patched fp32 oracle: 2e-3, the
    bound tests/test_long_clip_gpu.py holds 'wins' to, on all but 1e-3 of the elements, and 3e-2 of the [0, 1] output range (the bf16 bound of the module
    tests) everywhere.  The exception is the mode's own discontinuity: over 67 frames x 4096 pixels x 4 heads x 2 sweeps the two fp32 implementations
    decide 2.2 million maxima, a few of them between scores closer than fp32 round-off; such a flip swaps one head slice of one pixel and reaches the
    few hundred output pixels downstream of it (measured on the MI355X: max 3.7e-3).  The backward stays finite and reaches every parameter."""
    x, want = _long_oracle(max_oracle)
    m, _, _, _ = _tiny(torch.float32, T=67)
    m.eval()
    with torch.no_grad():
        got = m(x.cuda()).float().cpu()
    err = float((got - want).abs().max())
    share = float(((got - want).abs() > 2e-3).double().mean())
    print(f"tiny max T = 67 fp32: max |hip - oracle| = {err:.3e}, share of elements over 2e-3: {share:.2e}")
    assert got.shape == (1, 67, 3, 256, 256) and share <= 1e-3 and err <= 3e-2
    m, _, _, _ = _tiny(torch.float32, T=67)
    m.train()
    out = m(x.cuda())
    assert torch.equal(out.detach().float().cpu(), got)  # (call 1 again, now with the autograd nodes: the same bits)
    out.square().mean().backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert float(m.encoder_layers[0].traj_mixing.LTAM.proj.weight.grad.abs().max()) > 0


def test_tiny_model_on_a_67_frame_clip_bf16(max_oracle):
    """bf16 against the fp32 patched oracle: a flipped selection makes the output discontinuous, so the floor is the measured PSNR minus 3 dB
    ('wins' at the same length: 48.6 dB)."""
    from tests.util import psnr
    x, want = _long_oracle(max_oracle)
    m, _, _, _ = _tiny(torch.bfloat16, T=67)
    m.eval()
    with torch.no_grad():
        got = m(x.cuda()).float().cpu()
    p = psnr(got, want)
    print(f"tiny max T = 67 bf16: PSNR {p:.2f} dB against the fp32 oracle ('wins': 48.6 dB)")
    assert torch.isfinite(got).all()
    assert PSNR_BF16_MAX_T67 is not None, "the measured value has not been recorded"
    assert p >= PSNR_BF16_MAX_T67 - 3.0


@pytest.mark.parametrize("extra", [{}, {"recompute_chains": True}], ids=["plain", "recompute"])
def test_graphed_model_replays_the_eager_bits(extra):
    """infer.GraphedModel over the tiny max model, T = 5: calls 1 and 2 replayed are the bits of eager calls 1 and 2."""
    from oracle import recipe as R
    from vmg_amd import infer
    x = R.synthetic_clip(1, 5, 64, 64, 142).cuda()
    e, _, _, _ = _tiny(torch.float32, T=5, **extra)
    e.eval()
    with torch.no_grad():
        outs = [e(x).float().cpu() for _ in range(2)]
    m, _, _, _ = _tiny(torch.float32, T=5, **extra)
    m.eval()
    net = infer.GraphedModel(m)
    got = [net(x).float().cpu() for _ in range(2)]
    assert float((outs[0] - outs[1]).abs().max()) > 0
    assert torch.equal(got[0], outs[0]) and torch.equal(got[1], outs[1])


def test_fp8_chains_run_in_max_mode():
    from oracle import recipe as R
    x = R.synthetic_clip(1, 5, 64, 64, 143).cuda()
    m, _, _, _ = _tiny(torch.bfloat16, T=5)
    f, _, _, _ = _tiny(torch.bfloat16, T=5, fp8_chains=True)
    with torch.no_grad():
        a, b = m.eval()(x).float(), f.eval()(x).float()
    assert torch.isfinite(b).all() and float((a - b).abs().max()) <= 0.1


def test_captured_train_step_in_max_mode():
    """TrainStep.capture() on the tiny max model (deferred weight gradients, T = 5): the replayed steps' losses are finite, SPyNet (lr 0) stays
    bit-identical -- as tests/test_optim_gpu.py requires of 'wins' -- and the first replayed loss is that of the same step run eagerly."""
    from vmg_amd.data import synthetic_clip, synthetic_target
    from vmg_amd.train import TrainStep
    x = synthetic_clip(1, 5, 64, 64, seed=77, device="cuda")
    y = synthetic_target(x)
    losses = []
    for captured in (False, True):
        m, _, _, _ = _tiny(torch.float32, T=5)
        m.train()
        ts = TrainStep(m, lr=2e-4, spynet_lr=0.0)
        spy0 = torch.cat([p.detach().reshape(-1).clone() for p in m.spynet.parameters()])
        if captured:
            ts.capture(x, y, warmup=2)
            k = ts.iter
        ls = []
        for _ in range((3 if captured else 3 + 8)):
            ls.append((ts.iter, float(ts(x, y))))
        torch.cuda.synchronize()
        assert all(l == l and abs(l) < 1e6 for _, l in ls)
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in m.spynet.parameters()]), spy0)
        losses.append(dict(ls))
    for it, l in losses[1].items():  # (iteration number before the step -> loss)
        assert it in losses[0] and abs(l - losses[0][it]) <= 1e-3 * abs(losses[0][it]), (it, l, losses[0].get(it))
