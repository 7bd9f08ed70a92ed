"""The mixer's gate configurations through the whole model: the tiny few-levels model (T = 3, 64 x 64) against the reference's recorded output
(tests/golden/mixer_gates.npz: 'gelu' and if_symm=False) and against the oracle with its token mixer replaced by the gated restatement
(tests/mixer_gate_ref.morphfc_decay_gated, monkeypatched over oracle.vmg_oracle.morphfc_decay: O.tab looks the name up at call time).
Bounds are those of tests/test_traj_max_gpu.py."""
import numpy as np
import pytest
import torch

from tests import mixer_gate_ref as GR

pytestmark = pytest.mark.gpu
_oracle_out = {}


def _patched(monkeypatch, gate):
    from oracle import vmg_oracle as O
    monkeypatch.setattr(O, "morphfc_decay", GR.morphfc_decay_gated(gate))
    return O


def _tiny(gate, dtype=torch.float32, T=None, **extra):
    _, meta = GR.fixture()
    sd, cfg = GR.tiny_state_dict(meta, gate, T)
    m = GR.build_product_gated(cfg, gate, dtype, **extra)
    if extra.get("traj_mode") == "max":  # (that mode's attention has neither position table nor decay buffer: tests/test_traj_max_gpu.py)
        sd = {k: v for k, v in sd.items() if not k.endswith(("relative_pos_encoding", "decay_v"))}
    m.load_state_dict(sd, strict=True)
    return m, sd, cfg, meta


def _clip(meta):
    from oracle import recipe as R
    return R.synthetic_clip(1, meta["tiny"]["T"], 64, 64, meta["tiny"]["seed"])


def _oracle_output(monkeypatch, gate):
    """Call 1 of the fp32 oracle in configuration `gate` on the fixture's clip; computed once per configuration and never modified."""
    if gate not in _oracle_out:
        O = _patched(monkeypatch, gate)
        _, meta = GR.fixture()
        sd, cfg = GR.tiny_state_dict(meta, gate)
        with torch.no_grad():
            _oracle_out[gate] = O.vmg_forward({k: v.clone() for k, v in sd.items()}, cfg, _clip(meta))
    return _oracle_out[gate]


@pytest.mark.parametrize("gate", GR.NEW_GATES)
def test_tiny_model_fp32_output(gate, monkeypatch):
    """fp32, call 1: against the patched oracle (all six new configurations) and the reference's recorded output ('gelu', 'asym'): <= 2e-3."""
    from oracle import cases as C
    z, _ = GR.fixture()
    want = _oracle_output(monkeypatch, gate)
    m, _, _, meta = _tiny(gate)
    m.eval()
    with torch.no_grad():
        got = m(_clip(meta).cuda()).float().cpu()
    e = float((got - want).abs().max())
    print(f"tiny {gate} fp32: |hip - oracle| = {e:.3e}")
    assert got.shape == want.shape and e <= 2e-3
    if gate in meta["tiny"]["variants"]:
        assert tuple(got.shape) == tuple(z[f"tiny/{gate}/out/shape"])
        e1 = float(np.abs(C.subsample(got) - z[f"tiny/{gate}/out/sub"]).max())
        e2 = float(np.abs(C.subsample(want) - z[f"tiny/{gate}/out/sub"]).max())
        print(f"tiny {gate} fp32: |hip - reference| = {e1:.3e}, |oracle - reference| = {e2:.3e}")
        assert e1 <= 2e-3


@pytest.mark.parametrize("gate,mode", [(g, "autograd") for g in GR.NEW_GATES] + [("asym", "deferred"), ("none", "deferred")])
def test_tiny_model_loss_and_parameter_gradients(gate, mode, monkeypatch):
    """Loss relative <= 1e-5 and every parameter gradient (gating_fc.* included) relative <= 5e-3 against the patched oracle's autograd, as
    tests/test_grad_gpu.py::test_parameter_gradients_match_oracle_autograd; deferred weight gradients for the configuration with a new Linear and for
    the one whose mixer input has four consumers."""
    from oracle import recipe as R
    from tests.test_grad_gpu import _oracle_grads
    from vmg_amd import functional as FH
    _patched(monkeypatch, gate)
    _, meta = GR.fixture()
    x = _clip(meta)
    tgt = R.synthetic_target(x)
    FH.set_wgrad_mode(mode)
    try:
        m, sd, cfg, _ = _tiny(gate)
        m.train()
        loss = (m(x.cuda()) - tgt.cuda()).square().mean()
        loss.backward()
    finally:
        FH.set_wgrad_mode("autograd")
    osd, oloss = _oracle_grads(sd, cfg, x, tgt)
    assert abs(float(loss) - oloss) <= 1e-5 * max(1.0, abs(oloss))
    gmax = max(float(v.grad.abs().max()) for v in osd.values() if v.grad is not None)
    worst, seen = 0.0, 0
    for k, p in m.named_parameters():
        want = osd[k].grad
        assert p.grad is not None and want is not None, k
        scale = max(float(want.abs().max()), 1e-3 * gmax)
        err = float((p.grad.cpu() - want).abs().max()) / scale
        worst = max(worst, err)
        seen += ".gating_fc." in k
        assert err <= 5e-3, f"{k}: relative gradient error {err:.3e}"
    assert (seen > 0) == (gate == "asym")
    print(f"tiny {gate} {mode}: loss {float(loss):.6e} (oracle {oloss:.6e}), worst relative gradient error {worst:.2e}")


_bf16_psnr = {}


def _psnr_bf16(monkeypatch, gate):
    """PSNR of the bf16 model in configuration `gate` against the fp32 oracle of the same configuration (once per configuration)."""
    from tests.util import psnr
    if gate not in _bf16_psnr:
        want = _oracle_output(monkeypatch, gate)
        m, _, _, meta = _tiny(gate, torch.bfloat16)
        m.eval()
        with torch.no_grad():
            out = m(_clip(meta).cuda()).float().cpu()
        assert torch.isfinite(out).all(), gate
        _bf16_psnr[gate] = psnr(out, want)
    return _bf16_psnr[gate]


@pytest.mark.parametrize("gate", GR.NEW_GATES)
def test_tiny_model_bf16_psnr(gate, monkeypatch):
    """bf16 against the fp32 oracle of the same configuration: at least the PSNR the tanh model reaches here, minus 3.0 dB (the margin of the 67-frame
    bf16 test of tests/test_traj_max_gpu.py)."""
    tanh, got = _psnr_bf16(monkeypatch, "tanh"), _psnr_bf16(monkeypatch, gate)
    print(f"tiny bf16 PSNR against the fp32 oracle: {gate} {got:.2f} dB, tanh {tanh:.2f} dB")
    assert got >= tanh - 3.0


@pytest.mark.parametrize("gate", ["swish", "asym"])
def test_graphed_model_replays_the_eager_bits(gate):
    """infer.GraphedModel: calls 1 and 2 replayed are the bits of eager calls 1 and 2."""
    from vmg_amd import infer
    _, meta = GR.fixture()
    x = _clip(meta).cuda()
    e, _, _, _ = _tiny(gate)
    e.eval()
    with torch.no_grad():
        outs = [e(x).float().cpu() for _ in range(2)]
    m, _, _, _ = _tiny(gate)
    m.eval()
    net = infer.GraphedModel(m)
    got = [net(x).float().cpu() for _ in range(2)]
    assert float((outs[0] - outs[1]).abs().max()) > 0
    assert torch.equal(got[0], outs[0]) and torch.equal(got[1], outs[1])


@pytest.mark.parametrize("gate", ["swish", "asym"])
def test_captured_train_step(gate):
    """TrainStep.capture() (deferred weight gradients): three replayed steps with finite losses equal to the eager ones within 1e-3 relative, as
    tests/test_traj_max_gpu.py::test_captured_train_step_in_max_mode checks."""
    from vmg_amd.data import synthetic_clip, synthetic_target
    from vmg_amd.train import TrainStep
    x = synthetic_clip(1, 3, 64, 64, seed=77, device="cuda")
    y = synthetic_target(x)
    losses = []
    for captured in (False, True):
        m, _, _, _ = _tiny(gate)
        m.train()
        ts = TrainStep(m, lr=2e-4, spynet_lr=0.0)
        if captured:
            ts.capture(x, y, warmup=2)
        ls = []
        for _ in range((3 if captured else 3 + 8)):
            ls.append((ts.iter, float(ts(x, y))))
        torch.cuda.synchronize()
        assert all(l == l and abs(l) < 1e6 for _, l in ls)
        losses.append(dict(ls))
    assert len(losses[1]) == 3
    for it, l in losses[1].items():  # (iteration number before the step -> loss)
        assert it in losses[0] and abs(l - losses[0][it]) <= 1e-3 * abs(losses[0][it]), (it, l, losses[0].get(it))


@pytest.mark.parametrize("gate", ["relu", "asym", "none"])
def test_other_modes_keep_working(gate):
    """traj_mode 'max' with recompute_chains in bf16 trains (finite loss, a finite gradient for every parameter), and advance_calls(1) puts a fresh
    model on call 2 of the eager run, bit for bit."""
    _, meta = GR.fixture()
    x = _clip(meta).cuda()
    m, _, _, _ = _tiny(gate, torch.bfloat16, traj_mode="max", recompute_chains=True)
    m.train()
    loss = m(x).float().square().mean()
    loss.backward()
    assert torch.isfinite(loss)
    for k, p in m.named_parameters():
        if not k.startswith("spynet."):
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
    e, _, _, _ = _tiny(gate)
    e.eval()
    a, _, _, _ = _tiny(gate)
    a.eval()
    a.advance_calls(1)
    with torch.no_grad():
        e(x)
        assert torch.equal(e(x), a(x))
