"""ffn_type 'ffn_cnn_shift' through the module and the whole model: Mlp_cnn_shift against the reference's recorded outputs and gradients
(tests/golden/shift_ffn.npz), the tiny few-levels model (T = 3, 64 x 64) against the reference's recorded output and against the oracle with its
vanilla FFN replaced by the restatement (tests/shift_ffn_ref.mlp_cnn_shift, monkeypatched over oracle.vmg_oracle.mlp_vanilla: O.tab looks the name up
at call time and takes that branch for every ffn_type but 'ffn_cnn').  Bounds are those of tests/test_mixer_gate_model_gpu.py."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import shift_ffn_ref as SR

pytestmark = pytest.mark.gpu
_oracle_out = {}


def _patched(monkeypatch):
    from oracle import vmg_oracle as O
    monkeypatch.setattr(O, "mlp_vanilla", SR.mlp_cnn_shift)
    return O


def _tiny(dtype=torch.float32, cfg=None, **extra):
    _, meta = SR.fixture()
    cfg = cfg or SR.shift_cfg()
    m = SR.build_product_shift(cfg, dtype, **extra)
    sd = SR.tiny_state_dict(meta, cfg, traj_max=extra.get("traj_mode") == "max")
    m.load_state_dict(sd, strict=True)
    return m, sd, cfg, meta


def _clip(meta):
    from oracle import recipe as R
    return R.synthetic_clip(1, meta["tiny"]["T"], 64, 64, meta["tiny"]["seed"])


def _oracle_output(monkeypatch, m_scaling=1.0):
    """Call 1 of the fp32 oracle with the patch-shift FFN on the fixture's clip; computed once per m_scaling and never modified."""
    if m_scaling not in _oracle_out:
        O = _patched(monkeypatch)
        _, meta = SR.fixture()
        cfg = dataclasses.replace(SR.shift_cfg(), m_scaling=m_scaling)
        sd = SR.tiny_state_dict(meta, cfg)
        with torch.no_grad():
            _oracle_out[m_scaling] = O.vmg_forward({k: v.clone() for k, v in sd.items()}, cfg, _clip(meta))
    return _oracle_out[m_scaling]


@pytest.mark.parametrize("C,r", [(16, 2), (112, 6)])
def test_module_against_the_recorded_reference(C, r):
    """fp32 Mlp_cnn_shift on the recorded input: output and input gradient within 2e-3 of max(1, max |reference|), every parameter gradient within
    5e-3 of its own largest value (the three gradients recorded as a strided subsample: there, and whole against the fp64 restatement)."""
    from vmg_amd.model import Mlp_cnn_shift
    z, meta = SR.fixture()
    sd, x, dout = SR.module_case(meta, C, r)
    m = Mlp_cnn_shift(C, exp_r=r)
    m.load_state_dict(sd, strict=True)
    m.cuda()
    xg = x.cuda().requires_grad_(True)
    out = m(xg)
    out.backward(dout.cuda())
    key = f"module/{C}_{r}"
    for name, got in (("out", out.detach()), ("dx", xg.grad)):
        want = torch.from_numpy(z[f"{key}/{name}"])
        err, scale = float((got.cpu() - want).abs().max()), max(1.0, float(want.abs().max()))
        print(f"Mlp_cnn_shift({C}, {r}) {name}: max abs err {err:.3e} (scale {scale:.3g})")
        assert err <= 2e-3 * scale, name
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    SR.mlp_cnn_shift(sd64, "", x.double()).backward(dout.double())
    worst = 0.0
    for k, p in m.named_parameters():
        got = p.grad.cpu().double()
        if f"{key}/grad/{k}" in z.files:
            pairs = [(got, torch.from_numpy(z[f"{key}/grad/{k}"]).double())]
        else:
            pairs = [(got.reshape(-1)[::meta["big_stride"]], torch.from_numpy(z[f"{key}/grad/{k}/sub"]).double()), (got, sd64[k].grad)]
        for g, want in pairs:
            err = float((g - want).abs().max()) / float(want.abs().max())
            worst = max(worst, err)
            assert err <= 5e-3, f"{k}: relative gradient error {err:.3e}"
    print(f"Mlp_cnn_shift({C}, {r}): worst relative parameter-gradient error {worst:.2e}")


@pytest.mark.parametrize("m_scaling", [1.0, 0.7])
def test_tiny_model_fp32_output(m_scaling, monkeypatch):
    """fp32, call 1: against the patched oracle (also with m_scaling != 1) and the reference's recorded output: <= 2e-3."""
    from oracle import cases as C
    z, _ = SR.fixture()
    want = _oracle_output(monkeypatch, m_scaling)
    m, _, _, meta = _tiny(cfg=dataclasses.replace(SR.shift_cfg(), m_scaling=m_scaling))
    m.eval()
    with torch.no_grad():
        got = m(_clip(meta).cuda()).float().cpu()
    e = float((got - want).abs().max())
    print(f"tiny ffn_cnn_shift fp32, m_scaling {m_scaling}: |hip - oracle| = {e:.3e}")
    assert got.shape == want.shape and e <= 2e-3
    if m_scaling == 1.0:
        assert tuple(got.shape) == tuple(z["tiny/out/shape"])
        e1 = float(np.abs(C.subsample(got) - z["tiny/out/sub"]).max())
        e2 = float(np.abs(C.subsample(want) - z["tiny/out/sub"]).max())
        print(f"tiny ffn_cnn_shift fp32: |hip - reference| = {e1:.3e}, |oracle - reference| = {e2:.3e}")
        assert e1 <= 2e-3


@pytest.mark.parametrize("mode", ["autograd", "deferred"])
def test_tiny_model_loss_and_parameter_gradients(mode, monkeypatch):
    """Loss relative <= 1e-5 and every parameter gradient relative <= 5e-3 against the patched oracle's autograd, as
    tests/test_grad_gpu.py::test_parameter_gradients_match_oracle_autograd; every channel_mixing.* gradient is non-zero.  In deferred mode the
    re-weighting parameters' gradients go straight into .grad."""
    from oracle import recipe as R
    from tests.test_grad_gpu import _oracle_grads
    from vmg_amd import functional as FH
    _patched(monkeypatch)
    _, meta = SR.fixture()
    x = _clip(meta)
    tgt = R.synthetic_target(x)
    FH.set_wgrad_mode(mode)
    try:
        m, sd, cfg, _ = _tiny(drop_path_rate=0.0)  # (the oracle has no DropPath)
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
        assert err <= 5e-3, f"{k}: relative gradient error {err:.3e}"
        if ".channel_mixing." in k:
            seen += 1
            assert float(p.grad.abs().max()) > 0, k
    assert seen == 12 * 3  # twelve FFN parameters in each of the three TABs
    print(f"tiny ffn_cnn_shift {mode}: loss {float(loss):.6e} (oracle {oloss:.6e}), worst relative gradient error {worst:.2e}")


def test_tiny_model_bf16_psnr(monkeypatch):
    """bf16 against the fp32 oracle of the same configuration: at least the PSNR the same tiny model with 'ffn_cnn' reaches against its own oracle
    on the same clip, minus 3.0 dB."""
    from oracle import cases as C
    from oracle import recipe as R
    from oracle import vmg_oracle as O
    from tests.util import build_product, psnr
    _, meta = SR.fixture()
    x = _clip(meta)
    want = _oracle_output(monkeypatch)
    m, _, _, _ = _tiny(torch.bfloat16)
    m.eval()
    with torch.no_grad():
        out = m(x.cuda()).float().cpu()
    assert torch.isfinite(out).all()
    got = psnr(out, want)
    cfg = C.cfg_tiny_few(meta["tiny"]["T"])
    b = build_product(cfg, torch.bfloat16)
    chunk_of, window_of = R.vmg_chunk_lookup(cfg)
    sd = R.recipe_state_dict({k: list(v.shape) for k, v in b.state_dict().items()}, 0, chunk_of=chunk_of, window_of=window_of)
    b.load_state_dict(sd, strict=True)
    b.eval()
    with torch.no_grad():
        base_out = b(x.cuda()).float().cpu()
        base_want = O.vmg_forward({k: v.clone() for k, v in sd.items()}, cfg, x)
    base = psnr(base_out, base_want)
    print(f"tiny bf16 PSNR against the fp32 oracle: ffn_cnn_shift {got:.2f} dB, ffn_cnn {base:.2f} dB")
    assert got >= base - 3.0


def test_graphed_model_replays_the_eager_bits():
    """infer.GraphedModel: calls 1 and 2 replayed are the bits of eager calls 1 and 2, which differ (the mixers' retention decay still applies)."""
    from vmg_amd import infer
    _, meta = SR.fixture()
    x = _clip(meta).cuda()
    e, _, _, _ = _tiny()
    e.eval()
    with torch.no_grad():
        outs = [e(x).float().cpu() for _ in range(2)]
    m, _, _, _ = _tiny()
    m.eval()
    net = infer.GraphedModel(m)
    got = [net(x).float().cpu() for _ in range(2)]
    assert float((outs[0] - outs[1]).abs().max()) > 0
    assert torch.equal(got[0], outs[0]) and torch.equal(got[1], outs[1])


def test_captured_train_step():
    """TrainStep.capture() (deferred weight gradients) with drop_path_rate = 0.1: four replayed steps with finite losses equal to the eager ones
    within 1e-3 relative, as tests/test_mixer_gate_model_gpu.py::test_captured_train_step checks."""
    from vmg_amd.data import synthetic_clip, synthetic_target
    from vmg_amd.train import TrainStep
    x = synthetic_clip(1, 3, 64, 64, seed=77, device="cuda")
    y = synthetic_target(x)
    losses = []
    for captured in (False, True):
        m, _, _, _ = _tiny(drop_path_rate=0.1)
        m.train()
        ts = TrainStep(m, lr=2e-4, spynet_lr=0.0)
        if captured:
            ts.capture(x, y, warmup=2)
        ls = []
        for _ in range((4 if captured else 4 + 8)):
            ls.append((ts.iter, float(ts(x, y))))
        torch.cuda.synchronize()
        assert all(l == l and abs(l) < 1e6 for _, l in ls)
        losses.append(dict(ls))
    assert len(losses[1]) == 4
    for it, l in losses[1].items():  # (iteration number before the step -> loss)
        assert it in losses[0] and abs(l - losses[0][it]) <= 1e-3 * abs(losses[0][it]), (it, l, losses[0].get(it))


def test_other_modes_keep_working():
    """traj_mode 'max' with recompute_chains in bf16 trains with DropPath on and m_scaling != 1 (finite loss, a finite gradient for every parameter),
    and advance_calls(1) puts a fresh model on call 2 of the eager run, bit for bit."""
    _, meta = SR.fixture()
    x = _clip(meta).cuda()
    m, _, _, _ = _tiny(torch.bfloat16, cfg=dataclasses.replace(SR.shift_cfg(), m_scaling=0.7), traj_mode="max", recompute_chains=True, drop_path_rate=0.3)
    m.train()
    loss = m(x).float().square().mean()
    loss.backward()
    assert torch.isfinite(loss)
    for k, p in m.named_parameters():
        if not k.startswith("spynet."):
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
    e, _, _, _ = _tiny()
    e.eval()
    a, _, _, _ = _tiny()
    a.eval()
    a.advance_calls(1)
    with torch.no_grad():
        e(x)
        assert torch.equal(e(x), a(x))
