"""Per-module replays of the reference fixtures through the PRODUCT modules (HIP path), fp32 strict and bf16 with the stated
tolerance: the widths of the full VMG-REDS configuration (112 / 224 channels, chunk 12 with its padded Ch = 228 and Hp = 24,
groups = 4) as well as the 144-channel few_levels ones.  Each case is checked against the oracle on the same weights and
against the numbers the unmodified reference produced (tests/golden/*.npz).

bf16 tolerance (stated): max |diff| <= 3e-2 of the output scale (inputs and weights are rounded to bf16 by the product; the
oracle runs fp32 on the unrounded values)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _build(name):
    from vmg_amd import model as M
    if name.startswith("morphfc"):
        C, ch = (144, 8) if name == "morphfc_c144_chunk8" else (224, 12)
        return M.Enhanced_MorphFCs_decay(C, ch, ch, qkv_bias=True, channel_mixer="rcab")
    if name == "rcab_c144":
        return M.RCAB(144)
    if name == "mlp_cnn_c144":
        return M.Mlp_cnn(144, exp_r=2, n_groups=1)
    if name == "mlp_cnn_c112_g4":
        return M.Mlp_cnn(112, exp_r=2, n_groups=4)
    if name == "tab_c144":
        return M.TAB(144, 8, 8, 2, 1, True, 0.0, "ffn_cnn", 1.0, "rcab")
    if name == "updown_down":
        return M.UpdownkeepSampling(144, 144, "down")
    if name == "updown_up":
        return M.UpdownkeepSampling(144, 144, "up")
    raise KeyError(name)


CALLS = {"morphfc_c144_chunk8": 3, "tab_c144": 2}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["morphfc_c144_chunk8", "morphfc_c224_chunk12", "rcab_c144", "mlp_cnn_c144", "mlp_cnn_c112_g4", "tab_c144",
                                  "updown_down", "updown_up"])
def test_module_matches_oracle_and_reference_fixture(name, dtype):
    from oracle import cases as C
    case = C.CASES[name]
    shapes, ref_outs = C.load_fixture(os.path.join(GOLD, f"{name}.npz"))
    sd = C.case_state_dict(case, shapes)
    x = case["inputs"]()["x"]
    m = _build(name).cuda()
    m.load_state_dict(sd, strict=True)
    m.eval()
    calls = CALLS.get(name, 1)
    with torch.no_grad():
        got = [m(x.cuda().to(dtype)).float().cpu() for _ in range(calls)]  # calls #1.. (the mixer weights decay in place, T1)
        want = case["run"]({k: v.clone() for k, v in sd.items()}, {"x": x})
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    for i, (g, w) in enumerate(zip(got, want)):
        g = g.reshape(w.shape)
        scale = max(1.0, float(w.abs().max()))
        err = float((g - w).abs().max())
        assert err <= tol * scale, f"{name} call {i + 1} ({dtype}): max |hip - oracle| = {err} (scale {scale})"
        sub = C.subsample(g)
        assert float(np.abs(sub - ref_outs[i]["sub"]).max()) <= tol * scale, f"{name} call {i + 1}: differs from the reference fixture"


def test_spynet_matches_reference_fixture():
    """SPyNet through the product module vs the oracle and the reference's own flows (fp32)."""
    import vmg_amd
    from oracle import cases as C
    for name in ("spynet", "spynet_48x40"):
        case = C.CASES[name]
        shapes, ref_outs = C.load_fixture(os.path.join(GOLD, f"{name}.npz"))
        sd = C.case_state_dict(case, shapes)
        inp = case["inputs"]()
        m = vmg_amd.SPyNet(None).cuda()
        m.load_state_dict({k[len("spynet."):]: v for k, v in sd.items()}, strict=True)
        with torch.no_grad():
            got = m(inp["ref"].cuda(), inp["supp"].cuda()).float().cpu()
            want = case["run"]({k: v.clone() for k, v in sd.items()}, inp)[0]
        scale = max(1.0, float(want.abs().max()))
        assert float((got - want).abs().max()) <= 2e-3 * scale
        assert float(np.abs(C.subsample(got) - ref_outs[0]["sub"]).max()) <= 2e-3 * scale


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["updown_down", "updown_up"])
def test_updown_backward_matches_oracle_autograd(name, dtype):
    """UpdownkeepSampling backward (the fused space<->depth + LayerNorm scatters its input gradient): d/dx and every parameter
    gradient vs torch autograd through the oracle."""
    from oracle import cases as C, recipe as R, vmg_oracle as O
    case = C.CASES[name]
    shapes, _ = C.load_fixture(os.path.join(GOLD, f"{name}.npz"))
    sd = C.case_state_dict(case, shapes)
    x = case["inputs"]()["x"]
    if dtype == torch.bfloat16:
        x = x.to(dtype).float()
    mode = "down" if name.endswith("down") else "up"
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    want = O.updown(osd, "", xo, mode)
    go = R.seeded(tuple(want.shape), 95)
    if dtype == torch.bfloat16:
        go = go.to(dtype).float()
    wg = torch.autograd.grad(want, [xo] + [osd[k] for k in sorted(osd)], go)
    m = _build(name).cuda()
    m.load_state_dict(sd)
    xd = x.cuda().to(dtype).requires_grad_(True)
    got = m(xd)
    got.backward(go.cuda().to(dtype).reshape(got.shape))
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    assert float((got.float().cpu().reshape(want.shape) - want).abs().max()) <= tol * max(1.0, float(want.abs().max()))
    assert float((xd.grad.float().cpu() - wg[0]).abs().max()) <= tol * max(1.0, float(wg[0].abs().max()))
    params = dict(m.named_parameters())
    for k, gw in zip(sorted(osd), wg[1:]):
        err = float((params[k].grad.cpu() - gw).abs().max())
        assert err <= (5e-4 if dtype == torch.float32 else 5e-2) * max(1.0, float(gw.abs().max())), f"{k}: {err}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mdsc_skip_fwd_bwd(dtype):
    """The multi-scale skip (adaptive max-pool /4, conv1x1, GroupNorm(1), ReLU; models/vmg.py:388-400) on the HIP kernels vs the
    oracle's autograd: output, input gradient and all four parameter gradients."""
    import torch.nn as nn
    from oracle import recipe as R, vmg_oracle as O
    from vmg_amd.model import VMG
    B, T, H, W, C, C2 = 2, 2, 16, 24, 32, 64
    x = R.seeded((B, T, H, W, C), 71)
    sd = {"0.weight": R.seeded((C2, C, 1, 1), 72, C ** -0.5), "0.bias": R.seeded((C2,), 73, 0.1), "1.weight": 1 + R.seeded((C2,), 74, 0.1),
          "1.bias": R.seeded((C2,), 75, 0.1)}
    if dtype == torch.bfloat16:  # the product rounds activations and the conv weight to bf16: give the oracle the same values
        x = x.to(dtype).float()
        sd["0.weight"] = sd["0.weight"].to(dtype).float()
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    want = O.mdsc_skip(osd, "", xo)
    go = R.seeded(tuple(want.shape), 76)
    if dtype == torch.bfloat16:
        go = go.to(dtype).float()
    wg = torch.autograd.grad(want, [xo] + [osd[k] for k in sorted(osd)], go)
    seq = nn.Sequential(nn.Conv2d(C, C2, 1, 1, 0), nn.GroupNorm(1, C2), nn.ReLU()).cuda()
    seq.load_state_dict(sd)
    xd = x.cuda().to(dtype).requires_grad_(True)
    got = VMG._mdsc(None, seq, xd)
    got.backward(go.cuda().to(dtype))
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    assert float((got.float().cpu() - want).abs().max()) <= tol * max(1.0, float(want.abs().max()))
    assert float((xd.grad.float().cpu() - wg[0]).abs().max()) <= tol * max(1.0, float(wg[0].abs().max()))
    params = dict(seq.named_parameters())
    for k, gw in zip(sorted(osd), wg[1:]):
        err = float((params[k].grad.cpu().reshape(gw.shape) - gw).abs().max())
        assert err <= (5e-4 if dtype == torch.float32 else 5e-2) * max(1.0, float(gw.abs().max())), f"{k}: {err}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["swin_w2_t5", "swin_w4_t7"])
def test_swin_decoder_layer_fwd_bwd(name, dtype):
    """swin_3d.DecoderLayer (two blocks, the second shifted) through the product: the window attention kernel folds partition, the
    zero padding (20 x 20 -> 24 x 24 in swin_w2_t5), the roll, the -100 mask and the bias gather into its addressing; T = 5 / 7 exercise
    the frame repetition.  Forward vs the oracle and the reference fixture; input and parameter gradients vs the oracle's autograd."""
    from oracle import cases as C, recipe as R, vmg_oracle as O
    from vmg_amd.model import DecoderLayer
    case = C.CASES[name]
    shapes, ref_outs = C.load_fixture(os.path.join(GOLD, f"{name}.npz"))
    sd = C.case_state_dict(case, shapes)
    ws = case["window_of"]("")
    heads = 4 if name == "swin_w2_t5" else 8
    x = case["inputs"]()["x"]
    if dtype == torch.bfloat16:
        x = x.to(dtype).float()
    osd = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point else v) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    want = O.swin_decoder_layer(osd, "", xo, heads, ws)
    go = R.seeded(tuple(want.shape), 96)
    if dtype == torch.bfloat16:
        go = go.to(dtype).float()
    leaves = [k for k in sorted(osd) if osd[k].dtype.is_floating_point]
    wg = torch.autograd.grad(want, [xo] + [osd[k] for k in leaves], go)
    m = DecoderLayer(32, 2, heads, list(ws), 2, True).cuda()
    m.load_state_dict(sd, strict=True)
    xd = x.cuda().to(dtype).requires_grad_(True)
    got = m(xd)
    got.backward(go.cuda().to(dtype))
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    scale = max(1.0, float(want.abs().max()))
    assert float((got.float().cpu() - want).abs().max()) <= tol * scale
    if dtype == torch.float32:
        assert float(np.abs(C.subsample(got.float().cpu()) - ref_outs[0]["sub"]).max()) <= tol * scale
    assert float((xd.grad.float().cpu() - wg[0]).abs().max()) <= tol * max(1.0, float(wg[0].abs().max()))
    params = dict(m.named_parameters())
    for k, gw in zip(leaves, wg[1:]):
        err = float((params[k].grad.cpu() - gw).abs().max())
        assert err <= (5e-4 if dtype == torch.float32 else 5e-2) * max(1.0, float(gw.abs().max())), f"{k}: {err}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_swin_one_window_map_matches_oracle(dtype):
    """A feature map of exactly one spatial window (8 x 8) and exactly one temporal window (D = wt): models/swin_3d.py:88-101 then sets the
    window to the map and ZEROES the shift of the odd block -- the case of get_window_size that the reference can run (smaller maps fail in
    it, tests/test_host_logic.py::test_small_feature_maps_raise_like_the_reference).  Forward and all gradients vs the oracle."""
    from oracle import cases as C, recipe as R, vmg_oracle as O
    from vmg_amd.model import DecoderLayer
    case = C.CASES["swin_w2_t5"]
    shapes, _ = C.load_fixture(os.path.join(GOLD, "swin_w2_t5.npz"))
    sd = C.case_state_dict(case, shapes)
    ws, heads = (2, 8, 8), 4
    x = R.seeded((2, 2, 8, 8, 32), 97)
    if dtype == torch.bfloat16:
        x = x.to(dtype).float()
    osd = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point else v) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    want = O.swin_decoder_layer(osd, "", xo, heads, ws)
    go = R.seeded(tuple(want.shape), 98)
    if dtype == torch.bfloat16:
        go = go.to(dtype).float()
    leaves = [k for k in sorted(osd) if osd[k].dtype.is_floating_point]
    wg = torch.autograd.grad(want, [xo] + [osd[k] for k in leaves], go, allow_unused=True)
    m = DecoderLayer(32, 2, heads, list(ws), 2, True).cuda()
    m.load_state_dict(sd, strict=True)
    xd = x.cuda().to(dtype).requires_grad_(True)
    got = m(xd)
    got.backward(go.cuda().to(dtype))
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    assert float((got.float().cpu() - want).abs().max()) <= tol * max(1.0, float(want.abs().max()))
    assert float((xd.grad.float().cpu() - wg[0]).abs().max()) <= tol * max(1.0, float(wg[0].abs().max()))
    params = dict(m.named_parameters())
    for k, gw in zip(leaves, wg[1:]):
        if gw is None:
            continue
        err = float((params[k].grad.cpu() - gw).abs().max())
        assert err <= (5e-4 if dtype == torch.float32 else 5e-2) * max(1.0, float(gw.abs().max())), f"{k}: {err}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("heads,ws", [(8, (4, 8, 8)), (4, (2, 8, 8))], ids=["h8_w4_d18", "h4_w2_d36"])
def test_swin_decoder_layer_144_channels_fwd_bwd(heads, ws, dtype):
    """DecoderLayer at the few_levels width, the train_swin workload's: 144 channels / 8 heads / wt 4 (head dimension 18: the MFMA kernels
    on bf16) and 144 / 4 heads / wt 2 (head dimension 36: the VALU kernel, also on bf16).  Weights by recipe from the module's own
    state-dict shapes; T = 7 (frame repetition); a 13 x 18 map: remainders 5 and 2, so the shifted block's padded tokens are NOT alone in
    a mask slab and real queries attend to keys that hold the Linears' biases.  Forward and all gradients vs the oracle, tolerances as in
    test_swin_decoder_layer_fwd_bwd."""
    from oracle import recipe as R, vmg_oracle as O
    from vmg_amd.model import DecoderLayer
    m = DecoderLayer(144, 2, heads, list(ws), 2, True)
    sd = R.recipe_state_dict({k: list(v.shape) for k, v in m.state_dict().items()}, 0, None, lambda k: ws)
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    x = R.seeded((1, 7, 13, 18, 144), 131)
    if dtype == torch.bfloat16:
        x = x.to(dtype).float()
    osd = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point else v) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    want = O.swin_decoder_layer(osd, "", xo, heads, ws)
    go = R.seeded(tuple(want.shape), 132)
    if dtype == torch.bfloat16:
        go = go.to(dtype).float()
    leaves = [k for k in sorted(osd) if osd[k].dtype.is_floating_point]
    wg = torch.autograd.grad(want, [xo] + [osd[k] for k in leaves], go)
    xd = x.cuda().to(dtype).requires_grad_(True)
    got = m(xd)
    got.backward(go.cuda().to(dtype))
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    scale = max(1.0, float(want.abs().max()))
    err = float((got.float().cpu() - want).abs().max())
    print(f"[swin144] h{heads} wt{ws[0]} {dtype}: out {err / scale:.3e}, dx {float((xd.grad.float().cpu() - wg[0]).abs().max()) / max(1.0, float(wg[0].abs().max())):.3e}")
    assert err <= tol * scale
    assert float((xd.grad.float().cpu() - wg[0]).abs().max()) <= tol * max(1.0, float(wg[0].abs().max()))
    params = dict(m.named_parameters())
    for k, gw in zip(leaves, wg[1:]):
        err = float((params[k].grad.cpu() - gw).abs().max())
        print(f"[swin144]   {k}: {err / max(1.0, float(gw.abs().max())):.3e}")
        assert err <= (5e-4 if dtype == torch.float32 else 5e-2) * max(1.0, float(gw.abs().max())), f"{k}: {err}"


def _fixture(name):
    from oracle import cases as C
    case = C.CASES[name]
    shapes, ref_outs = C.load_fixture(os.path.join(GOLD, f"{name}.npz"))
    sd = C.case_state_dict(case, shapes) if shapes else {}
    return C, case, sd, ref_outs, case["inputs"]()


def _check(C, got, want, ref, tol, what):
    got = got.float().cpu().reshape(want.shape)
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"{what}: max |hip - oracle| = {err} (scale {scale})"
    assert float(np.abs(C.subsample(got) - ref["sub"]).max()) <= tol * scale, f"{what}: differs from the reference fixture"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_trajectory_fixture_through_the_product_module(dtype):
    """trajectory_c32 (the reference's Trajectory_multi_head on 5 frames, stride 2, two residual blocks, models/trajectory.py:300-490) replayed through
    vmg_amd.model.Trajectory_multi_head: lock-step sweeps, flow warp, location advection, window attention, residual chain, fusion."""
    from vmg_amd.model import Trajectory_multi_head
    C, case, sd, ref, inp = _fixture("trajectory_c32")
    m = Trajectory_multi_head(32, 2, 2, 4, True, 0.1, (2, 2)).cuda()
    m.load_state_dict(sd, strict=True)
    m.eval()
    with torch.no_grad():
        got = m(inp["x"].cuda().to(dtype), inp["ff"].cuda(), inp["fb"].cuda())
        want = case["run"]({k: v.clone() for k, v in sd.items()}, inp)[0]
    _check(C, got, want, ref[0], 2e-4 if dtype == torch.float32 else 4e-2, f"trajectory_c32 ({dtype})")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ltam_fixture_through_the_product_module(dtype):
    """ltam_wins (LTAM_multi_head.forward_wins incl. the output projection and the anchor add, models/trajectory.py:672-795) through
    vmg_amd.model.LTAM_multi_head."""
    from vmg_amd.model import LTAM_multi_head
    C, case, sd, ref, inp = _fixture("ltam_wins")
    m = LTAM_multi_head(144, 4, True, (2, 2)).cuda()
    m.load_state_dict(sd, strict=True)
    dev = lambda t: t.cuda().to(dtype).contiguous()
    with torch.no_grad():
        got = m(dev(inp["q"]), [dev(k) for k in inp["keys"].unbind(1)], dev(inp["anchor"]), [dev(v) for v in inp["vals"].unbind(1)], inp["loc"].cuda())
        want = case["run"]({k: v.clone() for k, v in sd.items()}, inp)[0]
    _check(C, got, want, ref[0], 2e-4 if dtype == torch.float32 else 3e-2, f"ltam_wins ({dtype})")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sr_head_fixture_through_the_product_head(dtype):
    """sr_head (upconv1 / PixelShuffle / lrelu, upconv2 / PixelShuffle / lrelu, HRconv / lrelu, conv_last; models/vmg.py:629-632) through
    VMG.reconstruct -- the fused PixelShuffle epilogue / the weight-streaming conv + shuffle pass, the 64-channel HR convs."""
    import types
    import torch.nn as nn
    from vmg_amd.model import VMG
    C, case, sd, ref, inp = _fixture("sr_head")
    holder = nn.Module()
    holder.upconv1, holder.upconv2 = nn.Conv2d(144, 576, 3, 1, 1), nn.Conv2d(144, 256, 3, 1, 1)
    holder.HRconv, holder.conv_last = nn.Conv2d(64, 64, 3, 1, 1), nn.Conv2d(64, 3, 3, 1, 1)
    holder.load_state_dict(sd, strict=True)
    holder.cuda()
    y = inp["y"]
    N, H, W, _ = y.shape
    with torch.no_grad():
        got = VMG.reconstruct(holder, y.cuda().to(dtype), N, H, W)
        want = case["run"]({k: v.clone() for k, v in sd.items()}, inp)[0]
    _check(C, got, want, ref[0], 2e-4 if dtype == torch.float32 else 3e-2, f"sr_head ({dtype})")


def test_flow_smoothing_fixture_on_the_gpu():
    """flow_smoothing (reflect pad to a multiple of 4, 4 x 4 mean, nearest x 4, crop; models/function.py:1466-1478) as the product runs
    it (Mlp_encoder.flow_smoothing, 30 x 26 maps: both paddings active), forward vs the fixture and the gradient vs the oracle's autograd."""
    from oracle import vmg_oracle as O
    from vmg_amd.model import Mlp_encoder
    C, case, sd, ref, inp = _fixture("flow_smoothing")
    f = inp["flow"]
    fo = f.clone().requires_grad_(True)
    want = O.flow_smoothing(fo, 4)
    go = torch.randn(want.shape, generator=torch.Generator().manual_seed(5))
    (wg,) = torch.autograd.grad(want, fo, go)
    fd = f.cuda().requires_grad_(True)
    got = Mlp_encoder.flow_smoothing(fd, 4)
    (gg,) = torch.autograd.grad(got, fd, go.cuda())
    _check(C, got.detach(), want.detach(), ref[0], 1e-5, "flow_smoothing")
    assert float((gg.cpu() - wg).abs().max()) <= 1e-5 * max(1.0, float(wg.abs().max()))
