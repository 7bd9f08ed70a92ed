"""The patch-shift FFN (ffn_type 'ffn_cnn_shift') without a GPU: the test-side closed form and restatement (tests/shift_ffn_ref.py) against what the
reference recorded (tests/golden/shift_ffn.npz, tools/gen_shift_ffn_golden.py), and the product's module tree, state-dict keys, refusals and the
kernel route function.  (On the parent commit constructing the model raises and the route function does not exist.)"""
import numpy as np
import pytest
import torch

from tests import shift_ffn_ref as SR


@pytest.mark.parametrize("shape", SR.SHIFT_SHAPES, ids=SR.shape_name)
def test_closed_form_shift_is_the_recorded_patchshift2d(shape):
    """Both directions, exactly: the shift copies values."""
    from oracle import recipe as R
    z, meta = SR.fixture()
    i = [tuple(s) for s in meta["shift_shapes"]].index(tuple(shape))
    x = R.seeded(shape, meta["shift_seed"] + i)
    for inv in (False, True):
        want = torch.from_numpy(z[f"shift/{SR.shape_name(shape)}/{'inv' if inv else 'fwd'}"])
        got = SR.patch_shift(x, inverse=inv)
        assert torch.equal(got, want), (shape, inv)
        assert torch.equal(SR.patch_shift(x[None], inverse=inv)[0], want)  # a leading (B, T) changes nothing


def test_shift_adjoint_is_the_opposite_shift():
    """<shift(x), y> == <x, shift_inv(y)> in fp64, for every recorded shape."""
    for i, shape in enumerate(SR.SHIFT_SHAPES):
        g = torch.Generator().manual_seed(900 + i)
        x, y = torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64)
        a, b = (SR.patch_shift(x) * y).sum(), (x * SR.patch_shift(y, inverse=True)).sum()
        assert abs(float(a - b)) <= 1e-12 * max(1.0, abs(float(a)))


@pytest.mark.parametrize("C,r", SR.MODULES)
def test_restatement_reproduces_the_recorded_module(C, r):
    """Output, input gradient and every parameter gradient of Mlp_cnn_shift: fp64 restatement against the reference's fp32, 1e-5 of
    max(1, max |reference|).  The three weight gradients recorded as a strided subsample are compared there and by their checksums."""
    z, meta = SR.fixture()
    sd32, x32, dout = SR.module_case(meta, C, r)
    rec = meta["modules"][f"{C}_{r}"]
    assert rec["keys"] == SR.KEY_ORDER and rec["shapes"] == SR.module_shapes(C, r)
    sd = {k: v.double().requires_grad_(True) for k, v in sd32.items()}
    x = x32.double().requires_grad_(True)
    out = SR.mlp_cnn_shift(sd, "", x)
    out.backward(dout.double())
    key = f"module/{C}_{r}"

    def close(name, got, want):
        err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
        assert err <= 1e-5 * scale, f"{name}: max abs err {err:.3e} (scale {scale:.3g})"

    close("out", out.detach(), torch.from_numpy(z[f"{key}/out"]).double())
    close("dx", x.grad, torch.from_numpy(z[f"{key}/dx"]).double())
    for k in SR.KEY_ORDER:
        g = sd[k].grad
        if f"{key}/grad/{k}" in z.files:
            close(k, g, torch.from_numpy(z[f"{key}/grad/{k}"]).double())
        else:
            assert g.numel() > meta["big"]
            close(k, g.reshape(-1)[::meta["big_stride"]], torch.from_numpy(z[f"{key}/grad/{k}/sub"]).double())
            s, sa = z[f"{key}/grad/{k}/sums"]
            assert abs(float(g.sum()) - s) <= 1e-5 * max(1.0, sa) and abs(float(g.abs().sum()) - sa) <= 1e-5 * max(1.0, sa)


def test_restatement_in_the_oracle_signature(monkeypatch):
    """oracle.vmg_oracle.tab with mlp_vanilla replaced takes the patch-shift branch for ffn_type 'ffn_cnn_shift': the TAB's FFN half is then the
    restatement (checked through the difference of two tab calls that differ only in the FFN)."""
    from oracle import recipe as R
    from oracle import vmg_oracle as O
    _, meta = SR.fixture()
    cfg = SR.shift_cfg()
    sd = SR.tiny_state_dict(meta, cfg)
    p = next(k for k in sd if k.endswith("channel_mixing.fc.weight"))[:-len("channel_mixing.fc.weight")]
    x = R.seeded((1, 2, 8, 8, sd[f"{p}norm3.weight"].shape[0]), 77)
    calls = []

    def spy(sd_, p_, x_):
        calls.append(p_)
        return SR.mlp_cnn_shift(sd_, p_, x_)

    monkeypatch.setattr(O, "mlp_vanilla", spy)
    chunk_of, _ = R.vmg_chunk_lookup(cfg)
    ch, cw = chunk_of(f"{p}spatial_mixing.gamma_h"), chunk_of(f"{p}spatial_mixing.gamma_w")
    with torch.no_grad():
        y = O.tab({k: v.clone() for k, v in sd.items()}, p, x, cfg, ch, cw)
    assert calls == [f"{p}channel_mixing."] and y.shape == x.shape and torch.isfinite(y).all()


def _tiny():
    _, meta = SR.fixture()
    cfg = SR.shift_cfg()
    return SR.build_product_shift(cfg, device=None), cfg, meta


def test_product_state_dict_keys_are_the_references():
    """Built on the CPU, the product has the reference's recorded key list, in the reference's order, the recorded shapes, and loads a recipe state
    dict with strict=True."""
    m, cfg, meta = _tiny()
    assert list(m.state_dict().keys()) == meta["tiny_keys"]
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == meta["tiny_shapes"]
    m.load_state_dict(SR.tiny_state_dict(meta, cfg), strict=True)
    assert meta["tiny_ffn_class"] == ["Mlp_cnn_shift"]


def test_module_key_order_and_parameter_free_children():
    from vmg_amd.model import Mlp_cnn_shift
    for C, r in SR.MODULES + [(144, 2.0), (18, 1.5)]:
        m = Mlp_cnn_shift(C, exp_r=r)
        assert list(m.state_dict().keys()) == SR.KEY_ORDER
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == SR.module_shapes(C, r)
        assert [n for n, _ in m.named_children()] == ["fc", "shift", "fc1", "shift_inv", "act", "fc2", "reweight", "proj", "drop"]
        for name in ("shift", "shift_inv", "act", "drop"):
            assert not list(getattr(m, name).parameters()) and not list(getattr(m, name).buffers())
        assert (m.shift.inv, m.shift_inv.inv) == (False, True)


def test_create_model_builds_the_shift_ffn_in_every_tab():
    import vmg_amd
    from vmg_amd.model import TAB, Mlp_cnn_shift
    net = dict(embed_dim=[16, 16, 16], depths=[1, 1, 1], num_heads=[2, 2, 2], window_sizes=[[2, 2, 2]] * 3, num_frames=3, mlp_ratio=2.0, n_groups=1,
               traj_win=[4, None], traj_keyframes_n=[2, None], traj_heads=[2, None], temporal_type=[False, None], temporal_empty=True,
               traj_res_n=[1, 0, 0], spatial_type=[False, False], ffn_type=SR.FFN, mixer_type=["mlps", "mlps"], mixer_n=[None, None],
               chunk_ratios=["1/4", "1/4"], channel_mixer="rcab", use_mdsc=False)
    m = vmg_amd.create_model({"model": "VMG", "network": net, "dataset": {"image_shape_r": [3, 128, 128]}, "scale": 4, "is_train": True})
    tabs = [t for t in m.modules() if isinstance(t, TAB)]
    assert tabs and all(isinstance(t.channel_mixing, Mlp_cnn_shift) and t.channel_mixing.hidden_features == 32 for t in tabs)
    # the FFN's parameters are under .mlp_blocks., where the weight-decay split looks for them
    names = [k for k, _ in m.named_parameters() if ".channel_mixing." in k]
    assert names and all(".mlp_blocks." in k for k in names)


@pytest.mark.parametrize("bad", ["irffn_single", "irffn_multi", "nope"])
def test_other_ffn_types_stay_refused(bad):
    import vmg_amd
    kw = SR.vmg_kwargs(SR.shift_cfg())
    kw["ffn_type"] = bad
    with pytest.raises(NotImplementedError) as e:
        vmg_amd.VMG(**kw)
    assert "reference cannot run" in str(e.value) and repr(bad) in str(e.value)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_patch_shift_route(dtype):
    """The route function (vmg_patch_shift_plan, no device needed) against the rule: vector when ceil(Cs / 9) and Cs are multiples of the 16-byte
    vector, and never with misaligned pointers."""
    from vmg_amd import kernels as K
    want = {288: "vector", 144: "vector", 32: "vector" if dtype == torch.float32 else "element", 16: "element", 112: "element", 672: "element",
            19: "element"}
    for Cs, route in want.items():
        assert SR.expected_route(Cs, dtype) == route
        assert K.patch_shift_route(Cs, dtype) == route, Cs
        assert K.patch_shift_route(Cs, dtype, aligned=False) == "element", Cs
    for Cs in range(1, 700):
        assert K.patch_shift_route(Cs, dtype) == SR.expected_route(Cs, dtype), Cs
    from vmg_amd import hip
    assert hip.lib().vmg_patch_shift_plan(hip.dtype_code(dtype), 0, 1) < 0 and hip.lib().vmg_patch_shift_plan(7, 16, 1) < 0


def test_shift_entries_refuse_bad_arguments_before_any_launch():
    """Null and misaligned pointers, N, H, W, Cs < 1, a sign other than +-1: refused on the host (the pointers here are never dereferenced)."""
    from vmg_amd import hip
    l = hip.lib()
    ok = 4096
    for dt, es in ((hip.F32, 4), (hip.BF16, 2)):
        bad = [l.vmg_patch_shift_fwd(dt, 1, 0, None, ok, 1, 2, 2, 9, None), l.vmg_patch_shift_fwd(dt, 1, 0, ok, None, 1, 2, 2, 9, None),
               l.vmg_patch_shift_fwd(dt, 1, 0, ok + es // 2, ok, 1, 2, 2, 9, None), l.vmg_patch_shift_fwd(dt, 1, 0, ok, ok + 1, 1, 2, 2, 9, None),
               l.vmg_patch_shift_fwd(dt, 0, 0, ok, ok, 1, 2, 2, 9, None), l.vmg_patch_shift_fwd(dt, 2, 0, ok, ok, 1, 2, 2, 9, None),
               l.vmg_patch_shift_fwd(dt, 1, 1, ok, ok, 1, 2, 2, 9, None),
               l.vmg_patch_shift_fwd(dt, 1, 0, ok, ok, 0, 2, 2, 9, None), l.vmg_patch_shift_fwd(dt, 1, 0, ok, ok, 1, 0, 2, 9, None),
               l.vmg_patch_shift_fwd(dt, 1, 0, ok, ok, 1, 2, 0, 9, None), l.vmg_patch_shift_fwd(dt, 1, 0, ok, ok, 1, 2, 2, 0, None),
               l.vmg_patch_shift_bwd(dt, 1, 3, ok, None, ok, 1, 2, 2, 9, None), l.vmg_patch_shift_bwd(dt, 1, 3, ok, ok + 1, ok, 1, 2, 2, 9, None),
               l.vmg_patch_shift_bwd(dt, 1, 0, None, None, ok, 1, 2, 2, 9, None), l.vmg_patch_shift_bwd(dt, -2, 0, ok, None, ok, 1, 2, 2, 9, None),
               l.vmg_mix2_fwd(dt, None, ok, ok, ok, 4, 2, 8, None), l.vmg_mix2_fwd(dt, ok, ok, None, ok, 4, 2, 8, None),
               l.vmg_mix2_fwd(dt, ok + es, ok, ok, ok, 4, 2, 8, None), l.vmg_mix2_fwd(dt, ok, ok, ok, ok, 4, 3, 8, None),
               l.vmg_mix2_fwd(dt, ok, ok, ok, ok, 4, 2, 7, None), l.vmg_mix2_bwd(dt, ok, ok, None, ok, ok, 4, 2, 8, None),
               l.vmg_mix2_bwd(dt, ok, ok, ok, ok, None, 4, 2, 8, None),
               l.vmg_group_reduce2(dt, None, ok, ok, ok, 2, 4, 8, 1.0, ok, 1 << 20, None), l.vmg_group_reduce2(dt, ok, ok + es, ok, ok, 2, 4, 8, 1.0, ok, 1 << 20, None),
               l.vmg_group_reduce2(dt, ok, ok, ok, ok, 2, 4, 7, 1.0, ok, 1 << 20, None), l.vmg_group_reduce2(dt, ok, ok, ok, ok, 2, 4, 8, 1.0, ok, 16, None),
               l.vmg_group_reduce2(dt, ok, ok, ok, ok, 0, 4, 8, 1.0, ok, 1 << 20, None), l.vmg_group_reduce2(dt, ok, ok, ok, ok, 2, 4, 514, 1.0, ok, 1 << 26, None)]
        assert all(rc != 0 for rc in bad), [i for i, rc in enumerate(bad) if rc == 0]
    bad = [l.vmg_se_mlp2_fwd(None, ok, ok, ok, ok, ok, ok, 2, 8, 2, None), l.vmg_se_mlp2_fwd(ok, ok, ok, ok, ok, ok + 2, ok, 2, 8, 2, None),
           l.vmg_se_mlp2_fwd(ok, ok, ok, ok, ok, ok, ok, 0, 8, 2, None), l.vmg_se_mlp2_fwd(ok, ok, ok, ok, ok, ok, ok, 2, 20000, 2, None),
           l.vmg_se_mlp2_bwd(ok, ok, ok, ok, ok, ok, ok, ok, ok, ok, ok, None, 2, 8, 2, 1.0, 0, None),
           l.vmg_se_mlp2_bwd(ok, ok, ok, ok, ok, ok, ok + 1, ok, ok, ok, ok, ok, 2, 8, 2, 1.0, 0, None),
           l.vmg_se_mlp2_bwd(ok, ok, ok, ok, ok, ok, ok, ok, ok, ok, ok, ok, 2, 0, 2, 1.0, 0, None)]
    assert all(rc != 0 for rc in bad), [i for i, rc in enumerate(bad) if rc == 0]
    assert l.vmg_last_error()
