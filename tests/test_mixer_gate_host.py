"""The mixer's gate configurations without a GPU: the test-side restatement (tests/mixer_gate_ref.py) against what the reference recorded
(tests/golden/mixer_gates.npz, tools/gen_mixer_gate_golden.py), and the product's module tree, state-dict keys and argument checks."""
import json

import pytest
import torch
import torch.nn as nn

from tests import mixer_gate_ref as GR


@pytest.mark.parametrize("gate", list(GR.GATES))
def test_restatement_reproduces_the_reference_fixture(gate):
    """Calls 1 and 2 (the weight decay is stateful) and the input gradient of call 1, all seven configurations; the bound
    tests/test_oracle_golden.py applies to the morphfc cases: 1e-5 of max(1, max |reference|)."""
    from oracle import recipe as R
    z, meta = GR.fixture()
    g = meta["mixer"]
    assert tuple(meta["gates"][gate]) == GR.GATES[gate]
    sd = R.recipe_state_dict(meta["mixer_shapes"][gate], 0, chunk_of=lambda k: g["chunk"])
    assert ("gating_fc.weight" in sd) == (gate == "asym") and not any(k.startswith("gating_fc") for k in sd if gate != "asym")
    x0, dout = R.seeded(g["shape"], g["seed"]), R.seeded(g["shape"], g["seed"] + 1)
    f = GR.morphfc_decay_gated(gate)
    x = x0.clone().requires_grad_(True)
    o1 = f(sd, "", x, g["chunk"], g["chunk"])
    o1.backward(dout)
    with torch.no_grad():
        o2 = f(sd, "", x0.clone(), g["chunk"], g["chunk"])
    for name, got in (("out1", o1.detach()), ("out2", o2), ("dx", x.grad)):
        want = torch.from_numpy(z[f"mixer/{gate}/{name}"])
        err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
        assert err <= 1e-5 * scale, f"{gate} {name}: max abs err {err:.3e} (scale {scale:.3g})"
    assert float((o1.detach() - o2).abs().max()) > 1e-6


def test_restatement_with_the_tanh_gate_is_the_oracle_itself():
    from oracle import recipe as R
    from oracle import vmg_oracle as O
    _, meta = GR.fixture()
    g = meta["mixer"]
    sd = R.recipe_state_dict(meta["mixer_shapes"]["tanh"], 0, chunk_of=lambda k: g["chunk"])
    x = R.seeded(g["shape"], g["seed"])
    with torch.no_grad():
        a = O.morphfc_decay({k: v.clone() for k, v in sd.items()}, "", x, g["chunk"], g["chunk"])
        b = GR.morphfc_decay_gated("tanh")({k: v.clone() for k, v in sd.items()}, "", x, g["chunk"], g["chunk"])
    assert torch.equal(a, b)


def _tiny(gate):
    from oracle import cases as C
    _, meta = GR.fixture()
    return GR.build_product_gated(C.cfg_tiny_few(meta["tiny"]["T"]), gate, device=None), meta


@pytest.mark.parametrize("gate", ["gelu", "asym"])
def test_product_state_dict_keys_are_the_references(gate):
    """Built on the CPU, the product has the reference's recorded key list, in the reference's order, and loads a state dict of the recorded shapes
    with strict=True.  (Fails on the parent: VMG.__init__ refused both configurations.)"""
    m, meta = _tiny(gate)
    assert list(m.state_dict().keys()) == meta["tiny_keys"][gate]
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == meta["tiny_shapes"][gate]
    sd, _ = GR.tiny_state_dict(meta, gate)
    m.load_state_dict(sd, strict=True)
    fcs = [k for k in meta["tiny_keys"][gate] if ".gating_fc." in k]
    assert (len(fcs) > 0) == (gate == "asym")


@pytest.mark.parametrize("gate", list(GR.GATES))
def test_every_gate_configuration_builds_with_the_references_keys(gate):
    m, meta = _tiny(gate)
    assert list(m.state_dict().keys()) == meta["tiny_keys"]["asym" if gate == "asym" else "gelu"]
    from vmg_amd.model import Enhanced_MorphFCs_decay
    for mix in (x for x in m.modules() if isinstance(x, Enhanced_MorphFCs_decay)):
        assert mix.n_handles == (4 if gate == "none" else 5)
        if gate == "asym":
            assert isinstance(mix.gating_fc, nn.Linear)
        elif gate not in ("none", "tanh"):
            assert not list(mix.gating_fc.parameters()) and not list(mix.gating_fc.buffers())
            y = torch.linspace(-3, 3, 13)
            assert torch.allclose(mix.gating_fc(y), GR.act_and_derivative(y, GR.GATES[gate][2])[0], atol=1e-6)


def test_tanh_builds_the_module_tree_and_keys_it_always_did():
    """symm_act='tanh' (the string, the class, and by default through tests.util.build_product): the module tree (names and classes) and the key
    list recorded from the commit before the gate configurations existed (tests/golden/mixer_gate_tanh_tree.json)."""
    from oracle import cases as C
    from tests.util import build_product
    rec = json.load(open(GR.TANH_TREE))
    cfg = C.cfg_tiny_few(3)
    import vmg_amd
    kw = GR.vmg_kwargs(cfg, "tanh")
    for m in (build_product(cfg, device=None), vmg_amd.VMG(**kw), vmg_amd.VMG(**{**kw, "symm_act": nn.Tanh})):
        if m.spynet is None:
            m.spynet = vmg_amd.SPyNet(None)
        assert [[n, type(x).__name__] for n, x in m.named_modules()] == rec["modules"]
        assert list(m.state_dict().keys()) == rec["keys"]


def test_symm_act_spellings():
    """The five strings, the four torch classes, and a class named sigmoid_symm (the reference passes its own)."""
    from vmg_amd.model import symm_act_name

    class sigmoid_symm(nn.Module):
        pass

    for name in GR.SYMM_ACTS:
        assert symm_act_name(name) == name
    assert [symm_act_name(c) for c in (nn.Tanh, nn.ReLU, nn.GELU, nn.SiLU, sigmoid_symm)] == ["tanh", "relu", "gelu", "swish", "sigmoid"]


@pytest.mark.parametrize("bad", ["Tanh", "softplus", "", None, nn.Sigmoid, nn.ELU, 3])
def test_unknown_symm_act_raises_value_error(bad):
    """(On the parent this was NotImplementedError, for every value but tanh.)"""
    from oracle import cases as C
    import vmg_amd
    kw = GR.vmg_kwargs(C.cfg_tiny_few(3), "tanh")
    kw["symm_act"] = bad
    with pytest.raises(ValueError) as e:
        vmg_amd.VMG(**kw)
    for name in GR.SYMM_ACTS:
        assert repr(name) in str(e.value)


def test_other_refusals_stay():
    from oracle import cases as C
    import vmg_amd
    kw = GR.vmg_kwargs(C.cfg_tiny_few(3), "gelu")
    for k, v in (("non_linear", False), ("relu_scale", False), ("relu_scale_norm", True), ("retention_decay", False), ("traj_mode", "average")):
        with pytest.raises(NotImplementedError):
            vmg_amd.VMG(**{**kw, k: v})


@pytest.mark.parametrize("gate", ["swish", "asym", "none"])
def test_create_model_passes_the_three_keys_through(gate):
    import vmg_amd
    from vmg_amd.model import Enhanced_MorphFCs_decay
    gating, symm, act = GR.GATES[gate]
    net = dict(embed_dim=[16, 16, 16], depths=[1, 1, 1], num_heads=[2, 2, 2], window_sizes=[[2, 2, 2]] * 3, num_frames=3, mlp_ratio=2.0, n_groups=1,
               traj_win=[4, None], traj_keyframes_n=[2, None], traj_heads=[2, None], temporal_type=[False, None], temporal_empty=True,
               traj_res_n=[1, 0, 0], spatial_type=[False, False], ffn_type="ffn_cnn", mixer_type=["mlps", "mlps"], mixer_n=[None, None],
               chunk_ratios=["1/4", "1/4"], channel_mixer="rcab", use_mdsc=False, gating=gating, if_symm=symm, symm_act=act)
    m = vmg_amd.create_model({"model": "VMG", "network": net, "dataset": {"image_shape_r": [3, 128, 128]}, "scale": 4, "is_train": True})
    mixers = [x for x in m.modules() if isinstance(x, Enhanced_MorphFCs_decay)]
    assert mixers and all((x.gating, x.symm, x.symm_act) == (gating, symm, act) for x in mixers)
    assert all(hasattr(x, "gating_fc") == (gate != "none") for x in mixers)
