"""The MBConv spatial mixer (mixer_type 'mbconv') without a GPU: the test-side restatement (tests/mbconv_ref.py) against what the reference
recorded (tests/golden/mbconv.npz, tools/gen_mbconv_golden.py), the product's module tree, state-dict keys and refusals, and the plan function
of the depthwise kernels.  (On the parent commit constructing the model raises NotImplementedError and the plan function does not exist.)"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import mbconv_ref as MR


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("src_act,act", [(None, None), ("relu6", None), (None, "relu6"), ("relu6", "relu6")])
def test_restated_depthwise_conv_is_torchs(src_act, act):
    """Forward and the three hand-written gradients against torch's conv2d(groups=C) + relu6 and its autograd, fp64, on an odd shape."""
    g = torch.Generator().manual_seed(31)
    N, H, W, C = 2, 3, 5, 7
    e = (3 * torch.randn(N, H, W, C, generator=g, dtype=torch.float64)).requires_grad_(True)
    w = torch.randn(C, 1, 3, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    b = (2 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    da = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    s = F.relu6(e) if src_act else e
    want = F.conv2d(s.permute(0, 3, 1, 2), w, b, padding=1, groups=C).permute(0, 2, 3, 1)
    want = F.relu6(want) if act else want
    want.backward(da)
    with torch.no_grad():
        a = MR.dwconv3(e, w, b, src_act, act)
        de, dW, db = MR.dwconv3_grads(e, w, a, da, src_act, act)
    for got, ref in ((a, want), (de, e.grad), (dW, w.grad), (db, b.grad)):
        assert float((got - ref.detach()).abs().max()) <= 1e-12 * max(1.0, float(ref.detach().abs().max()))


def test_relu6_derivative_is_zero_at_exactly_0_and_6():
    v = torch.tensor([-1.0, -0.0, 0.0, 1e-30, 5.999999, 6.0, 7.0], dtype=torch.float64, requires_grad=True)
    F.relu6(v).sum().backward()
    assert v.grad.tolist() == [0, 0, 0, 1, 1, 0, 0] and MR.relu6_grad(v.detach()).tolist() == v.grad.tolist()


@pytest.mark.parametrize("C,blocks", MR.MODULES)
def test_restatement_reproduces_the_recorded_module(C, blocks):
    """Output, input gradient and every parameter gradient of Multi_MBConv: fp64 restatement against the reference's fp32, 1e-5 of
    max(1, max |reference|) (the bound of tests/test_shift_ffn_ref.py for the same comparison)."""
    z, meta = MR.fixture()
    sd32, x32, dout = MR.module_case(meta, C, blocks)
    rec = meta["modules"][f"{C}_{blocks}"]
    assert rec["keys"] == MR.mixer_keys(blocks) and rec["shapes"] == MR.mixer_shapes(C, blocks)
    sd = {k: v.double().requires_grad_(True) for k, v in sd32.items()}
    x = x32.double().requires_grad_(True)
    out = MR.multi_mbconv(sd, "", x)
    out.backward(dout.double())
    key = f"module/{C}_{blocks}"

    def close(name, got, want):
        err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
        assert err <= 1e-5 * scale, f"{name}: max abs err {err:.3e} (scale {scale:.3g})"

    close("out", out.detach(), torch.from_numpy(z[f"{key}/out"]).double())
    close("dx", x.grad, torch.from_numpy(z[f"{key}/dx"]).double())
    for k in rec["keys"]:
        close(k, sd[k].grad, torch.from_numpy(z[f"{key}/grad/{k}"]).double())


# ------------------------------------------------------------------------------------------------ the product's module tree
@pytest.mark.parametrize("name", MR.TINY_MODELS)
def test_product_state_dict_keys_are_the_references(name):
    """Built on the CPU, the product has the reference's recorded key list, in the reference's order, the recorded shapes, the recorded mixer
    class per TAB, and loads a recipe state dict with strict=True."""
    _, meta = MR.fixture()
    rec = meta["tiny_models"][name]
    cfg = MR.tiny_cfg()
    m = MR.build_product(cfg, rec["mixer_type"], rec["mixer_n"], device=None)
    assert list(m.state_dict().keys()) == rec["keys"]
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == rec["shapes"]
    from vmg_amd.model import TAB
    assert [type(t.spatial_mixing).__name__ for t in m.modules() if isinstance(t, TAB)] == rec["mixer_classes"]
    m.load_state_dict(MR.tiny_state_dict(meta, name, cfg), strict=True)
    assert "encoder_layers.0.mlp_blocks.0.spatial_mixing.main.0.0.bottleneck.0.0.weight" in rec["keys"]


def test_module_tree_is_the_references():
    from vmg_amd.model import InvertedResidual, Multi_MBConv
    _, meta = MR.fixture()
    for C, blocks in MR.MODULES + [(144, 3)]:
        m = Multi_MBConv(C, expansion_factor=4, stride=1, num_blocks=blocks)
        assert list(m.state_dict().keys()) == MR.mixer_keys(blocks)
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == MR.mixer_shapes(C, blocks)
        assert m.n_handles == 2 and not list(m.buffers())
        for blk in m.main[0]:
            assert isinstance(blk, InvertedResidual)
            kinds = [[type(c).__name__ for c in seq] for seq in blk.bottleneck]
            assert kinds == [["Conv2d", "ReLU6"], ["Conv2d", "ReLU6"], ["Conv2d"]]
            assert blk.bottleneck[1][0].groups == 4 * C
    with pytest.raises(NotImplementedError):
        InvertedResidual(16, stride=2)


def _check_default_mixers(m):
    """The reference's default mixer lists on four encoder / three decoder stages: mixer_type ['mbconv', 'mbconv', 'mlps', 'mlps'], mixer_n
    [2, 3, None, None]; encoder stage i takes entry i, decoder stage i entry -i - 2."""
    from vmg_amd.model import Enhanced_MorphFCs_decay, Multi_MBConv
    enc = [{type(t.spatial_mixing) for t in st.mlp_blocks} for st in m.encoder_layers]
    dec = [{type(t.spatial_mixing) for t in st.mlp_blocks} for st in m.decoder_layers]
    assert enc == [{Multi_MBConv}, {Multi_MBConv}, {Enhanced_MorphFCs_decay}, {Enhanced_MorphFCs_decay}]
    assert dec == [{Enhanced_MorphFCs_decay}, {Multi_MBConv}, {Multi_MBConv}]
    blocks = lambda st: len(st.mlp_blocks[0].spatial_mixing.main[0])
    assert (blocks(m.encoder_layers[0]), blocks(m.encoder_layers[1]), blocks(m.decoder_layers[1]), blocks(m.decoder_layers[2])) == (2, 3, 3, 2)
    # the mixer's parameters are under .mlp_blocks., where the weight-decay split looks for them
    names = [k for k, _ in m.named_parameters() if ".spatial_mixing.main." in k]
    assert names and all(".mlp_blocks." in k for k in names)
    ids = {id(p) for p in m.mlp_wd_param}
    assert all(id(p) in ids for k, p in m.named_parameters() if ".spatial_mixing.main." in k)


def test_default_vmg_constructs():
    """VMG() with no argument but spynet_pretrained=None constructs, with the default mixer lists where the reference's indexing puts them.  (The
    four stage lists default to seven entries here; see the next test for the reference's eight.)"""
    import vmg_amd
    m = vmg_amd.VMG(spynet_pretrained=None)
    assert len(m.encoder_layers) == 4 and len(m.decoder_layers) == 3
    assert [len(st.mlp_blocks) for st in list(m.encoder_layers) + list(m.decoder_layers)] == [8] * 7
    _check_default_mixers(m)


def test_the_references_eight_entry_stage_lists_raise_as_they_do_there():
    """The reference's own stage-list defaults (models/vmg.py:177-181) passed explicitly: eight entries ask for five encoder and four decoder
    stages, the four-entry per-scale lists serve seven, and the constructor raises IndexError as the reference's VMG() does (:290).  The same
    lists cut to seven entries construct, with the default mixers in place."""
    import vmg_amd
    eight = dict(embed_dim=[112, 224, 224, 448, 448, 224, 224, 112], depths=[2] * 8, num_heads=[2, 4, 8, 16, 16, 8, 4, 2], window_sizes=[(4, 4)] * 8)
    with pytest.raises(IndexError):
        vmg_amd.VMG(spynet_pretrained=None, **eight)
    seven = {k: v[:4] + v[5:] for k, v in eight.items()}
    _check_default_mixers(vmg_amd.VMG(spynet_pretrained=None, **seven))


def test_create_model_forwards_the_mixer_keys():
    import vmg_amd
    from vmg_amd.model import TAB, Enhanced_MorphFCs_decay, Multi_MBConv
    net = dict(embed_dim=[16, 16, 16], depths=[1, 1, 1], num_heads=[2, 2, 2], window_sizes=[[2, 2, 2]] * 3, num_frames=3, mlp_ratio=2.0, n_groups=1,
               traj_win=[4, None], traj_keyframes_n=[2, None], traj_heads=[2, None], temporal_type=[False, None], temporal_empty=True,
               traj_res_n=[1, 0, 0], spatial_type=[False, False], ffn_type="ffn_cnn", mixer_type=["mbconv", "mlps"], mixer_n=[1, None],
               chunk_ratios=["1/4", "1/4"], channel_mixer="rcab", use_mdsc=False)
    m = vmg_amd.create_model({"model": "VMG", "network": net, "dataset": {"image_shape_r": [3, 128, 128]}, "scale": 4, "is_train": True})
    kinds = [type(t.spatial_mixing) for t in m.modules() if isinstance(t, TAB)]
    assert kinds == [Multi_MBConv, Enhanced_MorphFCs_decay, Multi_MBConv]


@pytest.mark.parametrize("bad", ["mlp", "MBConv", "nope"])
def test_other_mixer_types_are_refused(bad):
    import vmg_amd
    kw = MR.vmg_kwargs(MR.tiny_cfg(), ["mlps", bad], [None, 1])
    with pytest.raises(NotImplementedError) as e:
        vmg_amd.VMG(**kw)
    assert "'mlps'" in str(e.value) and "'mbconv'" in str(e.value) and repr(bad) in str(e.value)


def test_functional_entry_refuses_bad_arguments():
    from vmg_amd import functional as FH
    x, w, b = torch.zeros(1, 2, 2, 4), torch.zeros(4, 1, 3, 3), torch.zeros(4)
    with pytest.raises(ValueError):
        FH.depthwise_conv3x3(x, w, b, act="relu")
    with pytest.raises(ValueError):
        FH.depthwise_conv3x3(x, w, b, src_act="gelu")
    with pytest.raises(ValueError):
        FH.depthwise_conv3x3(x[0], w, b)


# ------------------------------------------------------------------------------------------------ the plan function
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_plan_route(dtype):
    """vmg_dwconv3_plan (no device needed) against the rule: vector where C is a multiple of the 16-byte vector, and never with misaligned pointers."""
    from vmg_amd import kernels as K
    want = {7: "element", 8: "vector", 12: "vector" if dtype == torch.float32 else "element", 448: "vector", 1792: "vector"}
    for C, route in want.items():
        assert MR.expected_route(C, dtype) == route
        assert K.dwconv3_route(C, dtype) == route, C
        assert K.dwconv3_route(C, dtype, aligned=False) == "element", C
        assert K.dwconv3_plan(2, 9, 11, C, dtype).route == route  # the route does not depend on N, H, W
    for C in range(1, 600):
        assert K.dwconv3_route(C, dtype) == MR.expected_route(C, dtype), C


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_plan_grid_and_partials_are_functions_of_the_geometry(dtype):
    """Tile, channel block, grid, LDS bytes and partial count from the plan's own fields; the same call gives the same plan; the partial count
    depends on neither route nor dtype and is what vmg_dwconv3_wgrad_ws_bytes sizes the workspace by."""
    from vmg_amd import hip
    from vmg_amd import kernels as K
    cd = lambda a, b: -(-a // b)
    es = 2 if dtype == torch.bfloat16 else 4
    for N, H, W, C in [(1, 1, 1, 8), (2, 3, 7, 19), (2, 9, 11, 32), (1, 6, 5, 448), (1, 3, 3, 1792), (28, 64, 64, 576), (28, 64, 64, 448), (3, 17, 33, 65)]:
        for aligned in (True, False):
            p = K.dwconv3_plan(N, H, W, C, dtype, aligned)
            assert p == K.dwconv3_plan(N, H, W, C, dtype, aligned)
            vec = p.route == "vector"
            assert p.chan_block == ((16 // es) * 8 if vec else 32) and p.tile_h >= 1 and p.tile_w >= 1
            tiles = N * cd(H, p.tile_h) * cd(W, p.tile_w)
            assert p.grid == tiles * cd(C, p.chan_block)
            assert 1 <= p.partials <= tiles and p.wgrad_grid == p.partials * cd(C, p.chan_block)
            assert p.lds_bytes == (p.tile_h + 2) * (p.tile_w + 2) * p.chan_block * es and p.lds_bytes <= 64 * 1024
            other = torch.float32 if dtype == torch.bfloat16 else torch.bfloat16
            assert p.partials == K.dwconv3_plan(N, H, W, C, other, not aligned).partials
            assert hip.lib().vmg_dwconv3_wgrad_ws_bytes(hip.dtype_code(dtype), N, H, W, C) == p.partials * C * 10 * 4


def test_plan_refuses_two_to_the_31_elements_and_bad_arguments():
    """N * H * W * C >= 2^31 is refused by the plan (so by every entry), one element less is served; so are a bad dtype, sizes < 1, a null result."""
    from vmg_amd import hip
    from vmg_amd import kernels as K
    l = hip.lib()
    out = (ctypes.c_int * hip.DWCONV_PLAN_INTS)()
    assert l.vmg_dwconv3_plan(hip.BF16, 1 << 10, 1 << 7, 1 << 7, 1 << 7, 1, out) != 0 and b"2^31" in l.vmg_last_error()
    assert l.vmg_dwconv3_plan(hip.BF16, (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1, 1, out) != 0
    assert l.vmg_dwconv3_plan(hip.BF16, 1, 1, (1 << 31) - 1, 1, 1, out) == 0  # 2^31 - 1 elements
    assert l.vmg_dwconv3_plan(hip.BF16, (1 << 10) - 1, 1 << 7, 1 << 7, 1 << 7, 1, out) == 0
    assert l.vmg_dwconv3_wgrad_ws_bytes(hip.BF16, 1 << 10, 1 << 7, 1 << 7, 1 << 7) < 0
    with pytest.raises(hip.HipError):
        K.dwconv3_plan(1 << 10, 1 << 7, 1 << 7, 1 << 7, torch.bfloat16)
    for args in [(7, 1, 1, 1, 8), (hip.F32, 0, 1, 1, 8), (hip.F32, 1, 0, 1, 8), (hip.F32, 1, 1, 0, 8), (hip.F32, 1, 1, 1, 0), (hip.F32, -1, 1, 1, 8)]:
        assert l.vmg_dwconv3_plan(*args, 1, out) != 0, args
    assert l.vmg_dwconv3_plan(hip.F32, 1, 1, 1, 8, 1, None) != 0


def test_entries_refuse_bad_arguments_before_any_launch():
    """Null and misaligned pointers, N, H, W, C < 1, an unknown dtype or flag, a short workspace: refused on the host (the pointers here are never
    dereferenced)."""
    from vmg_amd import hip
    l = hip.lib()
    ok = 4096
    for dt, es in ((hip.F32, 4), (hip.BF16, 2)):
        g = (1, 2, 2, 8)
        bad = [l.vmg_dwconv3_fwd(dt, 1, 1, None, ok, ok, ok, *g, None), l.vmg_dwconv3_fwd(dt, 1, 1, ok, None, ok, ok, *g, None),
               l.vmg_dwconv3_fwd(dt, 1, 1, ok, ok, None, ok, *g, None), l.vmg_dwconv3_fwd(dt, 1, 1, ok, ok, ok, None, *g, None),
               l.vmg_dwconv3_fwd(dt, 2, 0, ok, ok, ok, ok, *g, None), l.vmg_dwconv3_fwd(dt, 0, -1, ok, ok, ok, ok, *g, None),
               l.vmg_dwconv3_fwd(7, 0, 0, ok, ok, ok, ok, *g, None), l.vmg_dwconv3_fwd(dt, 0, 0, ok + es // 2, ok, ok, ok, *g, None),
               l.vmg_dwconv3_fwd(dt, 0, 0, ok, ok + 2, ok, ok, *g, None),
               l.vmg_dwconv3_fwd(dt, 0, 0, ok, ok, ok, ok, 0, 2, 2, 8, None), l.vmg_dwconv3_fwd(dt, 0, 0, ok, ok, ok, ok, 1, 0, 2, 8, None),
               l.vmg_dwconv3_fwd(dt, 0, 0, ok, ok, ok, ok, 1, 2, 0, 8, None), l.vmg_dwconv3_fwd(dt, 0, 0, ok, ok, ok, ok, 1, 2, 2, 0, None),
               l.vmg_dwconv3_fwd(dt, 0, 0, ok, ok, ok, ok, 1 << 10, 1 << 7, 1 << 7, 1 << 7, None),
               l.vmg_dwconv3_bwd_data(dt, 1, 1, None, ok, ok, ok, ok, *g, None), l.vmg_dwconv3_bwd_data(dt, 1, 1, ok, None, ok, ok, ok, *g, None),
               l.vmg_dwconv3_bwd_data(dt, 1, 1, ok, ok, None, ok, ok, *g, None), l.vmg_dwconv3_bwd_data(dt, 1, 1, ok, ok, ok, None, ok, *g, None),
               l.vmg_dwconv3_bwd_data(dt, 1, 1, ok, ok, ok, ok, None, *g, None), l.vmg_dwconv3_bwd_data(dt, 3, 1, ok, ok, ok, ok, ok, *g, None),
               l.vmg_dwconv3_bwd_data(dt, 1, 1, ok, ok + 1, ok, ok, ok, *g, None), l.vmg_dwconv3_bwd_data(dt, 0, 0, ok, None, None, ok, ok, 1, 2, 2, -8, None),
               l.vmg_dwconv3_bwd_weight(dt, 1, 1, None, ok, ok, ok, ok, *g, 0, ok, 1 << 20, None),
               l.vmg_dwconv3_bwd_weight(dt, 1, 1, ok, None, ok, ok, ok, *g, 0, ok, 1 << 20, None),
               l.vmg_dwconv3_bwd_weight(dt, 1, 1, ok, ok, None, ok, ok, *g, 0, ok, 1 << 20, None),
               l.vmg_dwconv3_bwd_weight(dt, 1, 1, ok, ok, ok, None, ok, *g, 0, ok, 1 << 20, None),
               l.vmg_dwconv3_bwd_weight(dt, 1, 1, ok, ok, ok, ok, None, *g, 0, ok, 1 << 20, None),
               l.vmg_dwconv3_bwd_weight(dt, 1, 1, ok, ok, ok, ok, ok, *g, 0, None, 1 << 20, None),
               l.vmg_dwconv3_bwd_weight(dt, 1, 1, ok, ok, ok, ok, ok, *g, 0, ok, 16, None),
               l.vmg_dwconv3_bwd_weight(dt, 1, 1, ok, ok, ok, ok, ok, *g, 2, ok, 1 << 20, None),
               l.vmg_dwconv3_bwd_weight(dt, 1, 4, ok, ok, ok, ok, ok, *g, 0, ok, 1 << 20, None),
               l.vmg_dwconv3_bwd_weight(dt, 1, 1, ok, ok, ok, ok + 2, ok, *g, 0, ok, 1 << 20, None)]
        assert all(rc == -1 for rc in bad), [i for i, rc in enumerate(bad) if rc != -1]  # (-1: refused by a check; -2 would be a failed launch)
    assert l.vmg_last_error()


def test_header_and_signatures_list_the_five_entries():
    import os
    import re
    from vmg_amd import hip
    names = ["vmg_dwconv3_plan", "vmg_dwconv3_fwd", "vmg_dwconv3_bwd_data", "vmg_dwconv3_wgrad_ws_bytes", "vmg_dwconv3_bwd_weight"]
    header = open(os.path.join(os.path.dirname(MR.HERE), "include", "vmg_hip.h")).read()
    for n in names:
        assert n in hip.SIGNATURES and hasattr(hip.lib(), n)
        proto = re.search(r"\b" + n + r"\(([^;]*)\);", header)
        assert proto and len(proto.group(1).split(",")) == len(hip.SIGNATURES[n][1]), n
