"""Host checks (no GPU) of the two decisions SPyNet's speed rests on: which kernels one basic module runs on (model.spy_module_route) and
which encoder scales run SPyNet at all (VMG.flow_scales)."""
import pytest
import torch


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (8, 14), (16, 16)])
def test_fused_route(h, w):
    from vmg_amd.model import SPY_FUSED, spy_module_route
    assert spy_module_route(torch.bfloat16, h, w, None, [8]) == SPY_FUSED


@pytest.mark.parametrize("dtype,h,w,inner,src", [
    (torch.bfloat16, 16, 17, None, [8]),            # one pixel column past the LDS maximum
    (torch.bfloat16, 32, 32, None, [8]),
    (torch.float32, 8, 8, None, [8]),               # fp32 (parity mode, spynet_dtype)
    (torch.float32, 8, 8, torch.bfloat16, [8]),     # edge_fp32: the middle convolutions change dtype
    (torch.bfloat16, 8, 8, torch.bfloat16, [8]),
    (torch.bfloat16, 8, 8, None, [3, 5]),           # a virtual concat of two sources
    (torch.bfloat16, 8, 8, None, [8, 8]),
    (torch.bfloat16, 1, 256, None, [8]),            # 256 pixels, but 7 x 262 with the border: no LDS tile
])
def test_per_conv_route(dtype, h, w, inner, src):
    from vmg_amd.model import SPY_PER_CONV, spy_module_route
    assert spy_module_route(dtype, h, w, inner, src) == SPY_PER_CONV


def test_route_limits_are_the_kernels():
    """The route admits exactly what K.spy_module_forward admits (one pair of constants)."""
    from vmg_amd import kernels as K
    from vmg_amd.model import SPY_FUSED, spy_module_route
    for h in range(1, 40):
        for w in range(1, 40):
            fits = h * w <= K.SPY_FUSED_MAX_PIXELS and (h + 6) * (w + 6) <= K.SPY_FUSED_MAX_TILE
            assert (spy_module_route(torch.bfloat16, h, w, None, (8,)) == SPY_FUSED) == fits, (h, w)
    assert K.SPY_FUSED_MAX_PIXELS == 256 and K.SPY_FUSED_MAX_TILE == 22 * 22


def _model(net, frames=3):
    import vmg_amd
    return vmg_amd.VMG(num_frames=frames, image_size=[64, 64], is_train=True, spynet_pretrained=None, **net)


def test_flow_scales_few_levels():
    from vmg_amd.data import REDS_FEW_LEVELS
    m = _model(REDS_FEW_LEVELS)
    assert m.num_enc_layers == 2 and m.flow_scales == {0}


def test_flow_scales_full():
    from vmg_amd.data import REDS_FULL
    m = _model(REDS_FULL)
    assert m.num_enc_layers == 4 and m.flow_scales == {0}


def test_flow_scales_temporal_not_empty():
    """temporal_empty = False: every stage has a temporal module, every scale keeps its flows."""
    from vmg_amd.data import REDS_FEW_LEVELS
    m = _model(dict(REDS_FEW_LEVELS, temporal_empty=False))
    assert m.flow_scales == {0, 1}
    from oracle import cases as C
    from tests.util import build_product
    m = build_product(C.cfg_tiny_few(temporal_empty=False), device=None)
    assert m.flow_scales == set(range(m.num_enc_layers))


def test_smoothing_only_where_flows_are_passed_on():
    from vmg_amd.data import REDS_FEW_LEVELS
    m = _model(REDS_FEW_LEVELS)
    assert m.encoder_layers[0].takes_flows and m.decoder_layers[0].takes_flows and not m.encoder_layers[1].takes_flows
    assert not any(s._smooth_unused for s in list(m.encoder_layers) + list(m.decoder_layers))
    assert [s.keeps_flow_scale for s in m.encoder_layers] == [True, False] and m.decoder_layers[0].keeps_flow_scale
    from vmg_amd.model import Mlp_encoder
    assert Mlp_encoder.flow_use(False, True) == (True, True) and Mlp_encoder.flow_use(None, True) == (False, False)
    assert Mlp_encoder.flow_use(None, False) == (False, True) and Mlp_encoder.flow_use(False, False) == (True, True)
    m._set_flows_all_scales(True)
    assert m._flows_all_scales and all(s._smooth_unused for s in list(m.encoder_layers) + list(m.decoder_layers))
