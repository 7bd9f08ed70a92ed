"""traj_mode 'max' on the host: construction, state-dict keys, the names of the new entry points.  No GPU."""
import pytest
import torch

CFG = {"model": "VMG", "scale": 4, "is_train": True, "dataset": {"image_shape_r": [3, 256, 256]},
       "network": {"embed_dim": [144, 144, 144], "depths": [4, 4, 4], "num_heads": [4, 8, 4], "num_frames": 6, "mlp_ratio": 2,
                   "n_groups": 1, "window_sizes": [[2, 8, 8], [4, 8, 8], [2, 8, 8]], "back_RBs": 0, "spynet": "no-such-file.pth",
                   "ltam": True, "traj_win": [16, None], "traj_keyframes_n": [3, None], "traj_heads": [4, None],
                   "temporal_type": [False, None], "temporal_empty": True, "traj_res_n": [15, 0, 15], "deform_groups": [8, 16, 8],
                   "max_res_scale": [1, 2, 1], "spatial_type": [False, False], "use_mdsc": False, "if_concat": False,
                   "flow_smooth": True, "smooth_region_range": 4, "ret_decay": True, "non_linear": True, "gating": True,
                   "if_symm": True, "symm_act": "tanh", "relu_scale": True, "relu_scale_norm": False, "ffn_type": "ffn_cnn",
                   "mixer_type": ["mlps", "mlps"], "mixer_n": [None, None], "r_scaling": 0.1, "chunk_ratios": ["1/8", "1/4"],
                   "traj_mode": "max", "twins": [2, 2], "traj_scale": True, "traj_refine": None, "m_scaling": 1.0,
                   "if_local_fuse": True, "channel_mixer": "rcab"}}


def _cfg(mode):
    return {**CFG, "network": {**CFG["network"], "traj_mode": mode}}


def test_create_model_with_traj_mode_max():
    """The config of tests/test_host_logic.py::test_create_model_from_yaml_like_config with traj_mode: max: 560 - 4 entries (each of the two LTAM modules
    loses relative_pos_encoding and decay_v)."""
    import vmg_amd
    with pytest.warns(UserWarning):
        m = vmg_amd.create_model(_cfg("max"))
    sd = m.state_dict()
    assert len(sd) == 556
    assert not any("relative_pos_encoding" in k or "decay_v" in k for k in sd)
    ltam = sorted(k for k in sd if ".LTAM." in k)
    assert len(ltam) == 4 and all(k.endswith(("LTAM.proj.weight", "LTAM.proj.bias")) for k in ltam)
    with pytest.warns(UserWarning):
        w = vmg_amd.create_model(_cfg("wins"))
    assert set(w.state_dict()) - set(sd) == {k.replace("proj.weight", x) for k in ltam if k.endswith("proj.weight") for x in ("relative_pos_encoding", "decay_v")}


@pytest.mark.parametrize("mode", ["average", "softmax"])
def test_other_traj_modes_are_refused(mode):
    import vmg_amd
    with pytest.raises(NotImplementedError, match="'wins' or 'max'"):
        vmg_amd.create_model(_cfg(mode))


def test_max_mode_state_dict_keys_are_the_references():
    """The tiny few-levels model in 'max' mode has exactly the key list the reference's model reported (tests/golden/ltam_max.npz): 192 entries
    against 196 in 'wins', so a reference checkpoint loads with strict=True."""
    from oracle import cases as C
    from tests.traj_max_util import build_product_max, fixture, tiny_state_dict
    _, meta = fixture()
    m = build_product_max(C.cfg_tiny_few(meta["tiny"]["T"]), device=None)
    assert list(m.state_dict().keys()) == meta["tiny_keys"] and len(meta["tiny_keys"]) == 192
    m.load_state_dict(tiny_state_dict(meta), strict=True)


def test_ltam_module_modes():
    from vmg_amd.model import LTAM_multi_head, Trajectory_multi_head
    mx = LTAM_multi_head(32, 4, True, (2, 2), mode="max")
    assert sorted(mx.state_dict()) == ["proj.bias", "proj.weight"] and mx.scale == 1.0
    assert sorted(LTAM_multi_head(32, 4, True, (2, 2)).state_dict()) == ["decay_v", "proj.bias", "proj.weight", "relative_pos_encoding"]
    assert Trajectory_multi_head(32, 2, 2, 4, True, 0.1, (2, 2), mode="max").LTAM.mode == "max"
    with pytest.raises(NotImplementedError):
        LTAM_multi_head(32, 4, True, (2, 2), mode="average")


def test_entry_points_are_declared():
    from vmg_amd import functional as FH
    from vmg_amd import hip, kernels as K
    for nm in ("vmg_ltam_max_fwd", "vmg_ltam_max_bwd", "vmg_ltam_max_fwd_tab", "vmg_ltam_max_bwd_tab"):
        assert nm in hip.SIGNATURES
    for nm in ("ltam_max_forward", "ltam_max_backward", "ltam_max_forward_tab", "ltam_max_backward_tab"):
        assert callable(getattr(K, nm))
    assert callable(FH.ltam_max_attention)


def test_product_in_max_mode_refuses_cpu():
    from oracle import cases as C
    from tests.traj_max_util import build_product_max
    from vmg_amd.hip import HipError
    m = build_product_max(C.cfg_tiny_few(3), device=None).eval()
    with pytest.raises(HipError):
        m(torch.rand(1, 3, 3, 64, 64))
