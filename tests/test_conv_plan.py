"""vmg_conv_fwd_plan (include/vmg_hip.h): the host function vmg_conv_fwd dispatches through, asked without a GPU (ncu = 256, the MI355X's
compute units; no pointer of a descriptor is dereferenced, so small aligned integers stand for the tensors).

The expected instances are written by hand from the rule in the vmg_conv_desc::deep comment of include/vmg_hip.h, in the case table of
tests/test_linear_kernels_gpu.py (Case.kernel) and in the tables below -- never by calling the plan."""
import ctypes

import pytest
import torch

from tests import test_linear_kernels_gpu as G

NCU = 256
IGEMM, KSPLIT, WS, WRES, WSTAT = 1, 2, 3, 4, 5  # VMG_CONV_FAM_*


def _hip():
    from vmg_amd import hip
    assert (hip.CONV_FAM_IGEMM, hip.CONV_FAM_KSPLIT, hip.CONV_FAM_WS, hip.CONV_FAM_LINEAR_WRES, hip.CONV_FAM_WSTAT) == (IGEMM, KSPLIT, WS, WRES, WSTAT)
    return hip


def _plan(d, ncu=NCU):
    hip = _hip()
    p = (ctypes.c_int * hip.CONV_PLAN_INTS)(*([-7] * hip.CONV_PLAN_INTS))
    rc = hip.lib().vmg_conv_fwd_plan(ctypes.byref(d), ncu, p)
    return (tuple(p), None) if rc == 0 else (None, hip.lib().vmg_last_error().decode())


def _desc(N, H, W, src_ch, co, tiles, deep, dtype=1, ks=1, mt=0, src_ps=None, out_ps=None, res=False, aux=False, pre=False, act=0, actgrad=0,
          pixel_shuffle=False, res_ps=None, aux_ps=None, src_off=0, res_off=0):
    """A descriptor whose pointers are numbers: distinct 1-MiB-spaced addresses, 16-byte aligned but for the stated element offsets."""
    hip = _hip()
    es = 2 if dtype == 1 else 4
    d = hip.ConvDesc()
    d.dtype, d.ks, d.cout_tiles, d.N, d.H, d.W, d.Cout, d.nsrc = dtype, ks, tiles, N, H, W, co, len(src_ch)
    for s, c in enumerate(src_ch):
        d.src[s], d.src_ps[s], d.src_ch[s] = (s + 1) << 20 | (src_off * es), (src_ps[s] if src_ps else c), c
    d.packed, d.bias, d.out, d.out_ps = 8 << 20, 9 << 20, 10 << 20, out_ps or (co // 4 if pixel_shuffle else co)
    if pre:
        d.out_pre = 11 << 20
    if res:
        d.res, d.res_ps = 12 << 20 | (res_off * es), res_ps or co
    if aux:
        d.aux, d.aux_ps, d.actgrad = 13 << 20, aux_ps or co, actgrad
    d.act, d.slope, d.alpha, d.pixel_shuffle, d.mt, d.deep = act, 0.25, 1.0, int(pixel_shuffle), mt, deep
    return d


def _case_desc(case, ncu=NCU):
    hip = _hip()
    N, H, W = G.rows_for(case, ncu)
    dt, tiles, mt, route = G.request(case)
    e = G.EPILOGUES[case.epi]
    lay = G.layout(case)
    deep = dict(general=hip.CONV_GENERAL, ksplit=hip.CONV_KSPLIT, wres=hip.CONV_LINEAR_WRES)[route]
    return _desc(N, H, W, case.src_ch, case.co, tiles, deep, dtype=1 if dt == torch.bfloat16 else 0, mt=mt, src_ps=lay.src_ps, out_ps=lay.out_ps,
                 res=e.get("res", False), aux=bool(e.get("actgrad")), pre=e.get("want_pre", False), act=e.get("act", 0), actgrad=e.get("actgrad", 0),
                 pixel_shuffle=e.get("pixel_shuffle", False), res_ps=lay.res_ps, aux_ps=lay.aux_ps, src_off=case.src_off if case.i_total else 0,
                 res_off=case.res_off)


def test_every_gpu_case_reaches_the_instance_it_names():
    for case in G.all_cases():
        plan, err = _plan(_case_desc(case))
        assert err is None, f"{case.id}: {err}"
        assert plan[:7] == G.expected_plan(case), f"{case.id}: the plan says {plan}, the case names {G.expected_plan(case)}"
        N, H, W = G.rows_for(case, NCU)
        ncb = -(-case.co // (16 * plan[4]))
        assert plan[8] == ncb
        if case.kernel[0] != G.WRES:
            assert plan[7] == -(-N * H * W // (64 * plan[3])) and plan[9] == 0  # a workgroup per 64 * MT rows
        if case.tpw:
            assert plan[9] == case.tpw


def test_the_case_table_reaches_all_28_instances_and_every_fallback_is_one():
    reached = {c.kernel for c in G.all_cases()}
    assert reached == set(G.INSTANCES) and len(G.INSTANCES) == 28, set(G.INSTANCES) ^ reached
    # every instance is also reached by an EXACT case at a ragged row count
    assert {c.kernel for c in G.exact_cases() if c.geom and (c.geom[0] * c.geom[1] * c.geom[2]) % 16} == set(G.INSTANCES)
    fallbacks = [c for c in G.all_cases() if c.hint]
    assert len(fallbacks) >= 30
    for c in fallbacks:
        plan, err = _plan(_case_desc(c))
        assert err is None and plan[0] == IGEMM and plan[3] == 1 and plan[5] == 0 and plan[9] == 0, f"{c.id}: {plan} {err}"
    # the sweep over the single sources says which belong to the wave-autonomous kernel: channels % 32 == 16 (the dense LDS stride)
    assert G.WRES_DENSE == tuple(c for c in range(8, 161, 8) if c % 32 == 16)
    sweep = [c for c in G._channel_cases() if c.geom == (1, 1, 80) and len(c.src_ch) == 1 and c.src_ch[0] <= 160 and not c.i_total and not c.o_total]
    assert {c.src_ch[0] for c in sweep if c.kernel[0] == G.WRES} == set(G.WRES_DENSE)
    assert {c.src_ch[0] for c in sweep if c.hint} == set(range(8, 161, 8)) - set(G.WRES_DENSE)
    assert {c.src_ch[0] for c in G._channel_cases() if c.kernel == (G.WRES, 3, 2) and c.geom == (1, 1, 80) and not c.i_total and not c.o_total} == \
        set(range(176, 321, 16))


# What the tables of two older tolerance tests of tests/test_conv_gpu.py really run (contiguous tensors; the three epilogues of a shape take the
# same kernel).  "fallback": the case reads as a test of the hinted kernel and runs the general one -- it tests the fallback, and stays.
WAVE_AUTONOMOUS_TABLE = {  # test_linear_wave_autonomous_variant: (M, Ci, Co) -> {tiles: (kernel, NS)}
    (1000, 144, 144): {5: ("wres", 1), 3: ("wres", 1)},
    (114688, 144, 144): {5: ("wres", 1), 3: ("wres", 1)},
    (4097, 144, 288): {5: ("wres", 1), 3: ("wres", 1)},
    (300, 160, 48): {5: ("fallback", 0), 3: ("fallback", 0)},     # 160 channels: padded LDS stride
    (777, 64, 144): {5: ("fallback", 0), 3: ("fallback", 0)},     # 64 channels: padded LDS stride
    (50, 8, 16): {5: ("fallback", 0), 3: ("fallback", 0)},        # 8 channels: padded LDS stride
    (4113, 288, 144): {5: ("fallback", 0), 3: ("wres", 2)},       # the two-block form exists for cout_tiles 3 only
    (70000, 288, 144): {5: ("fallback", 0), 3: ("wres", 2)},
    (333, 320, 96): {5: ("fallback", 0), 3: ("wres", 2)},
    (500, 224, 112): {5: ("fallback", 0), 3: ("wres", 2)},
}
WEIGHTS_STATIONARY_TABLE = {  # test_conv_weights_stationary_variant: (N, H, W, Ci, Co) -> (NCT, NB); none falls back
    (2, 40, 52, 64, 64): (4, 2), (1, 8, 16, 64, 64): (4, 2), (3, 19, 37, 64, 64): (4, 2), (1, 64, 300, 8, 64): (4, 1), (2, 33, 20, 32, 48): (3, 1),
    (1, 24, 48, 48, 16): (1, 2), (5, 128, 128, 64, 64): (4, 2), (1, 7, 5, 64, 16): (1, 2),
}


def _old_table(name):
    """The parametrize lists of tests/test_conv_gpu.py, read from the test functions themselves."""
    from tests import test_conv_gpu as T
    marks = {m.args[0]: list(m.args[1]) for m in getattr(T, name).pytestmark if m.name == "parametrize"}
    return marks


def test_what_the_hinted_tolerance_tests_really_run():
    hip = _hip()
    marks = _old_table("test_linear_wave_autonomous_variant")
    assert set(marks["shape"]) == set(WAVE_AUTONOMOUS_TABLE) and set(marks["tiles"]) == {5, 3}
    for (M, ci, co), per_tiles in WAVE_AUTONOMOUS_TABLE.items():
        for tiles, (kernel, ns) in per_tiles.items():
            for kw in (dict(pre=True, act=3), dict(res=True, aux=True, actgrad=1), dict(act=1)):
                plan, err = _plan(_desc(1, 1, M, (ci,), co, tiles, hip.CONV_LINEAR_WRES, **kw))
                assert err is None
                want = (WRES, 1, 1, 1, tiles, ns, 1) if kernel == "wres" else (IGEMM, 1, 1, 1, tiles, 0, 1)
                assert plan[:7] == want, f"{(M, ci, co)} tiles {tiles}: {plan}"
    marks = _old_table("test_conv_weights_stationary_variant")
    assert set(marks["case"]) == set(WEIGHTS_STATIONARY_TABLE)
    for (N, H, W, ci, co), (nct, nb) in WEIGHTS_STATIONARY_TABLE.items():
        assert nct == co // 16
        for full, kw in ((0, dict(act=2)), (1, dict(res=True, aux=True, actgrad=1)), (1, dict(pre=True, act=3))):
            plan, err = _plan(_desc(N, H, W, (ci,), co, nct, hip.CONV_WSTAT, ks=3, **kw))
            assert err is None and plan[:7] == (WSTAT, 1, 3, 1, nct, nb | full << 4, 1), f"{(N, H, W, ci, co)}: {plan} {err}"
            tiles = N * -(-H // 8) * -(-W // 16)
            assert plan[7] == min(NCU, 8 * -(-tiles // 8)) and plan[8] == 1  # a workgroup per CU, a multiple of 8, no more than the tiles need


def test_grid_rule_of_the_wave_autonomous_kernel():
    """launch_linear_wres at 256 compute units, values computed by hand: waves = max(1, (2 / NS) * 256 / ncb) * 4, tiles per wave =
    max(4, ceil(ntiles / waves)), workgroups = ceil(ceil(ntiles / tpw) / 4)."""
    hip = _hip()
    hand = [
        # (M, Ci, Co, tiles) -> (grid x, grid y, tiles per wave)
        ((1000, 16, 48, 3), (4, 1, 4)),          # ncb 1: 63 tiles on 2048 waves -> 4 per wave, 16 waves
        ((131073, 16, 48, 3), (410, 1, 5)),      # ncb 1: 8193 tiles = 4 * 2048 + 1 -> 5 per wave, 1639 waves
        ((131073, 16, 80, 5), (410, 1, 5)),
        ((64, 144, 144, 3), (1, 3, 4)),          # ncb 3: one wave
        ((65, 144, 144, 3), (1, 3, 4)),          # ... a second wave with one tile
        ((257, 144, 144, 3), (2, 3, 4)),         # 17 tiles: 5 waves, the second workgroup has one
        ((114688, 144, 144, 3), (163, 3, 11)),   # ncb 3: 170 workgroups x 4 = 680 waves; 7168 tiles -> 11 per wave, 652 waves
        ((114688, 144, 144, 5), (256, 2, 7)),    # ncb 2: 1024 waves -> 7 per wave
        ((70000, 288, 144, 3), (85, 3, 13)),     # NS 2, ncb 3: 85 x 4 = 340 waves; 4375 tiles -> 13 per wave, 337 waves
        ((43521, 288, 144, 3), (76, 3, 9)),      # 2721 tiles = 8 * 340 + 1 -> 9 per wave, 303 waves
    ]
    for (M, ci, co, tiles), want in hand:
        plan, err = _plan(_desc(1, 1, M, (ci,), co, tiles, hip.CONV_LINEAR_WRES))
        assert err is None and plan[0] == WRES, f"{(M, ci, co, tiles)}: {plan} {err}"
        assert (plan[7], plan[8], plan[9]) == want, f"{(M, ci, co, tiles)}: {plan}"
    for M in list(range(1, 300)) + [1000, 4097, 8 * 2048 * 16 + 1, 10 ** 6]:
        for ci, co, tiles in ((144, 144, 3), (16, 80, 5), (288, 144, 3)):
            plan, _ = _plan(_desc(1, 1, M, (ci,), co, tiles, hip.CONV_LINEAR_WRES))
            ntiles, tpw = -(-M // 16), plan[9]
            assert tpw >= 4 and plan[7] == -(-(-(-ntiles // tpw)) // 4) and plan[7] * 4 * tpw >= ntiles
    # the big cases of the GPU module choose their rows by the same rule
    for c in G.all_cases():
        if c.tpw:
            assert G.rows_for(c, NCU)[2] in (131073, 43521)


def test_the_plan_depends_on_the_compute_units_only_where_the_grid_does():
    hip = _hip()
    d = _desc(1, 1, 100000, (144,), 144, 3, hip.CONV_LINEAR_WRES)
    assert _plan(d, 256)[0] != _plan(d, 64)[0] and _plan(d, 64)[0][9] > _plan(d, 256)[0][9]
    d = _desc(1, 1, 100000, (144,), 144, 3, hip.CONV_GENERAL)
    assert _plan(d, 256) == _plan(d, 8) and _plan(d, 256)[0][7] == -(-100000 // 64)


def test_refusals_carry_the_message_of_conv_fwd():
    hip = _hip()
    bad = [
        (_desc(1, 1, 100, (144,), 144, 7, hip.CONV_KSPLIT), "conv (k-split): cout_tiles must be 1, 3, 4 or 5 (got 7)"),
        (_desc(1, 1, 100, (144,), 144, 3, hip.CONV_KSPLIT, dtype=0), "conv_fwd: the k-split variant is bf16, mt = 1"),
        (_desc(1, 1, 100, (144,), 144, 3, hip.CONV_KSPLIT, mt=2), "conv_fwd: the k-split variant is bf16, mt = 1"),
        (_desc(1, 1, 100, (12,), 16, 1, hip.CONV_GENERAL), "conv_fwd: source channel counts must be multiples of 8"),
        (_desc(1, 1, 100, (144,), 144, 2, hip.CONV_GENERAL), "conv: cout_tiles must be 1, 3, 4, 5, 7, 8 or 9 (got 2)"),
        (_desc(1, 1, 100, (144,), 144, 3, 5), "conv_fwd: unknown kernel route deep = 5"),
        (_desc(1, 1, 100, (144,), 144, 3, hip.CONV_GENERAL, src_off=1), "conv_fwd: source pointer must be 16-byte aligned"),
        (_desc(1, 1, 100, (144,), 144, 3, hip.CONV_GENERAL, out_ps=100), "conv_fwd: out pixel stride too small"),
        (_desc(1, 1, 100, (144,), 144, 9, hip.CONV_WS), "conv_fwd: the weight-streaming kernel is bf16 3x3 with 16-byte aligned rows, cout_tiles 3, 7, 8 or 9"),
    ]
    for d, msg in bad:
        plan, err = _plan(d)
        assert plan is None and err == msg, (plan, err)
    hip_lib = hip.lib()
    assert hip_lib.vmg_conv_fwd_plan(None, NCU, (ctypes.c_int * hip.CONV_PLAN_INTS)()) == -1
    assert hip_lib.vmg_conv_fwd_plan(ctypes.byref(_desc(1, 1, 100, (144,), 144, 3, 0)), -1, (ctypes.c_int * hip.CONV_PLAN_INTS)()) == -1


def test_the_3x3_and_7x7_families_are_reported():
    hip = _hip()
    plan, _ = _plan(_desc(2, 7, 15, (144,), 144, 9, hip.CONV_WS, ks=3))
    assert plan[:7] == (WS, 1, 3, 1, 9, 0, 1) and plan[7:10] == (2 * 1 * 1, 1, 0)
    plan, _ = _plan(_desc(2, 7, 15, (144,), 144, 3, hip.CONV_KSPLIT, ks=3))
    assert plan[:7] == (KSPLIT, 1, 3, 1, 3, 0, 1) and plan[7:10] == (2 * 2 * 1, 3, 0)
    plan, _ = _plan(_desc(2, 7, 15, (8,), 32, 2, hip.CONV_GENERAL, ks=7, dtype=0))
    assert plan[:7] == (IGEMM, 0, 7, 1, 2, 0, 0) and plan[7:10] == (4, 1, 0)


# ---- the table of tests/test_conv_general_kernels_gpu.py: the general 3x3 / 7x7 kernel and the weights-stationary kernel --------------------
from tests import test_conv_general_kernels_gpu as GG  # noqa: E402


def _full_grid(case, ncu):
    """What the GPU module asks the live plan: the grid of a weights-stationary launch that fills the device."""
    hip = _hip()
    N, H, W = GG.WSTAT_FILL
    plan, err = _plan(_desc(N, H, W, case.src_ch, case.co, case.kernel[1], hip.CONV_WSTAT, ks=3), ncu)
    assert err is None and plan[0] == WSTAT, f"{case.id}: {plan} {err}"
    return plan[7]


def _general_geom(case, ncu):
    return case.geom if case.geom is not None else GG.wstat_rows(_full_grid(case, ncu))


def _general_desc(case, ncu=NCU):
    hip = _hip()
    N, H, W = _general_geom(case, ncu)
    dt, ks, tiles, mt, route = GG.request(case)
    e = GG.EPILOGUES[case.epi]
    lay = GG.layout(case)
    deep = dict(general=hip.CONV_GENERAL, wstat=hip.CONV_WSTAT)[route]
    return _desc(N, H, W, case.src_ch, case.co, tiles, deep, dtype=1 if dt == torch.bfloat16 else 0, ks=ks, mt=mt, src_ps=lay.src_ps, out_ps=lay.out_ps,
                 res=e.get("res", False), aux=bool(e.get("actgrad")), pre=e.get("want_pre", False), act=e.get("act", 0), actgrad=e.get("actgrad", 0),
                 pixel_shuffle=e.get("pixel_shuffle", False), res_ps=lay.res_ps, aux_ps=lay.aux_ps, src_off=case.src_off if case.i_total else 0)


def test_every_general_and_weights_stationary_case_reaches_the_instance_it_names():
    cases = GG.all_cases()
    assert len(cases) > 700
    for case in cases:
        plan, err = _plan(_general_desc(case))
        assert err is None, f"{case.id}: {err}"
        assert plan[:7] == GG.expected_plan(case), f"{case.id}: the plan says {plan}, the case names {GG.expected_plan(case)}"
        N, H, W = _general_geom(case, NCU)
        assert plan[9] == 0 and plan[10] <= 160 * 1024
        if case.kernel[0] == GG.IG:
            assert (plan[7], plan[8]) == GG.expected_grid(case, (N, H, W)), f"{case.id}: {plan}"
        else:
            tiles = N * -(-H // 8) * -(-W // 16)
            assert plan[7] == min(NCU, 8 * -(-tiles // 8)) and plan[8] == -(-case.co // (16 * case.kernel[1])), f"{case.id}: {plan}"
            assert case.kernel[2] == (1 if case.src_ch[0] <= 32 else 2) and len(case.src_ch) == 1


def test_the_general_table_reaches_all_39_instances_and_every_fallback_is_one():
    hip = _hip()
    reached = {c.kernel for c in GG.all_cases()}
    assert reached == set(GG.INSTANCES) and len(GG.INSTANCES) == 39, set(GG.INSTANCES) ^ reached
    # every instance is also reached by an EXACT case on a ragged geometry (no pytest.skip / xfail anywhere in the module: nothing to leave out)
    ragged = {c.kernel for c in GG.exact_cases() if c.geom and (c.geom[1] % 8 or c.geom[2] % 16)}
    assert ragged == set(GG.INSTANCES), set(GG.INSTANCES) ^ ragged
    # both epilogue paths of the general kernel meet the chain module's whole table, for 3x3 in both dtypes and both MT, for 7x7 in both dtypes
    for vector in (True, False):
        for dt, ks, mt in (("bf16", 3, 1), ("bf16", 3, 2), ("f32", 3, 1), ("bf16", 7, 1), ("f32", 7, 1)):
            names = {c.epi for c in GG._epilogue_cases() if c.kernel[:4] == (GG.IG, dt, ks, mt) and (c.co % 16 == 0) == vector and c.out_pad == 8}
            assert names >= set(GG.CHAIN_TABLE), (vector, dt, ks, mt, set(GG.CHAIN_TABLE) - names)
    full = {c.epi for c in GG._wstat_cases() if c.kernel[0] == GG.WSTAT and c.kernel[3] == 1}
    simple = {c.epi for c in GG._wstat_cases() if c.kernel[0] == GG.WSTAT and c.kernel[3] == 0}
    assert full >= set(GG.WSTAT_FULL) and simple >= set(GG.WSTAT_SIMPLE) | {"plain", "bias"} and not (full & simple)
    # the probe set of every probed channel case meets every tap (9 / 49) in every 16-channel output tile
    assert GG.probe_taps_missing(GG.all_cases()) == {}
    assert {c.kernel[:3] for c in GG._probe_cases() if c.kernel[0] == GG.IG} == {(GG.IG, d, k) for d in ("bf16", "f32") for k in (3, 7)}
    assert {c.kernel[:3] for c in GG._probe_cases() if c.kernel[0] == GG.WSTAT} == {(GG.WSTAT, n, b) for n in (1, 3, 4) for b in (1, 2)}
    broken = [c for c in GG._probe_cases() if c.kernel[2] == 7][:3]  # (the check can fail: three of four 7x7 probes leave taps out)
    assert GG.probe_taps_missing(broken) != {}
    # the declared fallbacks: the hint (or mt = 2) is really asked for, and the general kernel with MT as named really runs
    fallbacks = [c for c in GG.all_cases() if c.fallback]
    assert {c.fallback for c in fallbacks} == {"wstat", "mt2"} and len(fallbacks) >= 9
    for c in fallbacks:
        d = _general_desc(c)
        plan, err = _plan(d)
        assert err is None and plan[0] == IGEMM and plan[5] == 0 and plan[3] == c.kernel[3], f"{c.id}: {plan} {err}"
        assert (d.deep == hip.CONV_WSTAT) == (c.fallback == "wstat") and (d.mt == 2 and plan[3] == 1) == (c.fallback == "mt2")
    assert all(c.fallback or GG.request(c)[4] == ("wstat" if c.kernel[0] == GG.WSTAT else "general") for c in GG.all_cases())
    # a source pixel stride that is no multiple of 8 is no fallback of the hint: 16-byte rows are demanded of every route
    for deep in (hip.CONV_WSTAT, hip.CONV_GENERAL):
        plan, err = _plan(_desc(2, 7, 15, (64,), 64, 4, deep, ks=3, src_ps=(68,)))
        assert plan is None and err == "conv_fwd: source pixel stride must be >= channels and 16-byte aligned"
    # the geometries the issue names, on one channel case per kernel family
    for fam in GG.G3:
        assert {c.geom for c in GG._geometry_cases() if c.kernel[:4] == fam} == set(GG.GEOMS)
    for fam in GG.G7:
        assert {c.geom for c in GG._geometry_cases() if c.kernel[:4] == fam} == set(GG.GEOMS7)
    for nb in (1, 2):
        assert {c.geom for c in GG._wstat_cases() if c.kernel[0] == GG.WSTAT and c.kernel[2] == nb and c.geom} >= set(GG.WGEOMS)
    for mt in (1, 2):
        blocks = lambda g: g[0] * -(-g[1] // (4 * mt)) * -(-g[2] // 16)  # noqa: E731
        assert blocks((2, 16, 32)) % 8 == 0 and blocks((1, 24, 81)) % 8 != 0 and blocks((1, 24, 81)) > 15  # 160 channels, 3x3: 5 blocks x 3 tap rows


@pytest.mark.parametrize("ncu", [256, 64])
def test_many_tile_weights_stationary_cases_follow_the_grid(ncu):
    """The rule the GPU module applies to the live grid, at 256 and at 64 compute units: a workgroup walks three tiles, the XCD bands are uneven."""
    many = [c for c in GG.all_cases() if c.geom is None]
    assert len(many) == 2 and {c.kernel for c in many} == {(GG.WSTAT, 1, 1, 0), (GG.WSTAT, 1, 1, 1)} and all(c.src_ch == (8,) and c.co == 16 for c in many)
    for c in many:
        grid = _full_grid(c, ncu)
        assert grid == ncu
        geom = GG.wstat_rows(grid)
        plan, err = _plan(_general_desc(c, ncu), ncu)
        assert err is None and plan[:7] == GG.expected_plan(c) and plan[7] == grid, f"{c.id}: {plan} {err}"
        ntiles = GG.assert_many_tiles(geom, plan[7])
        walks, bands = GG.wstat_walk(ntiles, grid)
        assert max(walks) == 3 and min(walks) >= 1 and 2 * grid < ntiles <= 2 * grid + 12
        assert geom == {256: (1, 821, 75), 64: (1, 205, 75)}[ncu] and ntiles == {256: 515, 64: 130}[ncu]
        assert bands == {256: [65] * 7 + [60], 64: [17] * 7 + [11]}[ncu]
    # the rule refuses what it must
    with pytest.raises(AssertionError):
        GG.assert_many_tiles((1, 821, 75), 512)   # two tiles per workgroup at most
    with pytest.raises(AssertionError):
        GG.assert_many_tiles((1, 8 * 104 - 3, 75), 256)  # 520 tiles: even bands
