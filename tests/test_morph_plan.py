"""vmg_morphfc_plan and vmg_morph_tokens_route (include/vmg_hip.h): the host functions vmg_morphfc_fwd and vmg_morph_tokens_gather / _scatter
dispatch through, asked without a GPU (ncu = 256, the MI355X's compute units), and the case tables of tests/test_morph_kernels_gpu.py held
against them.  The expected instances and routes are written by hand in those tables (NK_NCT, S_EVEN, Tok.route / cause) and below -- never
obtained by calling the plan.

The fused kernel has 20 instantiations, morph_linear_kernel<NK, NCT, EVEN, MASK>: (NK, NCT) = (5, 9), (4, 7), (2, 4), (1, 2), (1, 1) for Cp = 144,
112, 64, 32, 16, each with S = Cp / chunk even and odd, each plain and masked.  16 are reachable.  The four with (NK, NCT) = (2, 4) or (1, 2)
and EVEN = false are not: chunk 8 and 16 give S = 8, 4 at Cp 64 and S = 4, 2 at Cp 32, all even
(test_no_shipped_shape_reaches_the_four_odd_instances_of_cp_64_and_32).  The instantiations stay: the entry point goes by (NK, NCT), so a Cp
that is none of the five but shares them with one (56 or 24 at chunk 8) would run them; kernels.morph_fused_ok admits the five only, so the
product never asks."""
import ctypes

import pytest
import torch

from tests import test_morph_kernels_gpu as G

NCU = 256
REACHABLE = {(5, 9, True), (5, 9, False), (4, 7, True), (4, 7, False), (1, 1, True), (1, 1, False), (2, 4, True), (1, 2, True)}
UNREACHABLE = {(2, 4, False), (1, 2, False)}
INSTANTIATED = {(5, 9), (4, 7), (2, 4), (1, 2), (1, 1)}
GEOMETRY_MESSAGE = "morphfc: chunk must be 8 or 16 and divide Cp; C a multiple of 8, at most 160"


def _plan(axis, chunk, BT, H, W, C, Cp, mask, ncu=NCU):
    from vmg_amd import hip
    assert hip.MORPHFC_PLAN_INTS == 8
    p = (ctypes.c_int * 8)(*([-7] * 8))
    rc = hip.lib().vmg_morphfc_plan(0 if axis == "h" else 1, chunk, BT, H, W, C, Cp, int(mask), ncu, p)
    return (tuple(p), None) if rc == 0 else (None, hip.lib().vmg_last_error().decode())


def _case_plan(case, ncu=NCU):
    B, T, H, W = G.geometry(case, ncu)
    plan, err = _plan(case.axis, case.chunk, B * T, H, W, case.C, case.Cp, case.form == "mask", ncu)
    assert err is None, f"{case.id}: {err}"
    return plan


def test_the_fused_table_reaches_exactly_the_16_reachable_instances():
    assert len(REACHABLE) * 2 == 16 and len(UNREACHABLE) * 2 == 4 and {i[:2] for i in REACHABLE | UNREACHABLE} == INSTANTIATED
    seen, by_kind = set(), {}
    for case in G.FUSED:
        plan = _case_plan(case)
        assert plan[:4] == tuple(int(v) for v in G.instance(case)), f"{case.id}: the plan says {plan}, the case names {G.instance(case)}"
        seen.add(G.instance(case))
        by_kind.setdefault(case.kind[:5], set()).add(G.instance(case))
    want = {i + (m,) for i in REACHABLE for m in (False, True)}
    assert seen == want and len(seen) == 16
    assert by_kind["exact"] == want                                          # every reachable instance has exact cases
    assert by_kind["probe"] == {i + (False,) for i in REACHABLE}             # the probes are plain
    assert {i[:2] for i in by_kind["real"]} == INSTANTIATED and {i[3] for i in by_kind["real"]} == {False, True}
    # every (Cp, chunk) pair in both forms on both axes at every edge
    for Cp, chunk in G.PAIRS:
        for form in ("plain", "mask"):
            for axis in ("h", "w"):
                names = {c.id.split("-")[-1] for c in G.FUSED if (c.Cp, c.chunk, c.form, c.axis, c.kind) == (Cp, chunk, form, axis, "exact") and c.geom}
                assert names >= {"len1", "len3", "multiple", "rem1", "remcm1", "cpad", "single"}, (Cp, chunk, form, axis, names)
                assert ("dead17x5" in names) == (chunk == 8)


def test_no_shipped_shape_reaches_the_four_odd_instances_of_cp_64_and_32():
    from vmg_amd import kernels as K
    assert tuple(sorted(K.MORPH_FUSED_CP)) == (16, 32, 64, 112, 144) == tuple(sorted(G.NK_NCT))
    seen = set()
    for Cp in K.MORPH_FUSED_CP:
        for chunk in (8, 16):
            for mask in (False, True):
                for C in range(8, Cp + 1, 8):
                    if chunk * C // 8 > 320:
                        continue
                    plan, err = _plan("w", chunk, 2, 5, 19, C, Cp, mask)
                    assert err is None, (Cp, chunk, C, err)
                    assert plan[:2] == G.NK_NCT[Cp] and bool(plan[2]) == G.S_EVEN[(Cp, chunk)] and bool(plan[3]) == mask
                    seen.add((plan[0], plan[1], bool(plan[2])))
    assert seen == REACHABLE and not (seen & UNREACHABLE)


def test_loops_and_dead_group_cases_are_what_they_say():
    loops = dead = single = 0
    for case in G.FUSED:
        NK, NCT, EVEN, MASK, ngroups, ntiles, nwg, lds = _case_plan(case)
        B, T, H, W = G.geometry(case, NCU)
        length, lines = (H, W) if case.axis == "h" else (W, H)
        assert ngroups == B * T * lines * -(-length // case.chunk) and ntiles == -(-ngroups // (16 // case.chunk)) and nwg == min(NCU, -(-ntiles // 8))
        assert ("loops" in case.tags) == (ntiles > 8 * nwg) == (case.geom is None), case.id
        if "loops" in case.tags:
            loops += 1
            assert nwg == NCU and 8 * nwg < ntiles <= 8 * nwg + 8, case.id  # a partial last trip: only the first waves own two tiles
            assert length % case.chunk == 1                                   # and groups with one live position
        if "dead group" in case.tags:
            dead += 1
            assert case.chunk == 8 and ngroups % 2 == 1, case.id
        if "single tile" in case.tags:
            single += 1
            assert ntiles == 1, case.id
        assert ("channel padding" in case.tags) == (case.C < case.Cp)
        # the LDS the kernel asks for: weights (ceil(NK / 2) stages), bias, 8 waves x two 16-pixel blocks + 16 bytes
        stage = -(-2 * 4 * NCT * 16 * 16 // 4096) * 4096
        assert lds == -(-NK // 2) * stage + NCT * 64 + 8 * (2 * 16 * case.Cp * 2 + 16) and lds <= 160 * 1024
    # loops: once per reachable (NK, NCT, EVEN) plain, Cp 144 in both parities masked, and a real-valued one
    lp = [G.instance(c) for c in G.FUSED if "loops" in c.tags and c.kind == "exact"]
    assert {i[:3] for i in lp if not i[3]} == REACHABLE and {i[:3] for i in lp if i[3]} == {(5, 9, True), (5, 9, False)}
    assert any("loops" in c.tags and c.kind == "real" for c in G.FUSED)
    assert loops == 11 and dead >= 60 and single == 40
    # another device size: the loop cases still loop
    for ncu in (64, 304):
        for case in G.FUSED:
            if "loops" in case.tags:
                p = _case_plan(case, ncu)
                assert p[6] == ncu and 8 * ncu < p[5] <= 8 * ncu + 8


def test_every_fused_case_is_exact_and_not_degenerate_before_it_runs():
    for case in G.FUSED:
        G.fused_reference(case, NCU)


def _conditions(case):
    """The four element-wise conditions, from the rule in include/vmg_hip.h."""
    es = 2 if case.dtype == torch.bfloat16 else 4
    vn = 16 // es
    return {"C": case.C % vn != 0, "ld": case.ld % vn != 0, "lds": case.chunk * case.ld * es > 64 * 1024, "align": case.off % vn != 0}


def test_the_token_table_reaches_both_routes_for_both_dtypes_and_every_cause():
    from vmg_amd import hip, kernels as K
    assert (hip.MORPH_ROUTE_ELEMENT, hip.MORPH_ROUTE_LDS) == (G.ELEMENT_ROUTE, G.LDS_ROUTE) == (0, 1)
    reached, sole = set(), set()
    for case in G.TOKENS:
        conds = _conditions(case)
        assert case.route == (G.ELEMENT_ROUTE if any(conds.values()) else G.LDS_ROUTE), case.id
        got = hip.lib().vmg_morph_tokens_route(hip.dtype_code(case.dtype), case.chunk, case.C, case.ld, int(case.off == 0))
        assert got == case.route == K.morph_tokens_route(case.dtype, case.chunk, case.C, case.ld, case.off == 0), f"{case.id}: the route is {got}"
        if case.route == G.ELEMENT_ROUTE:
            assert conds[case.cause], case.id
            if case.sole:
                assert sum(conds.values()) == 1, f"{case.id}: {conds}"
                sole.add((case.dtype, case.cause))
        else:
            assert case.cause is None
        # each case launches the gather and the scatter: 2 kernels x 2 dtypes x 2 routes = the 8 kernel / dtype pairs
        reached |= {(k, case.dtype, case.route) for k in ("gather", "scatter")}
    assert len(reached) == 8
    assert sole == {(d, c) for d in (torch.bfloat16, torch.float32) for c in ("C", "ld", "lds", "align")}
    # the edges of the LDS route and both grid-stride loops
    lds = [c for c in G.TOKENS if c.route == G.LDS_ROUTE]
    for dt, vn in ((torch.bfloat16, 8), (torch.float32, 4)):
        mine = [c for c in lds if c.dtype == dt]
        assert {c.Cp // c.chunk for c in mine} >= {1, 2, 3}
        assert any(c.chunk * c.ld // vn < 256 for c in mine) and any(c.chunk * c.ld // vn > 256 for c in mine)
        assert any(G.MR.token_rows(c.axis, c.chunk, *c.geom) // c.chunk > 16384 for c in mine)
        el = [c for c in G.TOKENS if c.route == G.ELEMENT_ROUTE and c.dtype == dt]
        assert any(-(-G.MR.token_rows(c.axis, c.chunk, *c.geom) * c.ld // 256) > 8192 and -(-c.geom[0] * c.geom[1] * c.geom[2] * c.C // 256) > 8192 for c in el)
    assert any(c.ld > c.Cp for c in lds) and any(c.C < c.Cp for c in lds)
    # alignment alone decides for a shape the LDS kernel serves
    assert K.morph_tokens_route(torch.bfloat16, 8, 16, 16, True) == 1 and K.morph_tokens_route(torch.bfloat16, 8, 16, 16, False) == 0
    # 64 KiB exactly is still the LDS route
    assert K.morph_tokens_route(torch.bfloat16, 64, 8, 512, True) == 1 and K.morph_tokens_route(torch.bfloat16, 64, 8, 520, True) == 0
    assert K.morph_tokens_route(torch.float32, 64, 8, 256, True) == 1 and K.morph_tokens_route(torch.float32, 64, 8, 260, True) == 0


@pytest.mark.parametrize("what, args, message", [
    ("chunk 12", ("w", 12, 2, 5, 19, 144, 144, False), GEOMETRY_MESSAGE),
    ("chunk does not divide Cp", ("w", 16, 2, 5, 19, 8, 24, False), GEOMETRY_MESSAGE),
    ("C % 8", ("h", 8, 2, 5, 19, 12, 16, False), GEOMETRY_MESSAGE),
    ("C > Cp", ("h", 8, 2, 5, 19, 24, 16, False), GEOMETRY_MESSAGE),
    ("chunk * C / 8 > 320", ("h", 16, 2, 5, 19, 168, 176, True), GEOMETRY_MESSAGE),
    ("Cp 48", ("w", 16, 2, 5, 19, 48, 48, False), "morphfc: Cp = 48 is not instantiated (144, 112, 64, 32, 16)"),
    ("Cp 128", ("w", 8, 2, 5, 19, 128, 128, True), "morphfc: Cp = 128 is not instantiated (144, 112, 64, 32, 16)"),
    ("Cp 160", ("w", 16, 2, 5, 19, 160, 160, False), "morphfc: Cp = 160 is not instantiated (144, 112, 64, 32, 16)"),
    ("too many groups", ("w", 8, 2 ** 15, 2 ** 15, 17, 16, 16, False), "morphfc: too many groups"),
    ("no rows", ("w", 8, 2, 0, 19, 16, 16, False), "morphfc: bad arguments"),
])
def test_what_the_fused_kernel_does_not_serve_is_refused_with_its_message(what, args, message):
    from vmg_amd import kernels as K
    from vmg_amd.hip import HipError
    plan, err = _plan(*args)
    assert plan is None and err == message, f"{what}: {err!r}"
    with pytest.raises(HipError, match="not instantiated|chunk must be 8 or 16|too many groups|bad arguments"):
        K.morphfc_plan(*args, ncu=NCU)


def test_the_python_wrapper_names_the_plan_fields():
    from vmg_amd import kernels as K
    p = K.morphfc_plan("w", 8, 2, 41, 397, 144, 144, False, ncu=NCU)  # 2 x 41 lines of 50 groups: 4100 groups, 2050 tiles
    assert p == K.MorphfcPlan(NK=5, NCT=9, EVEN=True, MASK=False, ngroups=4100, ntiles=2050, nwg=256, lds_bytes=p.lds_bytes)
    assert p.ntiles > 8 * p.nwg and p.EVEN is True and p.MASK is False
    p = K.morphfc_plan("h", 16, 1, 17, 5, 8, 16, True, ncu=NCU)
    assert p[:7] == (1, 1, False, True, 10, 10, 2)
