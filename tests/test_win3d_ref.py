"""tests/win3d_ref.py is what the window-attention kernels are compared with (tests/test_win3d_gpu.py), so it is pinned first, here,
without a GPU: it must reproduce the oracle's swin_block on the reference fixtures' weights (the oracle itself is held to the
unmodified reference's outputs by tests/test_oracle_golden.py), and the geometries the GPU tests run must be ones on which a wrong
kernel would show: six deliberately wrong variants of the reference, built here by patching what it calls, must each move some
tensor by more than the loosest tolerance any comparison uses."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import win3d_cases as WC
from tests import win3d_ref as WR

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("block", [0, 1])
@pytest.mark.parametrize("name", ["swin_w2_t5", "swin_w4_t7"])
def test_reference_equals_the_oracle_block_on_the_fixture_weights(name, block):
    """LayerNorm -> q / kv Linears -> win3d_reference -> proj + residual -> MLP == O.swin_block in fp64, blocks 0 (plain) and 1 (shifted;
    swin_w2_t5 also pads D 5 -> 6 and 20 x 20 -> 24 x 24).  Bound: 1e-12 of the output scale (measured 0.0 on all four)."""
    from oracle import cases as C, vmg_oracle as O
    case = C.CASES[name]
    shapes, _ = C.load_fixture(os.path.join(GOLD, f"{name}.npz"))
    sd = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in C.case_state_dict(case, shapes).items()}
    ws = tuple(case["window_of"](""))
    heads = 4 if name == "swin_w2_t5" else 8
    x = case["inputs"]()["x"].double()
    B, D, H, W, Cc = x.shape
    shift = tuple(w // 2 for w in ws) if block == 1 else (0, 0, 0)
    Dp, Hp, Wp = -(-D // ws[0]) * ws[0], -(-H // 8) * 8, -(-W // 8) * 8
    p = f"blocks.{block}."
    want = O.swin_block(sd, p, x, O.shift_mask(Dp, Hp, Wp, ws, [w // 2 for w in ws]), heads, list(ws), list(shift))
    y = F.layer_norm(x, (Cc,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-5)
    q = F.linear(y, sd[p + "attn.q.weight"], sd[p + "attn.q.bias"])
    kv = F.linear(y, sd[p + "attn.kv.weight"], sd[p + "attn.kv.bias"])
    o, lse = WR.win3d_reference(q, kv, sd[p + "attn.q.bias"], sd[p + "attn.kv.bias"], sd[p + "attn.relative_position_bias_table"], heads, ws[0], shift)
    assert tuple(lse.shape) == (B * (Dp // ws[0]) * (Hp // 8) * (Wp // 8), heads, ws[0] * 64)
    h = x + F.linear(o, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    z = F.layer_norm(h, (Cc,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-5)
    got = h + F.linear(F.gelu(F.linear(z, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    err = float((got - want).abs().max())
    print(f"{name} block {block}: max |restatement - swin_block| = {err:.3e} at scale {float(want.abs().max()):.3e}")
    assert err <= 1e-12 * float(want.abs().max())


def test_lse_counts_the_unmasked_keys_when_every_logit_is_zero():
    """q = 0, bias-free, table = 0: every logit is the mask alone, so exp(lse) is the number of keys in the query's own region (an integer
    in 1 .. 64 for wt = 2), or, for a query all of whose keys lie in other regions, lse = -100 + log 64.  Both kinds occur."""
    g = WC.BY_ID["d4-wt2-D5-padeqshift"]  # (the last temporal window's two slices are regions 1 and 2 along D: no key of a query's own region)
    q, kv, _, _, table, _ = [None if t is None else t.double() for t in WC.make_inputs(g, torch.float32)]
    _, lse = WR.win3d_reference(torch.zeros_like(q), kv, None, None, torch.zeros_like(table), g.heads, g.wt, g.shift)
    assert tuple(lse.shape) == (2 * 3 * 1 * 2, g.heads, 128)
    lone = lse < -50.0
    assert lone.any() and not lone.all()
    assert float((lse[lone] - (-100.0 + torch.log(torch.tensor(64.0, dtype=torch.float64)))).abs().max()) <= 1e-9
    n = torch.exp(lse[~lone])
    assert float((n - n.round()).abs().max()) <= 1e-9 and float(n.min()) >= 1.0 - 1e-9 and float(n.max()) <= 64.0 + 1e-9


# ---------------------------------------------------------------------------------------------------- wrong variants of the reference
def _neg_roll(mp):
    orig = torch.roll
    mp.setattr(torch, "roll", lambda x, shifts, dims: orig(x, tuple(-s for s in shifts), dims))


def _boundary_off_by_one(mp):
    from oracle import vmg_oracle as O
    orig = O.shift_mask
    mp.setattr(O, "shift_mask", lambda D, H, W, ws, ss: orig(D, H, W, ws, [s + 1 if s else 0 for s in ss]))


def _mask_when_equal(mp):
    from oracle import vmg_oracle as O
    orig = O.shift_mask
    mp.setattr(O, "shift_mask", lambda *a: -100.0 - orig(*a))


def _rel_swapped(mp):
    from oracle import vmg_oracle as O
    orig = O.relative_position_index
    mp.setattr(O, "relative_position_index", lambda ws: orig(ws).t().contiguous())


def _own_slice_kept(mp):
    mp.setattr(WR, "other_slices", lambda i, wt: list(range(wt * 64)))


# name -> (patch or None, applies to geometry g)
MUTATIONS = {
    "pad_holds_zero": (None, lambda g: WC.padded(g) and g.biased),  # = the call with both biases null
    "roll_by_plus_shift": (_neg_roll, lambda g: any(g.shift)),
    "region_boundary_at_P_minus_shift_minus_1": (_boundary_off_by_one, lambda g: any(g.shift)),
    "mask_when_regions_equal": (_mask_when_equal, lambda g: any(g.shift)),
    "rel_index_query_key_swapped": (_rel_swapped, lambda g: True),
    "own_slice_not_excluded": (_own_slice_kept, lambda g: True),
}
CLASSES = sorted({g.cls for g in WC.GEOMS} - {"big"})
_right = {}


def _reference(g):
    if g.id not in _right:
        inp = WC.make_inputs(g, torch.bfloat16)
        _right[g.id] = (inp, WR.reference_all(*inp, g.heads, g.wt, g.shift))
    return _right[g.id]


def _visible(g, mutation, monkeypatch):
    """Does the wrong variant move out / dq / dkv / dtable / dbkv by more than the stated ceiling (2e-2 of the output's scale, 3e-2 of a
    gradient's: the loosest any comparison with a kernel may be, whatever its floor)?  lse is left out: the condition is the stricter for it."""
    inp, ref = _reference(g)
    q, kv, bq, bkv, table, dout = inp
    patch = MUTATIONS[mutation][0]
    with monkeypatch.context() as mp:
        if patch is None:
            bq = bkv = None
        else:
            patch(mp)
        bad = WR.reference_all(q, kv, bq, bkv, table, dout, g.heads, g.wt, g.shift)
    sc = WC.scales(ref)
    seen = {}
    for n in ("out", "dq", "dkv", "dtable", "dbkv"):
        if bad[n] is None or ref[n] is None:
            continue
        seen[n] = float((bad[n] - ref[n]).abs().max()) / sc[n][0]
    cap = WC.CAP[torch.bfloat16]
    return any(v > (cap["out"] if n == "out" else cap["grad"]) for n, v in seen.items()), seen


PAIRS = [(c, m) for c in CLASSES for m in MUTATIONS if any(MUTATIONS[m][1](g) for g in WC.GEOMS if g.cls == c)]


@pytest.mark.parametrize("cls,mutation", PAIRS, ids=[f"{c}-{m}" for c, m in PAIRS])
def test_every_class_of_geometry_shows_every_wrong_variant(cls, mutation, monkeypatch):
    """A class whose every member hides a mistake cannot catch it in a kernel either.  At least one geometry of the class must show it."""
    report = {}
    for g in (g for g in WC.GEOMS if g.cls == cls and MUTATIONS[mutation][1](g)):
        hit, seen = _visible(g, mutation, monkeypatch)
        report[g.id] = seen
        if hit:
            return
    pytest.fail(f"{mutation} is invisible on every geometry of class {cls}: {report}")


@pytest.mark.parametrize("gid", [g.id for g in WC.GEOMS if g.cls == "shiftpad"])
def test_padding_is_exposed_exactly_where_the_case_says(gid, monkeypatch):
    """WC.isolated (pad == shift in H / W, wt > 2): the roll leaves the padded rows alone in one mask slab, real queries see them at e^-100 and
    'a padded token holds the bias' cannot be told from 'holds zero' (every tensor moves by < 1e-6 of its scale; dbkv is ~0).  The other
    shifted + padded geometries are there because on each of them it can: the variant is visible, and dbkv is a real gradient, above the
    floor of its scale."""
    g = WC.BY_ID[gid]
    hit, seen = _visible(g, "pad_holds_zero", monkeypatch)
    _, ref = _reference(g)
    real_dbkv = float(ref["dbkv"].abs().max()) > 1e-3 * float(ref["dkv"].abs().max())
    if WC.isolated(g):
        assert not hit and max(seen.values()) < 1e-6 and not real_dbkv, seen
    else:
        assert hit and real_dbkv, seen


@pytest.mark.parametrize("gid", [g.id for g in WC.GEOMS if WC.padded(g) and g.biased and g.cls != "big"])
def test_no_gradient_reaches_the_q_bias(gid):
    """A padded query's output row is cropped away, so nothing flows back into q.bias through this operation: exactly zero."""
    _, ref = _reference(WC.BY_ID[gid])
    assert ref["dbq"] is not None and float(ref["dbq"].abs().max()) == 0.0


def test_the_matrix_holds_what_the_kernels_need():
    """Every row of the coverage table is present in the geometry list (the ids the GPU tests run are built from it)."""
    d = lambda g: g.C // g.heads
    on = lambda r: [g for g in WC.GEOMS if r in g.routes]
    assert {4, 8, 16, 18, 24, 28, 32} <= {d(g) for g in on("M")} and all(WC.mfma_expected(g, 1, torch.bfloat16) for g in on("M"))
    assert {36, 64} <= {d(g) for g in on("V")} and any(d(g) % 2 for g in on("V"))
    assert {18, 28, 36} <= {d(g) for g in on("F")}
    for r in "MV":
        assert {2, 4, 6, 8} <= {g.wt for g in on(r)}
    assert any((g.C, g.heads, g.wt, g.H, g.W) == (448, 16, 8, 8, 8) for g in on("M"))
    assert any((g.B, g.D, g.H, g.W, g.C, g.heads, g.wt) == (4, 8, 64, 64, 144, 8, 4) for g in on("M"))
    assert any(g.H % 8 not in (0, 4) and g.W % 8 not in (0, 4) and g.shift[1:] == (4, 4) for g in WC.GEOMS)
    assert any(g.wt == 4 and g.D in (5, 6) and g.shift[0] == 2 for g in WC.GEOMS)  # D padding 3 / 2 ... with D = 5: 3 != sd
    nw = lambda g: (-(-g.D // g.wt), -(-g.H // 8), -(-g.W // 8))
    assert any(g.B > 1 and min(nw(g)) > 1 and len(set(nw(g))) > 1 for g in WC.GEOMS)
    for s in [(0, 0, 0)] + [tuple(v if i == j else 0 for j in range(3)) for i, v in enumerate((1, 4, 4))]:
        assert any(tuple(bool(x) for x in g.shift) == tuple(bool(x) for x in s) for g in WC.GEOMS), s
    assert any(not g.biased and WC.padded(g) and any(g.shift) for g in WC.GEOMS)
    assert any(WC.isolated(g) for g in WC.GEOMS) and sum("padeqshift" in g.id for g in WC.GEOMS) >= 3  # the earlier pad == shift cases stay
