"""tests/ltam_max_ref.py (the float64 restatement of hard trajectory attention, traj_mode 'max') pinned without a GPU:
against the reference's own numbers (tests/golden/ltam_max.npz, written by tools/gen_ltam_max_golden.py from LTAM_multi_head(mode='max') and its
autograd), against autograd of its own forward in float64, and on the two properties a kernel gets wrong most easily -- the FIRST maximum wins an
exact tie, and the key gradient of a selected row is DENSE over all c channels although only one head's slice of dkn is non-zero.  Also asserts
the condition the GPU index test rests on: at most 1 % of the (pixel, head) pairs of any case have two key-frames within TAU of the maximum."""
import json
import os

import numpy as np
import pytest
import torch

from tests import ltam_max_cases as MC
from tests import ltam_max_ref as MR
from tests import traj_cases as TC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ltam_max.npz")
DTYPES = [torch.float32, torch.bfloat16]
_dn = lambda dt: "bf16" if dt == torch.bfloat16 else "fp32"


def fixture():
    z = np.load(GOLD)
    return z, json.loads(str(z["meta"]))


def fixture_ltam_inputs(g):
    """The seeded inputs of a recorded LTAM case (tools/gen_ltam_max_golden.py ltam_inputs)."""
    from oracle import cases as C
    from oracle import recipe as R
    n, t, h, w, c, s = g["n"], g["t"], g["h"], g["w"], g["c"], g["seed"]
    return dict(q=R.seeded((n, h, w, c), s), keys=R.seeded((n, t, h, w, c), s + 1), anchor=R.seeded((n, h, w, c), s + 2),
                vals=R.seeded((n, t, h, w, c), s + 3), loc=C.int_locations(n, t, h, w, s + 4), dout=R.seeded((n, h, w, c), s + 5))


def compare_recorded(z, name, got, whole, tol):
    from oracle import cases as C
    got = got.float()
    if whole:
        want = torch.from_numpy(z[name])
        scale = max(1.0, float(want.abs().max()))
        err = float((got.reshape(want.shape) - want).abs().max())
        assert err <= tol * scale, f"{name}: {err} (scale {scale})"
        return
    sub, sums, shape = z[name + "/sub"], z[name + "/sums"], tuple(z[name + "/shape"])
    assert tuple(got.shape) == shape, name
    scale = max(1.0, float(np.abs(sub).max()))
    err = float(np.abs(C.subsample(got) - sub).max())
    assert err <= tol * scale, f"{name}: {err} (scale {scale})"
    mine = C.checksums(got)
    assert abs(mine[0] - sums[0]) <= tol * sums[1] and abs(mine[1] - sums[1]) <= tol * sums[1], f"{name}: checksums {mine} vs {tuple(sums)}"


def test_restatement_reproduces_the_reference_module_forward_and_gradients():
    """(a): proj(attention) + anchor and its gradients w.r.t. q, keys, vals and anchor, to fp32 round-off of the recorded numbers (1e-5 of each tensor's
    scale: the reference ran in fp32 -- a c-term norm, a D-term score, a c-term projection)."""
    from oracle import recipe as R
    z, meta = fixture()
    for g in meta["ltam"]:
        inp = fixture_ltam_inputs(g)
        c, t = g["c"], g["t"]
        sd = R.recipe_state_dict({"proj.weight": [c, c], "proj.bias": [c]}, 0)
        W, b = sd["proj.weight"].double(), sd["proj.bias"].double()
        keys, vals = list(inp["keys"].unbind(1)), list(inp["vals"].unbind(1))
        att, idx, _, _ = MR.forward(inp["q"], keys, vals, inp["loc"])
        out = att @ W.t() + b + inp["anchor"].double()
        datt = inp["dout"].double() @ W
        dq, dk, dv = MR.backward(inp["q"], keys, vals, inp["loc"], idx, datt)
        compare_recorded(z, g["name"] + "/out", out, g["whole"], 1e-5)
        compare_recorded(z, g["name"] + "/dq", dq, g["whole"], 1e-5)
        compare_recorded(z, g["name"] + "/dkeys", torch.stack(dk, 1), g["whole"], 1e-5)
        compare_recorded(z, g["name"] + "/dvals", torch.stack(dv, 1), g["whole"], 1e-5)
        compare_recorded(z, g["name"] + "/danchor", inp["dout"].double(), g["whole"], 1e-5)
        assert int((TC.TR.ltam_gather_index(inp["loc"].numpy(), g["h"], g["w"]) < 0).sum()) > 0  # out-of-range locations are in the case


@pytest.mark.parametrize("gid,zero_rows", [("8x8-c32-t2-int", False), ("8x8-c32-t2-int", True), ("3x5-c32-t4-frac", False), ("10x12-c32-t3-dup", False),
                                           ("18x6-c144-t2-oneframe-out", False)])
def test_backward_equals_autograd_of_the_forward(gid, zero_rows):
    """float64 on both sides.  zero-rows: a zero query row and a zero key source row meet F.normalize's 1e-12 clamp; the restatement's backward must
    treat them as autograd does (factor 1 / eps, no projection)."""
    g = MC.BY_ID[gid]
    q, keys, vals, loc, dout = MC.inputs(g, torch.float32)
    if zero_rows:
        q[0, 1, 2] = 0
        keys[0][0, 3, 1] = 0
        loc[0, 0, 0, :4] = 1.0
        loc[0, 1, 0, :4] = 3.0
    leaves = [t.clone().requires_grad_(True) for t in [q] + keys + vals]
    out_t, idx_t = MR.torch_forward(leaves[0], leaves[1:1 + g.t], leaves[1 + g.t:], loc)
    out, idx, score, table = MR.forward(q, keys, vals, loc)
    assert torch.equal(idx_t, idx)
    assert float((out_t.detach() - out).abs().max()) <= 1e-12 * max(1.0, float(out.abs().max()))
    out_t.backward(dout)
    dq, dk, dv = MR.backward(q, keys, vals, loc, idx, dout)
    for got, leaf, nm in zip([dq] + dk + dv, leaves, ["dq"] + [f"dk{j}" for j in range(g.t)] + [f"dv{j}" for j in range(g.t)]):
        want = leaf.grad if leaf.grad is not None else torch.zeros_like(got)
        assert float((got - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max())), nm
    if zero_rows:
        assert float(dk[0][0, 3, 1].abs().max()) > 1e9  # the clamp's factor really is in the zero key row (some head selected it)


def test_first_maximum_wins_an_exact_tie():
    """Key-frame 1 duplicates key-frame 0 with other values: the scores tie exactly, the EARLIER frame is selected and its value comes out."""
    g = MC.BY_ID["10x12-c32-t3-dup"]
    q, keys, vals, loc, _ = MC.inputs(g, torch.float32)
    assert torch.equal(keys[0], keys[1]) and not torch.equal(vals[0], vals[1])
    out, idx, score, table = MR.forward(q, keys, vals, loc)
    assert torch.equal(table[:, :, :, 0], table[:, :, :, 1])
    assert not (idx == 1).any() and (idx == 0).any() and (idx == 2).any()
    D = g.c // MC.HEADS
    want0 = (score[..., None] * vals[0].reshape(g.n, g.h, g.w, MC.HEADS, D)).reshape(out.shape)
    sel0 = (idx == 0)[..., None].expand(g.n, g.h, g.w, MC.HEADS, D).reshape(out.shape)
    assert torch.equal(out[sel0], want0[sel0])
    # torch.max, the reference's operation, keeps the first maximum too
    assert torch.equal(torch.max(table, dim=3).indices, idx)
    # out-of-range key-frames all score exactly 0: among them the first wins as well
    g2 = MC.BY_ID["18x6-c144-t2-oneframe-out"]
    q, keys, vals, loc, _ = MC.inputs(g2, torch.float32)
    _, idx2, score2, table2 = MR.forward(q, keys, vals, loc)
    assert (table2[:, :, :, 0] == 0).all() and ((idx2 == 0) == (table2[:, :, :, 1] <= 0)).all()


def test_key_gradient_row_is_dense_over_all_channels():
    """One head alone selects key-frame 1 (idx= override): the row it adds to that frame's key gradient is non-zero in the OTHER heads' channels too
    (the normalisation runs over all c channels), and equals autograd's through a forward with the same forced selection."""
    g = MC.BY_ID["1x1-c16-t3-identity"]
    q, keys, vals, loc, dout = MC.inputs(g, torch.float32)
    idx = torch.tensor([1, 0, 0, 0]).reshape(1, 1, 1, 4)
    dq, dk, dv = MR.backward(q, keys, vals, loc, idx, dout)
    D = g.c // MC.HEADS
    row = dk[1][0, 0, 0]
    assert (row[:D] != 0).all() and (row[D:] != 0).all()
    assert (dv[1][0, 0, 0, :D] != 0).all() and (dv[1][0, 0, 0, D:] == 0).all()
    assert (dk[2] == 0).all() and (dv[2] == 0).all()
    # autograd of the same selection, spelled directly
    kl = [k.clone().requires_grad_(True) for k in keys]
    qn = q[0, 0, 0] / q[0, 0, 0].norm()
    outs = []
    for hd in range(4):
        j = int(idx[0, 0, 0, hd])
        kn = kl[j][0, 0, 0] / kl[j][0, 0, 0].norm()
        outs.append((qn[hd * D:hd * D + D] * kn[hd * D:hd * D + D]).sum() * vals[j][0, 0, 0, hd * D:hd * D + D])
    torch.cat(outs).backward(dout[0, 0, 0])
    for j in range(3):
        want = kl[j].grad if kl[j].grad is not None else torch.zeros_like(dk[j])
        assert float((dk[j] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_case_list_is_what_the_gpu_tests_expect():
    ids = [g.id for g in MC.CASES]
    assert len(set(ids)) == len(ids) and all(g in MC.CASES for g in TC.LTAM)
    assert {MC.route(g) for g in MC.CASES} == {"args", "table"} and MC.BY_ID[MC.BOTH_ROUTES].t == 17
    assert any(g.h == 1 and g.w == 1 for g in MC.CASES) and any(g.h % 8 and g.w % 8 for g in MC.CASES)
    assert {g.c // MC.HEADS for g in MC.CASES} == {4, 8, 28, 36}


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("g", MC.CASES, ids=[g.id for g in MC.CASES])
def test_near_ties_are_rare_in_every_case(g, dtype):
    """The condition of the GPU index test: (pixel, head) pairs with a second key-frame strictly within TAU of the maximum are at most 1 % of a case."""
    r = MC.reference(g, dtype)
    near = MC.near_ties(r["table"])
    share = float(near.double().mean())
    print(f"NEAR-TIES {g.id} {_dn(dtype)} {int(near.sum())} of {near.numel()} ({100 * share:.3f} %)")
    assert share <= MC.NEAR_TIE_CAP
    assert bool(MC.allowed(r["table"]).gather(3, r["idx"][:, :, :, None, :]).all())
