"""Host side of the long-clip support, without a GPU: the route rule of the trajectory attention, and the float64 reference of
tests/traj_ref.py pinned BEYOND 32 key-frames -- on the shapes of tests/long_clip_cases.py -- against oracle.vmg_oracle.ltam_wins and its
autograd, by the method of tests/test_traj_ref.py::test_ltam_reference_equals_the_oracle_and_its_autograd."""
import pytest
import torch

from tests import long_clip_cases as LC
from tests import traj_cases as TC
from tests import traj_ref as TR

D = torch.float64


def test_ltam_route_switches_after_32_key_frames():
    from vmg_amd import functional as FH
    assert FH.ltam_route(1) == "args" and FH.ltam_route(32) == "args"
    assert FH.ltam_route(33) == "table" and FH.ltam_route(100) == "table"
    assert FH.ltam_route(17) == "args"  # (the longest shipped shape: cfg4, ceil(50 / 3))


def _close(got, want, what):
    err, sc = float((got - want).abs().max()), float(want.abs().max())
    print(f"{what}: max |reference - oracle| = {err:.3e} at scale {sc:.3e}")
    assert err <= 1e-12 * sc, what


@pytest.mark.parametrize("g", LC.LTAM_LONG, ids=[g.id for g in LC.LTAM_LONG])
def test_ltam_reference_beyond_32_key_frames_equals_the_oracle_and_its_autograd(g):
    """O.ltam_wins in float64 with an identity projection and a zero anchor, gradients from autograd, on integer and clearly off-tie locations
    (whole pixels +- a quarter, a part of them outside the map): both precisions pick the same pixel there."""
    from oracle import vmg_oracle as O
    n, t, h, w, c, wh, ww = g.n, g.t, g.h, g.w, g.c, g.wh, g.ww
    gen = torch.Generator().manual_seed(70 + t)
    mk = lambda *s: torch.randn(s, generator=gen, dtype=D)
    q = mk(n, h, w, c).requires_grad_(True)
    keys, vals = mk(n, t, h, w, c).requires_grad_(True), mk(n, t, h, w, c).requires_grad_(True)
    rpe = (0.5 * mk(4, wh * ww, wh * ww)).requires_grad_(True)
    decay = torch.tensor([0.9, 0.95, 0.98, 0.999], dtype=torch.float32)
    loc = TC.ltam_locations(TC.Ltam("x", n, h, w, c, wh, ww, t, "int"), seed=8) + 0.25 * torch.randint(-1, 2, (n, 2 * t, h, w), generator=gen).float()
    dout = mk(n, h, w, c)
    sd = {"proj.weight": torch.eye(c, dtype=D), "proj.bias": torch.zeros(c, dtype=D), "relative_pos_encoding": rpe, "decay_v": decay.double()}
    want = O.ltam_wins(sd, "", q, keys, torch.zeros_like(q), vals, loc.double(), 4, (wh, ww))
    wq, wk, wv, wr = torch.autograd.grad(want, (q, keys, vals, rpe), dout)
    kl, vl = [keys.detach()[:, j] for j in range(t)], [vals.detach()[:, j] for j in range(t)]
    scale = (c // 4) ** -0.5
    out, lse = TR.ltam_reference(q.detach(), kl, vl, loc, rpe.detach(), decay, wh, ww, scale)
    assert tuple(lse.shape) == (n, h, w, 4) and bool(torch.isfinite(lse).all())
    _close(out, want.detach(), "out")
    dq, dk, dv, drpe = TR.ltam_reference_backward(q.detach(), kl, vl, loc, rpe.detach(), decay, wh, ww, scale, out, dout)
    _close(dq, wq, "dq")
    _close(torch.stack(dk, 1), wk, "dk")
    _close(torch.stack(dv, 1), wv, "dv")
    _close(drpe, wr, "drpe")


def test_the_long_case_list_holds_what_the_table_route_needs():
    """Every instantiated head dimension, the first key-frame count past the argument route, one past two fill launches (t > 64), a window other than
    2 x 2, two images, a map that is no multiple of the tile -- and bounds that grow with t / 32 only."""
    assert {g.c // TC.HEADS for g in LC.LTAM_LONG} == {4, 8, 28, 36}
    assert min(g.t for g in LC.LTAM_LONG) == 33 and max(g.t for g in LC.LTAM_LONG) > 64 and all(g.t > 32 for g in LC.LTAM_LONG)
    assert any((g.wh, g.ww) != (2, 2) for g in LC.LTAM_LONG) and any(g.n == 2 for g in LC.LTAM_LONG) and any(g.h % 8 or g.w % 8 for g in LC.LTAM_LONG)
    assert all(LC.factor(g) == g.t / 32.0 for g in LC.LTAM_LONG)
    assert all(TC.LTAM_BY_ID[i].t <= 32 for i in LC.ROUTE_EQUALITY)
    # the module shapes cross the limits they are there for: more than 32 key-frames attended to / more than 64 steps
    kf = [LC.key_frames(T, s) for (_, T, _, _, s) in LC.MODULE_SHAPES]
    assert kf == [34, 34, 22] and all(T > 64 for (_, T, _, _, _) in LC.MODULE_SHAPES)
