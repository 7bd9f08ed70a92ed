"""tests/traj_ref.py is what the trajectory kernels are compared with (tests/test_traj_ops_gpu.py), so it is pinned first, here, without a
GPU: against the oracle in float64 with autograd's gradients, the index choice bit for bit against float32 F.grid_sample on the very tie
and border cases the GPU file runs, and seven deliberately wrong variants of the reference, built by patching the function that holds the
convention, must each move some compared tensor of the GPU file's own case list by more than the loosest bound that file uses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import traj_cases as TC
from tests import traj_ref as TR

D = torch.float64


def _close(got, want, what):
    err, sc = float((got - want).abs().max()), float(want.abs().max())
    print(f"{what}: max |reference - oracle| = {err:.3e} at scale {sc:.3e}")
    assert err <= 1e-12 * sc, what


# ------------------------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("win", [(2, 2), (2, 4), (4, 2), (1, 8), (4, 4)], ids=lambda w: f"{w[0]}x{w[1]}")
def test_ltam_reference_equals_the_oracle_and_its_autograd(win):
    """O.ltam_wins in float64 with an identity projection and a zero anchor, gradients from autograd, on integer and clearly off-tie
    locations (whole pixels +- a quarter, a part of them outside the map): both precisions pick the same pixel there."""
    from oracle import vmg_oracle as O
    wh, ww = win
    n, t, h, w, c = 2, 3, 8, 16, 16
    gen = torch.Generator().manual_seed(7)
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
    _close(out, want.detach(), "out")
    dq, dk, dv, drpe = TR.ltam_reference_backward(q.detach(), kl, vl, loc, rpe.detach(), decay, wh, ww, scale, out, dout)
    _close(dq, wq, "dq")
    _close(torch.stack(dk, 1), wk, "dk")
    _close(torch.stack(dv, 1), wv, "dv")
    _close(drpe, wr, "drpe")
    # lse: the log of the sum the softmax divides by -- out * exp(lse) is the un-normalised P V, linear in the values
    out2, lse2 = TR.ltam_reference(q.detach(), kl, [2.0 * v for v in vl], loc, rpe.detach(), decay, wh, ww, scale)
    assert torch.equal(lse, lse2) and tuple(lse.shape) == (n, h, w, 4)
    # ... and a uniform shift of one head's table by s at decay 1 moves that head's lse by exactly s
    rp = rpe.detach().clone()
    rp[2] += 0.75
    _, lse3 = TR.ltam_reference(q.detach(), kl, vl, loc, rp, torch.ones(4), wh, ww, scale)
    _, lse4 = TR.ltam_reference(q.detach(), kl, vl, loc, rpe.detach(), torch.ones(4), wh, ww, scale)
    assert float((lse3 - lse4 - torch.tensor([0, 0, 0.75, 0], dtype=D)).abs().max()) <= 1e-12


def _dyadic_flow(n, h, w, seed):
    """Multiples of 1/8 up to +- 4 on a map whose size - 1 is a power of two: every float32 step of the coordinate chain is exact, so the
    float64 oracle samples the very same positions."""
    return torch.randint(-32, 33, (n, h, w, 2), generator=torch.Generator().manual_seed(seed)).float() / 8.0


@pytest.mark.parametrize("hw", [(9, 5), (1, 9), (5, 1), (2, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_warp_references_equal_the_oracle_and_its_autograd(hw):
    from oracle import vmg_oracle as O
    h, w = hw
    n, c = 2, 6
    gen = torch.Generator().manual_seed(17)
    x = torch.randn((n, h, w, c), generator=gen, dtype=D).requires_grad_(True)
    flow = _dyadic_flow(n, h, w, 18)
    dy = torch.randn((n, h, w, c), generator=gen, dtype=D)
    fl = flow.double().requires_grad_(True)
    want = O.flow_warp(x.permute(0, 3, 1, 2), fl, padding="border").permute(0, 2, 3, 1)
    wdx, wdf = torch.autograd.grad(want, (x, fl), dy)
    _close(TR.warp_bilinear_reference(x.detach(), flow), want.detach(), "out")
    dx, df, sc = TR.warp_bilinear_reference_backward(x.detach(), flow, dy, with_scales=True)
    _close(dx, wdx, "dx")
    _close(df, wdf, "dflow")
    assert bool((sc["dx"] >= dx.abs() - 1e-12).all()) and bool((sc["dflow"] >= df.abs() - 1e-12).all())
    off_tie = flow.clone()
    off_tie[(off_tie * 2 == (off_tie * 2).round()) & (off_tie != off_tie.round())] += 0.125
    loc = torch.randn((n, 4, h, w), generator=gen, dtype=D)
    assert torch.equal(TR.warp_nearest_reference(loc, off_tie), O.flow_warp(loc, off_tie.double(), mode="nearest", padding="border"))


def test_flow_smooth_reference_equals_the_torch_spelling_and_its_autograd():
    for (p, h, w, r) in [(2, 9, 7, 4), (1, 8, 8, 4), (3, 5, 5, 3), (1, 30, 26, 4)]:
        x = torch.randn((p, h, w), generator=torch.Generator().manual_seed(5), dtype=D).requires_grad_(True)
        hf, wf = -(-h // r) * r, -(-w // r) * r
        f = F.adaptive_avg_pool2d(F.pad(x[None], (0, wf - w, 0, hf - h), mode="reflect"), (hf // r, wf // r))
        want = F.interpolate(f, scale_factor=r, mode="nearest")[0, :, :h, :w]
        g = torch.randn((p, h, w), generator=torch.Generator().manual_seed(6), dtype=D)
        (wg,) = torch.autograd.grad(want, x, g)
        assert np.abs(TR.flow_smooth_reference(x.detach().numpy(), r) - want.detach().numpy()).max() <= 1e-14
        assert np.abs(TR.flow_smooth_reference_backward(g.numpy(), r) - wg.numpy()).max() <= 1e-14


# ------------------------------------------------------------------------------------------------------------------ index choice, bit for bit
def _grid32(pos_x, pos_y, h, w):
    """the oracle's normalisation, on float32 tensors"""
    gx = 2.0 * pos_x / max(w - 1, 1) - 1.0
    gy = 2.0 * pos_y / max(h - 1, 1) - 1.0
    return torch.stack((gx, gy), -1)


@pytest.mark.parametrize("g", TC.LTAM, ids=[g.id for g in TC.LTAM])
def test_gather_index_equals_float32_grid_sample_nearest_zeros(g):
    """A float64 oracle may pick another pixel at a tie or one ulp beside it; the operation is the float32 one."""
    loc = TC.ltam_locations(g)
    n, t, h, w = g.n, g.t, g.h, g.w
    idx = torch.from_numpy(TR.ltam_gather_index(loc.numpy(), h, w))
    number = (torch.arange(h * w, dtype=torch.float32) + 1.0).reshape(1, 1, h, w).expand(n * t, 1, h, w)  # 0 is what zeros padding returns
    l = loc.reshape(n * t, 2, h, w)
    got = F.grid_sample(number, _grid32(l[:, 0], l[:, 1], h, w), mode="nearest", padding_mode="zeros", align_corners=True)
    assert torch.equal(got.reshape(n, t, h, w).long() - 1, idx)
    if g.fam == "frac":  # the case holds what it is there for: exact ties towards both parities, and positions outside
        ix = TR.unnorm_coord(loc.numpy()[:, 0::2], w)
        tie = ix - np.floor(ix) == 0.5
        assert (tie & (np.floor(ix) % 2 == 0)).sum() > 8 and (tie & (np.floor(ix) % 2 == 1)).sum() > 8
    if g.fam in ("int", "frameout", "frac"):
        assert int((idx < 0).sum()) > 0
    if g.fam == "frameout":
        assert bool((idx[:, 0] < 0).all()) and bool((idx[:, 1:] >= 0).any())
    if g.fam == "onepixel":
        assert all(len(idx[:, j].unique()) == 1 for j in range(t))
    if g.fam == "winpixel":
        win = idx.reshape(n, t, h // g.wh, g.wh, w // g.ww, g.ww).permute(0, 1, 2, 4, 3, 5).reshape(n, t, -1, g.wh * g.ww)
        assert bool((win == win[..., :1]).all()) and len(idx.unique()) > 1


@pytest.mark.parametrize("g", TC.NEAREST, ids=[g.id for g in TC.NEAREST])
def test_location_advection_reference_equals_float32_grid_sample_nearest_border(g):
    loc, flow = TC.nearest_inputs(g)
    ys, xs = torch.meshgrid(torch.arange(g.h, dtype=torch.float32), torch.arange(g.w, dtype=torch.float32), indexing="ij")
    want = F.grid_sample(loc, _grid32(xs + flow[..., 0], ys + flow[..., 1], g.h, g.w), mode="nearest", padding_mode="border", align_corners=True)
    assert torch.equal(TR.warp_nearest_reference(loc, flow), want)


def test_half_offsets_of_the_advection_cases_hold_exact_ties():
    g = next(c for c in TC.NEAREST if c.fam == "half" and c.w == 9)
    _, flow = TC.nearest_inputs(g)
    ix, _, _, _ = TR.warp_coords(flow.numpy(), g.h, g.w)
    tie = (ix - np.floor(ix) == 0.5) & (ix > 0) & (ix < g.w - 1)
    assert (tie & (np.floor(ix) % 2 == 0)).any() and (tie & (np.floor(ix) % 2 == 1)).any()


@pytest.mark.parametrize("hw", TC.WARP_MAPS, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_zero_flow_round_trip_is_exact_where_size_minus_one_is_a_power_of_two(hw):
    """pixel -> normalised grid -> pixel in float32 returns every pixel when size - 1 is zero or a power of two; on the 7- and 24-wide maps
    some columns come back one ulp off (and blend in 2^-23 of a neighbour), yet at least a quarter of the pixels are exact.  The GPU file's
    zero-flow test asks for a bit-exact copy where the round trip is exact; this says where that is."""
    h, w = hw
    ix, iy, _, _ = TR.warp_coords(np.zeros((1, h, w, 2), dtype=np.float32), h, w)
    same = (ix == np.arange(w, dtype=np.float32)[None, None, :]) & (iy == np.arange(h, dtype=np.float32)[None, :, None])
    assert bool(same.all()) == (w != 7 and w != 24) and int(same.sum()) >= same.size // 4


# ------------------------------------------------------------------------------------------------------------------ wrong variants
def _decay_off_by_one(mp):
    mp.setattr(TR, "decay_powers", lambda decay, t: torch.stack([decay ** (t - j + 1) for j in range(t)], 1))


def _rpe_key_query(mp):
    mp.setattr(TR, "rpe_term", lambda rpe: rpe.transpose(1, 2))


def _round_half_up(mp):
    mp.setattr(TR, "round_index", lambda v: np.floor(v + np.float32(0.5)))


def _gather_pads_border(mp):
    mp.setattr(TR, "pad_index", lambda xn, yn, h, w: (np.clip(yn, 0, h - 1) * w + np.clip(xn, 0, w - 1)).astype(np.int64))


def _norm_per_head(mp):
    mp.setattr(TR, "norm_groups", lambda heads: heads)


def _border_keeps_grad(mp):
    mp.setattr(TR, "border_grad", lambda v, hi: np.ones(np.shape(v)))


def _weights_xy_swapped(mp):
    orig = TR.bilinear_weights
    mp.setattr(TR, "bilinear_weights", lambda tx, ty: orig(ty, tx))


LTAM_KINDS = ("out", "lse", "dq", "dk", "dv", "drpe")
LTAM_MUTATIONS = {
    "decay_power_off_by_one": (_decay_off_by_one, lambda g: True),
    "rpe_indexed_key_query": (_rpe_key_query, lambda g: g.wh * g.ww > 1),
    "round_half_up": (_round_half_up, lambda g: g.fam == "frac"),
    "gather_pads_with_the_border": (_gather_pads_border, lambda g: g.fam in ("int", "frameout", "frac")),
    "norm_per_head": (_norm_per_head, lambda g: True),
}
WARP_MUTATIONS = {
    "border_keeps_the_flow_gradient": (_border_keeps_grad, lambda g: g.fam in ("onborder", "clamped", "huge", "int", "random")),
    "weights_of_x_and_y_swapped": (_weights_xy_swapped, lambda g: g.fam in ("random", "half", "onborder", "clamped") and g.h > 1 and g.w > 1),
}


def _ltam_all(g, dtype):
    """the compared tensors of a case, computed afresh (under whatever patch is active), with the bf16 bounds of the right reference"""
    q, keys, vals, loc, rpe, decay, dout = TC.ltam_inputs(g, dtype)
    scale = (g.c // TC.HEADS) ** -0.5
    out, lse = TR.ltam_reference(q, keys, vals, loc, rpe, decay, g.wh, g.ww, scale)
    dq, dk, dv, drpe = TR.ltam_reference_backward(q, keys, vals, loc, rpe, decay, g.wh, g.ww, scale, TC.rnd(out, dtype), dout, lse=lse.float().double())
    return dict(out=out, lse=lse, dq=dq, dk=torch.stack(dk), dv=torch.stack(dv), drpe=drpe)


def _ltam_bounds(g, dtype):
    r = TC.ltam_reference(g, dtype)
    S = dict(out=r["vmax"], lse=r["lse"].abs().clamp_min(1.0), dq=float(r["dq"].abs().max()), dk=torch.stack(r["sc"]["dk"]), dv=torch.stack(r["sc"]["dv"]),
             drpe=r["sc"]["drpe"])
    ref = dict(out=r["out"], lse=r["lse"], dq=r["dq"], dk=torch.stack(r["dk"]), dv=torch.stack(r["dv"]), drpe=r["drpe"])
    return ref, {k: TC.bound(k, S[k], ref[k], dtype if k in TC.ROUNDED else torch.float32) for k in LTAM_KINDS}


@pytest.mark.parametrize("mutation", list(LTAM_MUTATIONS))
def test_every_wrong_attention_variant_shows_on_the_case_list(mutation, monkeypatch):
    """bf16 inputs and bf16 bounds: the loosest any comparison of the GPU file uses.  Every case the mistake applies to is tried until one shows it;
    it must show on at least one, by more than the bound, in at least one element of one compared tensor."""
    patch, applies = LTAM_MUTATIONS[mutation]
    report = {}
    for g in (g for g in TC.LTAM if applies(g)):
        ref, bounds = _ltam_bounds(g, torch.bfloat16)
        with monkeypatch.context() as mp:
            patch(mp)
            bad = _ltam_all(g, torch.bfloat16)
        report[g.id] = {k: float(((bad[k] - ref[k]).abs() - bounds[k]).max()) for k in LTAM_KINDS}
        if any(bool(((bad[k] - ref[k]).abs() > bounds[k]).any()) for k in LTAM_KINDS):
            return
    pytest.fail(f"{mutation} is invisible on every case: {report}")


@pytest.mark.parametrize("mutation", list(WARP_MUTATIONS))
def test_every_wrong_warp_variant_shows_on_the_case_list(mutation, monkeypatch):
    patch, applies = WARP_MUTATIONS[mutation]
    report = {}
    for g in (g for g in TC.WARP if applies(g)):
        r = TC.warp_reference(g)
        with monkeypatch.context() as mp:
            patch(mp)
            out = TR.warp_bilinear_reference(r["x"], r["flow"])
            dx, df = TR.warp_bilinear_reference_backward(r["x"], r["flow"], r["dy"])
        S = dict(wout=float(r["x"].abs().max()), dx=r["sc"]["dx"], dflow=r["sc"]["dflow"])
        ref, bad = dict(wout=r["out"], dx=r["dx"], dflow=r["dflow"]), dict(wout=out, dx=dx, dflow=df)
        over = {k: (bad[k] - ref[k]).abs() - TC.bound(k, S[k], ref[k], torch.bfloat16 if k in TC.ROUNDED else torch.float32) for k in ref}
        report[g.id] = {k: float(v.max()) for k, v in over.items()}
        if any(float(v.max()) > 0 for v in over.values()):
            return
    pytest.fail(f"{mutation} is invisible on every case: {report}")


def test_the_right_reference_is_inside_its_own_bounds_and_the_case_list_holds_what_the_kernels_need():
    """(the unpatched _ltam_all is the cached reference again: the variant tests compare like with like)"""
    g = TC.LTAM_BY_ID["8x8-c32-t2-int"]
    ref, _ = _ltam_bounds(g, torch.bfloat16)
    again = _ltam_all(g, torch.bfloat16)
    assert all(torch.equal(again[k], ref[k]) for k in LTAM_KINDS)
    assert {16, 32, 112, 144} == {c.c for c in TC.LTAM} and {1, 2, 7, 17, 32} == {c.t for c in TC.LTAM} and {1, 2} == {c.n for c in TC.LTAM}
    assert {(2, 2), (8, 8), (10, 12), (18, 6), (16, 8)} == {(c.h, c.w) for c in TC.LTAM}
    assert {(2, 2), (1, 1), (2, 4), (4, 2), (4, 4), (1, 8), (8, 1)} == {(c.wh, c.ww) for c in TC.LTAM}
    assert {"identity", "int", "frac", "frameout", "onepixel", "winpixel"} == {c.fam for c in TC.LTAM}
    assert any(c.c == 112 and (c.h % 8 or c.w % 8) for c in TC.LTAM) and any(c.c == 112 and c.n == 2 for c in TC.LTAM)
    ch = lambda dt: {c.c for c in TC.WARP if c.dtype == dt}
    assert ch(torch.bfloat16) == {8, 112, 128, 136, 144, 256, 264} and ch(torch.float32) == {4, 68, 132, 144}
    assert {(c.h, c.w) for c in TC.WARP} == set(TC.WARP_MAPS)
    assert {c.fam for c in TC.WARP} == {"random", "int", "half", "onborder", "huge", "clamped"}  # (zero flow: a test of its own, on every map)
    assert {c.k2 for c in TC.NEAREST} == {2, 64} and any(c.h == 1 for c in TC.NEAREST) and any(c.w == 1 and c.h > 1 for c in TC.NEAREST)
