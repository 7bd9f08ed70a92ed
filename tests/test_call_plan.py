"""Host logic of the call-index feature (no GPU): infer.plan_calls against the visiting order of the oracle's restatement of
tools/Tester.py, infer.shard_ranges, and the bookkeeping of VMG.forward_calls / advance_calls / set_forward_calls."""
import pytest
import torch


def _coordinate_clip(T, H, W):
    """(1, T, 3, H, W) whose channels hold the frame, row and column index of every pixel: a crop tells where it was taken."""
    x = torch.zeros(1, T, 3, H, W)
    x[:, :, 0] = torch.arange(T, dtype=torch.float32)[None, :, None, None]
    x[:, :, 1] = torch.arange(H, dtype=torch.float32)[None, None, :, None]
    x[:, :, 2] = torch.arange(W, dtype=torch.float32)[None, None, None, :]
    return x


def _visits(x, nf, of, spatial, ov):
    """(t, h, w, frames, rows, columns) of every network call IO.test_clips makes, in its order."""
    from oracle import infer_oracle as IO
    inner, seen = IO.fake_sr_model(scale=1), []

    def model(clip):
        seen.append((int(clip[0, 0, 0, 0, 0]), int(clip[0, 0, 1, 0, 0]), int(clip[0, 0, 2, 0, 0]), *(int(v) for v in clip.shape[1:2] + clip.shape[3:])))
        return inner(clip)

    IO.test_clips(model, x, nf, of, spatial, ov, 1)
    return seen


GRID = [(11, 5, 2, [16, 16], 4, 24, 28), (11, 5, 3, None, None, 24, 28), (11, 4, 0, [16, 16], 4, 24, 28), (3, 5, 2, None, None, 24, 28),
        (9, 3, 1, None, None, 24, 28), (5, 3, 1, [64, 64], 8, 72, 64)]


@pytest.mark.parametrize("T,nf,of,spatial,ov,H,W", GRID + [(100, 50, 25, [128, 128], 20, 180, 320)])
def test_plan_calls_is_the_oracles_visiting_order(T, nf, of, spatial, ov, H, W):
    from vmg_amd import infer
    x = _coordinate_clip(T, H, W)
    nf = min(nf, T)
    want = _visits(x, nf, of, spatial, ov)
    plan = infer.plan_calls(T, H, W, nf, of, spatial, ov)
    assert len(plan) == len(want)
    for i, (c, v) in enumerate(zip(plan, want)):
        assert c.index == i + 1
        assert (c.origin is None) == (ov is None)
        crop = plan.crop(x, c)
        assert (c.t, *(c.origin or (0, 0)), *(int(s) for s in crop.shape[1:2] + crop.shape[3:])) == v, f"call {i + 1}"
        assert torch.equal(crop[0, 0, :, 0, 0], torch.tensor([float(v[0]), float(v[1]), float(v[2])]))
    if T == 100:
        assert len(plan) == 18 and [c.t for c in plan][::6] == [0, 25, 50]
        assert [c.origin for c in plan[:6]] == [(0, 0), (0, 108), (0, 192), (52, 0), (52, 108), (52, 192)]


def test_shard_ranges_are_a_balanced_contiguous_partition():
    from vmg_amd import infer
    for n in range(1, 41):
        for world in range(1, 9):
            rs = infer.shard_ranges(n, world)
            assert len(rs) == world and all(r.step == 1 for r in rs)
            flat = [p for r in rs for p in r]
            assert flat == list(range(1, n + 1))  # contiguous, disjoint, in rank order, covering the plan
            lens = [len(r) for r in rs]
            assert max(lens) - min(lens) <= 1
            assert len(rs[0]) >= 1  # rank 0 announces the tile shape: it never goes without a call
    assert [list(r) for r in infer.shard_ranges(18, 4)] == [[1, 2, 3, 4, 5], [6, 7, 8, 9, 10], [11, 12, 13, 14], [15, 16, 17, 18]]


def test_run_calls_wants_a_contiguous_run_of_the_plan():
    from vmg_amd import infer
    plan = infer.plan_calls(11, 24, 28, 5, 2, [16, 16], 4)
    assert [c.index for c in infer._entries(plan, range(3, 6))] == [3, 4, 5] and infer._entries(plan, plan[2:5]) == plan[2:5]
    with pytest.raises(ValueError):
        infer._entries(plan, [1, 3])
    with pytest.raises(ValueError):
        infer._entries(plan, [2, 1])
    with pytest.raises(ValueError):
        infer._entries(plan, [infer.PlannedCall(1, 99, None)])  # an entry of some other plan


def test_call_counter_bookkeeping_on_the_host():
    """forward_calls is a plain attribute (the 560 state-dict keys stay the reference's), advance_calls / set_forward_calls refuse to go
    back, load_state_dict starts the count again; on host tensors the n-fold decay is n in-place multiplies."""
    from oracle import cases as C
    from tests.util import build_product
    m = build_product(C.CASES["vmg_tiny_few"]["cfg"], device=None).eval()
    keys = list(m.state_dict().keys())
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.forward_calls == 0
    with pytest.raises(AttributeError):
        m.forward_calls = 3  # read-only
    m.advance_calls(0)
    assert m.forward_calls == 0
    m.advance_calls(2)
    m.set_forward_calls(3)
    assert m.forward_calls == 3
    names = [k for k in keys if k.endswith("mlp_h.0.weight") or k.endswith("mlp_w.0.weight")]
    assert names
    for k in names:
        want = sd[k].clone()
        for _ in range(3):
            want.mul_(sd[k.replace("mlp_h.0.weight", "gamma_h").replace("mlp_w.0.weight", "gamma_w")])
        assert torch.equal(m.state_dict()[k], want), k
    with pytest.raises(ValueError):
        m.advance_calls(-1)
    with pytest.raises(ValueError):
        m.set_forward_calls(2)
    assert m.forward_calls == 3 and list(m.state_dict().keys()) == keys
    m.load_state_dict(sd)
    assert m.forward_calls == 0 and list(m.state_dict().keys()) == keys
