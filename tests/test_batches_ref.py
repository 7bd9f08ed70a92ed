"""vmg_amd.batches.draw_plan (the host's draws) and tests/batches_ref.py (the numpy restatement of crop / flip / transpose / mirrors /
BGR -> RGB / CHW / 255) against what the reference's own REDSDataset / VimeoDataset returned (tests/golden/train_batches.npz, written by
tools/gen_batches_golden.py).  No GPU.

Every comparison is of bits (view(int32)): the feature moves bytes and divides by 255 with a correctly rounded quotient, so no tolerance
exists.  Per fixture case the plan is drawn from random.Random(seed) (and RandomState(pre_seed + 1) where the case has a pre_seed), as the
reference drew from random.seed(seed) and its numpy stream; a draw made in another order, skipped or added gives another crop of random
bytes, which the comparison cannot miss.
"""
import random

import numpy as np
import pytest

from tests import batches_ref as R

CASES = R.fixture()[0]["cases"]
NAMES = [c["name"] for c in CASES]


def plan_of(case):
    from vmg_amd import batches
    py, npr = R.case_rngs(case)
    return batches.draw_plan(case["indices"], case["cfg"], py, npr, dataset=case["dataset"])


@pytest.mark.parametrize("name", NAMES)
def test_drawn_plan_and_restatement_give_the_reference_batch(name):
    meta, z = R.fixture()
    case = CASES[NAMES.index(name)]
    plan = plan_of(case)
    LRs, HRs = R.batch(z["hr"], z["lr"], plan, meta["scale"])
    want_l, want_h = z[name + "/LRs"], z[name + "/HRs"]
    assert LRs.dtype == np.float32 and HRs.dtype == np.float32 and want_l.dtype == np.float32
    assert LRs.shape == want_l.shape and HRs.shape == want_h.shape
    assert np.array_equal(LRs.view(np.int32), want_l.view(np.int32))
    assert np.array_equal(HRs.view(np.int32), want_h.view(np.int32))
    T = case["cfg"]["num_frames"] * (2 if case["cfg"]["use_mirrors"] else 1)
    assert plan.frames.shape == (len(case["indices"]), T) and list(plan.clip) == case["indices"]
    if case["cfg"]["use_mirrors"]:
        assert np.array_equal(plan.frames, plan.frames[:, ::-1])


def test_fixture_coverage():
    """What the issue asks of the fixture: the 8 flag combinations, reverse on and off, mirrors on and off, each use_* flag disabled
    somewhere, REDS with and without pre_seed, Vimeo, and a crop larger than the frame in one axis with rot off."""
    meta, z = R.fixture()
    combos, reversed_seen = set(), set()
    for case in CASES:
        plan, cfg = plan_of(case), case["cfg"]
        for b in range(len(plan)):
            combos.add((bool(plan.hflip[b]), bool(plan.vflip[b]), bool(plan.rot[b])))
            if cfg["random_reverse"] and not cfg["use_mirrors"]:
                reversed_seen.add(bool(plan.frames[b, 0] > plan.frames[b, 1]))
        for flag, arr in (("use_hflip", plan.hflip), ("use_vflip", plan.vflip), ("use_rot", plan.rot)):
            assert cfg[flag] or not arr.any()
    assert len(combos) == 8 and reversed_seen == {False, True}
    cfgs = [(c["dataset"], c["cfg"]) for c in CASES]
    assert {c["use_mirrors"] for _, c in cfgs} == {False, True} and {c["random_reverse"] for _, c in cfgs} == {False, True}
    for flag in ("use_hflip", "use_vflip", "use_rot"):
        assert any(not c[flag] for _, c in cfgs), flag
    assert any(d == "REDS" and c["pre_seed"] is not None for d, c in cfgs) and any(d == "REDS" and c["pre_seed"] is None for d, c in cfgs)
    assert any(d == "Vimeo" for d, _ in cfgs)
    H, W = z["lr"].shape[2:4]
    big = [c for _, c in cfgs if c["crop_size"] // c["scale"] > min(H, W)]
    assert big and all(not c["use_rot"] for c in big)
    assert z["reds_big_crop/LRs"].shape[-2:] == (6, 8) and z["reds_big_crop/HRs"].shape[-2:] == (24, 32)
    assert z["hr"].dtype == np.uint8 and z["hr"].shape[2:] == (24, 40, 3) and z["lr"].shape[2:] == (6, 10, 3)


def test_a_flag_that_is_off_draws_nothing():
    """use_* false short-circuits the draw (data/REDS.py:126-128): the stream position after a sample depends on the flags."""
    from vmg_amd import batches
    cfg = dict(CASES[0]["cfg"])
    for off in ((), ("use_hflip",), ("use_vflip", "use_rot"), ("use_hflip", "use_vflip", "use_rot"), ("random_reverse",)):
        c = dict(cfg, **{k: False for k in off})
        py, twin = random.Random(5), random.Random(5)
        batches.draw_plan([0], c, py, dataset="REDS")
        twin.choice(list(range(c["total_num_frames"] - c["num_frames"] + 1)))
        if c["random_reverse"]:
            twin.random()
        twin.randint(0, 2), twin.randint(0, 6)
        for k in ("use_hflip", "use_vflip", "use_rot"):
            if c[k]:
                twin.random()
        assert py.random() == twin.random(), off


def test_pre_seed_draws_the_start_from_numpy_only():
    from vmg_amd import batches
    from vmg_amd.hip import HipError
    cfg = dict(CASES[0]["cfg"], pre_seed=7)
    with pytest.raises(HipError, match="np_random"):
        batches.draw_plan([0], cfg, random.Random(1))
    py, npr = random.Random(1), np.random.RandomState(8)
    plan = batches.draw_plan([0, 1], cfg, py, npr)
    twin = np.random.RandomState(8)
    starts = [int(twin.choice(list(range(4)), 1)[0]) for _ in range(2)]
    assert [int(min(f)) for f in plan.frames] == starts
    # Vimeo never touches numpy's stream
    before = npr.get_state()[1].copy()
    batches.draw_plan([0], dict(cfg, num_frames=5), py, npr, dataset="Vimeo")
    assert np.array_equal(before, npr.get_state()[1])
    with pytest.raises(HipError, match="dataset"):
        batches.draw_plan([0], cfg, py, npr, dataset="Vid4")
    with pytest.raises(HipError, match="use_rot"):
        batches.draw_plan([0], {k: v for k, v in cfg.items() if k != "use_rot"}, py, npr)


@pytest.mark.parametrize("flags", [(h, v, r) for h in (0, 1) for v in (0, 1) for r in (0, 1)])
def test_restatement_obeys_the_index_mapping(flags):
    """Output (r, c) reads crop (i, j) = (c, r) if rot else (r, c); source row y0 + (vflip ? ch-1-i : i), column x0 + (hflip ? cw-1-j : j);
    channel k reads 2 - k of a BGR store: written out with loops, against the slicing of tests/batches_ref.py."""
    hf, vf, rot = flags
    rng = np.random.default_rng(3)
    lr, hr = rng.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8), rng.integers(0, 256, (2, 18, 22, 3), dtype=np.uint8)
    y0, x0, c, s = 3, 5, 5, 2
    L, Hh = R.sample(hr, lr, [1, 0], y0, x0, hf, vf, rot, c, s, as_bytes=True)
    for out, src, m in ((L, lr, 1), (Hh, hr, s)):
        n = m * c
        assert out.shape == (2, 3, n, n)
        for t, f in enumerate([1, 0]):
            for k in range(3):
                for r in range(n):
                    for col in range(n):
                        i, j = (col, r) if rot else (r, col)
                        assert out[t, k, r, col] == src[f, m * y0 + (n - 1 - i if vf else i), m * x0 + (n - 1 - j if hf else j), 2 - k]
