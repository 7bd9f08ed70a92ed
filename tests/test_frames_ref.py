"""The numpy restatement of Tester.evaluate's conversions (tests/frames_ref.py) against the restatement the merged REDS path is pinned to
(tests/best_window_ref.py), and the host logic of vmg_amd.infer.index_generation.  No GPU."""
import numpy as np
import pytest
import torch

from tests import best_window_ref as BR
from tests import frames_ref as FR


@pytest.mark.parametrize("flags", FR.ALL_FLAGS)
def test_reds_branch_agrees_with_best_window_ref(flags):
    """On best_window_ref's own evaluation inputs, for all eight flag combinations: the same bytes, and the network sees the same calls."""
    from oracle import infer_oracle as IO
    ref = FR.reds_reference(flags)
    rec = BR.Recorder(IO.fake_sr_model())
    want = BR.evaluate_reds(rec, ref["lr"], ref["hr"], 3, 1, None, None, 4, *flags)
    assert ref["want"].dtype == np.uint8 and ref["want"].shape == want.shape == (5, 48, 64, 3)
    assert np.array_equal(ref["want"], want)
    assert len(rec.ins) == len(ref["rec"].ins) == 2
    assert all(torch.equal(a, b) for a, b in zip(rec.ins, ref["rec"].ins))


def test_conversions_are_the_references():
    u = FR.u8_frames(2, 5, 7, 1)
    for flags in FR.ALL_FLAGS:
        x = FR.to_clip(u, *flags)
        assert x.dtype == np.float32 and x.shape == ((1, 2, 3, 7, 5) if flags[2] else (1, 2, 3, 5, 7))
        assert np.array_equal(x, BR.augment(torch.from_numpy(BR.as_unit(u))[None], *flags).numpy())
        assert np.array_equal(FR.augment_frames(u, *flags), np.round(FR.to_clip(u, *flags)[0].transpose(0, 2, 3, 1) * 255).astype(np.uint8))
        twice = FR.augment_frames(FR.augment_frames(u, *flags), *flags)
        assert np.array_equal(twice, u) == (flags in FR.UNDONE)
        if flags not in FR.UNDONE:
            assert np.array_equal(twice, u[:, ::-1, ::-1])  # (rotated by 180 degrees)
        assert np.array_equal(FR.to_frames(FR.to_clip(u, *flags), *flags), twice)
    assert len(FR.UNDONE) == 6


def test_half_steps_are_ties():
    """All 255 values float32((k + 0.5) / 255) times 255.0f are exactly k + 0.5: rounding them is rounding half to even."""
    h = FR.half_steps()
    prod = h * np.float32(255.0)
    assert prod.dtype == np.float32 and int(np.count_nonzero(prod == np.arange(255, dtype=np.float32) + 0.5)) == 255
    got = FR.to_frames(np.broadcast_to(h[None, None, None, :], (1, 3, 1, 255)))
    k = np.arange(255)
    assert np.array_equal(got[0, 0, :, 0], np.where(k % 2 == 0, k, k + 1))


INDEX_LISTS = {
    (7, 7): [[0, 1, 2, 3, 4, 5, 6]],
    (7, 14): [[0, 1, 2, 3, 4, 5, 6], [6, 7, 8, 9, 10, 11, 12], [7, 8, 9, 10, 11, 12, 13]],
    (50, 100): [list(range(0, 50)), list(range(49, 99)), list(range(50, 100))],
    (100, 100): [list(range(100))],
    (5, 3): [[-2, -1, 0, 1, 2]],
}


@pytest.mark.parametrize("args", list(INDEX_LISTS))
def test_index_generation_literal_lists(args):
    from vmg_amd import infer
    assert infer.index_generation(*args) == INDEX_LISTS[args]
    assert FR.index_generation(*args) == INDEX_LISTS[args]
