"""tests/best_window_ref.py (the numpy restatement the GPU tests of vmg_amd.infer.best_window_clips compare with) against the oracle's
test_clips_max and the reference's own fixture -- CPU only.  Also checks that no test input sits on a tie: the device's float64 log10 may
differ from numpy's in the last bit, which can matter only where two float32 scores of one frame coincide or are adjacent."""
import os

import numpy as np
import pytest
import torch

from tests import best_window_ref as BR

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _restated(ref):
    T, nf = ref["x"].shape[1], ref["nf"]
    ts = BR.tile_starts(T, nf, ref["of"])
    outs = BR.window_outputs(ref)
    errs = BR.window_errs(outs, ts, ref["hr"][0].numpy())
    return T, nf, ts, outs, errs


@pytest.mark.parametrize("name", list(BR.CLIP_CASES))
def test_restatement_equals_the_oracle_bit_for_bit(name):
    ref = BR.clip_reference(name)
    T, nf, ts, outs, errs = _restated(ref)
    table = BR.score_table(errs, ts, T)
    frames = BR.gather(outs, ts, BR.select_table(table), T)
    assert frames.dtype == np.float32 and np.array_equal(frames, ref["want"].numpy())


def test_restatement_agrees_with_the_reference_fixture():
    from oracle import cases as C
    ref = BR.clip_reference("fixture")
    T, nf, ts, outs, errs = _restated(ref)
    frames, _, _ = BR.select_streaming(outs, errs, ts, T)
    _, gold = C.load_fixture(os.path.join(GOLD, "infer_clips_max.npz"))
    assert tuple(frames.shape) == gold[0]["shape"]
    assert float(np.abs(C.subsample(torch.from_numpy(frames)) - gold[0]["sub"]).max()) <= 1e-6


@pytest.mark.parametrize("name", list(BR.CLIP_CASES))
def test_streaming_rule_equals_table_then_argmax(name):
    ref = BR.clip_reference(name)
    T, nf, ts, outs, errs = _restated(ref)
    table = BR.score_table(errs, ts, T)
    choice = BR.select_table(table)
    frames, best, choice_s = BR.select_streaming(outs, errs, ts, T)
    assert np.array_equal(choice_s, choice)
    assert np.array_equal(best, table.max(axis=1))
    assert np.array_equal(frames, BR.gather(outs, ts, choice, T))


def test_streaming_rule_on_uncovered_frames_and_zero_scores():
    """Constructed: a frame that window 0 does not cover and whose only score is 0 (err == 1) stays zero with choice 0; an exact match scores the cap."""
    outs = [np.full((2, 1, 2, 2), 0.25, np.float32), np.full((2, 1, 2, 2), 0.75, np.float32)]
    ts, T = [0, 1], 3
    errs = [np.array([0.01, 0.0]), np.array([0.0, 1.0])]
    table = BR.score_table(errs, ts, T)
    assert table[1, 0] == np.float32(BR.CAP) and table[1, 1] == np.float32(BR.CAP) and table[2, 1] == 0 and table[2, 0] == 0
    frames, best, choice = BR.select_streaming(outs, errs, ts, T)
    assert np.array_equal(choice, BR.select_table(table)) and list(choice) == [0, 0, 0]
    assert np.array_equal(frames, BR.gather(outs, ts, choice, T)) and not frames[2].any() and float(best[2]) == 0.0


@pytest.mark.parametrize("name", list(BR.CLIP_CASES))
def test_inputs_do_not_sit_on_a_tie(name):
    ref = BR.clip_reference(name)
    T, nf, ts, outs, errs = _restated(ref)
    gap = BR.tie_gap(BR.score_table(errs, ts, T), ts, nf)
    print(f"{name}: smallest gap between the best and second-best covered score = {gap:.4f} dB")
    assert gap >= BR.TIE_GAP_DB


def test_uint8_hr_inputs_do_not_sit_on_a_tie():
    ref = BR.clip_reference("t7_w3_o1")
    T, nf, ts, outs, _ = _restated(ref)
    gap = BR.tie_gap(BR.score_table(BR.window_errs(outs, ts, BR.u8_hr_of("t7_w3_o1")), ts, T), ts, nf)
    print(f"t7_w3_o1 against uint8 HR: smallest gap = {gap:.4f} dB")
    assert gap >= BR.TIE_GAP_DB


@pytest.mark.parametrize("flags", BR.EVAL_FLAGS)
def test_evaluate_inputs_do_not_sit_on_a_tie(flags):
    ref = BR.eval_reference(flags)
    ts = BR.tile_starts(5, 3, 1)
    outs = [o[0].numpy() for o in ref["rec"].outs]
    hr = BR.augment(torch.from_numpy(BR.as_unit(ref["hr"])), *flags).numpy() if any(flags) else BR.as_unit(ref["hr"])
    gap = BR.tie_gap(BR.score_table(BR.window_errs(outs, ts, hr), ts, 5), ts, 3)
    print(f"evaluate {flags}: smallest gap = {gap:.4f} dB")
    assert gap >= BR.TIE_GAP_DB


def test_wrong_rules_are_told_apart():
    """`>=` in place of `>`, and selection on float64 scores without the float32 rounding, each change the result on a constructed input."""
    a, b = np.full((1, 1, 2, 2), 0.25, np.float32), np.full((1, 1, 2, 2), 0.75, np.float32)
    outs, ts, T = [a, b], [0, 0], 1
    # equal scores: the first window keeps the frame
    errs = [np.array([0.01]), np.array([0.01])]
    right, _, c_right = BR.select_streaming(outs, errs, ts, T)
    wrong, _, c_wrong = BR.select_streaming(outs, errs, ts, T, strict=False)
    assert list(c_right) == [0] == list(BR.select_table(BR.score_table(errs, ts, T))) and list(c_wrong) == [1]
    assert np.array_equal(right[0], a[0]) and np.array_equal(wrong[0], b[0])
    # scores that differ in float64 and coincide in float32: the float32 table sees a tie, the first window keeps the frame
    e1 = 0.01
    e2 = e1 * (1 - 1e-9)
    assert BR.score(e2, np.float64) > BR.score(e1, np.float64) and BR.score(e2) == BR.score(e1)
    errs = [np.array([e1]), np.array([e2])]
    _, _, c32 = BR.select_streaming(outs, errs, ts, T)
    _, _, c64 = BR.select_streaming(outs, errs, ts, T, dtype=np.float64)
    assert list(c32) == [0] == list(BR.select_table(BR.score_table(errs, ts, T))) and list(c64) == [1]


def test_frame_err_forms():
    """uint8 HR is read as astype(float32) / 255 (not a multiply by a reciprocal), values outside [0, 1] are clamped in float32."""
    g = np.random.default_rng(7)
    hr8 = g.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    out = (g.standard_normal((3, 5, 7)) * 0.6 + 0.5).astype(np.float32)
    unit = BR.as_unit(hr8)
    assert BR.frame_err(out, hr8) == BR.frame_err(out, unit)
    assert BR.frame_err(unit, hr8) == 0.0
    assert np.any(unit != np.moveaxis(hr8.astype(np.float32) * np.float32(1 / 255.), -1, 0))  # the two roundings do differ for some bytes
    want = np.mean((np.clip(out, 0, 1).astype(np.float64) - unit.astype(np.float64)) ** 2)
    assert BR.frame_err(out, hr8) == float(want)


def test_augment_applied_twice():
    """Tester.augment_inverse is Tester.augment: a single flag (or all three) is undone by the second application, exactly one flip together with the transpose is not
    (the frames come back rotated by 180 degrees) -- the restatement follows the reference there."""
    x = torch.arange(2 * 3 * 4 * 6, dtype=torch.float32).reshape(1, 2, 3, 4, 6)
    for flags in [(True, False, False), (False, True, False), (False, False, True)]:
        assert torch.equal(BR.augment(BR.augment(x, *flags), *flags), x)
    twice = BR.augment(BR.augment(x, True, True, True), True, True, True)
    assert twice.shape == x.shape and torch.equal(twice, x)  # flipping both axes commutes with the transpose
    twice = BR.augment(BR.augment(x[..., :4], True, False, True), True, False, True)
    assert torch.equal(twice, x[..., :4].flip(-1).flip(-2))
