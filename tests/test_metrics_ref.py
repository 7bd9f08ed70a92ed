"""CPU checks of the frame-scoring reference chain and of the Scoreboard's bookkeeping (no GPU):
the reference's own values (tests/golden/metrics_frames.npz, tools/gen_metrics_golden.py) -> tests/metrics_ref.py -> the GPU tests."""
import json
import math
import os

import numpy as np
import pytest

from tests import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_pairs():
    z = np.load(os.path.join(ROOT, "tests", "golden", "metrics_frames.npz"))
    meta = json.loads(str(z["meta"]))
    return meta, {n: (z[n + "/out"], z[n + "/gt"], z[n + "/values"]) for n in meta["pairs"]}


def test_fixture_says_what_was_restated():
    meta, pairs = load_pairs()
    assert len(pairs) >= 3 and "cv2" in meta["restated"] and "scikit-image" in meta["restated"]
    for out, gt, vals in pairs.values():
        assert out.dtype == np.uint8 and out.shape == gt.shape and out.shape[2] == 3 and out.shape[0] <= 64 and out.shape[1] <= 96
        assert vals.shape == (8,) and np.isfinite(vals).all()


def test_restatement_reproduces_the_reference_values():
    """Every value the reference's own functions returned, to 1e-12 relative: the restatement differs from them only in the order the
    121 window terms and the map are summed (and in how the luma product is associated)."""
    meta, pairs = load_pairs()
    for name, (out, gt, vals) in pairs.items():
        got = R.frame_scores(out, gt) + R.frame_scores(out, gt, border=meta["border"])
        for g, w in zip(got, vals):
            assert abs(g - w) <= 1e-12 * abs(w), (name, g, w)


def test_psnr_equals_the_oracle_exactly():
    from oracle.vmg_oracle import psnr_uint8
    _, pairs = load_pairs()
    for name, (out, gt, vals) in pairs.items():
        assert R.psnr(out, gt) == psnr_uint8(out, gt) == vals[0], name
    assert R.psnr(out, out) == psnr_uint8(out, out) == float("inf")


def test_window_agrees_with_scipy_correlate():
    """A second spelling of the filter: scipy.ndimage.correlate with the 11 x 11 outer product, on the valid region."""
    import scipy.ndimage
    k = R.gaussian_kernel(11, 1.5)
    assert k.shape == (11, 1) and abs(k.sum() - 1.0) < 1e-15 and np.array_equal(k, k[::-1])
    assert abs(k[5, 0] / k[4, 0] - math.exp(0.5 / 2.25)) < 1e-15
    window = np.outer(k, k.transpose())
    img = np.random.default_rng(3).integers(0, 256, (40, 57)).astype(np.float64) ** 2
    ours = R.filter2d(img, window)[5:-5, 5:-5]
    theirs = scipy.ndimage.correlate(img, window, mode="constant")[5:-5, 5:-5]
    assert ours.shape == (30, 47)
    assert np.abs(ours - theirs).max() <= 1e-12 * np.abs(theirs).max()


def test_float32_would_miss_the_flat_pair():
    """Why the kernel is float64: the flat 200 / 201 pair's SSIM in float32 is off by more than 1e-5, five orders above the GPU test's bound."""
    a, b = np.full((32, 32), 200.0), np.full((32, 32), 201.0)
    want = R.ssim(a, b)
    w32 = np.outer(R.gaussian_kernel(), R.gaussian_kernel()).astype(np.float32)

    def f32(img):
        acc = np.zeros((22, 22), np.float32)
        for i in range(11):
            for j in range(11):
                acc += img[i:i + 22, j:j + 22] * w32[i, j]
        return acc

    x, y = a.astype(np.float32), b.astype(np.float32)
    m1, m2 = f32(x), f32(y)
    s1, s2, s12 = f32(x * x) - m1 * m1, f32(y * y) - m2 * m2, f32(x * y) - m1 * m2
    c1, c2 = np.float32(R.C1), np.float32(R.C2)
    got = float((((2 * m1 * m2 + c1) * (2 * s12 + c2)) / ((m1 * m1 + m2 * m2 + c1) * (s1 + s2 + c2))).mean())
    assert abs(want - 0.999988) < 1e-6
    assert abs(got - want) > 1e-5


# ---- Scoreboard: a hand-written walk through tools/test_reds4.py:136-283 ----------------------------------------------------------

def _cols(values):
    """Four metric columns from one number per frame: psnr = v, psnr_y = v + 1, ssim = v / 100, ssim_y = v / 50."""
    return [[v for v in values], [v + 1 for v in values], [v / 100 for v in values], [v / 50 for v in values]]


def test_scoreboard_skips_frames_already_scored():
    from vmg_amd.metrics import Scoreboard
    sb = Scoreboard()
    sb.start_sequence("000", "a")
    assert sb.add_clip([0, 1, 2], _cols([30.0, 31.0, 32.0])) == [0, 1, 2]
    # frames 1 and 2 come again with other values (an overlapping window): only frame 3 is new
    assert sb.add_clip([1, 2, 3], _cols([99.0, 99.0, 35.0])) == [2]
    res = sb.end_sequence()
    assert res["frames"] == 4
    assert res["psnr"] == (30.0 + 31.0 + 32.0 + 35.0) / 4
    assert res["psnr_y"] == (31.0 + 32.0 + 33.0 + 36.0) / 4
    assert res["ssim"] == pytest.approx((0.30 + 0.31 + 0.32 + 0.35) / 4, abs=1e-15)
    assert sb.frames["000", "a"][2]["psnr"] == 32.0


def test_scoreboard_mid_frame_and_mirror_rules():
    from vmg_amd.metrics import Scoreboard
    sb = Scoreboard(eval_mid_clip=True)
    sb.start_sequence("v", "s")
    assert sb.add_clip(list(range(7)), _cols([float(i) for i in range(7)])) == [3]  # 7 // 2
    assert sb.add_clip(list(range(10, 14)), _cols([10.0, 11.0, 12.0, 13.0])) == [2]  # 4 // 2
    assert sb.end_sequence()["psnr"] == (3.0 + 12.0) / 2
    # every frame was still scored (the reference writes each image), only two entered the mean
    assert len(sb.frames["v", "s"]) == 11

    sb = Scoreboard(eval_mid_clip=True, use_mirrors=True)
    sb.start_sequence("v", "m")
    assert sb.add_clip(list(range(14)), _cols([float(i) for i in range(14)])) == [3, 10]
    res = sb.end_sequence()
    assert res["psnr"] == (3.0 + 10.0) / 2 and res["frames"] == 2
    # use_mirrors without eval_mid_clip: the reference's outer test fails, every frame counts
    sb = Scoreboard(eval_mid_clip=False, use_mirrors=True)
    sb.start_sequence("v", "m")
    assert sb.add_clip([0, 1], _cols([1.0, 2.0])) == [0, 1]


def test_scoreboard_means_of_means():
    from vmg_amd.metrics import Scoreboard
    sb = Scoreboard()
    walk = {"A": {"a1": [10.0, 20.0, 30.0], "a2": [50.0]}, "B": {"b1": [70.0, 90.0]}}
    for folder, seqs in walk.items():
        for seq, vals in seqs.items():
            sb.start_sequence(folder, seq)
            sb.add_clip(list(range(len(vals))), _cols(vals))
            sb.end_sequence()
    assert sb.folder_average("A")["psnr"] == (20.0 + 50.0) / 2
    assert sb.folder_average("B")["psnr"] == 80.0
    assert sb.average()["psnr"] == (35.0 + 80.0) / 2
    flat = (10.0 + 20.0 + 30.0 + 50.0 + 70.0 + 90.0) / 6
    assert sb.average()["psnr"] != flat and sb.folder_average("A")["psnr"] != (10.0 + 20.0 + 30.0 + 50.0) / 4
    assert sb.average()["psnr_y"] == sb.average()["psnr"] + 1
    with pytest.raises(ValueError):
        sb.start_sequence("A", "a1")
    with pytest.raises(ValueError):
        sb.add_clip([0], _cols([1.0]))


def test_frame_metrics_refuses_host_tensors():
    import torch
    from vmg_amd.hip import HipError
    from vmg_amd.metrics import frame_metrics
    with pytest.raises(HipError):
        frame_metrics(torch.zeros(3, 16, 16, dtype=torch.uint8), torch.zeros(3, 16, 16, dtype=torch.uint8))


def test_workspace_query_and_argument_checks():
    """vmg_frame_metrics_ws_bytes counts one 48-byte record per 16 x 32 tile and frame; frames below 11 pixels are refused before anything
    is launched (the pointers here are never dereferenced)."""
    import ctypes
    from vmg_amd import hip
    l = hip.lib()
    assert l.vmg_frame_metrics_ws_bytes(1, 11, 11) == 48
    assert l.vmg_frame_metrics_ws_bytes(5, 720, 1280) == 5 * 45 * 40 * 48
    assert l.vmg_frame_metrics_ws_bytes(2, 37, 53) == 2 * 3 * 2 * 48
    assert l.vmg_frame_metrics_ws_bytes(1, 10, 64) == 0 and l.vmg_frame_metrics_ws_bytes(0, 64, 64) == 0
    st = (ctypes.c_int64 * 4)(3 * 64 * 64, 64 * 64, 64, 1)
    win = (ctypes.c_double * 11)(*([1.0 / 11] * 11))
    for (T, H, W, ws_bytes), what in (((1, 10, 64, 1 << 20), "smaller than the 11 x 11"), ((1, 64, 10, 1 << 20), "smaller than the 11 x 11"),
                                      ((0, 64, 64, 1 << 20), "frames per call"), ((1, 64, 64, 47), "workspace")):
        assert l.vmg_frame_metrics(16, st, 16, st, T, H, W, win, 16, ws_bytes, 16, 16, None) != 0
        assert what in l.vmg_last_error().decode(), (T, H, W)
