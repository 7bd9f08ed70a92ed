"""vmg_amd.metrics.frame_metrics (vmg_frame_metrics, csrc/metrics.hip) against the float64 reference: the reference's own values for
the fixture pairs (tests/golden/metrics_frames.npz), tests/metrics_ref.py for everything else.

Bounds (derived, not measured): RGB PSNR comes from exact integer sums and the reference's own quotient, so it is compared with ==.
PSNR-Y within 1e-9 dB, SSIM and SSIM-Y within 1e-10 absolute: float64 rounding at the sigma^2 = E[x^2] - mu^2 cancellation is
65 025 * 2^-53 ~ 7e-12 against C2 = 58.5, about 1e-13 per map position, and the order of summation is the only other difference; the
bound keeps three orders of margin over that and stays five orders below what float32 arithmetic gives on the flat 200 / 201 pair
(6.7e-5; tests/test_metrics_ref.py::test_float32_would_miss_the_flat_pair).

Worst differences measured on the MI355X: NOT MEASURED YET -- no GPU run of this file had completed when it was written (WORST_MEASURED
below holds None); every case prints its differences before it asserts, run with -s to see them.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_PSNR_Y_DB, TOL_SSIM = 1e-9, 1e-10
# measured on the MI355X (all cases of this file): PSNR-Y worst |difference| in dB, SSIM / SSIM-Y worst absolute difference
WORST_MEASURED = {"psnr_y_db": None, "ssim": None, "ssim_y": None}


def fixture_pairs():
    z = np.load(os.path.join(ROOT, "tests", "golden", "metrics_frames.npz"))
    meta = json.loads(str(z["meta"]))
    return meta, {n: (z[n + "/out"], z[n + "/gt"], z[n + "/values"]) for n in meta["pairs"]}


def synth_pair(h, w, seed, noise=6):
    """A smooth scene with texture and its noisy copy, (h, w, 3) uint8."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(x / 17.0 + seed) * np.cos(y / 13.0), 40 + 170.0 * x / w + 20 * np.sin(y / 5.0), 230 - 200.0 * y / h], -1)
    gt = np.clip(np.rint(base + rng.normal(0, 4, base.shape)), 0, 255).astype(np.uint8)
    out = np.clip(gt.astype(np.int32) + rng.integers(-noise, noise + 1, gt.shape), 0, 255).astype(np.uint8)
    return out, gt


def dev(frames, layout):
    """(T, H, W, 3) or (H, W, 3) numpy -> device tensor in the interleaved layout as it is, or planar."""
    t = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    if layout == "interleaved":
        return t
    return (t.permute(2, 0, 1) if t.dim() == 3 else t.permute(0, 3, 1, 2)).contiguous()


def compare(what, got, want_rows):
    """got: FrameMetrics of T frames; want_rows: T tuples (psnr, psnr_y, ssim, ssim_y) of the reference.  Prints every figure, then asserts."""
    assert all(c.dtype == torch.float64 and c.shape == (len(want_rows),) and not c.is_cuda for c in got)
    for t, want in enumerate(want_rows):
        g = [float(c[t]) for c in got]
        d_y = 0.0 if g[1] == want[1] else abs(g[1] - want[1])
        d_s, d_sy = abs(g[2] - want[2]), abs(g[3] - want[3])
        print(f"{what}[{t}]: psnr {g[0]!r} (ref {want[0]!r})  |d psnr_y| {d_y:.3e} dB  |d ssim| {d_s:.3e}  |d ssim_y| {d_sy:.3e}")
        assert g[0] == want[0], (what, t, g[0], want[0])
        assert d_y <= TOL_PSNR_Y_DB, (what, t, g[1], want[1])
        assert d_s <= TOL_SSIM, (what, t, g[2], want[2])
        assert d_sy <= TOL_SSIM, (what, t, g[3], want[3])


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_fixture_pairs_match_the_reference_values(layout):
    from vmg_amd.metrics import frame_metrics
    meta, pairs = fixture_pairs()
    for name, (out, gt, vals) in pairs.items():
        compare(f"{name}/{layout}", frame_metrics(dev(out, layout), dev(gt, layout)), [tuple(vals[:4])])
        compare(f"{name}/{layout}/border", frame_metrics(dev(out, layout), dev(gt, layout), border=meta["border"]), [tuple(vals[4:])])


def test_mixed_layouts_in_one_call():
    from vmg_amd.metrics import frame_metrics
    _, pairs = fixture_pairs()
    for name, (out, gt, vals) in pairs.items():
        compare(f"{name}/planar-vs-interleaved", frame_metrics(dev(out, "planar"), dev(gt, "interleaved")), [tuple(vals[:4])])


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_flat_200_201_pair(layout):
    """The pair a float32 kernel gets wrong in the fifth decimal."""
    from vmg_amd.metrics import frame_metrics
    out, gt = np.full((48, 80, 3), 200, np.uint8), np.full((48, 80, 3), 201, np.uint8)
    want = R.frame_scores(out, gt)
    assert abs(want[2] - 0.999988) < 1e-6
    compare(f"flat/{layout}", frame_metrics(dev(out, layout), dev(gt, layout)), [want])


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_identical_pair_gives_inf(layout):
    from vmg_amd.metrics import frame_metrics
    out, _ = synth_pair(40, 56, 1)
    got = frame_metrics(dev(out, layout), dev(out.copy(), layout))
    assert float(got.psnr[0]) == float("inf") and float(got.psnr_y[0]) == float("inf")
    compare(f"identical/{layout}", got, [R.frame_scores(out, out)])
    assert abs(float(got.ssim[0]) - 1.0) <= TOL_SSIM and abs(float(got.ssim_y[0]) - 1.0) <= TOL_SSIM


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
@pytest.mark.parametrize("shape", [(11, 11), (37, 53), (180, 320)])
def test_small_and_partial_tile_frames(shape, layout):
    """11 x 11 is the one-position map; 37 x 53 and 180 x 320 leave partial 16 x 32 tiles on both edges."""
    from vmg_amd.metrics import frame_metrics
    out, gt = synth_pair(*shape, seed=shape[0])
    compare(f"{shape}/{layout}", frame_metrics(dev(out, layout), dev(gt, layout)), [R.frame_scores(out, gt)])


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_720p_pair(layout):
    from vmg_amd.metrics import frame_metrics
    out, gt = synth_pair(720, 1280, seed=7, noise=3)
    compare(f"720p/{layout}", frame_metrics(dev(out, layout), dev(gt, layout)), [R.frame_scores(out, gt)])


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_frames_cut_from_a_larger_batch(layout):
    """T = 5 (every second frame) and T = 1 of a 12-frame batch, each a window of larger frames: non-contiguous views, no copy."""
    from vmg_amd.metrics import frame_metrics
    H, W = 45, 70
    rng = np.random.default_rng(11)
    big_gt = rng.integers(0, 256, (12, H + 8, W + 6, 3), dtype=np.uint8)
    big_out = np.clip(big_gt.astype(np.int32) + rng.integers(-5, 6, big_gt.shape), 0, 255).astype(np.uint8)
    d_out, d_gt = dev(big_out, layout), dev(big_gt, layout)
    for frames in (slice(2, 12, 2), slice(7, 8)):
        if layout == "planar":
            a, b = d_out[frames, :, 3:3 + H, 2:2 + W], d_gt[frames, :, 3:3 + H, 2:2 + W]
        else:
            a, b = d_out[frames, 3:3 + H, 2:2 + W, :], d_gt[frames, 3:3 + H, 2:2 + W, :]
        assert not a.is_contiguous()
        want = [R.frame_scores(o, g) for o, g in zip(big_out[frames, 3:3 + H, 2:2 + W], big_gt[frames, 3:3 + H, 2:2 + W])]
        assert len(want) == (5 if frames.start == 2 else 1)
        compare(f"batch{frames.start}/{layout}", frame_metrics(a, b), want)
        compare(f"batch{frames.start}/{layout}/border", frame_metrics(a, b, border=4),
                [R.frame_scores(o, g, border=4) for o, g in zip(big_out[frames, 3:3 + H, 2:2 + W], big_gt[frames, 3:3 + H, 2:2 + W])])


def test_two_calls_return_identical_bits():
    from vmg_amd import kernels as K
    from vmg_amd.metrics import frame_metrics
    outs, gts = zip(*(synth_pair(180, 320, seed=s) for s in range(4)))
    a, b = dev(np.stack(outs), "planar"), dev(np.stack(gts), "interleaved")
    first, second = frame_metrics(a, b), frame_metrics(a, b)
    for x, y in zip(first, second):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64))
    # and below the logarithm: the device sums themselves, with the workspace full of other bits in between
    bp = b.permute(0, 3, 1, 2)
    ws = torch.full((int(K.hip.lib().vmg_frame_metrics_ws_bytes(4, 180, 320)),), 0xA5, dtype=torch.uint8, device="cuda")
    s1 = [t.clone() for t in K.frame_metrics_sums(a, bp, ws)]
    ws.fill_(0x3C)
    s2 = K.frame_metrics_sums(a, bp, ws)
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1].view(torch.int64), s2[1].view(torch.int64))


def test_refusals():
    from vmg_amd.hip import HipError
    from vmg_amd.metrics import frame_metrics
    ok = torch.zeros(3, 16, 16, dtype=torch.uint8, device="cuda")
    for h, w in ((10, 32), (32, 10)):
        small = torch.zeros(3, h, w, dtype=torch.uint8, device="cuda")
        with pytest.raises(HipError, match="11 x 11"):
            frame_metrics(small, small)
    with pytest.raises(HipError, match="11 x 11"):
        frame_metrics(ok, ok, border=3)  # 16 - 6 = 10
    with pytest.raises(HipError, match="uint8"):
        frame_metrics(ok.float(), ok.float())
    with pytest.raises(HipError, match="uint8"):
        frame_metrics(ok, ok.to(torch.int16))
    with pytest.raises(HipError, match="device tensor"):
        frame_metrics(ok.cpu(), ok)
    with pytest.raises(HipError, match="device tensor"):
        frame_metrics(ok, ok.cpu())
    with pytest.raises(HipError, match="shape"):
        frame_metrics(ok, torch.zeros(3, 16, 17, dtype=torch.uint8, device="cuda"))
    with pytest.raises(HipError):
        frame_metrics(torch.zeros(4, 16, 16, dtype=torch.uint8, device="cuda"), torch.zeros(4, 16, 16, dtype=torch.uint8, device="cuda"))


def test_to_uint8_device_holds_the_bytes_of_to_uint8():
    from vmg_amd import infer
    x = (torch.rand(1, 4, 3, 24, 40, device="cuda") * 1.2 - 0.1)
    x[0, 0, 0, 0, :4] = torch.tensor([0.5 / 255, 1.5 / 255, 2.5 / 255, 254.5 / 255])  # ties: round half to even
    u = infer.to_uint8_device(x)
    assert u.dtype == torch.uint8 and u.is_cuda and tuple(u.shape) == (4, 3, 24, 40)
    assert np.array_equal(u.permute(0, 2, 3, 1).cpu().numpy(), infer.to_uint8(x))
    one = infer.to_uint8_device(x[:, :1])
    assert tuple(one.shape) == (1, 3, 24, 40) and torch.equal(one[0], u[0])


def test_scores_of_device_frames_feed_the_scoreboard():
    """The path a driver takes: network output -> to_uint8_device -> frame_metrics (planar against decoded interleaved GT) -> Scoreboard."""
    from vmg_amd import infer
    from vmg_amd.metrics import Scoreboard, frame_metrics
    rng = np.random.default_rng(5)
    gt = rng.integers(0, 256, (3, 32, 48, 3), dtype=np.uint8)
    outputs = torch.from_numpy(gt).cuda().permute(0, 3, 1, 2).float().div(255).add(0.004).unsqueeze(0)
    u8 = infer.to_uint8_device(outputs)
    m = frame_metrics(u8, torch.from_numpy(gt).cuda())
    out_np = u8.permute(0, 2, 3, 1).cpu().numpy()
    compare("driver", m, [R.frame_scores(o, g) for o, g in zip(out_np, gt)])
    sb = Scoreboard()
    sb.start_sequence("000", "clip")
    sb.add_clip([0, 1, 2], m)
    assert sb.end_sequence()["psnr"] == pytest.approx(float(m.psnr.mean()), rel=1e-15)
