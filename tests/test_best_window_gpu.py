"""Best window per frame on the GPU (vmg_amd.infer.best_window_clips / evaluate_reds over vmg_frame_sqerr and vmg_best_window_select) against
the numpy restatement (tests/best_window_ref.py, pinned to the oracle and the reference's fixture by tests/test_best_window_ref.py), the
oracle's test_clips_max and the product's own test_clips_max.

The network is replayed: the oracle's fake model runs once on the CPU, its outputs are recorded and handed out again on the device, so
both sides select among identical numbers and the selected frames must be bit-equal.  Scores: the float64 log10 of the device may differ
from numpy's in the last bit, which moves a float32 score by at most one unit in its last place; the inputs keep the scores of a frame
at least 1e-3 dB apart (checked on the CPU), so the choice cannot depend on it."""
import numpy as np
import pytest
import torch

from tests import best_window_ref as BR

pytestmark = pytest.mark.gpu


class _Replay:
    """Hands out the recorded outputs, already on the device (no copy, no synchronisation inside the call under test).  With `ins` it also
    checks that every call receives the recorded input bit for bit."""

    def __init__(self, outs, dtype=torch.float32, ins=None):
        self.outs, self.ins, self.i = [o.to(dtype).cuda() for o in outs], None if ins is None else [x.cuda() for x in ins], 0

    def __call__(self, x):
        o = self.outs[self.i]
        assert x.is_cuda and tuple(o.shape[-2:]) == (4 * x.shape[-2], 4 * x.shape[-1])
        if self.ins is not None:
            assert torch.equal(x.float(), self.ins[self.i]), f"call {self.i}: the network input differs from the reference's"
        self.i += 1
        return o


def _ulp32(ref: np.ndarray) -> np.ndarray:
    return np.spacing(np.abs(ref).astype(np.float32))


# ---- vmg_frame_sqerr ---------------------------------------------------------------------------------------------------------------
def _frames(n, C, h, w, dtype, strided, seed):
    """n frames with values on both sides of [0, 1]; strided: every second frame of a longer clip, starting at its second one."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        full = torch.randint(0, 256, (2 * n + 1 if strided else n, h, w, C), generator=g, dtype=torch.uint8).cuda()
    else:
        full = (0.6 * torch.randn((2 * n + 1 if strided else n, C, h, w), generator=g) + 0.5).to(dtype).cuda()
    return full[1::2] if strided else full


def _np_frames(t):
    return t.cpu().numpy() if t.dtype == torch.uint8 else t.float().cpu().numpy()


SQERR_SHAPES = [(3, 3, 5, 7, False), (3, 3, 20, 28, False), (2, 3, 259, 517, False), (3, 3, 5, 7, True), (3, 3, 20, 28, True)]


@pytest.mark.parametrize("n,C,h,w,strided", SQERR_SHAPES)
@pytest.mark.parametrize("hr_dtype", [torch.float32, torch.bfloat16, torch.uint8])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_frame_sqerr_matches_float64_numpy(out_dtype, hr_dtype, n, C, h, w, strided):
    from vmg_amd import kernels as K
    out = _frames(n, C, h, w, out_dtype, strided, 11)
    hr = _frames(n, C, h, w, hr_dtype, strided, 12)
    if strided:
        assert out.stride(0) == 2 * C * h * w and not out.is_contiguous()
    err = K.frame_sqerr(out, hr)
    again = K.frame_sqerr(out, hr)
    got = err.cpu().numpy()
    o, r = _np_frames(out), _np_frames(hr)
    assert (o.min() < 0 and o.max() > 1) and (hr_dtype == torch.uint8 or (r.min() < 0 and r.max() > 1))
    want = np.array([BR.frame_err(o[f], r[f]) for f in range(n)])
    rel = np.abs(got - want) / want
    print(f"frame_sqerr {out_dtype} vs {hr_dtype} {(n, C, h, w)} strided={strided}: max relative deviation {rel.max():.3e}")
    assert err.dtype == torch.float64 and rel.max() <= 1e-12
    assert torch.equal(err, again)  # fixed partition, fixed order: the same bits


@pytest.mark.parametrize("h,w", [(5, 7), (20, 28)])
def test_frame_sqerr_of_equal_frames_is_exactly_zero(h, w):
    from vmg_amd import kernels as K
    hr8 = _frames(3, 3, h, w, torch.uint8, False, 13)
    unit = torch.from_numpy(BR.as_unit(hr8.cpu().numpy())).cuda()  # numpy's astype(float32) / 255.: the kernel must form these very bits
    assert torch.count_nonzero(K.frame_sqerr(unit, hr8)).item() == 0
    assert torch.count_nonzero(K.frame_sqerr(unit, unit.clone())).item() == 0
    wide = unit * 3 - 1  # clamping: everything outside [0, 1] on one side only
    e = K.frame_sqerr(wide, wide.clamp(0, 1)).cpu()
    assert torch.count_nonzero(e).item() == 0


# ---- vmg_best_window_select --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,h,w", [(3, 5, 7), (3, 20, 28), (3, 33, 65)])
def test_best_window_select_rules(dtype, C, h, w):
    """Three windows over five frames: window 0 copies unconditionally (frames 0-2; an exact match scores the cap), window 1 (frames 2-4) ties on
    frame 2 (kept), wins the uncovered frame 3, scores 0 on the uncovered frame 4 (stays zero, choice 0), window 2 (frames 1-3) ties at the cap on
    frame 1 (kept), is strictly better on frame 2 (replaced), worse on frame 3 (kept).  3 x 5 x 7 frames start at odd addresses: scalar copies."""
    from vmg_amd import kernels as K
    T, ts = 5, [0, 2, 1]
    g = torch.Generator().manual_seed(21)
    outs = [(torch.rand((3, C, h, w), generator=g) + k).to(dtype) for k in range(3)]
    errs = [np.array([0.01, 0.0, 0.04]), np.array([0.04, 0.02, 1.0]), np.array([0.0, 0.03, 0.05])]
    canvas = torch.zeros(T, C, h, w, device="cuda")
    best = torch.zeros(2, T, device="cuda")
    choice = torch.zeros(2, T, dtype=torch.int32, device="cuda")
    table = torch.zeros(T, 3, device="cuda")
    for k in range(3):
        K.best_window_select(outs[k].cuda(), torch.from_numpy(errs[k]).cuda(), ts[k], k, BR.CAP, canvas, best[k & 1], choice[k & 1], best[(k + 1) & 1],
                             choice[(k + 1) & 1], table)
    np_outs = [o.float().numpy() for o in outs]
    frames, want_best, want_choice = BR.select_streaming(np_outs, errs, ts, T)
    assert list(want_choice) == [0, 0, 2, 1, 0] and not frames[4].any()  # (the scenario is the one described)
    assert np.array_equal(choice[1].cpu().numpy(), want_choice)
    assert np.array_equal(canvas.cpu().numpy(), frames)
    got_best = best[1].cpu().numpy()
    assert got_best[1] == np.float32(BR.CAP) and got_best[4] == 0.0
    assert np.all(np.abs(got_best - want_best) <= _ulp32(want_best))
    want_table = BR.score_table(errs, ts, T)
    assert np.all(np.abs(table.cpu().numpy() - want_table) <= _ulp32(want_table))
    assert np.array_equal(table.cpu().numpy() == 0, want_table == 0)


# ---- best_window_clips -------------------------------------------------------------------------------------------------------------
def _run_clips(name, return_scores=True):
    from vmg_amd import infer
    ref = BR.clip_reference(name)
    dt = torch.bfloat16 if ref["bf16"] else torch.float32
    x, hr = ref["x"].to(dt).cuda(), ref["hr"].to(dt).cuda()
    rep = _Replay(ref["rec"].outs, dt)
    got = infer.best_window_clips(rep, x, hr, ref["nf"], ref["of"], ref["spatial"], ref["ov"], 4, return_scores=return_scores)
    assert rep.i == len(ref["rec"].outs)
    return ref, x, hr, dt, got


@pytest.mark.parametrize("name", list(BR.CLIP_CASES))
def test_best_window_clips_equals_oracle_and_test_clips_max(name):
    from vmg_amd import infer
    ref, x, hr, dt, (got, (choice, best, table)) = _run_clips(name)
    T, nf = x.shape[1], ref["nf"]
    assert got.dtype == dt and tuple(got.shape) == (T, 3, 4 * x.shape[-2], 4 * x.shape[-1])
    assert torch.equal(got.float().cpu(), ref["want"])
    old = infer.test_clips_max(_Replay(ref["rec"].outs, dt), x, hr, nf, ref["of"], ref["spatial"], ref["ov"], 4)
    assert torch.equal(got, old)
    ts = BR.tile_starts(T, nf, ref["of"])
    want_table = BR.score_table(BR.window_errs(BR.window_outputs(ref), ts, ref["hr"][0].numpy()), ts, T)
    assert choice.dtype == torch.int32 and best.dtype == torch.float32 and tuple(table.shape) == (T, len(ts))
    assert np.array_equal(choice.cpu().numpy(), BR.select_table(want_table))
    tb = table.cpu().numpy()
    assert np.all(np.abs(tb - want_table) <= _ulp32(want_table)) and np.array_equal(tb == 0, want_table == 0)
    assert np.array_equal(best.cpu().numpy(), tb.max(axis=1))


def test_best_window_clips_is_reproducible_and_plain_return():
    _, _, _, _, (a, (ca, ba, ta)) = _run_clips("fixture")
    _, _, _, _, (b, (cb, bb, tb)) = _run_clips("fixture")
    assert torch.equal(a, b) and torch.equal(ca, cb) and torch.equal(ba, bb) and torch.equal(ta, tb)
    _, _, _, _, plain = _run_clips("fixture", return_scores=False)
    assert isinstance(plain, torch.Tensor) and torch.equal(plain, a)


def test_best_window_clips_uint8_hr_equals_float_hr():
    """HR as (T, 4H, 4W, 3) uint8 is scored in place: the same frames and choices as with the float HR built from byte / 255 (the two forms are
    summed in different orders, so a score may differ in its last place)."""
    from vmg_amd import infer
    ref = BR.clip_reference("t7_w3_o1")
    hr8 = BR.u8_hr_of("t7_w3_o1")
    hrf = torch.from_numpy(BR.as_unit(hr8)).unsqueeze(0)
    x = ref["x"].cuda()
    a, (ca, ba, _) = infer.best_window_clips(_Replay(ref["rec"].outs), x, torch.from_numpy(hr8).cuda(), 3, 1, return_scores=True)
    b, (cb, bb, _) = infer.best_window_clips(_Replay(ref["rec"].outs), x, hrf.cuda(), 3, 1, return_scores=True)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    assert np.all(np.abs(ba.cpu().numpy() - bb.cpu().numpy()) <= _ulp32(bb.cpu().numpy()))
    ts = BR.tile_starts(7, 3, 1)
    want = BR.score_table(BR.window_errs(BR.window_outputs(ref), ts, hr8), ts, 7)
    assert np.array_equal(ca.cpu().numpy(), BR.select_table(want))


def test_best_window_clips_refuses_a_batch():
    from vmg_amd import infer
    x = torch.zeros(2, 5, 3, 16, 16, device="cuda")
    with pytest.raises(ValueError):
        infer.best_window_clips(lambda c: None, x, torch.zeros(2, 5, 3, 64, 64, device="cuda"), 3, 1)


def test_best_window_clips_memory_and_no_synchronisation():
    """Replayed 3 x 64 x 64 outputs, T = 9: the call may own one canvas, one window's output and 1 MB, and must not synchronise."""
    from vmg_amd import infer
    ref = BR.clip_reference("fixture")
    x, hr = ref["x"].cuda(), ref["hr"].cuda()
    infer.best_window_clips(_Replay(ref["rec"].outs), x, hr, 4, 2)  # (library load, first launches)
    rep = _Replay(ref["rec"].outs)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = infer.best_window_clips(rep, x, hr, 4, 2)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    peak = torch.cuda.max_memory_allocated() - base
    canvas, window = 9 * 3 * 64 * 64 * 4, 4 * 3 * 64 * 64 * 4
    print(f"best_window_clips owns {peak} bytes at its peak; one canvas {canvas} + one window's output {window} + 1 MB = {canvas + window + (1 << 20)}")
    assert peak <= canvas + window + (1 << 20)
    assert torch.equal(got.cpu(), ref["want"])


# ---- evaluate_reds -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BR.EVAL_FLAGS)
def test_evaluate_reds_equals_tester_evaluate(flags):
    from vmg_amd import infer
    ref = BR.eval_reference(flags)
    rep = _Replay(ref["rec"].outs, ins=ref["rec"].ins)
    got = infer.evaluate_reds(rep, torch.from_numpy(ref["lr"]).cuda(), torch.from_numpy(ref["hr"]).cuda(), 3, 1, None, None, 4, *flags)
    assert rep.i == len(ref["rec"].outs)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == ref["want"].shape == (5, 48, 64, 3)
    assert np.array_equal(got.cpu().numpy(), ref["want"])
