"""Frame conversion on the GPU (vmg_convert_frames under vmg_amd.infer.frames_to_clip / clip_to_frames / augment_frames) and the device-resident
Tester.evaluate built on it (infer.evaluate / evaluate_sequence), against the numpy restatement of tests/frames_ref.py (pinned to
tests/best_window_ref.py by tests/test_frames_ref.py).

Everything here is compared for EQUALITY: the conversions are byte / 255 (a correctly rounded fp32 quotient), clamp * 255 rounded half to even,
and moves; the networks are replayed from the restatement's recorded calls, so both sides convert identical numbers."""
import os

import numpy as np
import pytest
import torch

from tests import frames_ref as FR

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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


def _bits(t: torch.Tensor) -> np.ndarray:
    """The tensor's bytes on the host: equality of bits, not of values (0.0 == -0.0, and bf16 has no numpy type)."""
    return t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy()  # (flat first: a size-1 axis may carry any stride)


def _views(frames_np: np.ndarray, planar: bool):
    """name -> device tensor holding `frames_np` (T, H, W, 3): contiguous, every second frame of a longer stack, and a crop of larger frames
    at an odd column offset (row stride beyond the width, base address odd)."""
    T, H, W, _ = frames_np.shape
    src = torch.from_numpy(frames_np)
    src = src.permute(0, 3, 1, 2).contiguous() if planar else src
    out = {"whole": src.cuda()}
    longer = torch.full((2 * T + 1,) + tuple(src.shape[1:]), 7, dtype=src.dtype)
    longer[1::2] = src
    out["second"] = longer.cuda()[1::2]
    big = torch.full((T, 3, H + 3, W + 5) if planar else (T, H + 3, W + 5, 3), 9, dtype=src.dtype)
    crop = (slice(None), slice(None), slice(2, 2 + H), slice(3, 3 + W)) if planar else (slice(None), slice(2, 2 + H), slice(3, 3 + W))
    big[crop] = src
    out["crop"] = big.cuda()[crop]
    # (a single frame is contiguous whatever its frame stride says: the stride is what is checked)
    assert out["crop"].data_ptr() % 2 == 1 and out["second"].stride(0) == 2 * 3 * H * W and (T == 1 or not out["second"].is_contiguous())
    return out


# ---- frames_to_clip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("H,W", FR.FRAME_SIZES)
def test_frames_to_clip_equals_restatement(H, W, T, planar):
    from vmg_amd import infer
    u = FR.u8_frames(T, H, W, 100 + H)
    views = _views(u, planar)
    for flags in FR.ALL_FLAGS:
        want = torch.from_numpy(FR.to_clip(u, *flags))
        for name, v in views.items():
            got = infer.frames_to_clip(v, torch.float32, *flags)
            assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == tuple(want.shape), (name, flags)
            assert np.array_equal(_bits(got), _bits(want)), (name, flags)
            got16 = infer.frames_to_clip(v, torch.bfloat16, *flags)
            assert got16.dtype == torch.bfloat16 and np.array_equal(_bits(got16), _bits(want.to(torch.bfloat16))), (name, flags)


def test_frames_to_clip_all_256_bytes_and_out():
    """Every byte value, in a row of 256 pixels x 3 channels (shifted per channel); with out= the clip lands in a view of a larger buffer."""
    from vmg_amd import infer
    u = np.stack([(np.arange(256) + 85 * c) % 256 for c in range(3)], axis=-1).astype(np.uint8)[None, None]  # (1, 1, 256, 3)
    assert all(len(np.unique(u[..., c])) == 256 for c in range(3))
    for flags in FR.ALL_FLAGS:
        want = torch.from_numpy(FR.to_clip(u, *flags))
        assert np.array_equal(_bits(infer.frames_to_clip(torch.from_numpy(u).cuda(), torch.float32, *flags)), _bits(want))
    buf = torch.full((1, 1, 3, 3, 300), -1.0, device="cuda")
    view = buf[:, :, :, 1:2, 5:261]
    assert infer.frames_to_clip(torch.from_numpy(u).cuda(), out=view) is view
    assert np.array_equal(_bits(view), _bits(torch.from_numpy(FR.to_clip(u))))
    assert int((buf == -1.0).sum()) == buf.numel() - 3 * 256


# ---- clip_to_frames ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("H,W", FR.FRAME_SIZES)
def test_clip_to_frames_equals_restatement(H, W, T, dtype):
    from vmg_amd import infer
    h, w = 4 * H, 4 * W
    clip = torch.from_numpy(FR.unit_clip(T, h, w, 200 + H)).to(dtype)
    c_np = clip.float().numpy()
    assert c_np.min() < 0 and c_np.max() > 1  # (both clamps are exercised)
    dev = clip.cuda()
    for flags in FR.ALL_FLAGS:
        want = FR.to_frames(c_np, *flags)
        for src in (dev, dev.unsqueeze(0)):
            got = infer.clip_to_frames(src, *flags)
            assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == want.shape, flags
            assert np.array_equal(got.cpu().numpy(), want), flags
        pl = infer.clip_to_frames(dev, *flags, planar=True)
        assert pl.is_contiguous() and np.array_equal(pl.cpu().numpy(), want.transpose(0, 3, 1, 2)), flags
        # out=: a view into a larger buffer, at an odd offset; everything around it stays
        hh, ww = want.shape[1:3]
        for planar in (False, True):
            buf = torch.full((T, 3, hh + 4, ww + 6) if planar else (T, hh + 4, ww + 6, 3), 0xAB, dtype=torch.uint8, device="cuda")
            view = buf[:, :, 1:1 + hh, 3:3 + ww] if planar else buf[:, 1:1 + hh, 3:3 + ww]
            assert infer.clip_to_frames(dev, *flags, planar=planar, out=view) is view
            assert np.array_equal(view.cpu().numpy(), want.transpose(0, 3, 1, 2) if planar else want), (flags, planar)
            view.fill_(0xAB)
            assert int((buf != 0xAB).sum()) == 0, (flags, planar)


def test_clip_to_frames_rounds_half_to_even():
    """The 255 values float32((k + 0.5) / 255): every product with 255 is exactly k + 0.5 (asserted), so each byte is k rounded to even."""
    from vmg_amd import infer
    h = FR.half_steps()
    assert int(np.count_nonzero(h * np.float32(255.0) == np.arange(255, dtype=np.float32) + 0.5)) == 255
    clip = np.ascontiguousarray(np.broadcast_to(h[None, None, None, :], (1, 3, 1, 255)))
    k = np.arange(255)
    for flags in FR.ALL_FLAGS:
        got = infer.clip_to_frames(torch.from_numpy(clip).cuda(), *flags).cpu().numpy()
        assert np.array_equal(got, FR.to_frames(clip, *flags)), flags
        assert np.array_equal(np.sort(got[..., 0].ravel()), np.sort(np.where(k % 2 == 0, k, k + 1))), flags


# ---- augment_frames, round trip --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", FR.FRAME_SIZES)
def test_augment_frames_equals_restatement_and_undoes_itself(H, W):
    from vmg_amd import infer
    u = FR.u8_frames(3, H, W, 300 + H)
    for planar in (False, True):
        for name, v in _views(u, planar).items():
            for flags in FR.ALL_FLAGS:
                want = FR.augment_frames(u, *flags)
                got = infer.augment_frames(v, *flags)
                assert got.dtype == torch.uint8 and got.is_contiguous()
                assert np.array_equal(got.cpu().numpy(), want.transpose(0, 3, 1, 2) if planar else want), (planar, name, flags)
                twice = infer.augment_frames(got, *flags)
                back = torch.equal(twice, v)
                assert back == np.array_equal(FR.augment_frames(want, *flags), u), (planar, name, flags)
                if flags in FR.UNDONE:
                    assert back


@pytest.mark.parametrize("H,W", FR.FRAME_SIZES)
def test_round_trip_returns_the_bytes(H, W):
    from vmg_amd import infer
    u = torch.from_numpy(FR.u8_frames(3, H, W, 400 + H)).cuda()
    for flags in FR.UNDONE:
        assert torch.equal(infer.clip_to_frames(infer.frames_to_clip(u, torch.float32, *flags), *flags), u), flags


# ---- evaluate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FR.ALL_FLAGS)
def test_evaluate_reds_branch_equals_evaluate_reds_and_restatement(flags):
    from vmg_amd import infer
    ref = FR.reds_reference(flags)
    lr, hr = torch.from_numpy(ref["lr"]).cuda(), torch.from_numpy(ref["hr"]).cuda()
    rep = _Replay(ref["rec"].outs, ins=ref["rec"].ins)
    got = infer.evaluate(rep, lr, hr, "REDS", 3, 1, None, None, 4, *flags)
    assert rep.i == len(ref["rec"].outs)
    assert got.dtype == torch.uint8 and got.is_cuda and got.is_contiguous() and tuple(got.shape) == ref["want"].shape == (5, 48, 64, 3)
    assert np.array_equal(got.cpu().numpy(), ref["want"])
    old = infer.evaluate_reds(_Replay(ref["rec"].outs, ins=ref["rec"].ins), lr, hr, 3, 1, None, None, 4, *flags)
    assert torch.equal(got, old)


@pytest.mark.parametrize("flags", [(False, False, False), (True, False, False), (False, True, True), (True, True, True)])
@pytest.mark.parametrize("name", list(FR.EVAL_CASES))
def test_evaluate_other_branches_equal_restatement(name, flags):
    from vmg_amd import infer
    ref = FR.eval_reference(name, flags)
    rep = _Replay(ref["rec"].outs, ins=ref["rec"].ins)
    got = infer.evaluate(rep, torch.from_numpy(ref["lr"]).cuda(), None, hflip=flags[0], vflip=flags[1], rot90=flags[2], **ref["kwargs"])
    assert rep.i == len(ref["rec"].outs) == {"vimeo": 1, "vimeo_tiled": 4, "vid4": 3}[name]
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == ref["want"].shape
    assert np.array_equal(got.cpu().numpy(), ref["want"])


def test_evaluate_on_a_real_network_equals_the_parts():
    """Tiny VMG (fp32), 5 frames of 64 x 64 in windows of 3 with overlap 1: evaluate == to_uint8_device(test_clips(byte / 255 clip)), both
    from a freshly loaded model moved to the same call count."""
    from oracle import cases as C
    from tests.util import build_product
    from vmg_amd import infer
    case = C.CASES["infer_vmg_clips"]
    shapes, _ = C.load_fixture(os.path.join(GOLD, "infer_vmg_clips.npz"))
    sd = C.case_state_dict(case, shapes)

    def fresh():
        m = build_product(case["cfg"], torch.float32)
        m.load_state_dict(sd, strict=True)
        m.eval()
        m.set_forward_calls(1)
        return m

    x01 = case["inputs"]()["x"][0, :, :, :64, :64]  # (5, 3, 64, 64) in [0, 1]
    lr = (x01.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()
    got = infer.evaluate(fresh(), lr, None, "Vid4", 3, 1)
    x = torch.from_numpy(FR.to_clip(lr.cpu().numpy())).cuda()
    want = infer.to_uint8_device(infer.test_clips(fresh(), x, 3, 1)).permute(0, 2, 3, 1)
    assert tuple(got.shape) == (5, 256, 256, 3) and torch.equal(got, want)
    assert len(torch.unique(got)) > 16  # (a picture, not a constant)


def _sequence_reference():
    """9 frames in index lists of 4 (frames 3, 5 and 6 are reached twice) through the 'Vid4' branch, windows of 3 with overlap 1, one
    stateful fake network across the lists: the frames as the first list that reaches each produces them."""
    from oracle import infer_oracle as IO
    lr, gt = FR.eval_inputs(9, 12, 16, seed=370)
    rec = FR.Recorder(IO.fake_sr_model())
    lists = FR.index_generation(4, 9)
    assert lists == [[0, 1, 2, 3], [3, 4, 5, 6], [5, 6, 7, 8]]
    frames, later = {}, {}
    for indices in lists:
        out = FR.evaluate(rec, lr[indices], None, "Vid4", 3, 1)
        for pos, f in enumerate(indices):
            (later if f in frames else frames)[f] = out[pos]
    assert sorted(later) == [3, 5, 6] and all(not np.array_equal(later[f], frames[f]) for f in later)  # (scoring one twice would show)
    return lr, gt, rec, np.stack([frames[f] for f in range(9)])


def test_evaluate_sequence_scores_every_frame_once():
    from vmg_amd import infer
    from vmg_amd import metrics as M
    lr, gt, rec, want = _sequence_reference()
    gt_d = torch.from_numpy(gt).cuda()
    board = M.Scoreboard()
    board.start_sequence("000", "0045")
    rep = _Replay(rec.outs, ins=rec.ins)
    got = infer.evaluate_sequence(rep, torch.from_numpy(lr).cuda(), gt_d, 4, board, dataset_name="Vid4", num_frames=3, overlap_frames=1)
    res = board.end_sequence()
    assert rep.i == len(rec.outs) == 6
    assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want)
    vals = M.frame_metrics(torch.from_numpy(want).cuda(), gt_d)
    assert res["frames"] == 9 and sorted(board.frames["000", "0045"]) == list(range(9))
    for k, name in enumerate(M.METRICS):
        col = [float(v) for v in vals[k]]
        assert [board.frames["000", "0045"][f][name] for f in range(9)] == pytest.approx(col, rel=1e-12)
        assert res[name] == pytest.approx(sum(col) / 9, rel=1e-12)


def test_evaluate_sequence_reds_branch_and_mid_clip():
    """The REDS branch takes gt_u8[indices] as HR; with eval_mid_clip only position len(indices) // 2 of a list counts, if it is new."""
    from oracle import infer_oracle as IO
    from vmg_amd import infer
    from vmg_amd import metrics as M
    lr, gt = FR.eval_inputs(9, 12, 16, seed=371)
    rec = FR.Recorder(IO.fake_sr_model())
    lists = FR.index_generation(4, 9)
    outs = [FR.evaluate(rec, lr[i], gt[i], "REDS", 3, 1) for i in lists]
    board = M.Scoreboard(eval_mid_clip=True)
    board.start_sequence("f", "s")
    got = infer.evaluate_sequence(_Replay(rec.outs, ins=rec.ins), torch.from_numpy(lr).cuda(), torch.from_numpy(gt).cuda(), 4, board,
                                  dataset_name="REDS", num_frames=3, overlap_frames=1)
    res = board.end_sequence()
    assert np.array_equal(got[:4].cpu().numpy(), outs[0]) and np.array_equal(got[4:7].cpu().numpy(), outs[1][1:])
    assert np.array_equal(got[7:].cpu().numpy(), outs[2][2:])
    # position 2 of each list: frames 2, 5 and 7 -- all new when their list arrives
    mid = M.frame_metrics(got[[2, 5, 7]], torch.from_numpy(gt[[2, 5, 7]]).cuda())
    assert res["frames"] == 3 and res["psnr"] == pytest.approx(float(mid.psnr.mean()), rel=1e-12)


# ---- synchronisation, memory, errors ---------------------------------------------------------------------------------------------------
def test_conversions_and_evaluate_do_not_synchronise_and_own_only_the_result():
    from vmg_amd import infer
    ref = FR.reds_reference((True, False, True))
    vid = FR.eval_reference("vid4", (False, True, False))
    lr, hr = torch.from_numpy(ref["lr"]).cuda(), torch.from_numpy(ref["hr"]).cuda()
    vlr = torch.from_numpy(vid["lr"]).cuda()
    clip = torch.from_numpy(FR.unit_clip(3, 256, 384, 500)).cuda()
    infer.clip_to_frames(infer.frames_to_clip(infer.augment_frames(lr, True, False, True)))  # (library load, first launches)
    infer.evaluate(_Replay(ref["rec"].outs), lr, hr, "REDS", 3, 1, None, None, 4, True, False, True)
    reps = _Replay(ref["rec"].outs), _Replay(vid["rec"].outs)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x = infer.frames_to_clip(lr, torch.bfloat16, True, True, True)
        a = infer.augment_frames(hr, False, True, True)
        got = infer.evaluate(reps[0], lr, hr, "REDS", 3, 1, None, None, 4, True, False, True)
        gotv = infer.evaluate(reps[1], vlr, None, vflip=True, **vid["kwargs"])
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        frames = infer.clip_to_frames(clip, True, False, True)
        peak = torch.cuda.max_memory_allocated() - base
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    result = 3 * 3 * 256 * 384
    print(f"clip_to_frames raises max_memory_allocated by {peak} bytes; the result has {result}, the bound is {result + (1 << 20)}")
    assert peak <= result + (1 << 20)
    assert np.array_equal(got.cpu().numpy(), ref["want"]) and np.array_equal(gotv.cpu().numpy(), vid["want"])
    assert np.array_equal(frames.cpu().numpy(), FR.to_frames(clip.cpu().numpy(), True, False, True))
    assert tuple(x.shape) == (1, 5, 3, 16, 12) and tuple(a.shape) == (5, 64, 48, 3)


def test_errors():
    from vmg_amd import infer
    from vmg_amd import kernels as K
    from vmg_amd.hip import HipError
    u = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    c = torch.zeros(1, 2, 3, 8, 8)
    for call in (lambda: infer.frames_to_clip(u), lambda: infer.clip_to_frames(c), lambda: infer.augment_frames(u, True, False, False),
                 lambda: infer.evaluate(lambda x: x, u, None, "Vid4", 2, 0)):
        with pytest.raises(HipError):
            call()
    u, c = u.cuda(), c.cuda()
    for call in (lambda: infer.frames_to_clip(u[0]),                       # rank
                 lambda: infer.frames_to_clip(u.float()),                  # dtype
                 lambda: infer.frames_to_clip(u, torch.float16),
                 lambda: infer.frames_to_clip(u, out=torch.empty(1, 2, 3, 8, 9, device="cuda")),
                 lambda: infer.clip_to_frames(c[0, 0]),
                 lambda: infer.clip_to_frames(c.half()),
                 lambda: infer.clip_to_frames(torch.zeros(2, 2, 3, 8, 8, device="cuda")),
                 lambda: infer.clip_to_frames(c, out=torch.empty(2, 8, 8, 3, device="cuda")),
                 lambda: infer.augment_frames(u.float(), True, False, False),
                 lambda: infer.augment_frames(u[0], True, False, False),
                 lambda: infer.evaluate(lambda x: x, u, None, "REDS", 2, 0),   # REDS without HR
                 lambda: infer.evaluate(lambda x: x, u.float(), None, "Vid4", 2, 0),
                 lambda: infer.evaluate(lambda x: x, u[0], None, "Vid4", 2, 0),
                 lambda: infer.evaluate(lambda x: x, u, torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device="cuda"), "REDS", 2, 0)):
        with pytest.raises(ValueError):
            call()
    # the entry point itself: type pair, destination strides that overlap, source and destination that overlap
    pu, pf = u.permute(0, 3, 1, 2), torch.empty(2, 3, 8, 8, device="cuda")
    for call in (lambda: K.convert_frames(pf, torch.empty_like(pf)),
                 lambda: K.convert_frames(pu, torch.empty(2, 3, 8, 1, device="cuda").expand(2, 3, 8, 8)),
                 lambda: K.convert_frames(pu, torch.empty(8, 8, device="cuda").expand(2, 3, 8, 8)),
                 lambda: K.convert_frames(pu, pu.permute(0, 1, 3, 2), rot90=True)):
        with pytest.raises(HipError):
            call()
