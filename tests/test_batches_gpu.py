"""vmg_amd.batches (vmg_crop_batch, csrc/batch.hip) against the reference's recorded batches (tests/golden/train_batches.npz) and against
the numpy restatement tests/batches_ref.py.

Every comparison is exact.  uint8 output: the bytes the restatement picks.  float32 / bfloat16 output: the bits of u8.float().div(255) and
of .to(torch.bfloat16) of it, evaluated on the HOST, where torch divides as numpy does in the dataset classes (data/REDS.py:116; on the
device torch multiplies by 1 / 255, see tests/test_lr_gpu.py); against the fixture: the reference's own float32 values.  The frames are
random bytes everywhere, inside and around every crop, so a read one pixel, row or channel off cannot pass.

The kernel works in 32 x 32 output tiles and does not cap its grid (no grid-stride loop to test); its fetch has three paths -- dwords from
interleaved rows, dwords from planar rows, bytes for row pitches that are no multiple of 4 -- and the sizes below are the smallest that
reach: less than a tile; a tile and a partial tile in both axes; several tiles; every path; misaligned starts.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import batches_ref as R

pytestmark = pytest.mark.gpu
LAYOUTS = ["interleaved", "planar"]
FIXTURE_NAMES = [c["name"] for c in R.fixture()[0]["cases"]]


def dev(a, layout):
    """(..., H, W, 3) numpy -> device tensor, interleaved as it is or planar (..., 3, H, W)."""
    t = torch.from_numpy(np.array(a)).cuda()   # a copy: fixtures are shared and read-only
    return t if layout == "interleaved" else t.movedim(-1, -3).contiguous()


def ref(a):
    return torch.from_numpy(np.array(a))   # a copy: the fixture's arrays are read-only


def window(t, layout, y, x, H, W):
    return t[..., y:y + H, x:x + W, :] if layout == "interleaved" else t[..., y:y + H, x:x + W]


def plan_of(clip, frames, y0, x0, flags, crop):
    from vmg_amd.batches import BatchPlan
    f = np.array(flags, dtype=np.int64).reshape(-1)
    return BatchPlan(clip=np.array(clip), frames=np.array(frames), y0=np.array(y0), x0=np.array(x0), hflip=(f & 1) != 0, vflip=(f & 2) != 0,
                     rot=(f & 4) != 0, crop=crop)


def want_forms(u8):
    """bytes (numpy) -> {dtype: host tensor} of the three output forms."""
    t = torch.from_numpy(np.ascontiguousarray(u8))
    f32 = t.float().div(255)   # on the host: a true division
    return {torch.uint8: t, torch.float32: f32, torch.bfloat16: f32.to(torch.bfloat16)}


def same_bits(got, want):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape) and got.is_contiguous() and got.is_cuda
    return torch.equal(got.cpu().view(torch.uint8), want.contiguous().view(torch.uint8))


def check_all_forms(store, plan, hr_np, lr_np, bgr=True, dtypes=(torch.uint8, torch.float32, torch.bfloat16)):
    from vmg_amd import batches
    wl, wh = R.batch(hr_np, lr_np, plan, store.scale, bgr, as_bytes=True)
    wl, wh = want_forms(wl), want_forms(wh)
    for dt in dtypes:
        lrs, hrs = batches.assemble(store, plan, dtype=dt)
        assert same_bits(lrs, wl[dt]), ("LRs", dt)
        assert same_bits(hrs, wh[dt]), ("HRs", dt)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_fixture_cases_match_the_reference_batches(name, layout):
    from vmg_amd import batches
    meta, z = R.fixture()
    case = meta["cases"][FIXTURE_NAMES.index(name)]
    store = batches.FrameStore(dev(z["hr"], layout), dev(z["lr"], layout), meta["scale"])
    py, npr = R.case_rngs(case)
    plan = batches.draw_plan(case["indices"], case["cfg"], py, npr, dataset=case["dataset"])
    lrs, hrs = batches.assemble(store, plan)
    assert same_bits(lrs, ref(z[name + "/LRs"])) and same_bits(hrs, ref(z[name + "/HRs"]))
    check_all_forms(store, plan, z["hr"], z["lr"], dtypes=(torch.uint8, torch.bfloat16))


# LR frame (H, W), LR crop edge, flags: (a) less than one tile, 4 x 4 / 16 x 16; (b) tile edge + 8 = 40 (LR: a tile and a partial tile in both
# axes, HR 160 = five tiles); (c) 28 clipped by a 20-row frame: 20 x 28 / 80 x 112, partial tiles in both axes of both, rot off
SIZES = {"a-4x4": ((13, 17), 4, range(8)), "b-40x40": ((43, 45), 40, range(8)), "c-20x28": ((20, 37), 28, range(4))}


@pytest.mark.parametrize("pitch", ["pitch-0-mod-4", "pitch-2-mod-4", "pitch-odd"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", list(SIZES))
def test_every_flag_combination_origin_and_fetch_path(size, layout, pitch):
    """All flag combinations x three origins in one batch (B = 24 or 12, T = 2), from stores that are windows of larger frames of random
    bytes, one pixel in from the left: the rows start misaligned, and the row pitch of the larger frame picks the dword or the byte path."""
    from vmg_amd import batches
    (H, W), c, flagset = SIZES[size]
    s = 4
    ch, cw = min(c, H), min(c, W)
    rng = np.random.default_rng(7)
    # interleaved pitch = 3 (W + pad) bytes, planar W + pad: pad so that both are 0 / 2 / odd mod 4
    pad = {"pitch-0-mod-4": (-W) % 4 or 4, "pitch-2-mod-4": (2 - W) % 4 or 4, "pitch-odd": (1 - W) % 2 or 2}[pitch]
    pad_hr = {"pitch-0-mod-4": 4, "pitch-2-mod-4": 2, "pitch-odd": 3}[pitch]
    big_lr = rng.integers(0, 256, (2, 3, H + 2, W + pad, 3), dtype=np.uint8)
    big_hr = rng.integers(0, 256, (2, 3, s * H + 2, s * W + pad_hr, 3), dtype=np.uint8)
    lr_np, hr_np = big_lr[:, :, 1:1 + H, 1:1 + W], big_hr[:, :, 1:1 + s * H, 1:1 + s * W]
    lr, hr = window(dev(big_lr, layout), layout, 1, 1, H, W), window(dev(big_hr, layout), layout, 1, 1, s * H, s * W)
    row = 0 if layout == "interleaved" else 1
    assert (lr.stride(2 + row) % 4 == 0) == (pitch == "pitch-0-mod-4") and (hr.stride(2 + row) % 4 == 0) == (pitch == "pitch-0-mod-4")
    store = batches.FrameStore(hr, lr, s)
    origins = [(0, 0), (H - ch, W - cw), (min(1, H - ch), min(3, W - cw))]   # the last: odd, so 3 x0 and 12 x0 + 3 are no multiples of 4
    clip, frames, y0, x0, flags = [], [], [], [], []
    for k, (f, (oy, ox)) in enumerate((f, o) for f in flagset for o in origins):
        clip.append(k % 2), frames.append([k % 3, (k + 1) % 3]), y0.append(oy), x0.append(ox), flags.append(f)
    check_all_forms(store, plan_of(clip, frames, y0, x0, flags, c), hr_np, lr_np)


def small_store(layout="interleaved", clips=4, frames=5, H=12, W=14, s=4, seed=1, bgr=True):
    from vmg_amd import batches
    rng = np.random.default_rng(seed)
    lr_np = rng.integers(0, 256, (clips, frames, H, W, 3), dtype=np.uint8)
    hr_np = rng.integers(0, 256, (clips, frames, s * H, s * W, 3), dtype=np.uint8)
    return batches.FrameStore(dev(hr_np, layout), dev(lr_np, layout), s, bgr=bgr), hr_np, lr_np


MIXED = dict(clip=[3, 0, 2, 1], y0=[0, 3, 1, 4], x0=[5, 0, 3, 6], flags=[5, 2, 7, 0])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_mixed_batch_reverse_and_mirrors(layout):
    """B = 4 samples with four different descriptors out of four different clips in one call; T = 3 forward and reversed, and the mirrored
    T' = 6: every (sample, frame) has its own pointer and the sample's descriptor."""
    store, hr_np, lr_np = small_store(layout)
    check_all_forms(store, plan_of(frames=[[1, 2, 3], [4, 3, 2], [0, 1, 2], [2, 1, 0]], crop=8, **MIXED), hr_np, lr_np)
    check_all_forms(store, plan_of(frames=[[1, 2, 3, 3, 2, 1], [4, 3, 2, 2, 3, 4], [0, 1, 2, 2, 1, 0], [2, 1, 0, 0, 1, 2]], crop=8, **MIXED), hr_np, lr_np)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_separate_allocations_and_strided_views_are_read_in_place(layout):
    from vmg_amd import batches
    rng = np.random.default_rng(2)
    s, H, W = 2, 10, 12
    # a list of per-clip tensors, each its own allocation, of different lengths
    lr_np = [rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8) for n in (3, 5, 4)]
    hr_np = [rng.integers(0, 256, (n, s * H, s * W, 3), dtype=np.uint8) for n in (3, 5, 4)]
    store = batches.FrameStore([dev(a, layout) for a in hr_np], [dev(a, layout) for a in lr_np], s)
    assert len({c.untyped_storage().data_ptr() for c in store.lr.clips}) == 3
    plan = plan_of(clip=[1, 2, 0], frames=[[4, 0], [3, 1], [2, 0]], y0=[0, 1, 2], x0=[1, 4, 0], flags=[4, 3, 6], crop=8)
    check_all_forms(store, plan, hr_np, lr_np)
    # every second frame of a larger tensor, a window of larger frames
    big_lr = rng.integers(0, 256, (2, 8, H + 3, W + 5, 3), dtype=np.uint8)
    big_hr = rng.integers(0, 256, (2, 8, s * H + 3, s * W + 5, 3), dtype=np.uint8)
    d_lr, d_hr = dev(big_lr, layout), dev(big_hr, layout)
    lr, hr = window(d_lr[:, 1::2], layout, 2, 3, H, W), window(d_hr[:, 1::2], layout, 1, 2, s * H, s * W)
    assert not lr.is_contiguous() and lr.shape[1] == 4
    store = batches.FrameStore(hr, lr, s)
    plan = plan_of(clip=[1, 0], frames=[[3, 0, 2], [1, 2, 3]], y0=[2, 0], x0=[4, 1], flags=[7, 1], crop=8)
    check_all_forms(store, plan, big_hr[:, 1::2, 1:1 + s * H, 2:2 + s * W], big_lr[:, 1::2, 2:2 + H, 3:3 + W])
    assert torch.equal(d_lr.cpu(), dev(big_lr, layout).cpu())   # the store was only read


def test_channel_order():
    """bgr=True: output channel k is stored channel 2 - k; bgr=False: k."""
    from vmg_amd import batches
    plan = plan_of(frames=[[0, 1]] * 4, crop=8, **MIXED)
    store, hr_np, lr_np = small_store(bgr=True)
    check_all_forms(store, plan, hr_np, lr_np, bgr=True)
    keep, _, _ = small_store(bgr=False)
    check_all_forms(keep, plan, hr_np, lr_np, bgr=False)
    a, b = batches.assemble(store, plan, torch.uint8), batches.assemble(keep, plan, torch.uint8)
    assert torch.equal(a[0], b[0].flip(2)) and torch.equal(a[1], b[1].flip(2)) and not torch.equal(a[1], b[1])


def test_out_buffers_are_written_in_place_or_refused():
    from vmg_amd import batches
    from vmg_amd.hip import HipError
    store, hr_np, lr_np = small_store()
    plan = plan_of(frames=[[0, 1, 2]] * 4, crop=8, **MIXED)
    for dt in (torch.uint8, torch.float32, torch.bfloat16):
        want = batches.assemble(store, plan, dt)
        lrs = torch.zeros((4, 3, 3, 8, 8), dtype=dt, device="cuda")
        hrs = torch.zeros((4, 3, 3, 32, 32), dtype=dt, device="cuda")
        pl, ph = lrs.data_ptr(), hrs.data_ptr()
        got = batches.assemble(store, plan, dt, out=(lrs, hrs))
        assert got[0] is lrs and got[1] is hrs and (lrs.data_ptr(), hrs.data_ptr()) == (pl, ph)
        assert torch.equal(lrs, want[0]) and torch.equal(hrs, want[1])
    ok_l, ok_h = torch.zeros((4, 3, 3, 8, 8), device="cuda"), torch.zeros((4, 3, 3, 32, 32), device="cuda")
    for bad in ((ok_l, ok_h[:, :2]), (ok_l.bfloat16(), ok_h), (ok_l, ok_h.cpu()), (ok_l,), ok_l, (ok_l, torch.zeros((4, 3, 32, 3, 32), device="cuda").transpose(2, 3)),
                (ok_l, torch.zeros((4, 3, 3, 32, 33), device="cuda")[..., :32])):
        with pytest.raises(HipError, match="out"):
            batches.assemble(store, plan, torch.float32, out=bad)
    torch.cuda.synchronize()
    assert not ok_l.any() and not ok_h.any()


def test_batches_yields_what_the_trainer_takes():
    import random
    from vmg_amd import batches
    meta, z = R.fixture()
    case = meta["cases"][0]
    store = batches.FrameStore(dev(z["hr"], "interleaved"), dev(z["lr"], "interleaved"), meta["scale"])
    got = list(batches.batches(store, case["cfg"], [case["indices"], [1, 0]], py_random=random.Random(case["seed"]), keys=meta["keys"]["REDS"]))
    assert len(got) == 2 and set(got[0]) == {"LRs", "HRs", "key"} and got[1]["key"] == ["001", "000"]
    assert same_bits(got[0]["LRs"], ref(z[case["name"] + "/LRs"])) and same_bits(got[0]["HRs"], ref(z[case["name"] + "/HRs"]))
    assert tuple(got[1]["HRs"].shape) == (2, 3, 3, 16, 16)


def test_from_hr_makes_the_lr_side_with_bicubic_lr():
    from vmg_amd import batches, degrade
    rng = np.random.default_rng(4)
    hr = dev(rng.integers(0, 256, (2, 3, 32, 48, 3), dtype=np.uint8), "interleaved")
    store = batches.FrameStore.from_hr(hr, 4)
    assert (store.lr.H, store.lr.W) == (8, 12) and len(store) == 2
    lrs, hrs = batches.assemble(store, plan_of(clip=[1], frames=[[2, 0]], y0=[0], x0=[0], flags=[0], crop=8), torch.uint8)
    assert torch.equal(lrs[0], degrade.bicubic_lr(hr[1], 4)[[2, 0]][:, [2, 1, 0]][..., :8, :8])
    assert torch.equal(hrs[0], hr[1][[2, 0]].permute(0, 3, 1, 2)[:, [2, 1, 0]][..., :32, :32])


def test_two_calls_return_identical_bits():
    from vmg_amd import batches
    store, _, _ = small_store("planar", H=40, W=44)
    plan = plan_of(frames=[[0, 1, 2, 3]] * 4, crop=36, clip=[3, 0, 2, 1], y0=[0, 3, 1, 4], x0=[5, 0, 3, 8], flags=[5, 2, 7, 0])
    for dt in (torch.uint8, torch.float32, torch.bfloat16):
        first = batches.assemble(store, plan, dt)
        torch.empty(1 << 22, dtype=torch.uint8, device="cuda").fill_(0xA5)  # other work on the device in between
        second = batches.assemble(store, plan, dt)
        for a, b in zip(first, second):
            assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_calls_in_a_row_do_not_share_their_tables():
    """Ten plans enqueued without a synchronise in between: a later call must not overwrite the staged tables of an earlier one."""
    from vmg_amd import batches
    store, hr_np, lr_np = small_store(frames=5)
    plans = [plan_of(clip=[k % 4, (k + 1) % 4], frames=[[k % 5, (k + 2) % 5]] * 2, y0=[k % 5, 0], x0=[0, k % 7], flags=[k % 8, (k + 3) % 8], crop=8) for k in range(10)]
    got = [batches.assemble(store, p, torch.uint8) for p in plans]
    for p, (lrs, hrs) in zip(plans, got):
        wl, wh = R.batch(hr_np, lr_np, p, 4, True, as_bytes=True)
        assert np.array_equal(lrs.cpu().numpy(), wl) and np.array_equal(hrs.cpu().numpy(), wh)


def raw_tables(store, plan):
    """Device tables of the LR side for a direct call of the entry."""
    side = store.lr
    ptr = (side.base[plan.clip][:, None] + plan.frames * side.fstride[plan.clip][:, None]).reshape(-1)
    flags = plan.hflip.astype(np.int32) + 2 * plan.vflip + 4 * plan.rot
    desc = np.stack([np.repeat(a, plan.frames.shape[1]) for a in (plan.y0, plan.x0, flags)], axis=1).astype(np.int32)
    return torch.from_numpy(ptr).cuda(), torch.from_numpy(desc).cuda()


@pytest.mark.parametrize("dt", [torch.uint8, torch.float32, torch.bfloat16])
def test_the_entry_writes_no_byte_past_its_output(dt):
    from vmg_amd import kernels as K
    store, hr_np, lr_np = small_store(H=37, W=41)
    plan = plan_of(frames=[[0, 1]] * 4, crop=33, clip=[3, 0, 2, 1], y0=[0, 3, 1, 4], x0=[5, 0, 3, 8], flags=[5, 2, 7, 0])
    ptr, desc = raw_tables(store, plan)
    n = 8 * 3 * 33 * 33
    es = torch.empty((), dtype=dt).element_size()
    buf = torch.full(((n + 4099) * es,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[:n * es].view(dt)
    K.crop_batch(ptr, store.lr.strides, desc, 37, 41, 33, 33, True, out)
    want = want_forms(R.batch(hr_np, lr_np, plan, 4, True, as_bytes=True)[0])[dt]
    assert torch.equal(out.cpu().view(torch.uint8), want.reshape(-1).view(torch.uint8))
    assert bool((buf[n * es:] == 0xA5).all())


def test_python_layer_refusals():
    from vmg_amd import batches
    from vmg_amd.hip import HipError
    store, hr_np, lr_np = small_store()   # 4 clips x 5 frames, LR 12 x 14, x4
    good = dict(clip=[0], frames=[[0, 1]], y0=[0], x0=[0], flags=[0], crop=8)
    for change, word in ((dict(clip=[4]), "clip index"), (dict(clip=[-1]), "clip index"), (dict(frames=[[0, 5]]), "frame index"), (dict(frames=[[-1, 0]]), "frame index"),
                         (dict(y0=[5]), "origin"), (dict(x0=[7]), "origin"), (dict(y0=[-1]), "origin"), (dict(crop=0), "crop"),
                         (dict(crop=13, flags=[4]), "rot"), (dict(y0=[0, 1]), "one entry per sample")):
        with pytest.raises(HipError, match=word):
            batches.assemble(store, plan_of(**dict(good, **change)))
    batches.assemble(store, plan_of(**dict(good, crop=13, flags=[3])))   # 12 x 13, no rot: fine
    with pytest.raises(HipError, match="dtype"):
        batches.assemble(store, plan_of(**good), dtype=torch.float16)
    with pytest.raises(HipError, match="BatchPlan"):
        batches.assemble(store, good)
    lr, hr = dev(lr_np, "interleaved"), dev(hr_np, "interleaved")
    for args, word in (((hr.cpu(), lr, 4), "no CPU path"), ((hr, lr.cpu(), 4), "no CPU path"), ((hr.float(), lr, 4), "uint8"), ((hr, lr, 2), "hr frames / 2"),
                       ((hr, lr[:3], 4), "differ in their clips"), ((hr, lr[:, :4], 4), "differ in their clips"), ((hr[0], lr[0], 4), "clips, frames"),
                       ((hr, lr, 0), "scale"), ((hr, [lr[0], lr[1, :, :, :7]], 4), "frame size"), ((hr, lr[..., :2], 4), "channel axis"),
                       ((hr, [lr[0], lr[1].permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), lr[2], lr[3]], 4), "strides")):
        with pytest.raises(HipError, match=word):
            batches.FrameStore(*args)


def test_the_entry_point_refuses_by_itself():
    """Below the Python checks: vmg_crop_batch returns an error, names the reason and launches nothing (the output keeps its bytes)."""
    from vmg_amd import hip
    store, _, _ = small_store()
    plan = plan_of(clip=[0], frames=[[0, 1]], y0=[0], x0=[0], flags=[0], crop=8)
    ptr, desc = raw_tables(store, plan)
    out = torch.full((2 * 3 * 8 * 8 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    strides = (ctypes.c_int64 * 3)(*store.lr.strides)
    lib = hip.lib()
    good = dict(frames=ptr.data_ptr(), strides=strides, desc=desc.data_ptr(), N=2, H=12, W=14, ch=8, cw=8, crev=1, out_type=0, out=out.data_ptr())

    def call(**change):
        a = dict(good, **change)
        rc = lib.vmg_crop_batch(a["frames"], a["strides"], a["desc"], a["N"], a["H"], a["W"], a["ch"], a["cw"], a["crev"], a["out_type"], a["out"], hip.stream_ptr())
        return rc, lib.vmg_last_error().decode()

    for change, word in ((dict(frames=None), "null"), (dict(strides=None), "null"), (dict(desc=None), "null"), (dict(out=None), "null"),
                         (dict(N=0), "at least one"), (dict(N=-3), "at least one"), (dict(ch=0), "empty"), (dict(cw=-1), "empty"),
                         (dict(ch=13), "larger"), (dict(cw=15), "larger"), (dict(out_type=3), "output type"), (dict(out_type=-1), "output type"),
                         (dict(out_type=1, out=out.data_ptr() + 2), "misaligned"), (dict(strides=(ctypes.c_int64 * 3)(42, 3, -1)), "negative"),
                         (dict(N=1 << 24), "tiles")):
        rc, msg = call(**change)
        assert rc != 0 and word in msg, (change, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    rc, msg = call()
    torch.cuda.synchronize()
    assert rc == 0 and bool((out[:384] != 0xA5).any()) and bool((out[384:] == 0xA5).all())
