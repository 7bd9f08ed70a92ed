"""vmg_amd.degrade (vmg_bicubic_down, csrc/resize.hip) against the float64 restatement tests/lr_ref.py and against the reference's own
float32 outputs (tests/golden/lr_bicubic.npz).

Bounds (derived, not measured):
* unquantised float64 output against tests/lr_ref.py: 1e-10 absolute on the 0..255 scale.  Both evaluate the same <= 36 float64
  operations per value on magnitudes <= ~410, about 2e-12; only the order of summation differs.
* against the reference's float32 values: 1e-3 (two passes of <= 18 float32 products of magnitude <= ~330: worst case about 6e-4).
* uint8 output against rint / clamp of tests/lr_ref.py: equal at every pixel; the cases have no reference value within 1e-9 of a rounding
  tie (asserted here and, on the CPU, in tests/test_lr_ref.py).
* uint8 output against rint / clamp of the float32 reference values: equal wherever that value is more than 1e-3 from a half-integer,
  at most one level apart elsewhere, and at most 1 % of a case's values may be such.
* float32 / bfloat16 outputs: the bits of u8.float().div(255) and of .to(torch.bfloat16) of it, with the division a true one: evaluated on
  the host, where torch divides as numpy does in the dataset classes (img.astype(np.float32) / 255., data/REDS.py:116).  On the device
  torch turns a division by a Python scalar into a multiplication by 1 / 255, which is one ulp off for 126 of the 256 bytes; the first
  GPU run of this file showed exactly that difference against the kernel's correctly rounded quotient.

Worst differences measured on the MI355X (all cases of this file, WORST_MEASURED below): float64 output against tests/lr_ref.py 0 at x2
and x4 (dyadic weights and integer pixels: every float64 sum is exact) and 3.4e-13 at x3; against the reference's float32 values 4.8e-5
(edges x3); at most 0.74 % of a fixture case's values lie within 1e-3 of a tie (noise x4) and no byte differs from the rounded reference
value, there or elsewhere.  Every case prints its differences before it asserts (run with -s).
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import lr_cases as C
from tests import lr_ref as R

pytestmark = pytest.mark.gpu
TOL_F64, TOL_VS_REFERENCE, TIE_BAND_REFERENCE, TIE_SHARE_CAP = 1e-10, 1e-3, 1e-3, 0.01
# measured on the MI355X (all cases of this file): worst |float64 output - tests/lr_ref.py|, worst |float64 output - reference float32|,
# largest share of a fixture case's values left out of the byte comparison, bytes that differ from the float32 reference's rounding
WORST_MEASURED = {"f64_vs_restatement": 3.411e-13, "f64_vs_reference": 4.835e-05, "tie_share": 0.00741, "bytes_off_by_one": 0}
LAYOUTS = ["planar", "interleaved"]


def dev(frames, layout):
    """(T, H, W, 3) numpy -> device tensor, interleaved as it is or planar (T, 3, H, W)."""
    t = torch.from_numpy(np.array(frames)).cuda()   # a copy: the cases are shared and read-only
    return t if layout == "interleaved" else t.permute(0, 3, 1, 2).contiguous()


def host(lr):
    """planar device (T, 3, h, w) -> numpy (T, h, w, 3)."""
    return lr.permute(0, 2, 3, 1).cpu().numpy()


def check_against_restatement(what, hr_dev, s, ref):
    """All four output forms of one input against the float64 reference values `ref` (T, h, w, 3)."""
    from vmg_amd import degrade
    assert float(R.half_integer_distance(ref).min()) > C.TIE_BAND, "the case has a rounding tie: pick other inputs"
    f64 = degrade.bicubic_lr(hr_dev, s, out=torch.float64)
    u8 = degrade.bicubic_lr(hr_dev, s, out=torch.uint8)
    f32 = degrade.bicubic_lr(hr_dev, s, out=torch.float32)
    b16 = degrade.bicubic_lr(hr_dev, s, out=torch.bfloat16)
    shape = (ref.shape[0], 3, ref.shape[1], ref.shape[2])
    for t, dt in ((f64, torch.float64), (u8, torch.uint8), (f32, torch.float32), (b16, torch.bfloat16)):
        assert t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.is_cuda
    d = float(np.abs(host(f64) - ref).max())
    wrong = int((host(u8) != R.to_uint8(ref)).sum())
    print(f"{what}: max |f64 - restatement| = {d:.3e}; bytes that differ: {wrong} of {ref.size}")
    assert d <= TOL_F64
    assert wrong == 0
    want32 = u8.cpu().float().div(255)     # on the host: a true division (see the module docstring)
    assert np.array_equal(want32.numpy().view(np.int32), (u8.cpu().numpy().astype(np.float32) / 255.).view(np.int32))  # data/REDS.py:116
    assert torch.equal(f32.cpu().view(torch.int32), want32.view(torch.int32))
    assert torch.equal(b16.cpu().view(torch.int16), want32.to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", list(C.CASES))
def test_all_output_forms_match_the_restatement(cid, layout):
    s, hr, ref = C.case(cid)
    check_against_restatement(f"{cid}/{layout}", dev(hr, layout), s, ref)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fixture_frames_match_the_reference_outputs(layout):
    from vmg_amd import degrade
    meta, z = C.fixture()
    seen_clamped = 0
    for name, s in meta["cases"]:
        hr, want = z[name + "/hr"], z[f"{name}/x{s}"].astype(np.float64)
        d_hr = dev(hr[None], layout)
        f64 = host(degrade.bicubic_lr(d_hr, s, out=torch.float64))[0]
        u8 = host(degrade.bicubic_lr(d_hr, s, out=torch.uint8))[0].astype(np.int32)
        d = float(np.abs(f64 - want).max())
        near_tie = R.half_integer_distance(want) <= TIE_BAND_REFERENCE
        diff = np.abs(u8 - R.to_uint8(want).astype(np.int32))
        print(f"{name} x{s}/{layout}: max |f64 - reference| = {d:.3e}; near a tie: {near_tie.mean():.3%}; bytes off by one there: {int((diff[near_tie] != 0).sum())}")
        assert d <= TOL_VS_REFERENCE
        assert near_tie.mean() <= TIE_SHARE_CAP
        assert int(diff[~near_tie].max(initial=0)) == 0
        assert int(diff[near_tie].max(initial=0)) <= 1
        if name in meta["clamped"]:
            assert want.min() < -0.5 and want.max() > 255.5 and (u8 == 0).any() and (u8 == 255).any()
            assert np.array_equal(u8[want < -0.5], np.zeros_like(u8[want < -0.5])) and np.array_equal(u8[want > 255.5], np.full_like(u8[want > 255.5], 255))
            seen_clamped += 1
    assert seen_clamped >= 3


@pytest.mark.parametrize("pad", [(8, 8), (8, 6), (5, 7)], ids=["rows-4-apart", "rows-2-apart", "odd"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_frames_cut_from_a_larger_batch(layout, pad):
    """T = 5 (every second frame) of a 12-frame batch, a window of larger frames: a non-contiguous view, read in place.  The paddings make
    the rows of the view start 4-byte-congruent at an odd offset (dword fetch from a misaligned start), or not congruent (byte fetch)."""
    H, W, s = 40, 52, 4
    rng = np.random.default_rng(11)
    big = np.stack([C.synth_hr(H + pad[0], W + pad[1], 500 + i) for i in range(12)])
    big[:, :, :3] = rng.integers(0, 256, big[:, :, :3].shape, dtype=np.uint8)  # what lies left of the window must not leak in
    d_big = dev(big, layout)
    frames, y0, x0 = slice(2, 12, 2), 3, 2
    view = d_big[frames, :, y0:y0 + H, x0:x0 + W] if layout == "planar" else d_big[frames, y0:y0 + H, x0:x0 + W, :]
    assert not view.is_contiguous() and view.data_ptr() != d_big.data_ptr() and view.shape[0] == 5
    ref = np.stack([R.bicubic_down(f, s) for f in big[frames, y0:y0 + H, x0:x0 + W]])
    check_against_restatement(f"window/{layout}/{pad}", view, s, ref)


def test_one_frame_and_channel_order():
    """A single (3, H, W) / (H, W, 3) frame is a batch of one; the filter is per channel, so reversed channels in give reversed channels out."""
    from vmg_amd import degrade
    s, hr, ref = C.case("x4-64x96")
    one = degrade.bicubic_lr(torch.from_numpy(hr[0].copy()).cuda(), s)
    assert tuple(one.shape) == (1, 3, 16, 24) and np.array_equal(host(one)[0], R.to_uint8(ref[0]))
    planar = torch.from_numpy(hr[0].copy()).cuda().permute(2, 0, 1)
    assert torch.equal(degrade.bicubic_lr(planar, s), one)
    assert torch.equal(degrade.bicubic_lr(planar.flip(0).contiguous(), s), one.flip(1))


def test_lr_clip_is_what_the_network_takes():
    from vmg_amd import degrade
    s, hr, _ = C.case("x4-64x96")
    frames = dev(np.concatenate([hr, hr[::-1], hr]), "planar")        # 6 frames
    want = degrade.bicubic_lr(frames, s).cpu().float().div(255).cuda()    # divided on the host: a true division
    clip = degrade.lr_clip(frames, s)
    assert clip.dtype == torch.float32 and tuple(clip.shape) == (1, 6, 3, 16, 24) and clip.is_contiguous() and torch.equal(clip[0], want)
    assert torch.equal(degrade.lr_clip(frames.permute(0, 2, 3, 1).contiguous(), s), clip)      # interleaved frames
    batch = frames.view(2, 3, 3, 64, 96)
    got = degrade.lr_clip(batch, s, dtype=torch.bfloat16)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (2, 3, 3, 16, 24) and got.is_contiguous()
    assert torch.equal(got, want.to(torch.bfloat16).view(2, 3, 3, 16, 24))
    strided = frames.view(2, 3, 3, 64, 96)[:, ::2]                                              # (2, 2, ...): no (B*T) view exists
    assert torch.equal(degrade.lr_clip(strided, s), want.view(2, 3, 3, 16, 24)[:, ::2])
    assert float(clip.min()) == 0.0 and float(clip.max()) == 1.0


def test_two_calls_return_identical_bits():
    from vmg_amd import degrade
    s, hr, _ = C.case("x4-148x212")
    a = dev(hr, "interleaved")
    for out in (torch.float64, torch.uint8, torch.bfloat16):
        first = degrade.bicubic_lr(a, s, out=out)
        torch.empty(1 << 22, dtype=torch.uint8, device="cuda").fill_(0xA5)  # other work on the device in between
        second = degrade.bicubic_lr(a, s, out=out)
        assert first.data_ptr() != second.data_ptr()
        assert torch.equal(first.view(torch.uint8), second.view(torch.uint8))


def test_crop_to_scale_is_a_view():
    from vmg_amd import degrade
    planar = torch.zeros(2, 3, 50, 70, dtype=torch.uint8, device="cuda")
    inter = torch.zeros(2, 50, 70, 3, dtype=torch.uint8, device="cuda")
    for s, (h, w) in ((4, (48, 68)), (3, (48, 69)), (2, (50, 70))):
        p, i = degrade.crop_to_scale(planar, s), degrade.crop_to_scale(inter, s)
        assert tuple(p.shape) == (2, 3, h, w) and p.data_ptr() == planar.data_ptr() and p.stride() == planar.stride()
        assert tuple(i.shape) == (2, h, w, 3) and i.data_ptr() == inter.data_ptr() and i.stride() == inter.stride()
    assert tuple(degrade.crop_to_scale(planar[0], 4).shape) == (3, 48, 68)
    assert tuple(degrade.crop_to_scale(planar.view(1, 2, 3, 50, 70), 4).shape) == (1, 2, 3, 48, 68)
    assert tuple(degrade.bicubic_lr(degrade.crop_to_scale(planar, 4), 4).shape) == (2, 3, 12, 17)


def test_refusals():
    from vmg_amd import degrade
    from vmg_amd.hip import HipError
    ok = torch.zeros(3, 32, 32, dtype=torch.uint8, device="cuda")
    for scale in (1, 5, 0, 2.5):
        with pytest.raises(HipError, match="scale"):
            degrade.bicubic_lr(ok, scale)
        with pytest.raises(HipError, match="scale"):
            degrade.crop_to_scale(ok, scale)
    with pytest.raises(HipError, match="crop_to_scale"):
        degrade.bicubic_lr(torch.zeros(3, 50, 70, dtype=torch.uint8, device="cuda"), 4)
    with pytest.raises(HipError, match="smaller"):
        degrade.bicubic_lr(torch.zeros(3, 12, 64, dtype=torch.uint8, device="cuda"), 4)
    with pytest.raises(HipError, match="smaller"):
        degrade.bicubic_lr(torch.zeros(3, 64, 12, dtype=torch.uint8, device="cuda"), 4)
    with pytest.raises(HipError, match="uint8"):
        degrade.bicubic_lr(ok.float(), 4)
    with pytest.raises(HipError, match="device tensor"):
        degrade.bicubic_lr(ok.cpu(), 4)
    with pytest.raises(HipError, match="length 3"):
        degrade.bicubic_lr(torch.zeros(4, 32, 32, dtype=torch.uint8, device="cuda"), 4)
    with pytest.raises(HipError, match="out must be"):
        degrade.bicubic_lr(ok, 4, out=torch.float16)
    with pytest.raises(HipError, match="dtype"):
        degrade.lr_clip(ok, 4, dtype=torch.uint8)


def test_the_entry_point_refuses_by_itself():
    """Below the Python checks: vmg_bicubic_down returns an error, names the reason and launches nothing (the output keeps its bytes)."""
    from vmg_amd import hip
    from vmg_amd import kernels as K
    lib = hip.lib()
    src = torch.zeros(1, 3, 50, 64, dtype=torch.uint8, device="cuda")
    out = torch.full((1, 3, 16, 16), 7, dtype=torch.uint8, device="cuda")
    strides = (ctypes.c_int64 * 4)(*src.stride())

    def call(ptr, st, H, W, scale, out_ptr=out.data_ptr(), out_type=0):
        return lib.vmg_bicubic_down(ptr, st, 1, H, W, scale, out_type, out_ptr, hip.stream_ptr()), lib.vmg_last_error().decode()

    for args, word in (((src.data_ptr(), strides, 48, 64, 1), "scale"), ((src.data_ptr(), strides, 48, 64, 5), "scale"),
                       ((src.data_ptr(), strides, 50, 64, 4), "multiple"), ((src.data_ptr(), strides, 48, 62, 4), "multiple"),
                       ((src.data_ptr(), strides, 12, 64, 4), "smaller"), ((src.data_ptr(), strides, 48, 12, 4), "smaller"),
                       ((None, strides, 48, 64, 4), "null"), ((src.data_ptr(), None, 48, 64, 4), "null"),
                       ((src.data_ptr(), strides, 48, 64, 4, None), "null"), ((src.data_ptr(), strides, 48, 64, 4, out.data_ptr(), 9), "output type")):
        rc, msg = call(*args)
        assert rc != 0 and word in msg, (args[2:], rc, msg)
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    with pytest.raises(hip.HipError, match="multiple"):
        K.bicubic_down(src, 4)
