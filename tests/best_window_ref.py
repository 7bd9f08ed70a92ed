"""Numpy restatement of the reference's best-window selection (tools/Tester.py:180-213 with psnr_exceed_check :24-34 and skimage's
peak_signal_noise_ratio on clamped float images) and of Tester.evaluate for REDS (:215-252) -- TEST INFRASTRUCTURE ONLY.

Four pieces, each as the streamed GPU path (vmg_amd.infer.best_window_clips) has to reproduce them:
  frame_err        float64 mean of (clamp(out) - clamp(hr))^2, clamped in float32; uint8 HR read as astype(float32) / 255.
  score            float32 of 10 log10(1 / err), the cap where err == 0 (the reference stores its scores in a float32 table)
  select_table     torch.max's first maximum over the (T, n_windows) table whose uncovered entries are 0
  select_streaming the same decision taken window by window: window 0 always, later ones only on a strictly higher score
and the test cases both test files share.  No torch device code.
"""
from __future__ import annotations

import functools
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

CAP = float(10 * np.log10(255.0 ** 2 / 0.65025))
TIE_GAP_DB = 1e-3  # every test input keeps its best and second-best covered score of a frame at least this far apart


def tile_starts(total: int, size: int, overlap: int) -> List[int]:
    stride = size - overlap
    return list(range(0, total - size, stride)) + [max(0, total - size)]


def as_unit(hr_u8: np.ndarray) -> np.ndarray:
    """Tester.evaluate: HR.astype(np.float32) / 255., (..., h, w, 3) -> (..., 3, h, w)."""
    return np.ascontiguousarray(np.moveaxis(hr_u8.astype(np.float32) / 255., -1, -3))


def frame_err(out: np.ndarray, hr: np.ndarray) -> float:
    """out (C, h, w) float32; hr (C, h, w) float32 or (h, w, 3) uint8."""
    a = np.clip(np.asarray(out, dtype=np.float32), 0, 1)
    b = as_unit(hr) if hr.dtype == np.uint8 else np.clip(np.asarray(hr, dtype=np.float32), 0, 1)
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2, dtype=np.float64))


def score(err: float, dtype=np.float32):
    with np.errstate(divide="ignore"):
        return dtype(CAP if err == 0 else 10 * np.log10(1.0 / err))


def score_table(errs: Sequence[np.ndarray], ts: Sequence[int], T: int, dtype=np.float32) -> np.ndarray:
    """errs[k][i] = error of frame ts[k] + i in window k -> (T, n_windows) scores, 0 where a window does not cover a frame."""
    table = np.zeros((T, len(ts)), dtype=dtype)
    for k, (t, e) in enumerate(zip(ts, errs)):
        for i, v in enumerate(e):
            table[t + i, k] = score(float(v), dtype)
    return table


def select_table(table: np.ndarray) -> np.ndarray:
    """torch.max(psnrs, dim=-1)'s index: the first maximum."""
    return np.argmax(table, axis=1).astype(np.int32)


def gather(outs: Sequence[np.ndarray], ts: Sequence[int], choice: np.ndarray, T: int) -> np.ndarray:
    """The reference's gather over its (T, n_windows, ...) canvas of zeros + outputs."""
    frames = np.zeros((T,) + tuple(outs[0].shape[1:]), dtype=np.float32)
    for t in range(T):
        k = int(choice[t])
        i = t - ts[k]
        if 0 <= i < outs[k].shape[0]:
            frames[t] = outs[k][i]
    return frames


def select_streaming(outs: Sequence[np.ndarray], errs: Sequence[np.ndarray], ts: Sequence[int], T: int, strict: bool = True, dtype=np.float32):
    """Window by window over one canvas.  strict / dtype exist so that the tests can show what a wrong rule (>=, float64 scores) changes."""
    frames = np.zeros((T,) + tuple(outs[0].shape[1:]), dtype=np.float32)
    best, choice = np.zeros(T, dtype=dtype), np.zeros(T, dtype=np.int32)
    for k, (t0, out, e) in enumerate(zip(ts, outs, errs)):
        for i in range(out.shape[0]):
            s = score(float(e[i]), dtype)
            if k == 0 or (s > best[t0 + i] if strict else s >= best[t0 + i]):
                frames[t0 + i], best[t0 + i], choice[t0 + i] = out[i], s, k
    return frames, best, choice


def window_errs(outs: Sequence[np.ndarray], ts: Sequence[int], hr: np.ndarray) -> List[np.ndarray]:
    """hr: (T, C, h, w) float32 or (T, h, w, 3) uint8."""
    return [np.array([frame_err(o[i], hr[t + i]) for i in range(o.shape[0])], dtype=np.float64) for t, o in zip(ts, outs)]


def tie_gap(table: np.ndarray, ts: Sequence[int], nf: int) -> float:
    """Smallest distance in dB, over the frames, between the best and the second-best score of the windows that cover the frame."""
    gap = np.inf
    for t in range(table.shape[0]):
        cov = sorted((float(table[t, k]) for k, t0 in enumerate(ts) if t0 <= t < t0 + nf), reverse=True)
        if len(cov) > 1:
            gap = min(gap, cov[0] - cov[1])
    return gap


# ---- Tester.evaluate, REDS branch --------------------------------------------------------------------------------------------------
def augment(clip: torch.Tensor, hflip: bool, vflip: bool, rot90: bool) -> torch.Tensor:
    """Tester.augment == Tester.augment_inverse (tools/Tester.py:387-445), frame by frame on numpy views like the reference."""
    def one(img):
        if hflip:
            img = img[..., ::-1]
        if vflip:
            img = img[..., ::-1, :]
        if rot90:
            img = np.swapaxes(img, -1, -2)
        return torch.from_numpy(np.ascontiguousarray(img)).float()
    return torch.cat([one(f.numpy()) for f in torch.chunk(clip, clip.shape[-4], dim=-4)], dim=-4)


def evaluate_reds(model: Callable, lr_u8: np.ndarray, hr_u8: np.ndarray, num_frames: int, overlap_frames: int, test_spatial=None, overlap_spatial=None,
                  scale: int = 4, hflip: bool = False, vflip: bool = False, rot90: bool = False) -> np.ndarray:
    """(T, H, W, 3) and (T, 4H, 4W, 3) uint8 -> (T, 4H, 4W, 3) uint8.  The selection itself is the oracle's test_clips_max."""
    from oracle import infer_oracle as IO
    x = torch.from_numpy(lr_u8.astype(np.float32) / 255.).permute(0, 3, 1, 2).contiguous().unsqueeze(0)
    hr = torch.from_numpy(hr_u8.astype(np.float32) / 255.).permute(0, 3, 1, 2).contiguous().unsqueeze(0)
    enhance = hflip or vflip or rot90
    if enhance:
        x, hr = augment(x, hflip, vflip, rot90), augment(hr, hflip, vflip, rot90)
    out = IO.test_clips_max(model, x, hr, num_frames, overlap_frames, test_spatial, overlap_spatial, scale)
    if enhance:
        out = augment(out, hflip, vflip, rot90)
    return IO.to_uint8(out)


# ---- shared cases ------------------------------------------------------------------------------------------------------------------
class Recorder:
    """Wraps the oracle-side model: keeps every call's input and output so that the GPU side can replay the identical numbers.
    round_bf16: the outputs are rounded to bf16 values (kept as fp32), what a bf16 network hands to an fp32 oracle."""

    def __init__(self, model, round_bf16: bool = False):
        self.model, self.round_bf16, self.ins, self.outs = model, round_bf16, [], []

    def __call__(self, x):
        o = self.model(x)
        if self.round_bf16:
            o = o.bfloat16().float()
        self.ins.append(x.clone())
        self.outs.append(o.clone())
        return o


def _hr_for(x: torch.Tensor, seed: int) -> torch.Tensor:
    from oracle import recipe as R
    up = x.repeat_interleave(4, -2).repeat_interleave(4, -1)
    return 0.5 * up + 0.2 + R.seeded(up.shape, seed, 0.05)


def _clip_case(T, H, W, seed, nf, of, spatial=None, ov=None, bf16=False):
    def make():
        from oracle import recipe as R
        x = R.seeded((1, T, 3, H, W), seed, 0.3) + 0.5
        hr = _hr_for(x, seed + 1)
        if bf16:
            x, hr = x.bfloat16().float(), hr.bfloat16().float()
        return dict(x=x, hr=hr, nf=nf, of=of, spatial=spatial, ov=ov, bf16=bf16)
    return make


def _fixture_case():
    from oracle import cases as C
    inp = C.CASES["infer_clips_max"]["inputs"]()
    return dict(x=inp["x"], hr=inp["hr"], nf=4, of=2, spatial=None, ov=None, bf16=False)


CLIP_CASES = {
    "fixture": _fixture_case,                                  # T = 9, windows of 4, overlap 2, 16 x 16 LR
    "one_window": _clip_case(5, 16, 16, 310, 5, 2),
    "t7_w3_o1": _clip_case(7, 16, 16, 320, 3, 1),
    "bf16": _clip_case(7, 16, 16, 330, 3, 1, bf16=True),
    "tiled": _clip_case(5, 20, 16, 340, 3, 1, spatial=(12, 12), ov=4),
}


@functools.lru_cache(maxsize=None)
def clip_reference(name: str):
    """The oracle's run of a case, computed once: inputs, recorded network calls, the oracle's frames."""
    from oracle import infer_oracle as IO
    case = CLIP_CASES[name]()
    rec = Recorder(IO.fake_sr_model(), round_bf16=case["bf16"])
    want = IO.test_clips_max(rec, case["x"], case["hr"], case["nf"], case["of"], case["spatial"], case["ov"], 4)
    return dict(case, rec=rec, want=want)


def window_outputs(ref) -> List[np.ndarray]:
    """The (nf, C, 4H, 4W) float32 output of every temporal window of a case (spatial tiles blended as the oracle blends them)."""
    from oracle import infer_oracle as IO
    x, nf = ref["x"], ref["nf"]
    ts = tile_starts(x.shape[1], nf, ref["of"])
    if ref["spatial"] is None:
        return [o[0].numpy() for o in ref["rec"].outs]
    per = len(ref["rec"].outs) // len(ts)
    outs = []
    for k, t in enumerate(ts):
        calls = iter(ref["rec"].outs[k * per:(k + 1) * per])
        outs.append(IO.test_image(lambda _x: next(calls).clone(), x[:, t:t + nf], ref["spatial"], ref["ov"], 4)[0].numpy())
    return outs


def u8_hr_of(name: str) -> np.ndarray:
    """The HR clip of a case as (T, 4H, 4W, 3) uint8 frames (rounded), for the form of HR that is scored in place."""
    hr = clip_reference(name)["hr"][0]
    return (hr.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()


EVAL_FLAGS = [(False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, True)]


def eval_inputs():
    """uint8 RGB clips as read_seq_images yields them: LR (5, 12, 16, 3), HR (5, 48, 64, 3)."""
    g = torch.Generator().manual_seed(350)
    lr = torch.randint(0, 256, (5, 12, 16, 3), generator=g, dtype=torch.uint8)
    up = lr.repeat_interleave(4, 1).repeat_interleave(4, 2).float()
    hr = (0.5 * up + 51.0 + 12.0 * torch.randn(up.shape, generator=g)).round().clamp(0, 255).to(torch.uint8)
    return lr.numpy(), hr.numpy()


@functools.lru_cache(maxsize=None)
def eval_reference(flags):
    from oracle import infer_oracle as IO
    lr, hr = eval_inputs()
    rec = Recorder(IO.fake_sr_model())
    want = evaluate_reds(rec, lr, hr, 3, 1, None, None, 4, *flags)
    return dict(lr=lr, hr=hr, rec=rec, want=want)
