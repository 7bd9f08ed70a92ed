"""Numpy restatement of Tester.evaluate's conversions (tools/Tester.py:215-252 with Tester.augment / augment_inverse :387-445) and of the test
driver's index lists (utils/eval_utils.py:38-61) -- TEST INFRASTRUCTURE ONLY, written the way the reference writes them:

  to_clip     frames.astype(np.float32) / 255., transpose(0, 3, 1, 2), then the three augment steps
  augment     flip the width axis, flip the height axis, swap the two -- in this order (augment_inverse is the same function)
  to_frames   the augment steps, clamp(0, 1), np.round(transpose(0, 2, 3, 1) * 255.0).astype(np.uint8)
  evaluate    the three branches of Tester.evaluate over the oracle's window functions (oracle/infer_oracle.py)

and the inputs both test files share.  No torch device code.
"""
from __future__ import annotations

import functools
import itertools
from typing import Callable, List, Optional

import numpy as np
import torch

ALL_FLAGS = list(itertools.product((False, True), repeat=3))  # (hflip, vflip, rot90)
# augment applied twice is the identity unless exactly one flip meets rot90 (then it is a rotation by 180 degrees)
UNDONE = [f for f in ALL_FLAGS if not (f[2] and f[0] != f[1])]


def augment(x: np.ndarray, hflip: bool, vflip: bool, rot90: bool) -> np.ndarray:
    """(..., H, W) planar arrays."""
    if hflip:
        x = x[..., ::-1]
    if vflip:
        x = x[..., ::-1, :]
    if rot90:
        x = np.swapaxes(x, -1, -2)
    return np.array(x, order="C", copy=True)  # (a fresh array: a flipped axis of length 1 keeps its negative stride through ascontiguousarray)


def augment_frames(frames_u8: np.ndarray, hflip: bool, vflip: bool, rot90: bool) -> np.ndarray:
    """The same steps on interleaved (T, H, W, 3) frames."""
    return np.ascontiguousarray(augment(frames_u8.transpose(0, 3, 1, 2), hflip, vflip, rot90).transpose(0, 2, 3, 1))


def to_clip(frames_u8: np.ndarray, hflip: bool = False, vflip: bool = False, rot90: bool = False) -> np.ndarray:
    """(T, H, W, 3) uint8 -> (1, T, 3, H', W') float32."""
    x = frames_u8.astype(np.float32) / 255.
    x = np.ascontiguousarray(x.transpose(0, 3, 1, 2))[None]
    return augment(x, hflip, vflip, rot90)


def to_frames(clip: np.ndarray, hflip: bool = False, vflip: bool = False, rot90: bool = False) -> np.ndarray:
    """(1, T, 3, h, w) or (T, 3, h, w) float32 -> (T, H', W', 3) uint8."""
    o = np.asarray(clip, dtype=np.float32)
    o = o[0] if o.ndim == 5 else o
    o = np.clip(augment(o, hflip, vflip, rot90), 0, 1)
    return np.round(np.ascontiguousarray(o.transpose(0, 2, 3, 1)) * 255.0).astype(np.uint8)


def evaluate(model: Callable, lr_u8: np.ndarray, hr_u8: Optional[np.ndarray] = None, dataset_name: str = "REDS", num_frames: int = 7,
             overlap_frames: int = 0, test_spatial=None, overlap_spatial=None, scale: int = 4, hflip: bool = False, vflip: bool = False,
             rot90: bool = False) -> np.ndarray:
    from oracle import infer_oracle as IO
    x = torch.from_numpy(to_clip(lr_u8, hflip, vflip, rot90))
    if dataset_name == "Vimeo90k_septuplet":
        out = model(x) if overlap_spatial is None else IO.test_image(model, x, test_spatial, overlap_spatial, scale)
    elif dataset_name == "REDS":
        hr = torch.from_numpy(to_clip(hr_u8, hflip, vflip, rot90))
        out = IO.test_clips_max(model, x, hr, num_frames, overlap_frames, test_spatial, overlap_spatial, scale)
    else:
        out = IO.test_clips(model, x, num_frames, overlap_frames, test_spatial, overlap_spatial, scale)
    out = out.numpy()
    return to_frames(out.reshape((-1,) + out.shape[-3:]), hflip, vflip, rot90)


def index_generation(num_output_frames: int, num_GT: int) -> List[List[int]]:
    indices_list = []
    right = num_output_frames
    while right <= num_GT:
        indices_list.append(list(range(right - num_output_frames, right)))
        right += num_output_frames - 1
    if right - num_output_frames < num_GT - 1:
        indices_list.append(list(range(num_GT - num_output_frames, num_GT)))
    return indices_list


# ---- shared inputs -------------------------------------------------------------------------------------------------------------------
FRAME_SIZES = [(1, 1), (5, 7), (33, 18), (31, 65), (64, 96)]  # (H, W): one pixel, less than a tile, odd sizes on both sides of it, whole tiles


def u8_frames(T: int, H: int, W: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (T, H, W, 3), dtype=np.uint8)


def unit_clip(T: int, h: int, w: int, seed: int) -> np.ndarray:
    """(T, 3, h, w) float32 spread to both sides of [0, 1]."""
    return (0.6 * np.random.default_rng(seed).standard_normal((T, 3, h, w)) + 0.5).astype(np.float32)


def half_steps() -> np.ndarray:
    """float32((k + 0.5) / 255) for k = 0 .. 254: the values whose product with 255 is a tie (where it is exactly k + 0.5)."""
    return ((np.arange(255, dtype=np.float64) + 0.5) / 255).astype(np.float32)


class Recorder:
    """Keeps every call's input and output of the oracle-side model so that the GPU side can replay the identical numbers."""

    def __init__(self, model):
        self.model, self.ins, self.outs = model, [], []

    def __call__(self, x):
        o = self.model(x)
        self.ins.append(x.clone())
        self.outs.append(o.clone())
        return o


EVAL_CASES = {
    # name: (dataset_name, T, H, W, num_frames, overlap_frames, test_spatial, overlap_spatial)
    "vimeo": ("Vimeo90k_septuplet", 7, 12, 16, 7, 0, None, None),
    "vimeo_tiled": ("Vimeo90k_septuplet", 7, 20, 16, 7, 0, (12, 12), 4),
    "vid4": ("Vid4", 7, 12, 16, 3, 1, None, None),
}


def eval_inputs(T: int, H: int, W: int, seed: int = 360):
    """uint8 RGB clips as read_seq_images yields them: LR (T, H, W, 3) and a noisy 4x HR."""
    g = torch.Generator().manual_seed(seed)
    lr = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8)
    up = lr.repeat_interleave(4, 1).repeat_interleave(4, 2).float()
    hr = (0.5 * up + 51.0 + 12.0 * torch.randn(up.shape, generator=g)).round().clamp(0, 255).to(torch.uint8)
    return lr.numpy(), hr.numpy()


@functools.lru_cache(maxsize=None)
def eval_reference(name: str, flags=(False, False, False)):
    """One run of the restatement on a case, computed once: inputs, recorded network calls, the frames."""
    from oracle import infer_oracle as IO
    ds, T, H, W, nf, of, spatial, ov = EVAL_CASES[name]
    lr, hr = eval_inputs(T, H, W)
    rec = Recorder(IO.fake_sr_model())
    want = evaluate(rec, lr, None, ds, nf, of, spatial, ov, 4, *flags)
    return dict(lr=lr, hr=hr, rec=rec, want=want, kwargs=dict(dataset_name=ds, num_frames=nf, overlap_frames=of, test_spatial=spatial,
                                                              overlap_spatial=ov, scale=4))


@functools.lru_cache(maxsize=None)
def reds_reference(flags):
    """The REDS branch on tests/best_window_ref.py's own evaluation inputs (5 frames of 12 x 16, windows of 3, overlap 1)."""
    from oracle import infer_oracle as IO
    from tests import best_window_ref as BR
    lr, hr = BR.eval_inputs()
    rec = Recorder(IO.fake_sr_model())
    want = evaluate(rec, lr, hr, "REDS", 3, 1, None, None, 4, *flags)
    return dict(lr=lr, hr=hr, rec=rec, want=want)
