"""LR clips from HR frames on the GPU: the bicubic ("BI") degradation the reference's datasets are made with (datasets/generate_LR.py:
crop to a multiple of the scale, utils/image_resize.py imresize_np(img, 1 / scale, True), cv2.imwrite's rounding to uint8) and what the
dataset classes do with the stored image (/ 255 as float32, data/REDS.py:116).

bicubic_lr filters uint8 frames where they are -- planar (T, 3, H, W) frames as infer.to_uint8_device returns them, interleaved
(T, H, W, 3) frames as decoded images have them, crops and frame subsets of either -- with one kernel launch (vmg_bicubic_down: float64
accumulation in a fixed order, bit-reproducible) and no host synchronisation.  There is no CPU path.  The filter is per channel: BGR in
gives BGR out.
"""
from __future__ import annotations

import torch

from . import kernels as K
from .hip import HipError

SCALES = (2, 3, 4)


def _planar_view(t: torch.Tensor, what: str) -> torch.Tensor:
    """The (T, 3, H, W) view of a planar (T, 3, H, W) / (3, H, W) or interleaved (T, H, W, 3) / (H, W, 3) tensor (no copy)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipError(f"{what}: the frames must be a device tensor (there is no CPU path)")
    if t.dtype != torch.uint8:
        raise HipError(f"{what}: the frames must be uint8, got {t.dtype}")
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4:
        raise HipError(f"{what}: the frames must be (T, 3, H, W), (T, H, W, 3) or one such frame, got {tuple(t.shape)}")
    if t.shape[1] == 3:
        return t
    if t.shape[3] == 3:
        return t.permute(0, 3, 1, 2)
    raise HipError(f"{what}: the frames have no channel axis of length 3: {tuple(t.shape)}")


def _check_scale(scale, what: str) -> int:
    if scale not in SCALES:
        raise HipError(f"{what}: scale must be one of {SCALES}, got {scale!r}")
    return int(scale)


def crop_to_scale(frames: torch.Tensor, scale: int) -> torch.Tensor:
    """The top-left crop of the frames to multiples of `scale` in height and width (generate_LR.py:32-34), as a view: same storage, same
    layout.  frames: (..., 3, H, W) planar or (..., H, W, 3) interleaved."""
    scale = _check_scale(scale, "crop_to_scale")
    if frames.dim() < 3:
        raise HipError(f"crop_to_scale: frames with a channel axis expected, got {tuple(frames.shape)}")
    if frames.shape[-3] == 3:  # planar first, as _planar_view decides
        H, W = frames.shape[-2:]
        return frames[..., :H - H % scale, :W - W % scale]
    if frames.shape[-1] == 3:
        H, W = frames.shape[-3:-1]
        return frames[..., :H - H % scale, :W - W % scale, :]
    raise HipError(f"crop_to_scale: the frames have no channel axis of length 3: {tuple(frames.shape)}")


@torch.no_grad()
def bicubic_lr(hr_u8: torch.Tensor, scale: int = 4, out: torch.dtype = torch.uint8) -> torch.Tensor:
    """T HR frames (or one) -> the contiguous planar (T, 3, H/scale, W/scale) LR frames.
    out = torch.uint8: the bytes generate_LR.py stores; torch.float32 / torch.bfloat16: those bytes / 255, what the datasets feed the
    network; torch.float64: the filter's unrounded, unclamped values on the 0..255 scale (imresize_np's own output).
    Nothing is cropped silently: a frame size that is no multiple of `scale` is refused (crop_to_scale makes the reference's crop)."""
    scale = _check_scale(scale, "bicubic_lr")
    v = _planar_view(hr_u8, "bicubic_lr")
    H, W = v.shape[2:]
    if H % scale or W % scale:
        raise HipError(f"bicubic_lr: a {H} x {W} frame is no multiple of the scale {scale}; crop_to_scale(frames, {scale}) makes the reference's crop")
    if H < 4 * scale or W < 4 * scale:
        raise HipError(f"bicubic_lr: a {H} x {W} frame is smaller than the filter's support of {4 * scale} pixels")
    if out not in K.LR_OUT_TYPES:
        raise HipError(f"bicubic_lr: out must be torch.uint8, float32, bfloat16 or float64, got {out}")
    return K.bicubic_down(v, scale, out)


@torch.no_grad()
def lr_clip(hr_u8: torch.Tensor, scale: int = 4, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """HR frames -> the (B, T, 3, h, w) clip in [0, 1] that model(...) and infer.test_clips take.  hr_u8: T frames in any layout bicubic_lr
    reads (one clip, B = 1) or planar (B, T, 3, H, W)."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise HipError(f"lr_clip: dtype must be torch.float32 or torch.bfloat16, got {dtype}")
    if isinstance(hr_u8, torch.Tensor) and hr_u8.dim() == 5:
        B, T = hr_u8.shape[:2]
        if hr_u8.shape[2] != 3:
            raise HipError(f"lr_clip: a batch of clips must be planar (B, T, 3, H, W), got {tuple(hr_u8.shape)}")
        if _flattens(hr_u8):
            lr = bicubic_lr(hr_u8.flatten(0, 1), scale, dtype)
            return lr.view(B, T, *lr.shape[1:])
        return torch.stack([bicubic_lr(clip, scale, dtype) for clip in hr_u8])
    return bicubic_lr(hr_u8, scale, dtype).unsqueeze(0)


def _flattens(t: torch.Tensor) -> bool:
    """Whether (B, T, ...) merges into (B*T, ...) as a view: one launch for the whole batch."""
    return t.shape[0] == 1 or t.stride(0) == t.shape[1] * t.stride(1)
