"""Training batches from frames that stay on the GPU: what the reference's dataset classes (data/REDS.py:143-215, data/Vimeo.py:141-206)
return from __getitem__ and its DataLoader stacks -- a window of frames, optionally reversed, a random LR crop with the HR crop at scale x
its offsets, horizontal / vertical flip and transpose, the mirrored sequence, BGR -> RGB, HWC -> CHW, / 255 -- for B samples at once.

The frames are resident uint8 tensors (FrameStore).  The host draws a few integers per sample (draw_plan: the reference's draws from the
same generators in the same order, so a seeded run sees the same crops) and assemble writes the (B, T, 3, h, w) / (B, T, 3, s h, s w)
tensors with one kernel launch per store (vmg_crop_batch, csrc/batch.hip), into buffers the caller may own.  Nothing is synchronised.
There is no CPU path.  The kernel moves bytes and divides by 255 with the correctly rounded quotient: float32 output has the bits of the
reference's batch, uint8 output is the bytes themselves, bfloat16 the rounded float32.
"""
from __future__ import annotations

import dataclasses
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import degrade
from . import kernels as K
from .hip import HipError

DTYPES = (torch.float32, torch.bfloat16, torch.uint8)
CFG_KEYS = ("scale", "num_frames", "total_num_frames", "crop_size", "image_shape", "random_reverse", "use_hflip", "use_vflip", "use_rot",
            "use_mirrors", "pre_seed")


@dataclasses.dataclass
class BatchPlan:
    """What the host decides for B samples; plain numpy arrays.  clip (B): index of the clip in the store; frames (B, T'): the frames in
    output order, after reverse and mirrors; y0, x0 (B): crop origin in LR pixels (the HR origin is scale x it); hflip, vflip, rot (B):
    bool; crop: the LR crop edge c = crop_size // scale as configured (assemble clips it to the frame as the reference's slicing does)."""
    clip: np.ndarray
    frames: np.ndarray
    y0: np.ndarray
    x0: np.ndarray
    hflip: np.ndarray
    vflip: np.ndarray
    rot: np.ndarray
    crop: int

    def __len__(self):
        return len(self.clip)


def _side(x, what: str):
    """Frames as given -> (list of per-clip (F, ...) tensors, planar?, H, W)."""
    clips = list(x) if isinstance(x, (list, tuple)) else None
    if clips is None:
        if not isinstance(x, torch.Tensor):
            raise HipError(f"FrameStore: {what} must be a device tensor or a list of per-clip device tensors, got {type(x).__name__}")
        if x.dim() != 5:
            raise HipError(f"FrameStore: {what} must be (clips, frames, H, W, 3) or (clips, frames, 3, H, W), got {tuple(x.shape)}")
        clips = [x[i] for i in range(x.shape[0])]
    if not clips:
        raise HipError(f"FrameStore: {what} holds no clip")
    for c in clips:
        if not isinstance(c, torch.Tensor) or not c.is_cuda:
            raise HipError(f"FrameStore: {what} must live on the device (there is no CPU path)")
        if c.dtype != torch.uint8:
            raise HipError(f"FrameStore: {what} must be uint8, got {c.dtype}")
        if c.dim() != 4 or c.shape[0] < 1:
            raise HipError(f"FrameStore: every clip of {what} must be (frames, H, W, 3) or (frames, 3, H, W), got {tuple(c.shape)}")
        if c.shape[1:] != clips[0].shape[1:] or c.device != clips[0].device:
            raise HipError(f"FrameStore: the clips of {what} differ in frame size or device: {tuple(c.shape)} and {tuple(clips[0].shape)}")
    shape = clips[0].shape
    if shape[1] == 3:  # planar first, as degrade decides
        planar, H, W = True, shape[2], shape[3]
    elif shape[3] == 3:
        planar, H, W = False, shape[1], shape[2]
    else:
        raise HipError(f"FrameStore: the frames of {what} have no channel axis of length 3: {tuple(shape)}")
    return clips, planar, int(H), int(W)


class _Side:
    """One resolution of the store: per-clip base address and frame stride (host arrays), the byte strides every frame shares."""

    def __init__(self, x, what: str):
        self.clips, planar, self.H, self.W = _side(x, what)
        st = [(c.stride(2), c.stride(3), c.stride(1)) if planar else (c.stride(1), c.stride(2), c.stride(3)) for c in self.clips]
        if any(s != st[0] for s in st):
            raise HipError(f"FrameStore: the clips of {what} differ in their strides; one layout per store")
        if min(st[0]) < 0 or min(c.stride(0) for c in self.clips) < 0:
            raise HipError(f"FrameStore: {what} has a negative stride")
        self.strides = tuple(int(s) for s in st[0])  # row, pixel, channel (bytes: uint8)
        self.base = np.array([c.data_ptr() for c in self.clips], dtype=np.int64)
        self.fstride = np.array([c.stride(0) for c in self.clips], dtype=np.int64)
        self.nframes = np.array([c.shape[0] for c in self.clips], dtype=np.int64)


class _Slot:
    """Pinned staging and device tables of one assemble call; reused once the call's kernels have run."""

    def __init__(self, cap: int, device):
        self.cap = cap
        self.h_ptr = torch.empty(2 * cap, dtype=torch.int64).pin_memory()
        self.h_desc = torch.empty((2 * cap, 3), dtype=torch.int32).pin_memory()
        self.d_ptr = torch.empty(2 * cap, dtype=torch.int64, device=device)
        self.d_desc = torch.empty((2 * cap, 3), dtype=torch.int32, device=device)
        self.done = torch.cuda.Event()
        self.used = False

    def free(self) -> bool:
        return not self.used or self.done.query()


class FrameStore:
    """Resident uint8 frames of a training set: hr and lr, each (clips, frames, H, W, 3) interleaved or (clips, frames, 3, H, W) planar,
    or a list of per-clip (frames, ...) tensors of one frame size (separate allocations, views: read in place).  lr is hr / scale in frame
    size, clip for clip and frame for frame.  bgr: the stored channel order is B, G, R as cv2 decodes (the reference's stores): the
    output is R, G, B; bgr=False keeps the order."""

    def __init__(self, hr, lr, scale: int, bgr: bool = True):
        if not isinstance(scale, int) or isinstance(scale, bool) or scale < 1:
            raise HipError(f"FrameStore: scale must be a positive integer, got {scale!r}")
        self.scale, self.bgr = scale, bool(bgr)
        self.hr, self.lr = _Side(hr, "hr"), _Side(lr, "lr")
        if (self.hr.H, self.hr.W) != (self.lr.H * scale, self.lr.W * scale):
            raise HipError(f"FrameStore: {self.lr.H} x {self.lr.W} lr frames are not {self.hr.H} x {self.hr.W} hr frames / {scale}")
        if len(self.hr.clips) != len(self.lr.clips) or not np.array_equal(self.hr.nframes, self.lr.nframes):
            raise HipError("FrameStore: hr and lr differ in their clips or frames per clip")
        self.device = self.hr.clips[0].device
        if self.lr.clips[0].device != self.device:
            raise HipError("FrameStore: hr and lr live on different devices")
        self._slots: List[_Slot] = []

    @classmethod
    def from_hr(cls, hr, scale: int, bgr: bool = True) -> "FrameStore":
        """The LR side made here with degrade.bicubic_lr (planar uint8), clip by clip.  The HR frames must be multiples of scale in size:
        degrade.crop_to_scale makes the reference's crop."""
        clips, _, _, _ = _side(hr, "hr")
        return cls(hr, [degrade.bicubic_lr(c, scale) for c in clips], scale, bgr)

    def __len__(self):
        return len(self.hr.clips)

    def _slot(self, n: int) -> _Slot:
        for s in self._slots:
            if s.cap >= n and s.free():
                return s
        self._slots = [s for s in self._slots if s.cap >= n or not s.free()]  # too small and idle: dropped
        s = _Slot(max(n, 64), self.device)
        self._slots.append(s)
        return s


def _cfg(cfg, key):
    try:
        return cfg[key]
    except (KeyError, TypeError):
        raise HipError(f"draw_plan: the dataset config lacks '{key}'") from None


def draw_plan(indices: Sequence[int], cfg, py_random, np_random=None, dataset: str = "REDS") -> BatchPlan:
    """The reference's __getitem__ draws for each index of `indices`, in its order, from the caller's generators:
        REDS   sample_point from range(0, total_num_frames - num_frames + 1): np_random.choice(list, 1) if cfg['pre_seed'] is set (the
               reference seeds numpy's global stream with pre_seed + rank + 1 in __init__: pass numpy.random.RandomState(that)), else
               py_random.choice(list);  Vimeo: frames 1 .. num_frames (index v - 1 here), no draw
        py_random.random() < 0.5 reverses the frames, drawn only if random_reverse
        rnd_h = py_random.randint(0, max(0, H_lr - c)), then rnd_w likewise, c = crop_size // scale
        hflip, vflip, rot: one py_random.random() < 0.5 each, drawn ONLY if its use_* flag is true
        use_mirrors appends the reversed frame list.
    cfg: the reference's `dataset:` block (keys read: scale, num_frames, total_num_frames (REDS), crop_size, image_shape = (3, H, W) of the
    HR frames, random_reverse, use_hflip, use_vflip, use_rot, use_mirrors, pre_seed).  py_random: a random.Random (or the random module
    itself); index i is clip i of the store.
    The streams equal the reference's for in-process loading (n_workers: 0), where one process makes every draw in sample order.  With
    worker processes the reference's own streams depend on which worker loads which sample, and there is nothing to equal."""
    if dataset not in ("REDS", "Vimeo"):
        raise HipError(f"draw_plan: dataset must be 'REDS' or 'Vimeo', got {dataset!r}")
    scale, T, crop_size = int(_cfg(cfg, "scale")), int(_cfg(cfg, "num_frames")), int(_cfg(cfg, "crop_size"))
    shape = tuple(_cfg(cfg, "image_shape"))
    H, W, c = shape[1] // scale, shape[2] // scale, crop_size // scale
    reverse, mirrors = _cfg(cfg, "random_reverse"), _cfg(cfg, "use_mirrors")
    use_h, use_v, use_r = _cfg(cfg, "use_hflip"), _cfg(cfg, "use_vflip"), _cfg(cfg, "use_rot")
    pre_seed = _cfg(cfg, "pre_seed")
    if c < 1 or T < 1:
        raise HipError(f"draw_plan: crop_size {crop_size} at scale {scale} and {T} frames leave nothing to draw")
    if dataset == "REDS":
        total = int(_cfg(cfg, "total_num_frames"))
        if total < T:
            raise HipError(f"draw_plan: {T} frames out of clips of {total}")
        sample_list = list(range(0, total - T + 1))
        if pre_seed is not None and np_random is None:
            raise HipError("draw_plan: with pre_seed the start frame comes from numpy's stream: pass np_random = numpy.random.RandomState(pre_seed + rank + 1)")
    rows = []
    for index in indices:
        if dataset == "REDS":
            start = py_random.choice(sample_list) if pre_seed is None else int(np_random.choice(sample_list, 1)[0])
            frames = list(range(start, start + T))
        else:
            frames = list(range(0, T))
        if reverse and py_random.random() < 0.5:
            frames.reverse()
        y0 = py_random.randint(0, max(0, H - c))
        x0 = py_random.randint(0, max(0, W - c))
        hflip = bool(use_h and py_random.random() < 0.5)
        vflip = bool(use_v and py_random.random() < 0.5)
        rot = bool(use_r and py_random.random() < 0.5)
        if mirrors:
            frames = frames + frames[::-1]
        rows.append((int(index), frames, y0, x0, hflip, vflip, rot))
    return BatchPlan(clip=np.array([r[0] for r in rows], dtype=np.int64), frames=np.array([r[1] for r in rows], dtype=np.int64).reshape(len(rows), -1),
                     y0=np.array([r[2] for r in rows], dtype=np.int64), x0=np.array([r[3] for r in rows], dtype=np.int64),
                     hflip=np.array([r[4] for r in rows], dtype=bool), vflip=np.array([r[5] for r in rows], dtype=bool),
                     rot=np.array([r[6] for r in rows], dtype=bool), crop=c)


def _checked_plan(store: FrameStore, plan: BatchPlan):
    """The plan's arrays, validated against the store: everything the kernel trusts."""
    if not isinstance(plan, BatchPlan):
        raise HipError(f"assemble: a BatchPlan expected, got {type(plan).__name__}")
    clip, frames = np.asarray(plan.clip, dtype=np.int64), np.asarray(plan.frames, dtype=np.int64)
    B = clip.shape[0] if clip.ndim == 1 else 0
    if B < 1 or frames.ndim != 2 or frames.shape[0] != B or frames.shape[1] < 1:
        raise HipError(f"assemble: the plan needs B >= 1 clips and (B, T) frames, got {clip.shape} and {frames.shape}")
    arrs = []
    for name in ("y0", "x0", "hflip", "vflip", "rot"):
        a = np.asarray(getattr(plan, name))
        if a.shape != (B,):
            raise HipError(f"assemble: the plan's {name} must have one entry per sample, got {a.shape}")
        arrs.append(a.astype(np.int64))
    y0, x0 = arrs[:2]
    hflip, vflip, rot = ((a != 0).astype(np.int64) for a in arrs[2:])
    if clip.min() < 0 or clip.max() >= len(store):
        raise HipError(f"assemble: clip index out of range of the store's {len(store)} clips")
    if frames.min() < 0 or (frames >= store.lr.nframes[clip][:, None]).any():
        raise HipError("assemble: frame index out of range of its clip")
    c = int(plan.crop)
    if c < 1:
        raise HipError(f"assemble: crop {c}")
    ch, cw = min(c, store.lr.H), min(c, store.lr.W)  # the reference's slices clip a crop larger than the frame
    if y0.min() < 0 or y0.max() > store.lr.H - ch or x0.min() < 0 or x0.max() > store.lr.W - cw:
        raise HipError(f"assemble: crop origin outside 0..{store.lr.H - ch} x 0..{store.lr.W - cw}")
    if rot.any() and ch != cw:
        raise HipError(f"assemble: rot with a {ch} x {cw} crop: the samples of the batch would differ in shape")
    return clip, frames, y0, x0, hflip + 2 * vflip + 4 * rot, ch, cw


@torch.no_grad()
def assemble(store: FrameStore, plan: BatchPlan, dtype: torch.dtype = torch.float32,
             out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The batch of a plan: (LRs (B, T', 3, h, w), HRs (B, T', 3, s h, s w)) as dtype (float32 / bfloat16: byte / 255; uint8: the bytes),
    channels R, G, B for a bgr store.  out = (lrs, hrs): contiguous device tensors of exactly those shapes and dtype, written in place
    (the static inputs of a captured TrainStep, say); anything else is refused.  Two small non-blocking uploads (frame addresses,
    descriptors) from pinned buffers the store owns and two launches on the current stream; the host waits for nothing."""
    if not isinstance(store, FrameStore):
        raise HipError(f"assemble: a FrameStore expected, got {type(store).__name__}")
    if dtype not in DTYPES:
        raise HipError(f"assemble: dtype must be torch.float32, torch.bfloat16 or torch.uint8, got {dtype}")
    clip, frames, y0, x0, flags, ch, cw = _checked_plan(store, plan)
    B, T = frames.shape
    N, s = B * T, store.scale
    shapes = ((B, T, 3, ch, cw), (B, T, 3, s * ch, s * cw))
    if out is None:
        out = tuple(torch.empty(sh, dtype=dtype, device=store.device) for sh in shapes)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise HipError("assemble: out must be the pair (lrs, hrs)")
        for t, sh, what in zip(out, shapes, ("lrs", "hrs")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != store.device:
                raise HipError(f"assemble: out {what} must be a tensor on the store's device")
            if tuple(t.shape) != sh or t.dtype != dtype or not t.is_contiguous():
                raise HipError(f"assemble: out {what} must be contiguous {sh} {dtype}, got {tuple(t.shape)} {t.dtype}")
    slot = store._slot(N)
    ptr, desc = slot.h_ptr.numpy(), slot.h_desc.numpy()
    for k, side, m in ((0, store.lr, 1), (1, store.hr, s)):
        ptr[k * N:(k + 1) * N] = (side.base[clip][:, None] + frames * side.fstride[clip][:, None]).reshape(-1)
        d = desc[k * N:(k + 1) * N].reshape(B, T, 3)
        d[:, :, 0], d[:, :, 1], d[:, :, 2] = (m * y0)[:, None], (m * x0)[:, None], flags[:, None]
    slot.d_ptr[:2 * N].copy_(slot.h_ptr[:2 * N], non_blocking=True)
    slot.d_desc[:2 * N].copy_(slot.h_desc[:2 * N], non_blocking=True)
    K.crop_batch(slot.d_ptr[:N], store.lr.strides, slot.d_desc[:N], store.lr.H, store.lr.W, ch, cw, store.bgr, out[0])
    K.crop_batch(slot.d_ptr[N:2 * N], store.hr.strides, slot.d_desc[N:2 * N], store.hr.H, store.hr.W, s * ch, s * cw, store.bgr, out[1])
    slot.done.record()
    slot.used = True
    return out[0], out[1]


def batches(store: FrameStore, cfg, sampler: Iterable[Sequence[int]], py_random=None, np_random=None, dataset: str = "REDS",
            dtype: torch.dtype = torch.float32, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, keys: Optional[Sequence] = None):
    """A generator of {'LRs', 'HRs', 'key'} dicts, what the reference's DataLoader hands tools/Trainer.py:126-127, for every index list of
    `sampler` (any iterable of index lists; index i is clip i of the store; samplers and dataset_expand_ratio are the caller's).
    py_random defaults to the random module, as the reference uses it.  key: keys[i] per sample, or the indices themselves.  With out=,
    every batch is written into the same two buffers: consume one before asking for the next."""
    if py_random is None:
        import random as py_random
    for indices in sampler:
        indices = [int(i) for i in indices]
        lrs, hrs = assemble(store, draw_plan(indices, cfg, py_random, np_random, dataset), dtype, out)
        yield {"LRs": lrs, "HRs": hrs, "key": [keys[i] for i in indices] if keys is not None else indices}
