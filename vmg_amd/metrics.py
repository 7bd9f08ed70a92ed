"""Scoring of output frames on the GPU: PSNR, PSNR-Y, SSIM and SSIM-Y as the reference's test driver computes them
(tools/test_reds4.py:194-283 with utils/metrics.py:11-70 and scikit-image's rgb2ycbcr), and the driver's bookkeeping of averages.

frame_metrics scores uint8 frames where they are -- the planar (T, 3, H, W) frames infer.to_uint8_device returns, or interleaved
(T, H, W, 3) frames as decoded images have them -- with one kernel launch per call (vmg_frame_metrics: float64 and integer arithmetic,
bit-reproducible) and ONE host synchronisation, for the logarithm.  There is no CPU path.

Scoreboard is host logic: which frames count, and the means of means frames -> clip -> sequence -> folder.
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

from . import kernels as K
from .hip import HipError

METRICS = ("psnr", "psnr_y", "ssim", "ssim_y")


class FrameMetrics(NamedTuple):
    """Four float64 host tensors of length T, one value per frame pair."""
    psnr: torch.Tensor
    psnr_y: torch.Tensor
    ssim: torch.Tensor
    ssim_y: torch.Tensor


def _planar_view(t: torch.Tensor, name: str) -> torch.Tensor:
    """The (T, 3, H, W) view of a planar (T, 3, H, W) / (3, H, W) or interleaved (T, H, W, 3) / (H, W, 3) tensor (no copy)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipError(f"frame_metrics: {name} must be a device tensor (there is no CPU path)")
    if t.dtype != torch.uint8:
        raise HipError(f"frame_metrics: {name} must be uint8, got {t.dtype}")
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4:
        raise HipError(f"frame_metrics: {name} must be (T, 3, H, W), (T, H, W, 3) or one such frame, got {tuple(t.shape)}")
    if t.shape[1] == 3:
        return t
    if t.shape[3] == 3:
        return t.permute(0, 3, 1, 2)
    raise HipError(f"frame_metrics: {name} has no RGB axis of length 3: {tuple(t.shape)}")


def _psnr(sse: float, count: int) -> float:
    """utils/metrics.py:23-26 on the exact sum: np.mean of integer-valued float64 squares is sum / count."""
    mse = sse / count
    if mse == 0:
        return float("inf")
    return 20 * math.log10(255.0 / math.sqrt(mse))


@torch.no_grad()
def frame_metrics(out_u8: torch.Tensor, gt_u8: torch.Tensor, border: int = 0) -> FrameMetrics:
    """Scores T frame pairs (or one).  `border` pixels are cut from every side of both frames first (calculate_psnr's `border`,
    utils/metrics.py:17-19; the driver passes 0), and all four metrics are those of the cropped pair.  Identical frames give a PSNR of
    inf, as in the reference.  Frames that the crop leaves smaller than the 11 x 11 SSIM window are refused."""
    a, b = _planar_view(out_u8, "out_u8"), _planar_view(gt_u8, "gt_u8")
    if a.shape != b.shape:
        raise HipError(f"frame_metrics: the frames differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
    border = int(border)
    if border < 0:
        raise HipError("frame_metrics: negative border")
    if border:
        a, b = (t[:, :, border:t.shape[2] - border, border:t.shape[3] - border] for t in (a, b))
    T, _, H, W = a.shape
    if H < 11 or W < 11:
        raise HipError(f"frame_metrics: a {H} x {W} frame is smaller than the 11 x 11 SSIM window")
    sse, sums = K.frame_metrics_sums(a, b)
    # the one synchronisation: both results cross in one copy (the integer sums travel as their own bits)
    host = torch.cat([sse.view(torch.float64).unsqueeze(1), sums], dim=1).cpu()
    sse, sums = host[:, 0].contiguous().view(torch.int64).tolist(), host[:, 1:].tolist()
    n_pix, n_map = H * W, (H - 10) * (W - 10)
    rows = [(_psnr(float(e), 3 * n_pix), _psnr(s[0], n_pix), (s[1] / n_map + s[2] / n_map + s[3] / n_map) / 3, s[4] / n_map) for e, s in zip(sse, sums)]
    return FrameMetrics(*(torch.tensor([r[k] for r in rows], dtype=torch.float64) for k in range(4)))


class _Mean:
    """AverageMeter of the reference (a sum and a count)."""

    def __init__(self):
        self.sum, self.count = 0.0, 0

    def update(self, v: float) -> None:
        self.sum += float(v)
        self.count += 1

    def average(self) -> float:
        return self.sum / self.count if self.count else float("nan")


class Scoreboard:
    """The bookkeeping of tools/test_reds4.py:136-283.  A FOLDER holds sequences, a sequence is scored clip by clip (index list by index list):

        board.start_sequence("000", "0045")
        for indices in indices_list:
            board.add_clip(indices, frame_metrics(out_u8, gt_u8))     # values in the order of `indices`
        board.end_sequence()
        board.folder_average("000"), board.average()

    - a frame index already scored in this sequence is skipped (`tested_index`, :195-197);
    - eval_mid_clip keeps only position len(indices) // 2 of each index list; with use_mirrors positions 3 and 10 (:225-239);
    - a sequence's value is the mean of its kept frames, a folder's the mean of its sequences, the total the mean of the folders.
    select_topk and writing images stay with the caller."""

    def __init__(self, eval_mid_clip: bool = False, use_mirrors: bool = False):
        self.eval_mid_clip, self.use_mirrors = bool(eval_mid_clip), bool(use_mirrors)
        self.folders: Dict[str, Dict[str, Dict[str, float]]] = {}  # folder -> sequence -> metric -> mean over its kept frames
        self.frames: Dict[tuple, Dict[int, Dict[str, float]]] = {}  # (folder, sequence) -> frame index -> metric -> value (every scored frame)
        self._cur = None

    def start_sequence(self, folder: str, sequence: str) -> None:
        if self._cur is not None:
            raise ValueError("Scoreboard: end_sequence() the open sequence first")
        if sequence in self.folders.get(folder, {}):
            raise ValueError(f"Scoreboard: sequence {folder}/{sequence} was scored already")
        self._cur = (folder, sequence, set(), {m: _Mean() for m in METRICS})
        self.frames[folder, sequence] = {}

    def _kept(self, pos: int, n: int) -> bool:
        if not self.eval_mid_clip:
            return True
        if self.use_mirrors:
            return pos in (3, 10)
        return pos == n // 2

    def add_clip(self, indices: Sequence[int], metrics) -> List[int]:
        """metrics: a FrameMetrics (or any four sequences in METRICS order) with one value per entry of `indices`.  Returns the positions
        of `indices` that entered the sequence's average."""
        if self._cur is None:
            raise ValueError("Scoreboard: start_sequence() first")
        folder, sequence, tested, means = self._cur
        cols = [[float(v) for v in col] for col in metrics]
        if len(cols) != 4 or any(len(c) != len(indices) for c in cols):
            raise ValueError("Scoreboard: four metric columns with one value per frame index expected")
        used = []
        for pos, frame in enumerate(indices):
            frame = int(frame)
            if frame in tested:
                continue
            tested.add(frame)
            vals = {m: cols[k][pos] for k, m in enumerate(METRICS)}
            self.frames[folder, sequence][frame] = vals
            if self._kept(pos, len(indices)):
                for m in METRICS:
                    means[m].update(vals[m])
                used.append(pos)
        return used

    def end_sequence(self) -> Dict[str, float]:
        if self._cur is None:
            raise ValueError("Scoreboard: no open sequence")
        folder, sequence, _, means = self._cur
        self._cur = None
        res = {m: means[m].average() for m in METRICS}
        res["frames"] = means["psnr"].count
        self.folders.setdefault(folder, {})[sequence] = res
        return res

    def folder_average(self, folder: str) -> Dict[str, float]:
        seqs = self.folders[folder].values()
        return {m: sum(s[m] for s in seqs) / len(seqs) for m in METRICS}

    def average(self) -> Dict[str, float]:
        """Mean over the folders of their averages (the reference's final np.mean over its per-folder lists)."""
        per = [self.folder_average(f) for f in self.folders]
        return {m: sum(p[m] for p in per) / len(per) for m in METRICS}
