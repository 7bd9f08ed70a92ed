"""Sliding-window inference for the VMG hot path: counterpart of the reference's tools/Tester.py:107-251.

Same window lists, same visiting order (the network is stateful, SURVEY T1, so the order is part of the result), same
half-overlap conventions (`-overlap//2:` drops ceil(overlap/2) trailing rows/frames, `:overlap//2` floor(overlap/2) leading
ones, counted in OUTPUT pixels with the LOW-resolution overlap, exactly as the reference slices them).  The canvases stay
in HBM; each tile is folded in by one HIP kernel (vmg_tile_accumulate) and the division / clamp / uint8 rounding is one
more (vmg_tile_finalize).  There is no CPU path: tensors must live on the GPU.

The three window functions are plan_calls -> run_calls -> blend: the list of network calls in visiting order (host logic), a
contiguous run of them executed at the right call index (VMG.set_forward_calls), and the fold of all tile outputs in plan
order.  test_clips_sharded spreads the calls of one sequence over the ranks of a torch.distributed group and folds on rank 0:
the same bits as one process walking all calls.
"""
from __future__ import annotations

import math
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip
from .hip import HipError


class GraphedModel:
    """model(x) replayed from a captured hipGraph, one graph per input shape (the sliding-window harness calls the network 18 times per sequence on
    (1, 50, 3, 128, 128) tiles: ~7 000 launches per call issued from Python otherwise).  The network is STATEFUL (every call multiplies
    the MorphFC mixer weights by Gamma in place) and the capture procedure needs warm-up calls: the mixer weights are saved before and put back
    after them, so the first replay is call #1 exactly as without the wrapper; the decay itself is part of the graph (it runs at every replay).
    Results are the same bits as the eager calls (the same kernels on the same data; tests/test_infer_gpu.py)."""

    def __init__(self, model: torch.nn.Module, warmup: int = 3):
        self.model, self.warmup, self.graphs = model, int(warmup), {}

    def _mixer_weights(self):
        return [p for n, p in self.model.named_parameters() if n.endswith("mlp_h.0.weight") or n.endswith("mlp_w.0.weight")]

    # the model's call index (VMG.forward_calls): the warm-up calls do not count, every replay does
    @property
    def forward_calls(self) -> int:
        return self.model.forward_calls

    def advance_calls(self, n: int) -> None:
        self.model.advance_calls(n)

    def set_forward_calls(self, k: int) -> None:
        self.model.set_forward_calls(k)

    @torch.no_grad()
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        hip.require_cuda(x)
        # the mirrored-clip test (models/vmg.py:426-432) is a host decision on device data: taken here, once per call, and part of the graph's key
        self.model.check_frames_mirror(lrs=x.float())
        mirror = bool(self.model.frames_mirror)
        self.model._mirror_known = mirror
        try:
            return self._call(x, mirror)
        finally:
            self.model._mirror_known = None

    def _call(self, x: torch.Tensor, mirror: bool) -> torch.Tensor:
        key = (tuple(x.shape), x.dtype, mirror)
        ent = self.graphs.get(key)
        if ent is None:
            from . import functional as FH
            static_in = x.clone()
            ws = self._mixer_weights()
            saved = [w.detach().clone() for w in ws]
            calls0 = self.model._forward_calls
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for i in range(max(self.warmup, 6)):  # until the cached weight packs / repack plans have settled (see train.TrainStep.capture)
                    stamp = FH.PACKS.stamp
                    self.model(static_in)
                    if i + 1 >= self.warmup and FH.PACKS.settled(stamp, with_repack=False):
                        break
                for w, s0 in zip(ws, saved):
                    w.copy_(s0)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                static_out = self.model(static_in)
            self.model._forward_calls = calls0  # (the warm-up calls were undone above, and capturing runs nothing)
            ent = self.graphs[key] = (g, static_in, static_out)
        g, static_in, static_out = ent
        static_in.copy_(x)
        g.replay()
        self.model._forward_calls += 1  # (the decay is part of the graph)
        return static_out.clone()


def tile_starts(total: int, size: int, overlap: int) -> List[int]:
    """Window starts of tools/Tester.py:113-114 / :151-152: every (size - overlap), plus one window flush with the end."""
    stride = size - overlap
    if stride <= 0:
        raise ValueError(f"overlap {overlap} must be smaller than the window {size}")
    return list(range(0, total - size, stride)) + [max(0, total - size)]


def _accumulate(patch: torch.Tensor, E: torch.Tensor, Wt: torch.Tensor, oh: int, ow: int, margins) -> None:
    hip.require_cuda(patch, E, Wt)
    if E.dtype != torch.float32 or Wt.dtype != torch.float32 or not E.is_contiguous() or not Wt.is_contiguous():
        raise HipError("canvases must be contiguous fp32")
    p = patch.contiguous()
    ph, pw = p.shape[-2:]
    planes = p.numel() // (ph * pw)
    EH, EW = E.shape[-2:]
    if E.numel() // (EH * EW) != planes:
        raise HipError("tile and canvas disagree on the number of planes")
    top, bottom, left, right = margins
    hip.check(hip.lib().vmg_tile_accumulate(hip.dtype_code(p.dtype), p.data_ptr(), E.data_ptr(), Wt.data_ptr(), planes, ph, pw, EH, EW, oh, ow,
                                            top, bottom, left, right, hip.stream_ptr()), "vmg_tile_accumulate")


def _finalize(E: torch.Tensor, Wt: torch.Tensor, want_u8: bool = False):
    out = None if want_u8 else torch.empty_like(E)
    u8 = torch.empty(E.shape, dtype=torch.uint8, device=E.device) if want_u8 else None
    hip.check(hip.lib().vmg_tile_finalize(E.data_ptr(), Wt.data_ptr(), out.data_ptr() if out is not None else None,
                                          u8.data_ptr() if u8 is not None else None, E.numel(), hip.stream_ptr()), "vmg_tile_finalize")
    return u8 if want_u8 else out


class PlannedCall(NamedTuple):
    """One network call of a sequence: `index` = its 1-based position in the visiting order, `t` = first frame of its temporal window,
    `origin` = (h, w) of its spatial tile in LR pixels, None for whole frames."""
    index: int
    t: int
    origin: Optional[Tuple[int, int]]


class CallPlan:
    """The ordered network calls of one sequence (tools/Tester.py:107-175: outer loop temporal windows, inner loops tile rows then
    columns) with the window arithmetic the fold needs.  Behaves as the list of its PlannedCall entries."""

    def __init__(self, T: int, H: int, W: int, num_frames: int, overlap_frames: int, test_spatial: Optional[Sequence[int]] = None,
                 overlap_spatial: Optional[int] = None):
        self.T, self.H, self.W, self.num_frames, self.overlap_frames = int(T), int(H), int(W), int(num_frames), int(overlap_frames)
        self.ts = tile_starts(self.T, self.num_frames, self.overlap_frames)
        self.overlap_spatial = None if overlap_spatial is None else int(overlap_spatial)
        if self.overlap_spatial is None:
            self.th = self.tw = self.hs = self.ws = None
            origins = [None]
        else:
            self.th, self.tw = (int(v) for v in test_spatial)
            self.hs, self.ws = tile_starts(self.H, self.th, self.overlap_spatial), tile_starts(self.W, self.tw, self.overlap_spatial)
            origins = [(h, w) for h in self.hs for w in self.ws]
        self.per_window = len(origins)
        self.calls = [PlannedCall(i * self.per_window + j + 1, t, o) for i, t in enumerate(self.ts) for j, o in enumerate(origins)]

    def __len__(self):
        return len(self.calls)

    def __iter__(self):
        return iter(self.calls)

    def __getitem__(self, i):
        return self.calls[i]

    def crop(self, inputs: torch.Tensor, call: PlannedCall) -> torch.Tensor:
        """The call's input: its temporal window of (B, T, C, H, W), cut to its spatial tile."""
        clip = inputs[:, call.t:call.t + self.num_frames]
        if call.origin is None:
            return clip
        h, w = call.origin
        return clip[..., h:h + self.th, w:w + self.tw]

    def margins(self, call: PlannedCall, out: torch.Tensor):
        """(top, bottom, left, right) output rows / columns of the tile that its neighbours cover instead."""
        ov, hs, ws = self.overlap_spatial, self.hs, self.ws
        h, w = call.origin
        lead = ov // 2  # `:overlap//2` of the reference
        # `-overlap//2:` drops the last ceil(overlap/2) rows -- and, faithfully, EVERY row when overlap == 0 (the slice is
        # then `0:`; the reference yields 0/0 = NaN there: tiles without overlap are not a supported setting of it)
        trail_h = -(-ov // 2) if ov > 0 else out.shape[-2]
        trail_w = -(-ov // 2) if ov > 0 else out.shape[-1]
        return (lead if h > hs[0] else 0, trail_h if h < hs[-1] else 0, lead if w > ws[0] else 0, trail_w if w < ws[-1] else 0)


def plan_calls(T: int, H: int, W: int, num_frames: int, overlap_frames: int, test_spatial: Optional[Sequence[int]] = None,
               overlap_spatial: Optional[int] = None) -> CallPlan:
    """The network calls test_clips makes on a (B, T, C, H, W) sequence, in its visiting order.  Host logic only."""
    return CallPlan(T, H, W, num_frames, overlap_frames, test_spatial, overlap_spatial)


def shard_ranges(n_calls: int, world: int) -> List[range]:
    """1-based plan positions of each of `world` ranks: contiguous runs in rank order, lengths within one call of each other (the first
    n_calls % world ranks take the longer ones; a rank beyond the plan's length gets an empty range)."""
    if n_calls < 0 or world < 1:
        raise ValueError("shard_ranges: n_calls >= 0 and world >= 1 expected")
    q, r = divmod(n_calls, world)
    out, lo = [], 1
    for k in range(world):
        n = q + (1 if k < r else 0)
        out.append(range(lo, lo + n))
        lo += n
    return out


def _has_counter(model) -> bool:
    return hasattr(model, "forward_calls") and hasattr(model, "set_forward_calls")


def _entries(plan: CallPlan, calls) -> List[PlannedCall]:
    ents = [c if isinstance(c, PlannedCall) else plan[int(c) - 1] for c in calls]
    for a, b in zip(ents, ents[1:]):
        if b.index != a.index + 1:
            raise ValueError("run_calls: the calls must be a contiguous run of the plan, in plan order")
    for e in ents:
        if not 1 <= e.index <= len(plan) or plan[e.index - 1] != e:
            raise ValueError(f"run_calls: call {e.index} is not an entry of this plan")
    return ents


@torch.no_grad()
def run_calls(model: Callable, inputs: torch.Tensor, plan: CallPlan, calls, first_call: Optional[int] = None) -> List[torch.Tensor]:
    """Runs a contiguous sub-range of the plan -- `calls`: 1-based positions (e.g. range(3, 5)) or plan entries (plan[2:4]) -- and returns
    the tile outputs in that order.  The network is stateful (every call decays the mixer weights): with first_call = k the model is first
    moved to k - 1 applied calls (model.set_forward_calls), so that the first call made here is call k since the checkpoint was loaded;
    without it a model that counts its calls must stand exactly in front of the first position given.  Plain callables without a
    counter are called as they are."""
    hip.require_cuda(inputs)
    ents = _entries(plan, calls)
    if tuple(inputs.shape[1:2] + inputs.shape[3:]) != (plan.T, plan.H, plan.W):
        raise ValueError(f"run_calls: the plan is for (T, H, W) = {(plan.T, plan.H, plan.W)}, the inputs are {tuple(inputs.shape)}")
    if not ents:
        return []
    if first_call is not None:
        if not _has_counter(model):
            raise ValueError("run_calls: first_call needs a model that counts its calls (forward_calls / set_forward_calls)")
        model.set_forward_calls(int(first_call) - 1)
    elif _has_counter(model) and model.forward_calls + 1 != ents[0].index:
        raise ValueError(f"run_calls: the model has made {model.forward_calls} calls, so its next one is not call {ents[0].index} of the plan; "
                         "pass first_call to move it there")
    return [model(plan.crop(inputs, c)) for c in ents]


def _blend_window(plan: CallPlan, calls: Sequence[PlannedCall], outs: Sequence[torch.Tensor], dtype: torch.dtype, scale: int) -> torch.Tensor:
    """One temporal window from its calls' outputs (tools/Tester.py:107-141): the sole whole-frame output, or the spatial tiles folded in
    plan order."""
    if plan.overlap_spatial is None:
        return outs[0]
    B, tf, C = outs[0].shape[:3]
    E = torch.zeros(B, tf, C, plan.H * scale, plan.W * scale, dtype=torch.float32, device=outs[0].device)
    Wt = torch.zeros_like(E)
    for c, out in zip(calls, outs):
        _accumulate(out, E, Wt, c.origin[0] * scale, c.origin[1] * scale, plan.margins(c, out))
    return _finalize(E, Wt).to(dtype)


@torch.no_grad()
def blend(plan: CallPlan, outputs: Sequence[torch.Tensor], dtype: Optional[torch.dtype] = None, scale: int = 4) -> torch.Tensor:
    """Folds the tile outputs of ALL calls of the plan, given in plan order, into the (B, T, C, H * scale, W * scale) frames: spatial
    tiles by vmg_tile_accumulate / vmg_tile_finalize per temporal window, the windows by slice adds (tools/Tester.py:143-175).  fp32 sums
    depend on their order, so the fold always runs in plan order on one device: who computed which tile does not show in the result."""
    if len(outputs) != len(plan):
        raise ValueError(f"blend: the plan has {len(plan)} calls, {len(outputs)} outputs were given")
    hip.require_cuda(*outputs)
    dtype = outputs[0].dtype if dtype is None else dtype
    B, _, C = outputs[0].shape[:3]
    E = torch.zeros(B, plan.T, C, plan.H * scale, plan.W * scale, dtype=torch.float32, device=outputs[0].device)
    N = torch.zeros(B, plan.T, 1, 1, 1, dtype=torch.float32, device=outputs[0].device)
    ts, nf, of, pw = plan.ts, plan.num_frames, plan.overlap_frames, plan.per_window
    lead, trail = of // 2, -(-of // 2)
    for i, t in enumerate(ts):
        out = _blend_window(plan, plan[i * pw:(i + 1) * pw], outputs[i * pw:(i + 1) * pw], dtype, scale)
        lo = lead if (of > 0 and t > ts[0]) else 0
        hi = nf - (trail if (of > 0 and t < ts[-1]) else 0)
        # frames are whole planes: a slice add is already one pass
        E[:, t + lo:t + hi].add_(out[:, lo:hi].float())
        N[:, t + lo:t + hi].add_(1.0)
    return E.div_(N).to(dtype)


def _run_all(model: Callable, inputs: torch.Tensor, plan: CallPlan) -> List[torch.Tensor]:
    """Every call of the plan, continuing from wherever the model's call count stands (the reference keeps decaying across sequences)."""
    return run_calls(model, inputs, plan, plan.calls, first_call=model.forward_calls + 1 if _has_counter(model) else None)


@torch.no_grad()
def test_image(model: Callable, inputs: torch.Tensor, test_spatial: Sequence[int], overlap: int, scale: int = 4) -> torch.Tensor:
    """tools/Tester.py:107-141: spatial tiles of `test_spatial` with `overlap` LR pixels between neighbours."""
    hip.require_cuda(inputs)
    B, T, C, H, W = inputs.shape
    plan = CallPlan(T, H, W, max(T, 1), 0, test_spatial, overlap)  # one temporal window: all frames
    return _blend_window(plan, plan.calls, _run_all(model, inputs, plan), inputs.dtype, scale)


@torch.no_grad()
def test_clips(model: Callable, inputs: torch.Tensor, num_frames: int, overlap_frames: int, test_spatial: Optional[Sequence[int]] = None,
               overlap_spatial: Optional[int] = None, scale: int = 4) -> torch.Tensor:
    """tools/Tester.py:143-175: temporal windows of `num_frames` with `overlap_frames` shared frames: plan -> run all -> blend."""
    hip.require_cuda(inputs)
    B, T, C, H, W = inputs.shape
    plan = plan_calls(T, H, W, num_frames, overlap_frames, test_spatial, overlap_spatial)
    return blend(plan, _run_all(model, inputs, plan), inputs.dtype, scale)


@torch.no_grad()
def test_clips_sharded(model: Callable, inputs: torch.Tensor, num_frames: int, overlap_frames: int, test_spatial: Optional[Sequence[int]] = None,
                       overlap_spatial: Optional[int] = None, scale: int = 4, group=None) -> Optional[torch.Tensor]:
    """test_clips with the network calls of ONE sequence spread over the ranks of an initialised torch.distributed group: rank r runs a
    contiguous run of the plan (shard_ranges) starting at the right call index, the tile outputs travel to rank 0 in the model's output
    dtype, rank 0 folds them in plan order -- the bits of the single-process result -- and returns the frames; the other ranks return
    None.  Every replica must hold the same weights at the same call count on entry; all leave with the count of a single process that
    ran the whole sequence, so the next sequence continues the same way.  World size 1 or no group: test_clips."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return test_clips(model, inputs, num_frames, overlap_frames, test_spatial, overlap_spatial, scale)
    hip.require_cuda(inputs)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    B, T, C, H, W = inputs.shape
    plan = plan_calls(T, H, W, num_frames, overlap_frames, test_spatial, overlap_spatial)
    ranges = shard_ranges(len(plan), world)
    mine = ranges[rank]
    counted = _has_counter(model)
    base = model.forward_calls if counted else 0
    outs = run_calls(model, inputs, plan, mine, first_call=base + mine.start if counted and len(mine) else None)
    if counted:
        model.set_forward_calls(base + len(plan))
    src_of = (lambda r: dist.get_global_rank(group, r)) if group is not None else (lambda r: r)
    # every tile of a plan has one shape; rank 0 (never without a call) tells the others what a tile looks like
    meta = [(tuple(outs[0].shape), outs[0].dtype) if rank == 0 else None]
    dist.broadcast_object_list(meta, src=src_of(0), group=group)
    shape, odtype = meta[0]
    tiles: List[torch.Tensor] = []
    for r in range(world):
        if not len(ranges[r]):
            continue
        # one broadcast per shard: the collective both gloo and RCCL carry for device tensors (no gather / send there on gloo).  The
        # tiles move as the BYTES of the model's output dtype: gloo knows neither bf16 nor int16, every backend knows uint8
        buf = torch.stack([o.contiguous() for o in outs]) if r == rank else torch.empty((len(ranges[r]), *shape), dtype=odtype, device=inputs.device)
        dist.broadcast(buf.view(torch.uint8), src=src_of(r), group=group)
        if rank == 0:
            tiles.extend(buf.unbind(0))
    return blend(plan, tiles, inputs.dtype, scale) if rank == 0 else None


def _psnr01(a: torch.Tensor, b: torch.Tensor) -> float:
    """skimage.metrics.peak_signal_noise_ratio on [0,1]-clamped float images (data_range 1), float64 mean, with the
    reference's replacement of an infinite value (tools/Tester.py:24-34, :204-210)."""
    err = float(((a.clamp(0, 1).double() - b.clamp(0, 1).double()) ** 2).mean())
    if err == 0.0:
        return float(10 * np.log10(255.0 ** 2 / 0.65025))
    v = 10.0 * math.log10(1.0 / err)
    if v < 0:
        raise Exception("Wrong way of calculating psnr.")
    return v


@torch.no_grad()
def test_clips_max(model: Callable, inputs: torch.Tensor, HR: torch.Tensor, num_frames: int, overlap_frames: int,
                   test_spatial: Optional[Sequence[int]] = None, overlap_spatial: Optional[int] = None, scale: int = 4) -> torch.Tensor:
    """tools/Tester.py:178-216 (REDS): per frame, the window whose output scores the highest PSNR against HR.  Returns
    (T, C, 4H, 4W) like the reference's .squeeze() for its batch of one."""
    hip.require_cuda(inputs, HR)
    B, T, C, H, W = inputs.shape
    ts = tile_starts(T, num_frames, overlap_frames)
    E = torch.zeros(B, T, len(ts), C, H * scale, W * scale, dtype=torch.float32, device=inputs.device)
    psnrs = torch.zeros(B, T, len(ts), dtype=torch.float32)
    for idx, t in enumerate(ts):
        clip = inputs[:, t:t + num_frames]
        out = (model(clip) if overlap_spatial is None else test_image(model, clip, test_spatial, overlap_spatial, scale)).float()
        for i in range(num_frames):
            psnrs[:, t + i, idx] = _psnr01(out[:, i], HR[:, t + i].float())
        E[:, t:t + num_frames, idx].add_(out)
    _, max_idx = torch.max(psnrs, dim=-1)
    max_idx = max_idx.to(inputs.device)[:, :, None, None, None, None].expand(-1, -1, -1, C, H * scale, W * scale)
    return torch.gather(E, dim=2, index=max_idx).squeeze().to(inputs.dtype)


PSNR_CAP = float(10 * np.log10(255.0 ** 2 / 0.65025))  # psnr_exceed_check's replacement of an infinite score (tools/Tester.py:24-34)


@torch.no_grad()
def best_window_clips(model: Callable, inputs: torch.Tensor, HR: torch.Tensor, num_frames: int, overlap_frames: int,
                      test_spatial: Optional[Sequence[int]] = None, overlap_spatial: Optional[int] = None, scale: int = 4, return_scores: bool = False):
    """test_clips_max streamed: the same windows in the same order and the same frames out, (T, C, 4H, 4W) in inputs.dtype, but one window
    at a time.  Per window: the network, one vmg_frame_sqerr call (float64 error of every frame against HR), one vmg_best_window_select call
    (float32 score, "first maximum wins", copy of the winning frames).  No score visits the host and nothing is synchronised; the function owns
    one (T, C, 4H, 4W) fp32 canvas, two (T,) float32 and two (T,) int32 arrays and the reduction workspace.
    HR: (1, T, 3, 4H, 4W) fp32 / bf16, or (T, 4H, 4W, 3) uint8, scored in place as byte / 255 (Tester.evaluate's HR.astype(np.float32) / 255.).
    return_scores: also (choice (T,) int32, best (T,) float32, table (T, n_windows) float32 with 0 where a window does not cover a frame),
    all on the device."""
    from . import kernels as K
    hip.require_cuda(inputs, HR)
    B, T, C, H, W = inputs.shape
    if B != 1:
        raise ValueError(f"best_window_clips: one sequence at a time (the reference's selection is defined for a batch of one), got B = {B}")
    hh, ww = H * scale, W * scale
    if HR.dtype == torch.uint8:
        if tuple(HR.shape) != (T, hh, ww, 3) or C != 3:
            raise ValueError(f"best_window_clips: uint8 HR must be (T, 4H, 4W, 3) = {(T, hh, ww, 3)}, got {tuple(HR.shape)}")
        hr = HR
    else:
        if tuple(HR.shape) != (1, T, C, hh, ww):
            raise ValueError(f"best_window_clips: float HR must be (1, T, C, 4H, 4W) = {(1, T, C, hh, ww)}, got {tuple(HR.shape)}")
        hr = HR[0]
    if not hr[0].is_contiguous():
        hr = hr.contiguous()
    ts = tile_starts(T, num_frames, overlap_frames)
    if ts[-1] + num_frames > T:
        raise ValueError(f"best_window_clips: windows of {num_frames} frames do not fit {T} frames")
    dev = inputs.device
    canvas = torch.zeros(T, C, hh, ww, dtype=torch.float32, device=dev)
    best = torch.zeros(2, T, dtype=torch.float32, device=dev)
    choice = torch.zeros(2, T, dtype=torch.int32, device=dev)
    table = torch.zeros(T, len(ts), dtype=torch.float32, device=dev) if return_scores else None
    ws = torch.empty(max(K.frame_sqerr_ws_bytes(num_frames, C, hh, ww), 8), dtype=torch.uint8, device=dev)
    err = torch.empty(num_frames, dtype=torch.float64, device=dev)
    for idx, t in enumerate(ts):
        clip = inputs[:, t:t + num_frames]
        out = model(clip) if overlap_spatial is None else test_image(model, clip, test_spatial, overlap_spatial, scale)
        if tuple(out.shape) != (1, num_frames, C, hh, ww):
            raise ValueError(f"best_window_clips: the network returned {tuple(out.shape)} for window {idx}, expected {(1, num_frames, C, hh, ww)}")
        o = out[0]
        if o.dtype not in (torch.float32, torch.bfloat16):
            o = o.float()
        if not o[0].is_contiguous():
            o = o.contiguous()
        cur, nxt = idx & 1, (idx + 1) & 1
        K.frame_sqerr(o, hr[t:t + num_frames], ws, err)
        K.best_window_select(o, err, t, idx, PSNR_CAP, canvas, best[cur], choice[cur], best[nxt], choice[nxt], table)
    frames = canvas.to(inputs.dtype)
    if return_scores:
        last = len(ts) & 1
        return frames, (choice[last], best[last], table)
    return frames


def _augment(x: torch.Tensor, hflip: bool, vflip: bool, rot90: bool, interleaved: bool = False) -> torch.Tensor:
    """Tester.augment / augment_inverse (tools/Tester.py:387-445; the two are the same function): flip the width axis, flip the height axis,
    swap the two, in this order.  Planar (..., H, W) tensors, or interleaved (T, H, W, 3) ones."""
    ax_h, ax_w = (1, 2) if interleaved else (x.dim() - 2, x.dim() - 1)
    if hflip:
        x = x.flip(ax_w)
    if vflip:
        x = x.flip(ax_h)
    if rot90:
        x = x.transpose(ax_h, ax_w)
    return x.contiguous()


_U8_TO_UNIT = {}


def _u8_to_unit(device: torch.device) -> torch.Tensor:
    """The 256 values of numpy's byte.astype(np.float32) / 255. -- numpy's own quotients, so the bits are the reference's."""
    lut = _U8_TO_UNIT.get(device)
    if lut is None:
        lut = _U8_TO_UNIT[device] = torch.from_numpy(np.arange(256).astype(np.float32) / 255.).to(device)
    return lut


@torch.no_grad()
def evaluate_reds(model: Callable, lr_u8: torch.Tensor, hr_u8: torch.Tensor, num_frames: int, overlap_frames: int,
                  test_spatial: Optional[Sequence[int]] = None, overlap_spatial: Optional[int] = None, scale: int = 4, hflip: bool = False,
                  vflip: bool = False, rot90: bool = False) -> torch.Tensor:
    """Tester.evaluate for dataset_name == 'REDS' (tools/Tester.py:215-252) from uint8 frames to uint8 frames on the device: lr_u8 (T, H, W, 3)
    and hr_u8 (T, 4H, 4W, 3) RGB -> (T, 4H, 4W, 3) uint8, the frames metrics.frame_metrics scores.  The LR clip becomes (1, T, 3, H, W) fp32 as
    byte / 255; HR stays uint8 and is scored where it lies (best_window_clips).
    hflip / vflip / rot90: the reference's data_enhance.  Tester.augment runs on both clips before the network and Tester.augment_inverse --
    the same three steps in the same order -- on the output.  A single flag (or all three) is undone by that; exactly one flip together with rot90 comes
    back rotated by 180 degrees, as the reference's frames do.  With flags on the HR clip is materialised once more, as flipped uint8."""
    hip.require_cuda(lr_u8, hr_u8)
    if lr_u8.dtype != torch.uint8 or hr_u8.dtype != torch.uint8 or lr_u8.dim() != 4 or hr_u8.dim() != 4 or lr_u8.shape[3] != 3 or hr_u8.shape[3] != 3:
        raise ValueError(f"evaluate_reds: uint8 (T, H, W, 3) and (T, 4H, 4W, 3) expected, got {lr_u8.dtype} {tuple(lr_u8.shape)} and "
                         f"{hr_u8.dtype} {tuple(hr_u8.shape)}")
    x = _u8_to_unit(lr_u8.device)[lr_u8.permute(0, 3, 1, 2).long()].unsqueeze(0)  # 1, T, 3, H, W
    hr = hr_u8
    enhance = hflip or vflip or rot90
    if enhance:
        x = _augment(x, hflip, vflip, rot90)
        hr = _augment(hr, hflip, vflip, rot90, interleaved=True)
    out = best_window_clips(model, x.contiguous(), hr, num_frames, overlap_frames, test_spatial, overlap_spatial, scale)
    if enhance:
        out = _augment(out, hflip, vflip, rot90)
    return to_uint8_device(out).permute(0, 2, 3, 1)


@torch.no_grad()
def to_uint8_device(outputs: torch.Tensor) -> torch.Tensor:
    """tools/Tester.py:249-250 without the host copy: clamp, *255, round half to even -> torch.uint8 (T, 3, H, W) on the device (the
    values of to_uint8; what metrics.frame_metrics scores)."""
    hip.require_cuda(outputs)
    o = outputs.float().squeeze().contiguous()
    if o.dim() == 3:  # (a single frame: .squeeze() took its T axis too)
        o = o.unsqueeze(0)
    return _finalize(o, torch.ones_like(o), want_u8=True)


@torch.no_grad()
def to_uint8(outputs: torch.Tensor) -> np.ndarray:
    """tools/Tester.py:249-250: clamp, *255, round half to even, uint8, (T, H, W, C) on the host."""
    hip.require_cuda(outputs)
    o = outputs.float().squeeze().contiguous()
    ones = torch.ones_like(o)
    u8 = _finalize(o, ones, want_u8=True)
    return np.ascontiguousarray(u8.cpu().numpy().transpose(0, 2, 3, 1))


# ---- Tester.evaluate on the device: uint8 frames in, uint8 frames out (one conversion kernel each way) ----------------------------------
def _frames_view(frames: torch.Tensor, what: str, dtypes) -> torch.Tensor:
    """The (T, 3, H, W) view (no copy) of planar (T, 3, H, W) or interleaved (T, H, W, 3) frames, themselves views of any strides.  A length-3
    axis in front is taken for the channels (as metrics.frame_metrics reads its frames), else the one at the end."""
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
        raise ValueError(f"{what}: (T, H, W, 3) or (T, 3, H, W) frames expected, got {tuple(frames.shape) if isinstance(frames, torch.Tensor) else type(frames)}")
    if frames.dtype not in dtypes:
        raise ValueError(f"{what}: {' / '.join(str(d) for d in dtypes)} expected, got {frames.dtype}")
    if frames.shape[1] == 3:
        return frames
    if frames.shape[3] == 3:
        return frames.permute(0, 3, 1, 2)
    raise ValueError(f"{what}: no RGB axis of length 3 in {tuple(frames.shape)}")


def _check_out(out: torch.Tensor, shape, dtype, what: str) -> torch.Tensor:
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype:
        raise ValueError(f"{what}: out must be {dtype} {tuple(shape)}, got {getattr(out, 'dtype', None)} {tuple(getattr(out, 'shape', ()))}")
    return out


@torch.no_grad()
def frames_to_clip(frames_u8: torch.Tensor, dtype: torch.dtype = torch.float32, hflip: bool = False, vflip: bool = False, rot90: bool = False,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Tester.evaluate's way in (tools/Tester.py:217-221): uint8 (T, H, W, 3) or (T, 3, H, W) frames, or views of them, -> the (1, T, 3, H', W')
    clip of byte / 255 in `dtype` (fp32: numpy's quotients bit for bit; bf16: those rounded once), Tester.augment applied ((H', W') = (W, H) with
    rot90).  One launch of vmg_convert_frames; the frames are read where they lie.  out: a (1, T, 3, H', W') tensor of `dtype`, any strides."""
    from . import kernels as K
    hip.require_cuda(frames_u8, out)
    src = _frames_view(frames_u8, "frames_to_clip", (torch.uint8,))
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"frames_to_clip: the clip is float32 or bfloat16, got {dtype}")
    T, _, H, W = src.shape
    shape = (1, T, 3, W, H) if rot90 else (1, T, 3, H, W)
    out = torch.empty(shape, dtype=dtype, device=src.device) if out is None else _check_out(out, shape, dtype, "frames_to_clip")
    K.convert_frames(src, out[0], hflip, vflip, rot90)
    return out


@torch.no_grad()
def clip_to_frames(clip: torch.Tensor, hflip: bool = False, vflip: bool = False, rot90: bool = False, planar: bool = False,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Tester.evaluate's way out (tools/Tester.py:245-250): a (1, T, 3, h, w) or (T, 3, h, w) fp32 / bf16 clip of any strides -> contiguous uint8
    (T, H', W', 3) frames -- (T, 3, H', W') with planar -- of clamp(0, 1) * 255 rounded half to even, Tester.augment_inverse applied first
    ((H', W') = (w, h) with rot90).  One launch; the result is the only allocation.  out: uint8 of the result's shape, any strides (a view
    into a larger buffer is written in place and nothing around it is touched)."""
    from . import kernels as K
    hip.require_cuda(clip, out)
    if not isinstance(clip, torch.Tensor) or clip.dim() not in (4, 5) or (clip.dim() == 5 and clip.shape[0] != 1) or clip.shape[-3] != 3:
        raise ValueError(f"clip_to_frames: a (1, T, 3, h, w) or (T, 3, h, w) clip expected, got {tuple(getattr(clip, 'shape', ()))}")
    if clip.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"clip_to_frames: a float32 or bfloat16 clip expected, got {clip.dtype}")
    src = clip[0] if clip.dim() == 5 else clip
    T, _, h, w = src.shape
    hh, ww = (w, h) if rot90 else (h, w)
    shape = (T, 3, hh, ww) if planar else (T, hh, ww, 3)
    out = torch.empty(shape, dtype=torch.uint8, device=src.device) if out is None else _check_out(out, shape, torch.uint8, "clip_to_frames")
    K.convert_frames(src, out if planar else out.permute(0, 3, 1, 2), hflip, vflip, rot90)
    return out


@torch.no_grad()
def augment_frames(frames_u8: torch.Tensor, hflip: bool, vflip: bool, rot90: bool) -> torch.Tensor:
    """Tester.augment (== augment_inverse) on uint8 frames, (T, H, W, 3) or (T, 3, H, W) or views of them: contiguous frames of the same layout,
    one launch."""
    from . import kernels as K
    hip.require_cuda(frames_u8)
    src = _frames_view(frames_u8, "augment_frames", (torch.uint8,))
    T, _, H, W = src.shape
    hh, ww = (W, H) if rot90 else (H, W)
    if frames_u8.shape[1] == 3:
        out = torch.empty((T, 3, hh, ww), dtype=torch.uint8, device=src.device)
        K.convert_frames(src, out, hflip, vflip, rot90)
    else:
        out = torch.empty((T, hh, ww, 3), dtype=torch.uint8, device=src.device)
        K.convert_frames(src, out.permute(0, 3, 1, 2), hflip, vflip, rot90)
    return out


@torch.no_grad()
def evaluate(model: Callable, lr_u8: torch.Tensor, hr_u8: Optional[torch.Tensor] = None, dataset_name: str = "REDS", num_frames: int = 7,
             overlap_frames: int = 0, test_spatial: Optional[Sequence[int]] = None, overlap_spatial: Optional[int] = None, scale: int = 4,
             hflip: bool = False, vflip: bool = False, rot90: bool = False) -> torch.Tensor:
    """Tester.evaluate (tools/Tester.py:215-252) on the device: uint8 RGB frames lr_u8 (T, H, W, 3) -> uint8 (T, 4H, 4W, 3), the frames
    metrics.frame_metrics scores.  The three branches of the reference, chosen by dataset_name:
      'Vimeo90k_septuplet'  one network call on the whole clip, or test_image when overlap_spatial is set;
      'REDS'                best_window_clips against hr_u8 (T, 4H, 4W, 3), which is required (scored in place as byte / 255);
      any other name        test_clips (Vid4, UDM10, ...).
    The clip goes in through frames_to_clip (fp32, as the reference feeds the network) and comes out through clip_to_frames, one launch each.
    hflip / vflip / rot90: the reference's data_enhance, folded into those two launches -- Tester.augment on the way in (and on the HR clip, one
    more launch, uint8 -> uint8) and augment_inverse, the same three steps in the same order, on the way out.  As in the reference a single
    flag, both flips, or all three are undone by that; exactly one flip together with rot90 comes back rotated by 180 degrees (see evaluate_reds,
    whose bytes the REDS branch reproduces)."""
    hip.require_cuda(lr_u8, hr_u8)
    if not isinstance(lr_u8, torch.Tensor) or lr_u8.dtype != torch.uint8 or lr_u8.dim() != 4 or lr_u8.shape[3] != 3:
        raise ValueError(f"evaluate: uint8 (T, H, W, 3) frames expected, got {getattr(lr_u8, 'dtype', None)} {tuple(getattr(lr_u8, 'shape', ()))}")
    reds = isinstance(dataset_name, str) and dataset_name == "REDS"
    if reds:
        T, H, W, _ = lr_u8.shape
        if hr_u8 is None:
            raise ValueError("evaluate: the REDS branch picks each frame's window by its PSNR against HR: hr_u8 is required")
        if hr_u8.dtype != torch.uint8 or tuple(hr_u8.shape) != (T, H * scale, W * scale, 3):
            raise ValueError(f"evaluate: hr_u8 must be uint8 {(T, H * scale, W * scale, 3)}, got {hr_u8.dtype} {tuple(hr_u8.shape)}")
    x = frames_to_clip(lr_u8.permute(0, 3, 1, 2), torch.float32, hflip, vflip, rot90)
    if reds:
        hr = hr_u8
        if hflip or vflip or rot90:
            from . import kernels as K
            hr = torch.empty((T, W * scale, H * scale, 3) if rot90 else (T, H * scale, W * scale, 3), dtype=torch.uint8, device=hr_u8.device)
            K.convert_frames(hr_u8.permute(0, 3, 1, 2), hr.permute(0, 3, 1, 2), hflip, vflip, rot90)
        out = best_window_clips(model, x, hr, num_frames, overlap_frames, test_spatial, overlap_spatial, scale)
    elif isinstance(dataset_name, str) and dataset_name == "Vimeo90k_septuplet":
        out = model(x) if overlap_spatial is None else test_image(model, x, test_spatial, overlap_spatial, scale)
    else:
        out = test_clips(model, x, num_frames, overlap_frames, test_spatial, overlap_spatial, scale)
    if out.dtype not in (torch.float32, torch.bfloat16):
        out = out.float()
    return clip_to_frames(out, hflip, vflip, rot90)


def index_generation(num_output_frames: int, num_GT: int) -> List[List[int]]:
    """utils/eval_utils.py:38-61: the index lists a sequence of num_GT frames is evaluated in -- runs of num_output_frames frames that share
    one frame with their predecessor, plus one flush with the end when the last frame is not reached.  Host logic."""
    indices_list = []
    right = num_output_frames
    while right <= num_GT:
        indices_list.append(list(range(right - num_output_frames, right)))
        right += num_output_frames - 1
    if right - num_output_frames < num_GT - 1:
        indices_list.append(list(range(num_GT - num_output_frames, num_GT)))
    return indices_list


def _runs(positions: Sequence[int]) -> List[Tuple[int, int]]:
    """[lo, hi) runs of consecutive integers in an ascending list."""
    runs: List[Tuple[int, int]] = []
    for p in positions:
        if runs and runs[-1][1] == p:
            runs[-1] = (runs[-1][0], p + 1)
        else:
            runs.append((p, p + 1))
    return runs


@torch.no_grad()
def evaluate_sequence(model: Callable, lr_u8: torch.Tensor, gt_u8: torch.Tensor, num_out_frames: int, board, **evaluate_kwargs) -> torch.Tensor:
    """The per-sequence body of tools/test_reds4.py:155-250 between board.start_sequence(...) and board.end_sequence(), which stay with the
    caller: for every index list of index_generation(num_out_frames, N) the frames lr_u8[indices] (N, H, W, 3) go through evaluate (with
    gt_u8[indices] as HR on the REDS branch); the frames of the list that no earlier list has scored are scored against gt_u8 (N, 4H, 4W, 3) by
    metrics.frame_metrics and handed to board.add_clip, which keeps the reference's eval_mid_clip / use_mirrors positions.  Returns the
    (N, 4H, 4W, 3) uint8 frames, each as the first list that reached it produced it (the frames the reference writes to disk).  The host is
    synchronised only where frame_metrics reads its sums back, once per scored run of frames."""
    from . import metrics as M
    hip.require_cuda(lr_u8, gt_u8)
    if lr_u8.dim() != 4 or gt_u8.dim() != 4 or lr_u8.shape[0] != gt_u8.shape[0]:
        raise ValueError(f"evaluate_sequence: (N, H, W, 3) and (N, 4H, 4W, 3) frames expected, got {tuple(lr_u8.shape)} and {tuple(gt_u8.shape)}")
    N = lr_u8.shape[0]
    if not 1 <= int(num_out_frames) <= N:
        raise ValueError(f"evaluate_sequence: index lists of {num_out_frames} frames do not fit a sequence of {N}")
    reds = evaluate_kwargs.get("dataset_name", "REDS") == "REDS"
    frames = torch.empty_like(gt_u8, memory_format=torch.contiguous_format)
    scored = set()
    nan = float("nan")
    for indices in index_generation(int(num_out_frames), N):
        lo, hi = indices[0], indices[-1] + 1  # (an index list is a run of consecutive frames: a view, not a gather)
        out = evaluate(model, lr_u8[lo:hi], gt_u8[lo:hi] if reds else None, **evaluate_kwargs)
        new = [pos for pos, fr in enumerate(indices) if fr not in scored]
        cols = [[nan] * len(indices) for _ in M.METRICS]  # (add_clip skips the positions scored before; their slots are never read)
        for p0, p1 in _runs(new):
            frames[lo + p0:lo + p1].copy_(out[p0:p1])
            vals = M.frame_metrics(out[p0:p1], gt_u8[lo + p0:lo + p1])
            for col, v in zip(cols, vals):
                col[p0:p1] = v.tolist()
        scored.update(indices)
        board.add_clip(indices, cols)
    return frames
