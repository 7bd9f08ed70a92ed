"""Deferred, batched weight gradients: the scheduler behind vmg_amd.train.TrainStep's weight-gradient mode.

The recurrence applies one conv module to every frame in both directions (2T uses per step).  A weight gradient
per use has K = B*H*W pixels against a 144x144x9 fp32 output, so its float-atomic epilogue dominates.  Instead,
backward only RECORDS (input, output-gradient) pairs; when the last use of a parameter has been seen the pairs
are summed by ONE batched launch straight into param.grad (no zero-fill, no autograd accumulate kernels).
288 GB of HBM make keeping the pairs alive until then a non-issue.
"""
from __future__ import annotations

import collections
import contextlib
from typing import Optional

import torch

from . import kernels as K
from .hip import HipError


# one recorded use of a weight: the sources of the (virtually concatenated) input, their channel counts, the gradient of the pre-activation
# output, the convolution's geometry, the factor on this use's gradient and its first output channel
Use = collections.namedtuple("Use", "srcs src_ch dpre ks N H W scale o0")
# a parameter and the uses recorded for it so far
Pending = collections.namedtuple("Pending", "weight bias uses")
# what complete parameters must have in common to share one vmg_conv_wgrad3_multi / vmg_linear_wgrad2_multi launch
Sig = collections.namedtuple("Sig", "wshape nuses src_ch N H W xstride dstride ks")


def recorded(srcs, src_ch, dpre, ks, N, H, W, scale: float = 1.0, o0: int = 0) -> Use:
    """The one place a Use is made.  o0: first output channel of this use (a group of a grouped convolution writes rows o0 .. o0 + dpre
    channels of the gradient)."""
    return Use._make((srcs, tuple(src_ch), dpre, ks, N, H, W, float(scale), int(o0)))  # (_make: tuple.__new__, without the keyword-capable constructor's frame)


def _bias_grad(bias) -> Optional[torch.Tensor]:
    return bias.grad if (bias is not None and bias.requires_grad) else None


class _DeferredWgrad:
    """mode 'autograd' (default): every conv / Linear backward computes its weight gradient at once and returns it through
    autograd -- standard semantics, so torch DistributedDataParallel, GradScaler, clip_grad_norm_ and hooks all see it.
    mode 'deferred' (vmg_amd.train.TrainStep switches it on): backward only records the pairs, see above.

    Use counts are kept PER FORWARD PASS (a generation token taken in VMG.forward and stored in each autograd node), so
    a grad-enabled forward that is never back-propagated (an eval / logging call, a batch dropped after an exception)
    cannot leave counts behind that would silence a later step; and whatever is still pending when a backward() call ends
    is flushed by an end-of-backward engine callback, so no caller has to flush explicitly."""

    KEEP_GENERATIONS = 8

    def __init__(self):
        self.mode = "autograd"
        self.gen = 0
        self.uses = {}      # (generation, id(param)) -> outstanding forward uses
        self.pending = {}   # id(param) -> Pending
        self.callbacks = []  # called with each parameter whose .grad has just been completed
        self.managed = set()  # ids of the parameters (weights and their biases) whose gradient is completed HERE, not by autograd
        self._queued = False
        self.ready = []     # Pending whose last use has been seen, not batchable: launched by drain()
        self.waiting = {}   # Sig -> complete parameters waiting for company (launched at eight, or by drain())
        self.hold = 0       # > 0: a node that completes many parameters at once (a residual chain) is collecting them
        self.extra = {}     # (generation, id(param)) -> outstanding contributions of OTHER nodes to a managed bias (note_extra)
        self.held = {}      # id(param) -> param whose weight-gradient launch is done while such a contribution is still outstanding
        self.bw_gen = 0     # generation of the backward pass that is running (taken from the recorded uses)

    def begin_forward(self):
        """New top-level forward pass: a fresh generation; counts of passes older than KEEP_GENERATIONS are dropped."""
        self.gen += 1
        if self.uses or self.extra:
            lo = self.gen - self.KEEP_GENERATIONS
            for d in (self.uses, self.extra):
                for key in [k for k in d if k[0] < lo]:
                    del d[key]

    # -- the counts: one more outstanding in the forward (_count), one less in the backward (_last)
    def _count(self, counts, params) -> int:
        for p in params:
            key = (self.gen, id(p))
            counts[key] = counts.get(key, 0) + 1
            self.managed.add(id(p))
        return self.gen

    @staticmethod
    def _last(counts, key) -> bool:
        """One less outstanding under `key` (a key that was never counted stands for one): was it the last?"""
        left = counts.get(key, 1) - 1
        if left > 0:
            counts[key] = left
            return False
        counts.pop(key, None)
        return True

    def _report(self, p):
        for cb in self.callbacks:
            cb(p)

    def defers(self, weight, bias, wanted: bool) -> bool:
        """A conv / Linear node records this weight's gradient here (add) instead of returning it through autograd."""
        return self.mode == "deferred" and isinstance(weight, torch.nn.Parameter) and wanted and \
            (bias is None or isinstance(bias, torch.nn.Parameter))

    def note_use(self, weight, bias=None) -> int:
        if bias is not None:
            self.managed.add(id(bias))  # managed, not counted: the weight's launch writes it and reports it with the weight (_launch)
        return self._count(self.uses, (weight,))

    # -- small parameters (LayerNorm affine, squeeze-excite MLPs): in mode 'deferred' their backward kernels add straight into .grad
    #    (no zero-filled temporaries, no AccumulateGrad add per parameter)
    def direct(self, *params) -> bool:
        return self.mode == "deferred" and all(p is not None and p.requires_grad and p.is_leaf for p in params)

    def note_params(self, *params) -> int:
        return self._count(self.uses, params)

    # the three steps of a node with such parameters: claim() in its forward, into() and done() in its backward
    def claim(self, ctx, *params):
        """Decides whether the node's backward adds straight into .grad (ctx.direct) and, if so, counts this use of the parameters."""
        ctx.direct = self.direct(*params)
        if ctx.direct:
            ctx.params, ctx.gen = params, self.note_params(*params)

    def into(self, ctx):
        """The parameters' .grad buffers for the backward kernel to add into, or None: the gradients are returned through autograd."""
        return tuple(self.grad_of(p) for p in ctx.params) if ctx.direct else None

    def done(self, ctx):
        """This use of the parameters is complete, whether the backward kernel ran or the node had nothing to add."""
        if ctx.direct:
            self.written(ctx.gen, *ctx.params)

    # -- a bias that a Linear / conv manages (its gradient is written by the deferred weight-gradient launch) may ALSO receive gradient from
    #    another node -- the 3-D window attention's q / kv biases, through the zero-padded positions (models/swin_3d.py: the padding is added
    #    before the Linears, so a padded token's q is the bias).  That node adds straight into .grad and the bias counts as complete only
    #    when BOTH have written: reporting it at the weight-gradient launch alone let the gradient reducer start the bucket's all-reduce
    #    while the attention backward's add was still to come (replicas diverge).
    def note_extra(self, *params) -> int:
        return self._count(self.extra, params)

    def extra_written(self, gen: int, *params):
        for p in params:
            if self._last(self.extra, (gen, id(p))) and self.held.pop(id(p), None) is not None:
                self._report(p)

    def _complete(self, p):
        """The deferred launch that writes p's gradient has been issued: report p, unless another node still owes it a contribution."""
        if self.extra and self.extra.get((self.bw_gen, id(p)), 0) > 0:
            self.held[id(p)] = p
            return
        self._report(p)

    @staticmethod
    def grad_of(p: torch.Tensor) -> torch.Tensor:
        if p.grad is None:
            p.grad = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
        return p.grad

    def written(self, gen: int, *params):
        for p in params:
            if self._last(self.uses, (gen, id(p))):
                self._report(p)

    def add(self, weight, bias, srcs, src_ch, dpre, ks, N, H, W, scale: float = 1.0, gen: int = 0, o0: int = 0):
        """Records one use (see recorded()); the parameter's gradient is launched when its last use of this pass has been seen."""
        pend = self.pending.get(id(weight))
        if pend is None:
            pend = self.pending[id(weight)] = Pending(weight, bias, [])
        pend.uses.append(recorded(srcs, src_ch, dpre, ks, N, H, W, scale, o0))
        self.bw_gen = gen
        if not self._queued:  # whatever is still pending when this backward() call ends is completed then
            torch.autograd.Variable._execution_engine.queue_callback(self._end_of_backward)
            self._queued = True
        if self._last(self.uses, (gen, id(weight))):
            self.flush(weight)

    def _end_of_backward(self):
        self._queued = False
        for key in list(self.pending):
            self.flush(self.pending[key].weight)
        self.hold = 0
        self.drain()
        if self.held:  # (a contribution that never came -- its node was not part of this backward: the gradient is what it is)
            held, self.held = self.held, {}
            for p in held.values():
                self._report(p)

    def flush(self, weight):
        pend = self.pending.pop(id(weight), None)
        if pend is None:
            return
        sig = self._multi_sig(pend)  # computed ONCE per parameter and step (this runs on the autograd thread, with the GPU waiting behind it)
        if sig is None:
            if self.hold:
                self.ready.append(pend)
            else:
                self._launch([pend], None)
            return
        lst = self.waiting.setdefault(sig, [])
        lst.append(pend)
        if len(lst) >= 8 and not self.hold:
            self._launch(self.waiting.pop(sig), sig)

    @staticmethod
    def _multi_sig(pend):
        """Signature under which complete parameters can share one vmg_conv_wgrad3_multi / vmg_linear_wgrad2_multi launch, or None."""
        weight, _, uses = pend
        u0 = uses[0]
        ks, src_ch, x0, d0 = u0.ks, u0.src_ch, u0.srcs[0], u0.dpre
        if len(src_ch) != 1 or ks not in (1, 3) or weight.shape[1] != src_ch[0] or (ks == 3 and weight.dim() != 4):
            return None
        if any(u.o0 for u in uses) or d0.shape[-1] != weight.shape[0]:
            return None  # (groups of a grouped convolution: the general batched kernel, per output-row range)
        if x0.shape[-1] != src_ch[0] or not K.conv_wgrad3_multi_ok(x0, d0, ks):
            return None
        xs0, ds0, xt0, dt0, g0 = x0.shape, d0.shape, x0.stride(), d0.stride(), (ks, u0.N, u0.H, u0.W, u0.scale)
        for u in uses[1:]:
            x, d = u.srcs[0], u.dpre
            if u.src_ch != src_ch or (u.ks, u.N, u.H, u.W, u.scale) != g0 or x.shape != xs0 or d.shape != ds0 or x.stride() != xt0 or d.stride() != dt0 or \
                    not K.conv_wgrad3_multi_ok(x, d, ks):
                return None
        return Sig(tuple(weight.shape), len(uses), src_ch, u0.N, u0.H, u0.W, tuple(xt0), tuple(dt0), ks)

    def _launch(self, pends, sig):
        """The gradients of the complete parameters `pends`: one by one (sig None or a single parameter) or eight per launch."""
        for weight, bias, _ in pends:
            self.grad_of(weight)
            if bias is not None and bias.requires_grad:
                self.grad_of(bias)
        if sig is None or len(pends) < 2:
            for weight, bias, uses in pends:
                _wgrad_entries(uses, weight.grad, _bias_grad(bias))
        else:
            probs = [([u.srcs[0] for u in uses], [u.dpre for u in uses], weight.grad, _bias_grad(bias), uses[0].scale) for weight, bias, uses in pends]
            if sig.ks == 3:
                K.conv_wgrad3_multi(probs, sig.N, sig.H, sig.W)
            else:
                K.linear_wgrad2_multi(probs, sig.N * sig.H * sig.W)
        for weight, bias, _ in pends:
            self._report(weight)
            if bias is not None and bias.requires_grad:
                self._complete(bias)

    @contextlib.contextmanager
    def collecting(self):
        """Around the add() calls of a node that completes many parameters at once (a residual chain): nothing is launched inside, and at
        the outermost exit everything complete is (drain), so the node's parameters share launches.  A body that raises leaves the hold
        to the end of the backward pass."""
        self.hold += 1
        yield
        self.hold -= 1
        if not self.hold:
            self.drain()

    def drain(self):
        """Launch everything that is complete: parameters of one shape share launches (eight per launch).  Between drains (a residual
        chain completing, the end of the backward pass) shapes that can share a launch wait in `waiting` until eight of them are complete
        -- the two 3x3 convs of every RCAB, one per TAB, cost three launches per step instead of 24."""
        if self.ready:
            ready, self.ready = self.ready, []
            self._launch(ready, None)
        if self.waiting:
            waiting, self.waiting = self.waiting, {}
            for sig, pends in waiting.items():
                self._launch(pends, sig)

    def flush_all(self):
        self._end_of_backward()
        self.uses.clear()


def _wgrad_entries(uses, dW, db):
    """dW (+= ) the weight gradient of every recorded use, batched by shape."""
    groups = {}
    for u in uses:
        groups.setdefault((u.src_ch, u.ks, u.N, u.H, u.W, u.scale, u.o0, u.dpre.dtype, u.dpre.shape[-1]), []).append(u)
    for (src_ch, ks, N, H, W, scale, o0, _, _), us in groups.items():
        off = 0
        for i, c in enumerate(src_ch):
            xs = [u.srcs[i][..., :c] if u.srcs[i].shape[-1] != c else u.srcs[i] for u in us]
            K.conv_wgrad_batched(xs, [u.dpre for u in us], dW, db if i == 0 else None, ks, N, H, W, scale=scale, i0=off, o0=o0)
            off += c


def _wgrad_now(weight, bias_needed: bool, srcs, src_ch, dpre, ks, N, H, W, scale: float = 1.0):
    """(dW, db) of one use, as fresh fp32 tensors (mode 'autograd')."""
    dW = torch.zeros(weight.shape, dtype=torch.float32, device=weight.device)
    db = torch.zeros(weight.shape[0], dtype=torch.float32, device=weight.device) if bias_needed else None
    _wgrad_entries([recorded(srcs, src_ch, dpre, ks, N, H, W, scale)], dW, db)
    return dW, db


DEFERRED = _DeferredWgrad()


def set_wgrad_mode(mode: str):
    """'autograd' (default; weight gradients flow through autograd, DDP-compatible) or 'deferred' (batched per parameter,
    written straight into .grad; the mode of vmg_amd.train.TrainStep / GradBucketReducer)."""
    if mode not in ("autograd", "deferred"):
        raise HipError(f"wgrad mode {mode!r}: 'autograd' or 'deferred'")
    if mode != DEFERRED.mode:
        DEFERRED.flush_all()
        DEFERRED.managed.clear()
        DEFERRED.mode = mode


def flush_deferred_wgrads():
    """Completes every pending deferred gradient now (the end-of-backward callback does this by itself; kept for callers
    that read .grad from inside a backward hook)."""
    DEFERRED.flush_all()
