"""The deferred weight-gradient scheduler (vmg_amd.wgrad, re-exported as vmg_amd.functional.DEFERRED) on its own, on the host: the three launch functions are replaced
by recorders and the scheduler is driven from a small autograd node on CPU tensors, so every rule it keeps -- use counts per forward pass,
eight parameters per launch, hold and drain around a residual chain, the end-of-backward flush, the order of the completion callbacks, the
bias that waits for another node's contribution -- is pinned as WHICH launches are made, in which order, and what is reported when.  The
expected values are the rules as the scheduler's comments state them."""
import collections
import types

import pytest
import torch

import vmg_amd.functional as FH
import vmg_amd.kernels as K
from vmg_amd.hip import HipError

D = FH.DEFERRED

# one recorded launch: dW / db are indices into the test's parameter list (None: a buffer that is no parameter's .grad, or no bias gradient)
Launch = collections.namedtuple("Launch", "kind nprob pairs dW db ks scale o0 i0 dims cin")


_collecting = D.collecting  # what a residual chain's backward puts around its add() calls


class _Node(torch.autograd.Function):
    """Passes x through; the forward runs fwd() (note_use / note_params / note_extra: returns the generation), the backward runs bwd(generation)."""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd, ctx.gen = bwd, fwd()
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.bwd(ctx.gen)
        return g, None, None


class _World:
    def __init__(self):
        self.P, self.log, self.fired = [], [], []

    def param(self, *shape, requires_grad=True):
        p = torch.nn.Parameter(torch.zeros(shape), requires_grad=requires_grad)
        self.P.append(p)
        return p

    def layer(self, cout=16, cin=16, ks=3, bias_grad=True):
        """(weight, bias) of a ks x ks convolution (ks 1: a Linear's 2-D weight)."""
        w = self.param(cout, cin, ks, ks) if ks > 1 else self.param(cout, cin)
        return w, self.param(cout, requires_grad=bias_grad)

    def ix(self, p):
        return next(i for i, q in enumerate(self.P) if q is p)

    def grad_ix(self, t):
        return None if t is None else next((i for i, q in enumerate(self.P) if q.grad is t), None)

    def forward(self, fwd, bwd):
        x = torch.zeros(1, requires_grad=True)
        return _Node.apply(x, fwd, bwd)

    def run(self, fwd, bwd):
        self.forward(fwd, bwd).sum().backward()

    # the launches a test expects
    def batched(self, w, b, pairs=1, ks=3, scale=1.0, o0=0, i0=0, dims=(1, 4, 4), cin=16):
        return Launch("batched", 1, (pairs,), (self.ix(w),), (None if b is None else self.ix(b),), ks, (scale,), o0, i0, dims, cin)

    def multi(self, layers, pairs=1, scales=None, kind="multi3", dims=(1, 4, 4), cin=16):
        n = len(layers)
        return Launch(kind, n, (pairs,) * n, tuple(self.ix(w) for w, _ in layers), tuple(self.ix(b) for _, b in layers),
                      3 if kind == "multi3" else 1, tuple(scales) if scales else (1.0,) * n, 0, 0, dims, cin)

    def both(self, layers):
        """Callback order of one launch: each weight, then its bias, in the launch's parameter order."""
        return [self.ix(p) for w, b in layers for p in (w, b)]


@pytest.fixture(autouse=True)
def world(monkeypatch):
    wd = _World()

    def rec_batched(xs, dys, dW, db, ks, N, H, W, scale=1.0, o0=0, i0=0):
        assert len(xs) == len(dys)
        wd.log.append(Launch("batched", 1, (len(xs),), (wd.grad_ix(dW),), (wd.grad_ix(db),), ks, (scale,), o0, i0, (N, H, W), xs[0].shape[-1]))

    def rec_multi(kind, ks):
        def rec(probs, *dims):
            wd.log.append(Launch(kind, len(probs), tuple(len(p[0]) for p in probs), tuple(wd.grad_ix(p[2]) for p in probs),
                                 tuple(wd.grad_ix(p[3]) for p in probs), ks, tuple(p[4] for p in probs), 0, 0, tuple(dims), probs[0][0][0].shape[-1]))
        return rec

    monkeypatch.setattr(K, "conv_wgrad_batched", rec_batched)
    monkeypatch.setattr(K, "conv_wgrad3_multi", rec_multi("multi3", 3))
    monkeypatch.setattr(K, "linear_wgrad2_multi", rec_multi("linear2", 1))
    saved = list(D.callbacks)
    FH.set_wgrad_mode("deferred")
    D.callbacks[:] = [lambda p: wd.fired.append(wd.ix(p))]
    D.begin_forward()
    yield wd
    FH.set_wgrad_mode("autograd")  # (while the recorders are still in place)
    D.callbacks[:] = saved


def act(c=16, dtype=torch.bfloat16, shape=(1, 4, 4)):
    return torch.zeros(*shape, c, dtype=dtype)


def add(layer, gen, x=None, d=None, src_ch=None, ks=3, dims=(1, 4, 4), **kw):
    """One recorded use of `layer`: bf16 (1,4,4,16) activations unless given."""
    w, b = layer
    xs = x if isinstance(x, list) else [act() if x is None else x]
    D.add(w, b, xs, src_ch or [t.shape[-1] for t in xs], act(w.shape[0]) if d is None else d, ks, *dims, gen=gen, **kw)


def fp32_layer(wd):
    """A layer that can share no launch (fp32 activations): its gradient is launched the moment its last use is recorded."""
    layer = wd.layer()
    return layer, dict(x=act(dtype=torch.float32), d=act(dtype=torch.float32))


# ---- use counts per forward pass -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_parameter_used_k_times_launches_once_after_its_kth_use(world, k):
    layer, io = fp32_layer(world)

    def fwd():
        for _ in range(k):
            gen = D.note_use(*layer)
        return gen

    def bwd(gen):
        for i in range(k):
            assert world.log == [] and world.fired == []
            add(layer, gen, **io)
        assert world.log == [world.batched(*layer, pairs=k)]
        assert world.fired == world.both([layer])

    world.run(fwd, bwd)
    assert len(world.log) == 1 and world.fired == world.both([layer])


def test_forward_without_backward_does_not_delay_the_next_pass(world):
    layer, io = fp32_layer(world)
    world.forward(lambda: D.note_use(*layer), None)  # a grad-enabled forward that is never back-propagated
    D.begin_forward()

    def bwd(gen):
        add(layer, gen, **io)
        assert world.log == [world.batched(*layer)]  # at once: the first pass's count is not this pass's

    world.run(lambda: D.note_use(*layer), bwd)
    assert world.log == [world.batched(*layer)] and world.fired == world.both([layer])


@pytest.mark.parametrize("passes, dropped", [(D.KEEP_GENERATIONS, False), (D.KEEP_GENERATIONS + 1, True)])
def test_counts_older_than_keep_generations_are_dropped(world, passes, dropped):
    layer, io = fp32_layer(world)

    def fwd():
        D.note_use(*layer)
        return D.note_use(*layer)

    y = world.forward(fwd, lambda gen: (add(layer, gen, **io), seen.append(list(world.log))))
    seen = []
    for _ in range(passes):
        D.begin_forward()
    y.sum().backward()  # ONE of the two counted uses arrives
    # count kept: the parameter still waits for its second use when the node returns (the end of the backward pass completes it);
    # count dropped: an uncounted use completes the parameter at once
    assert seen == [[world.batched(*layer)] if dropped else []]
    assert world.log == [world.batched(*layer)]


# ---- eight per launch, the end-of-backward flush ---------------------------------------------------------------------------------------------------
def test_eight_complete_parameters_share_a_launch_the_ninth_goes_alone(world):
    layers = [world.layer() for _ in range(9)]

    def bwd(gen):
        for i, layer in enumerate(layers):
            assert world.log == ([] if i < 8 else [world.multi(layers[:8])])
            add(layer, gen)
        assert world.fired == world.both(layers[:8])

    world.run(lambda: [D.note_use(*layer) for layer in layers][-1], bwd)
    assert world.log == [world.multi(layers[:8]), world.batched(*layers[8])]
    assert world.fired == world.both(layers)


def test_nine_one_use_parameters_and_a_second_use_of_the_first(world):
    layers = [world.layer() for _ in range(9)]

    def bwd(gen):
        for layer in layers:
            add(layer, gen)
        assert world.log == [world.multi(layers[1:])]  # the eighth COMPLETE parameter triggers the launch; the first still waits for its second use
        add(layers[0], gen)

    world.run(lambda: [D.note_use(*layer) for layer in layers + layers[:1]][-1], bwd)
    assert world.log == [world.multi(layers[1:]), world.batched(*layers[0], pairs=2)]
    assert sorted(world.fired) == list(range(18)) and world.fired == world.both(layers[1:] + layers[:1])


def test_two_same_signature_parameters_at_the_end_of_backward(world):
    a, b = world.layer(), world.layer()

    def bwd(gen):
        for _ in range(2):
            add(a, gen, scale=0.1)
            add(b, gen)
        assert world.log == []

    world.run(lambda: [D.note_use(*layer) for layer in (a, b, a, b)][-1], bwd)
    assert world.log == [world.multi([a, b], pairs=2, scales=(0.1, 1.0))]
    assert world.fired == world.both([a, b])


def test_different_use_counts_do_not_share_a_launch(world):
    a, b = world.layer(), world.layer()
    world.run(lambda: [D.note_use(*layer) for layer in (a, b, b)][-1], lambda gen: [add(layer, gen) for layer in (a, b, b)])
    assert world.log == [world.batched(*a), world.batched(*b, pairs=2)]


# ---- 1x1 ------------------------------------------------------------------------------------------------------------------------------------------
def test_linear_with_2048_pixels_goes_through_linear_wgrad2_multi(world):
    a, b = world.layer(ks=1), world.layer(ks=1)
    io = lambda: dict(x=act(shape=(2048,)), d=act(shape=(2048,)), ks=1, dims=(1, 1, 2048))
    world.run(lambda: [D.note_use(*layer) for layer in (a, b)][-1], lambda gen: [add(layer, gen, **io()) for layer in (a, b)])
    assert world.log == [world.multi([a, b], kind="linear2", dims=(2048,))]
    assert world.fired == world.both([a, b])


@pytest.mark.parametrize("M, c", [(2047, 16), (2048, 12)])
def test_small_or_unaligned_linear_goes_one_by_one(world, M, c):
    a, b = world.layer(cin=c, ks=1), world.layer(cin=c, ks=1)
    io = lambda: dict(x=act(c, shape=(M,)), d=act(shape=(M,)), ks=1, dims=(1, 1, M))
    world.run(lambda: [D.note_use(*layer) for layer in (a, b)][-1], lambda gen: [add(layer, gen, **io()) for layer in (a, b)])
    assert world.log == [world.batched(*layer, ks=1, dims=(1, 1, M), cin=c) for layer in (a, b)]


# ---- what never shares a launch --------------------------------------------------------------------------------------------------------------------
def _unbatchable(world, name):
    """(layer, add() keywords, expected launches) of one use that has no multi-launch signature."""
    if name == "two_sources":
        layer = world.layer()
        return layer, dict(x=[act(8), act(8)]), [world.batched(*layer, cin=8), world.batched(layer[0], None, i0=8, cin=8)]  # (the bias with the first source)
    if name == "src_ch_below_weight":
        layer = world.layer()
        return layer, dict(x=act(8)), [world.batched(*layer, cin=8)]
    if name == "padded_source":  # a 12-channel source carried in a 16-channel tensor: the launch reads the 12-channel slice
        layer = world.layer(cin=12)
        return layer, dict(x=act(16), src_ch=[12]), [world.batched(*layer, cin=12)]
    if name == "o0":
        layer = world.layer(cout=32)
        return layer, dict(d=act(16), o0=16), [world.batched(*layer, o0=16)]
    if name == "fp32":
        layer = world.layer()
        return layer, dict(x=act(dtype=torch.float32), d=act(dtype=torch.float32)), [world.batched(*layer)]
    if name == "misaligned":
        layer = world.layer()
        x = act(24)[..., 4:20]  # 8 bytes past a 16-byte boundary
        assert x.data_ptr() % 16 == 8
        return layer, dict(x=x), [world.batched(*layer)]
    if name == "ks7":
        layer = world.layer(ks=7)
        return layer, dict(ks=7), [world.batched(*layer, ks=7)]
    raise KeyError(name)


@pytest.mark.parametrize("name", ["two_sources", "src_ch_below_weight", "padded_source", "o0", "fp32", "misaligned", "ks7"])
def test_no_signature_goes_through_conv_wgrad_batched(world, name):
    """Two such parameters complete in one backward: one conv_wgrad_batched call per parameter and source, at once, never a multi launch."""
    cases = [_unbatchable(world, name) for _ in range(2)]

    def bwd(gen):
        want = []
        for layer, kw, launches in cases:
            add(layer, gen, **kw)
            want += launches
            assert world.log == want

    world.run(lambda: [D.note_use(*layer) for layer, _, _ in cases][-1], bwd)
    assert world.fired == world.both([layer for layer, _, _ in cases])


def test_uses_with_different_strides_do_not_share_a_multi_launch(world):
    layers = [world.layer(), world.layer()]
    strided = act(32)[..., :16]  # 16-byte aligned, pixel stride 32
    assert K.conv_wgrad3_multi_ok(strided, act(), 3)

    def bwd(gen):
        for layer in layers:
            add(layer, gen)
            add(layer, gen, x=strided)

    world.run(lambda: [D.note_use(*layer) for layer in layers + layers][-1], bwd)
    assert [l.kind for l in world.log] == ["batched", "batched"] and [l.dW for l in world.log] == [(world.ix(w),) for w, _ in layers]
    assert sum(sum(l.pairs) for l in world.log) == 4


# ---- hold and drain ----------------------------------------------------------------------------------------------------------------------------------
def test_hold_collects_and_drains_ready_before_waiting(world):
    same = [world.layer() for _ in range(3)]
    odd, io = fp32_layer(world)

    def bwd(gen):
        with _collecting():
            add(same[0], gen)
            add(same[1], gen)
            add(odd, gen, **io)
            add(same[2], gen)
            assert world.log == [] and world.fired == []
        assert world.log == [world.batched(*odd), world.multi(same)]
        assert world.fired == world.both([odd] + same)

    world.run(lambda: [D.note_use(*layer) for layer in same + [odd]][-1], bwd)
    assert len(world.log) == 2 and len(world.fired) == 8


def test_hold_keeps_more_than_eight_together(world):
    layers = [world.layer() for _ in range(9)]

    def bwd(gen):
        with _collecting():
            for layer in layers:
                add(layer, gen)
            assert world.log == []
        assert world.log == [world.multi(layers)]  # (the launch function slices nine problems into eight and one)

    world.run(lambda: [D.note_use(*layer) for layer in layers][-1], bwd)


def test_nested_holds_drain_at_the_outermost_release_only(world):
    a, b = world.layer(), world.layer()

    def bwd(gen):
        with _collecting():
            with _collecting():
                add(a, gen)
            assert world.log == []
            add(b, gen)
        assert world.log == [world.multi([a, b])]

    world.run(lambda: [D.note_use(*layer) for layer in (a, b)][-1], bwd)


def test_a_hold_whose_body_raised_does_not_drain_and_the_end_of_backward_recovers(world):
    a, b = world.layer(), world.layer()

    def bwd(gen):
        with pytest.raises(ZeroDivisionError):
            with _collecting():
                add(a, gen)
                add(b, gen)
                1 / 0
        assert world.log == []

    world.run(lambda: [D.note_use(*layer) for layer in (a, b)][-1], bwd)
    assert world.log == [world.multi([a, b])]
    odd, io = fp32_layer(world)  # the next backward is not held
    world.run(lambda: D.note_use(*odd), lambda gen: (add(odd, gen, **io), world.log.append("returned")))
    assert world.log[1:] == [world.batched(*odd), "returned"]


# ---- callbacks -----------------------------------------------------------------------------------------------------------------------------------------
def test_callbacks_fire_once_per_parameter_in_launch_order(world):
    layers = [world.layer() for _ in range(3)]
    nobias = (world.param(16, 16, 3, 3), None)
    frozen = world.layer(bias_grad=False)  # a bias that takes no gradient: neither written nor reported
    everyone = [layers[2], nobias, layers[0], frozen, layers[1]]

    def fwd():
        for w, b in everyone:
            gen = D.note_use(w, b)
        return gen

    world.run(fwd, lambda gen: [add(layer, gen) for layer in everyone])
    assert world.log == [Launch("multi3", 5, (1,) * 5, tuple(world.ix(w) for w, _ in everyone),
                                (world.ix(layers[2][1]), None, world.ix(layers[0][1]), None, world.ix(layers[1][1])), 3, (1.0,) * 5, 0, 0, (1, 4, 4), 16)]
    assert world.fired == [world.ix(p) for w, b in everyone for p in (w, b) if p is not None and p.requires_grad]
    assert frozen[1].grad is None


@pytest.mark.parametrize("when", ["after_launch", "never", "before_launch"])
def test_bias_with_an_outstanding_contribution_is_held(world, when):
    layer, io = fp32_layer(world)
    w, b = world.ix(layer[0]), world.ix(layer[1])

    def fwd():
        D.note_extra(layer[1])
        return D.note_use(*layer)

    def bwd(gen):
        if when == "before_launch":
            D.extra_written(gen, layer[1])
            assert world.fired == []  # (the other node's add alone completes nothing)
        add(layer, gen, **io)
        assert world.log == [world.batched(*layer)]
        assert world.fired == ([w, b] if when == "before_launch" else [w])
        if when == "after_launch":
            D.extra_written(gen, layer[1])
            assert world.fired == [w, b]

    world.run(fwd, bwd)
    assert world.fired == [w, b]  # ("never": the end of the backward pass reports it)


def test_two_outstanding_contributions_release_the_bias_at_the_second(world):
    layer, io = fp32_layer(world)
    w, b = world.ix(layer[0]), world.ix(layer[1])

    def bwd(gen):
        add(layer, gen, **io)
        D.extra_written(gen, layer[1])
        assert world.fired == [w]
        D.extra_written(gen, layer[1])
        assert world.fired == [w, b]

    world.run(lambda: (D.note_extra(layer[1]), D.note_extra(layer[1]), D.note_use(*layer))[-1], bwd)
    assert world.fired == [w, b]


# ---- small parameters: claim / into / done ----------------------------------------------------------------------------------------------------------
def test_claim_into_done(world):
    w, b = world.param(16), world.param(16)
    ctxs = [types.SimpleNamespace() for _ in range(2)]
    for ctx in ctxs:
        D.claim(ctx, w, b)
        assert ctx.direct is True
    assert id(w) in D.managed and id(b) in D.managed
    into = D.into(ctxs[0])
    assert into[0] is w.grad and into[1] is b.grad and w.grad.dtype == torch.float32 and not w.grad.any()
    D.done(ctxs[0])
    assert world.fired == []  # one of two uses
    assert D.into(ctxs[1])[0] is w.grad
    D.done(ctxs[1])
    assert world.fired == [world.ix(w), world.ix(b)] and world.log == []


@pytest.mark.parametrize("other", ["none", "not_leaf", "no_grad"])
def test_claim_declines_what_is_no_trainable_leaf(world, other):
    w = world.param(16)
    b = {"none": None, "not_leaf": world.param(16) * 1, "no_grad": world.param(16, requires_grad=False)}[other]
    ctx = types.SimpleNamespace()
    D.claim(ctx, w, b)
    assert ctx.direct is False and D.into(ctx) is None
    D.done(ctx)
    assert world.fired == [] and w.grad is None and id(w) not in D.managed


def test_direct_only_in_deferred_mode(world):
    w = world.param(16)
    assert D.direct(w)
    FH.set_wgrad_mode("autograd")
    assert not D.direct(w)


# ---- .grad buffers ------------------------------------------------------------------------------------------------------------------------------------
def test_grad_of_creates_contiguous_fp32_zeros_and_keeps_an_existing_one(world):
    p = torch.nn.Parameter(torch.ones(16, 16, 3, 3).to(memory_format=torch.channels_last))
    g = D.grad_of(p)
    assert g is p.grad and g.dtype == torch.float32 and g.is_contiguous() and g.shape == p.shape and not g.any()
    g.fill_(2.0)
    assert D.grad_of(p) is g and bool((g == 2.0).all())


def test_launch_creates_missing_grads_and_keeps_existing_ones(world):
    a, b = world.layer(), world.layer()
    kept = torch.full_like(a[0], 3.0)
    a[0].grad = kept
    world.run(lambda: [D.note_use(*layer) for layer in (a, b)][-1], lambda gen: [add(layer, gen) for layer in (a, b)])
    assert a[0].grad is kept and bool((kept == 3.0).all())
    for p in (a[1], b[0], b[1]):
        assert p.grad.dtype == torch.float32 and p.grad.is_contiguous() and p.grad.shape == p.shape and not p.grad.any()
    assert world.log == [world.multi([a, b])]


# ---- modes ------------------------------------------------------------------------------------------------------------------------------------------------
def test_set_wgrad_mode_flushes_what_is_pending_and_clears_managed(world):
    layer = world.layer()

    def bwd(gen):
        add(layer, gen)
        assert world.log == [] and id(layer[0]) in D.managed and id(layer[1]) in D.managed
        FH.set_wgrad_mode("autograd")
        assert world.log == [world.batched(*layer)] and world.fired == world.both([layer])
        assert D.mode == "autograd" and not D.managed

    world.run(lambda: [D.note_use(*layer) for _ in range(2)][-1], bwd)
    assert len(world.log) == 1 and len(world.fired) == 2
    FH.set_wgrad_mode("autograd")  # (no change: nothing happens)
    assert len(world.log) == 1


def test_unknown_mode_raises(world):
    with pytest.raises(HipError):
        FH.set_wgrad_mode("eager")
    assert D.mode == "deferred"


def test_flush_deferred_wgrads_completes_what_is_pending(world):
    layer = world.layer()

    def bwd(gen):
        add(layer, gen)
        FH.flush_deferred_wgrads()
        assert world.log == [world.batched(*layer)] and world.fired == world.both([layer])

    world.run(lambda: [D.note_use(*layer) for _ in range(2)][-1], bwd)
    assert len(world.log) == 1 and len(world.fired) == 2


def test_wgrad_now_returns_fresh_fp32_gradients(world):
    FH.set_wgrad_mode("autograd")
    w, b = world.layer(cout=32)
    dW, db = FH._wgrad_now(w, True, [act()], [16], act(32), 3, 1, 4, 4, scale=0.5)
    assert dW.dtype == db.dtype == torch.float32 and dW.shape == w.shape and db.shape == b.shape and not dW.any() and not db.any()
    assert w.grad is None and b.grad is None
    assert world.log == [Launch("batched", 1, (1,), (None,), (None,), 3, (0.5,), 0, 0, (1, 4, 4), 16)]
    dW, db = FH._wgrad_now(w, False, [act()], [16], act(32), 3, 1, 4, 4)
    assert db is None and dW.shape == w.shape
    assert world.fired == []
