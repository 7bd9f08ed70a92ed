"""The kernels of the patch-shift FFN (csrc/shift_ffn.hip) through vmg_amd.functional / vmg_amd.kernels: the shift against its closed form
(tests/shift_ffn_ref.patch_shift), bit for bit where it is a copy and against fp64 on pre-rounded inputs where it carries the GELU; the two-branch
re-weighting against an fp64 evaluation with autograd.

Tolerances are those of tests/test_mixer_gate_kernels_gpu.py: fp32 1e-4 forward / 5e-4 gradients, bf16 3e-2 / 5e-2, relative to max(1, max |want|), on
the whole tensor and on the seeded (not planted) part alone.  Every frame of a shift case comes from its own seed, so a value that crossed a frame
boundary would show up."""
import pytest
import torch

from tests import shift_ffn_ref as SR

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["fp32", "bf16"]
PLANTED = [0.0, -0.0, 1e-8, -1e-8, 20.0, -20.0, 100.0, -100.0]
MIX_SHAPES = [(1, 7, 8), (2, 360, 144), (3, 257, 16)]  # (G, R, C)
_frames = {}


def frames(shape, salt=0):
    """fp32 CPU (N, H, W, Cs), frame n from seed 600 + 1000 * salt + 37 * (index of the shape) + n.  Computed once, never modified."""
    key = (tuple(shape), salt)
    if key not in _frames:
        from oracle import recipe as R
        i = SR.SHIFT_SHAPES.index(tuple(shape))
        _frames[key] = torch.stack([R.seeded(shape[1:], 600 + 1000 * salt + 37 * i + n) for n in range(shape[0])])
    return _frames[key]


def planted(shape, salt=0):
    """frames() with the PLANTED values in the first elements, and the mask of the elements that are still seeded."""
    x = frames(shape, salt).clone()
    n = min(x.numel() - 1, len(PLANTED))
    x.view(-1)[:n] = torch.tensor(PLANTED[:n])
    seeded = torch.ones(x.shape, dtype=torch.bool)
    seeded.view(-1)[:n] = False
    return x, seeded


def check(name, got, want, seeded, tol):
    got = got.detach().to(torch.float64).cpu()
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = (got - want).abs()
    whole = float(err.max()) / max(1.0, float(want.abs().max()))
    part = float(err[seeded].max()) / max(1.0, float(want[seeded].abs().max())) if seeded.any() else 0.0
    print(f"{name}: max error {whole:.3e} of the scale; seeded part alone {part:.3e}")
    assert whole <= tol and part <= tol, name


def assert_route(t, Cs, dtype):
    """The route this launch takes (the function the entry itself calls, with the operand's real alignment) is the one the rule gives."""
    from vmg_amd import kernels as K
    assert t.data_ptr() % 16 == 0
    assert K.patch_shift_route(Cs, dtype, aligned=True) == SR.expected_route(Cs, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SR.SHIFT_SHAPES, ids=SR.shape_name)
def test_identity_shift_is_a_copy_both_ways(shape, dtype):
    """Both signs: the bits of the closed form; the backward is the forward with the opposite sign, bit for bit."""
    from vmg_amd import functional as FH
    x = frames(shape).to(dtype)
    d = frames(shape, salt=1).to(dtype)
    xg, dg = x.cuda(), d.cuda()
    assert_route(xg, shape[-1], dtype)
    for inverse in (False, True):
        leaf = xg.clone().requires_grad_(True)
        y = FH.patch_shift(leaf, inverse=inverse)
        assert y.shape == x.shape and torch.equal(y.detach().cpu(), SR.patch_shift(x, inverse=inverse)), (shape, inverse)
        (gx,) = torch.autograd.grad(y, leaf, dg)
        assert torch.equal(gx, FH.patch_shift(dg, inverse=not inverse))
        assert torch.equal(gx.cpu(), SR.patch_shift(d, inverse=not inverse))
        y5 = FH.patch_shift(xg[None], inverse=inverse)  # (B, T, H, W, C)
        assert y5.shape == (1, *x.shape) and torch.equal(y5[0], y.detach())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SR.SHIFT_SHAPES, ids=SR.shape_name)
@pytest.mark.parametrize("inverse", [False, True], ids=["shift", "shift_inv"])
def test_gelu_shift_against_fp64(inverse, shape, dtype):
    """y = shift(gelu(x)) and dx = gelu'(x) * shift^T(dy) against fp64 on the rounded inputs, with planted 0, -0, +-1e-8, +-20, +-100."""
    from vmg_amd import functional as FH
    x32, seeded = planted(shape)
    x64 = x32.to(dtype).to(torch.float64)
    d64 = frames(shape, salt=1).to(dtype).to(torch.float64)
    g64, dg64 = SR.gelu_and_derivative(x64)
    want = SR.patch_shift(g64, inverse=inverse)
    want_dx = dg64 * SR.patch_shift(d64, inverse=not inverse)
    out_seeded = SR.patch_shift((~seeded).to(torch.float64), inverse=inverse) == 0  # what did not come from a planted element
    leaf = x64.to(dtype).cuda().requires_grad_(True)
    assert_route(leaf, shape[-1], dtype)
    y = FH.patch_shift(leaf, inverse=inverse, act="gelu")
    (gx,) = torch.autograd.grad(y, leaf, d64.to(dtype).cuda())
    ftol, gtol = (1e-4, 5e-4) if dtype == torch.float32 else (3e-2, 5e-2)
    tag = f"gelu {'shift_inv' if inverse else 'shift'} {SR.shape_name(shape)} {str(dtype)[6:]}"
    check(tag + " forward", y, want, out_seeded, ftol)
    check(tag + " d/dx", gx, want_dx, seeded, gtol)
    assert torch.equal((y.detach().cpu() == 0) | (want != 0), torch.ones_like(seeded))  # where the closed form is zero (fill, gelu(+-0)), so is the kernel


def _mix_case(G, R, C, dtype):
    from oracle import recipe as Rc
    h, w, d = (Rc.seeded((G, R, C), 700 + i).to(dtype) for i in range(3))
    ps = [Rc.seeded((C // 4, C), 710) / C ** 0.5, 0.1 * Rc.seeded((C // 4,), 711), Rc.seeded((2 * C, C // 4), 712) / (C // 4) ** 0.5,
          0.1 * Rc.seeded((2 * C,), 713)]
    return h, w, d, ps


def _mix_run(h, w, d, ps):
    from vmg_amd import functional as FH
    hl, wl = h.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    pl = [p.cuda().requires_grad_(True) for p in ps]
    y = FH.reweight_mix2(hl, wl, *pl)
    return [y.detach(), *torch.autograd.grad(y, [hl, wl, *pl], d.cuda())]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", MIX_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_reweight_mix2_against_fp64(case, dtype):
    """Forward, dh, dw and the four parameter gradients against fp64 autograd through the restatement on the rounded operands; two runs give the same
    bits (ordered partial sums, no atomics)."""
    G, R, C = case
    h, w, d, ps = _mix_case(G, R, C, dtype)
    h64, w64 = h.double().requires_grad_(True), w.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in ps]
    want = SR.reweight_mix2(h64, w64, *p64)
    wants = [want.detach(), *torch.autograd.grad(want, [h64, w64, *p64], d.double())]
    got = _mix_run(h, w, d, ps)
    again = _mix_run(h, w, d, ps)
    ftol, gtol = (1e-4, 5e-4) if dtype == torch.float32 else (3e-2, 5e-2)
    everything = torch.ones(1, dtype=torch.bool)
    for name, g, wv, tol in zip(["forward", "dh", "dw", "dfc1w", "dfc1b", "dfc2w", "dfc2b"], got, wants, [ftol] + [gtol] * 6):
        assert g.shape == wv.shape
        check(f"reweight_mix2 {case} {str(dtype)[6:]} {name}", g, wv, everything.expand(wv.shape), tol)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_misaligned_and_noncontiguous_operands_give_the_same_bits(dtype):
    """Through the functional entries (which copy such operands to aligned storage) and, for the shift, through the kernel wrapper itself (an
    element-aligned pointer off the 16-byte grid takes the per-element kernel)."""
    from vmg_amd import functional as FH
    from vmg_amd import kernels as K
    shape = (2, 4, 4, 144)
    x, d = frames(shape).to(dtype).cuda(), frames(shape, salt=1).to(dtype).cuda()

    def off_grid(t):  # the same values one element off a 16-byte boundary
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 != 0
        return v

    def strided(t):  # the same values, not contiguous
        v = t.transpose(1, 2).contiguous().transpose(1, 2)
        assert not v.is_contiguous() and torch.equal(v, t)
        return v

    def run(make):
        outs = []
        for act in (None, "gelu"):
            for inverse in (False, True):
                leaf = x.clone().requires_grad_(True)
                y = FH.patch_shift(make(leaf), inverse=inverse, act=act)
                (g,) = torch.autograd.grad(y, leaf, make(d))
                outs += [y.detach(), g]
        return outs

    base = run(lambda t: t)
    for make in (off_grid, strided):
        for a, b in zip(base, run(make)):
            assert torch.equal(a, b)
    assert K.patch_shift_route(144, dtype, aligned=False) == "element" and K.patch_shift_route(144, dtype) == "vector"
    for gelu in (False, True):
        assert torch.equal(K.patch_shift_forward(off_grid(x), 1, gelu), K.patch_shift_forward(x, 1, gelu))
        assert torch.equal(K.patch_shift_backward(off_grid(d), -1, off_grid(x) if gelu else None), K.patch_shift_backward(d, -1, x if gelu else None))

    G, R, C = 2, 360, 144
    h, w, dd, ps = _mix_case(G, R, C, dtype)
    ref = _mix_run(h, w, dd, ps)
    hl, wl = h.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    pl = [p.cuda().requires_grad_(True) for p in ps]
    y = FH.reweight_mix2(off_grid(hl), off_grid(wl), *pl)
    got = [y.detach(), *torch.autograd.grad(y, [hl, wl, *pl], off_grid(dd.cuda()))]
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    y = FH.reweight_mix2(strided(hl.view(G, 18, 20, C)), strided(wl.view(G, 18, 20, C)), *pl)
    got = [y.detach().reshape(G, R, C), *torch.autograd.grad(y, [hl, wl, *pl], strided(dd.cuda().view(G, 18, 20, C)))]
    for a, b in zip(ref, got):
        assert torch.equal(a, b)


def test_entry_points_refuse_null_and_misaligned_pointers():
    """On real device tensors: a valid call returns 0, a null or misaligned pointer a non-zero code and an error text, before anything is launched."""
    from vmg_amd import hip
    l, st, p = hip.lib(), hip.stream_ptr(), (lambda t: t.data_ptr())
    t = torch.zeros(2, 3, 3, 16, device="cuda")
    o, o2 = torch.empty_like(t), torch.empty_like(t)
    coef, add = torch.ones(2, 16, 2, device="cuda"), torch.zeros(2, 16, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    red = torch.empty(2, 16, 2, device="cuda")
    ok = [l.vmg_patch_shift_fwd(hip.F32, 1, 0, p(t), p(o), 2, 3, 3, 16, st), l.vmg_patch_shift_bwd(hip.F32, 1, 3, p(t), p(t), p(o), 2, 3, 3, 16, st),
          l.vmg_patch_shift_bwd(hip.F32, -1, 0, p(t), None, p(o), 2, 3, 3, 16, st), l.vmg_mix2_fwd(hip.F32, p(t), p(t), p(coef), p(o), 18, 9, 16, st),
          l.vmg_mix2_bwd(hip.F32, p(t), p(coef), p(add), p(o), p(o2), 18, 9, 16, st),
          l.vmg_group_reduce2(hip.F32, p(t), p(t), p(t), p(red), 2, 9, 16, 1.0, p(ws), ws.numel(), st)]
    assert ok == [0] * len(ok), ok
    bad = [l.vmg_patch_shift_fwd(hip.F32, 1, 0, None, p(o), 2, 3, 3, 16, st), l.vmg_patch_shift_fwd(hip.F32, 1, 0, p(t), None, 2, 3, 3, 16, st),
           l.vmg_patch_shift_fwd(hip.F32, 1, 0, p(t) + 2, p(o), 2, 3, 3, 16, st), l.vmg_patch_shift_fwd(hip.BF16, 1, 0, p(t), p(o) + 1, 2, 3, 3, 16, st),
           l.vmg_patch_shift_bwd(hip.F32, 1, 3, p(t), None, p(o), 2, 3, 3, 16, st), l.vmg_patch_shift_bwd(hip.F32, 1, 3, p(t), p(t) + 1, p(o), 2, 3, 3, 16, st),
           l.vmg_patch_shift_fwd(hip.F32, 1, 0, p(t), p(o), 0, 3, 3, 16, st), l.vmg_patch_shift_fwd(hip.F32, 1, 0, p(t), p(o), 2, 3, 3, 0, st),
           l.vmg_mix2_fwd(hip.F32, p(t), None, p(coef), p(o), 18, 9, 16, st), l.vmg_mix2_fwd(hip.F32, p(t) + 4, p(t), p(coef), p(o), 18, 9, 16, st),
           l.vmg_mix2_bwd(hip.F32, p(t), p(coef), None, p(o), p(o2), 18, 9, 16, st),
           l.vmg_group_reduce2(hip.F32, p(t), None, p(t), p(red), 2, 9, 16, 1.0, p(ws), ws.numel(), st),
           l.vmg_group_reduce2(hip.F32, p(t), p(t) + 4, p(t), p(red), 2, 9, 16, 1.0, p(ws), ws.numel(), st),
           l.vmg_se_mlp2_fwd(None, p(t), p(t), p(t), p(t), p(o), p(o2), 2, 16, 4, st), l.vmg_se_mlp2_fwd(p(t), p(t), p(t), p(t), p(t), p(o) + 2, p(o2), 2, 16, 4, st),
           l.vmg_se_mlp2_bwd(p(t), p(t), p(t), p(t), p(t), p(t), p(o), p(o), p(o), p(o), p(o), None, 2, 16, 4, 1.0, 0, st)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad), [i for i, rc in enumerate(bad) if rc == 0]
    assert l.vmg_last_error()
