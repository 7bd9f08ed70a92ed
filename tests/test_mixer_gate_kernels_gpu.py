"""The gate kernel family (vmg_gate_fwd/bwd, vmg_gate_res_fwd/bwd through vmg_amd.functional) against an fp64 evaluation of the formulas
(tests/mixer_gate_ref.gate_formulas) on the same, pre-rounded inputs: every activation, every form, forward and both gradients, fp32 and bf16; and
bit for bit against the tanh ops and against the two-pass form (gate, then residual_drop_path).

Tolerances are those tests/test_tab_kernels_gpu.py::test_reweight_mix_and_gate_fwd_bwd applies to the tanh gate: fp32 1e-4 forward / 5e-4 gradients,
bf16 3e-2 / 5e-2, relative to max(1, max |want|).  The planted +-100 make max |want| large, so the same bounds are also applied to the seeded part of
each tensor alone, relative to max(1, max |want|) over that part.

Measured on the MI355X, worst error over all shapes relative to max(1, max |want|) of the seeded part, forward / gradients: see DESIGN.md section 4."""
import pytest
import torch

from tests import mixer_gate_ref as GR

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
# (rows split as leading dims, C, G): one bf16 vector per row and fewer elements than one workgroup; distinct coefficients per group, one of them 0
# (a dropped sample); rows not a multiple of the 256 threads
SHAPES = {"7x8": ((1, 7), 8, 1), "2x360x144": ((2, 3 * 10 * 12), 144, 2), "3x257x16": ((3, 257), 16, 3)}
PLANTED = [0.0, -0.0, 1e-8, -1e-8, 20.0, -20.0, 100.0, -100.0]
FORMS = [(act, False) for act in GR.SYMM_ACTS] + [("gelu", True)]  # (activation, asymmetric)
FORM_IDS = GR.SYMM_ACTS + ["asym"]
_inputs = {}


def _q(t, dtype):
    return t.to(dtype).to(torch.float64)


def inputs(shape_id, dtype):
    """Seeded a (x or g), y, res, dout of the shape, rounded to dtype, as fp64 CPU tensors; every pair of PLANTED values in (a, y) that fits; the
    (G, C) fp32 coefficient; the mask of the seeded (not planted) elements.  Computed once per (shape, dtype) and never modified."""
    key = (shape_id, dtype)
    if key not in _inputs:
        from oracle import recipe as R
        lead, C, G = SHAPES[shape_id]
        shp = (*lead, C)
        a, y, res, d = (R.seeded(shp, 500 + i) for i in range(4))
        n = min(a.numel(), len(PLANTED) ** 2)
        k = torch.arange(n)
        a.view(-1)[:n] = torch.tensor(PLANTED)[k // len(PLANTED)]
        y.view(-1)[:n] = torch.tensor(PLANTED)[k % len(PLANTED)]
        seeded = torch.ones(shp, dtype=torch.bool)
        seeded.view(-1)[:n] = False
        base = torch.tensor([1.25, 0.0, 0.5][:G] if G > 1 else [1.25])
        coef = (base[:, None] * (1 + 0.01 * torch.arange(C, dtype=torch.float32))[None]).contiguous()
        _inputs[key] = dict(a=_q(a, dtype), y=_q(y, dtype), res=_q(res, dtype), d=_q(d, dtype), coef=coef, seeded=seeded, G=G)
    return _inputs[key]


def check(name, got, want, seeded, tol):
    got = got.detach().to(torch.float64).cpu()
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = (got - want).abs()
    whole = float(err.max()) / max(1.0, float(want.abs().max()))
    part = float(err[seeded].max()) / max(1.0, float(want[seeded].abs().max())) if seeded.any() else 0.0
    print(f"{name}: max error {whole:.3e} of the scale; seeded part alone {part:.3e}")
    assert whole <= tol and part <= tol, name


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape_id", list(SHAPES))
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("residual", [False, True], ids=["alone", "residual"])
def test_gate_against_fp64(residual, form, shape_id, dtype):
    from vmg_amd import functional as FH
    act, asym = form
    inp = inputs(shape_id, dtype)
    a64, y64, r64, d64, coef, G = inp["a"], inp["y"], inp["res"], inp["d"], inp["coef"], inp["G"]
    cb = coef.to(torch.float64).reshape(G, 1, -1)  # (the leading dimension of every shape is its G)
    dev = lambda t: t.to(dtype).cuda().contiguous().requires_grad_(True)
    a, y, res = dev(a64), dev(y64), dev(r64)
    if residual:
        want, wda, wdy = GR.gate_formulas(a64, y64, d64 * cb, act, asym)
        want = r64 + want * cb
        got = FH._GateRes.apply(a, y, res, coef.cuda(), act, asym)
        ga, gy, gr = torch.autograd.grad(got, [a, y, res], d64.to(dtype).cuda())
        assert torch.equal(gr.cpu().to(torch.float64), d64)
    else:
        want, wda, wdy = GR.gate_formulas(a64, y64, d64, act, asym)
        got = FH.asym_gate(a, y) if asym else FH.symm_gate(a, y, act)
        ga, gy = torch.autograd.grad(got, [a, y], d64.to(dtype).cuda())
    ftol, gtol = (1e-4, 5e-4) if dtype == torch.float32 else (3e-2, 5e-2)
    tag = f"{FORM_IDS[FORMS.index(form)]} {'residual' if residual else 'alone'} {shape_id} {str(dtype)[6:]}"
    check(tag + " forward", got, want, inp["seeded"], ftol)
    check(tag + " d/da", ga, wda, inp["seeded"], gtol)
    check(tag + " d/dy", gy, wdy, inp["seeded"], gtol)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape_id", list(SHAPES))
def test_tanh_instance_has_the_bits_of_the_tanh_ops(shape_id, dtype):
    """The family at act = tanh against tanh_gate / _GateResidual (tab_ew_kernel's OP_GATE_* and OP_GATE_RES_*), forward and backward, with an explicit
    coefficient tensor."""
    from vmg_amd import functional as FH
    inp = inputs(shape_id, dtype)
    coef = inp["coef"].cuda()
    outs = []
    for new in (False, True):
        a, y, res = (inp[k].to(dtype).cuda().requires_grad_(True) for k in ("a", "y", "res"))
        d = inp["d"].to(dtype).cuda()
        o1 = FH.symm_gate(a, y, "tanh") if new else FH.tanh_gate(a, y)
        g1 = torch.autograd.grad(o1, [a, y], d)
        o2 = FH._GateRes.apply(a, y, res, coef, "tanh", False) if new else FH._GateResidual.apply(a, y, res, coef)
        g2 = torch.autograd.grad(o2, [a, y, res], d)
        outs.append([o1, *g1, o2, *g2])
    for i, (p, q) in enumerate(zip(*outs)):
        assert torch.equal(p, q), i


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape_id", list(SHAPES))
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_fused_residual_has_the_bits_of_the_two_pass_form(form, shape_id, dtype):
    """res + DropPath(gate) in one pass against the gate followed by residual_drop_path: at p = 0 (through the public functions), and with both
    driven by the same explicit coefficient tensor (one group dropped, per-channel values)."""
    from vmg_amd import functional as FH
    act, asym = form
    inp = inputs(shape_id, dtype)
    coef = inp["coef"].cuda()
    d = inp["d"].to(dtype).cuda()
    leaves = lambda: [inp[k].to(dtype).cuda().requires_grad_(True) for k in ("a", "y", "res")]
    gate = (lambda a, y: FH.asym_gate(a, y)) if asym else (lambda a, y: FH.symm_gate(a, y, act))
    a, y, res = leaves()
    two = FH.residual_drop_path(res, gate(a, y), 0.0, True, 1.0)
    g_two = torch.autograd.grad(two, [a, y, res], d)
    a, y, res = leaves()
    one = FH.asym_gate_residual(a, y, res, 0.0, True, 1.0) if asym else FH.symm_gate_residual(a, y, res, 0.0, True, 1.0, act=act)
    g_one = torch.autograd.grad(one, [a, y, res], d)
    for i, (p, q) in enumerate(zip([two, *g_two], [one, *g_one])):
        assert torch.equal(p, q), ("p = 0", i)
    a, y, res = leaves()
    two = FH._ResidualDropPath.apply(res, gate(a, y), coef)
    g_two = torch.autograd.grad(two, [a, y, res], d)
    a, y, res = leaves()
    one = FH._GateRes.apply(a, y, res, coef, act, asym)
    g_one = torch.autograd.grad(one, [a, y, res], d)
    for i, (p, q) in enumerate(zip([two, *g_two], [one, *g_one])):
        assert torch.equal(p, q), ("coef", i)
    assert torch.isfinite(one).all() and all(torch.isfinite(g).all() for g in g_one)


def test_entry_points_refuse_bad_arguments():
    """Null pointer, C not a multiple of the vector width, rows not divisible by G, unknown activation / form: an error and a non-zero return."""
    from vmg_amd import hip
    from vmg_amd import kernels as K
    t = torch.zeros(6, 8, device="cuda")
    c = torch.ones(2, 8, device="cuda")
    o1, o2 = torch.empty_like(t), torch.empty_like(t)
    l, st, p = hip.lib(), hip.stream_ptr(), (lambda x: x.data_ptr())
    ok = l.vmg_gate_res_bwd(hip.F32, 0, 4, p(t), p(t), p(t), p(c), p(o1), p(o2), 6, 2, 8, st)
    assert ok == 0
    bad = [l.vmg_gate_fwd(hip.F32, 0, 0, None, p(t), p(o1), 6, 8, st), l.vmg_gate_fwd(hip.F32, 0, 0, p(t), p(t), None, 6, 8, st),
           l.vmg_gate_bwd(hip.F32, 0, 0, p(t), p(t), p(t), p(o1), None, 6, 8, st),
           l.vmg_gate_res_fwd(hip.F32, 0, 0, p(t), p(t), p(t), None, p(o1), 6, 2, 8, st),
           l.vmg_gate_res_fwd(hip.F32, 0, 0, p(t), p(t), None, p(c), p(o1), 6, 2, 8, st),
           l.vmg_gate_fwd(hip.F32, 0, 0, p(t), p(t), p(o1), 8, 6, st),      # C = 6: not a multiple of 4
           l.vmg_gate_fwd(hip.BF16, 0, 0, p(t), p(t), p(o1), 12, 4, st),    # C = 4: not a multiple of 8 in bf16
           l.vmg_gate_res_fwd(hip.F32, 0, 0, p(t), p(t), p(t), p(c), p(o1), 6, 4, 8, st),  # 6 rows, G = 4
           l.vmg_gate_fwd(hip.F32, 0, 5, p(t), p(t), p(o1), 6, 8, st), l.vmg_gate_fwd(hip.F32, 0, -1, p(t), p(t), p(o1), 6, 8, st),
           l.vmg_gate_fwd(hip.F32, 2, 0, p(t), p(t), p(o1), 6, 8, st), l.vmg_gate_fwd(7, 0, 0, p(t), p(t), p(o1), 6, 8, st)]
    assert all(rc != 0 for rc in bad), bad
    assert l.vmg_last_error().decode()
    with pytest.raises(K.HipError):
        K.gate_forward(t, t, "softplus")
    with pytest.raises(K.HipError):
        K.gate_forward(t, t, "tanh", res=t, coef=torch.ones(4, 8, device="cuda"), G=4)
    torch.cuda.synchronize()
