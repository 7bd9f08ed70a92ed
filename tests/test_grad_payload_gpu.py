"""vmg_grad_pack_bf16 / vmg_grad_unpack_bf16 (csrc/optim.hip: the bfloat16 payload of the staged data-parallel exchange) through the C ABI,
bit for bit against torch's own float32 -> bfloat16 -> float32 conversions computed on the host.

Sizes: tail only (1, 7), one vector (8), vector + tail (9, 255, 4096 + 3), many blocks (1 << 20) and, because the grid is capped at 2048 blocks of
256 lanes of 8 elements, one size beyond a whole grid pass (2048 * 256 * 8 + 43) so that the grid stride and the tail behind it run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 8, 9, 255, 4096 + 3, 1 << 20, 2048 * 256 * 8 + 43]
_INPUT = {}


def _specials():
    f32 = torch.float32
    ties = []
    for e in (0x3f80, 0x4049, 0xbf81, 0x0080, 0x7f00, 0x3f7f):  # kept mantissa bit even and odd, both signs, small and large exponents
        for k in (0, 1, 2, 3):
            ties.append(((e + k) << 16 | 0x8000) - (1 << 32 if (e + k) & 0x8000 else 0))
    near = [((0x3f80 << 16) | 0x7fff), ((0x3f80 << 16) | 0x8001), ((0x3f81 << 16) | 0x7fff), ((0x3f81 << 16) | 0x8001)]  # just off a tie
    tie_t = torch.tensor(ties + near, dtype=torch.int32).view(f32)
    fi = torch.finfo(f32)
    other = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), -float("nan"), fi.max, -fi.max, fi.tiny, -fi.tiny,
                          1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38, 3.3895314e38, -3.3961775e38, 1.0, -1.0, 65504.0], dtype=f32)
    return torch.cat([tie_t, other])


def _input(n):
    """The same n values for every scale: the special values first (as many as fit), then normals scaled by 1e-6 ... 1e3."""
    if n not in _INPUT:
        gen = torch.Generator().manual_seed(n)
        mag = 10.0 ** (torch.rand(n, generator=gen) * 9.0 - 6.0)
        g = torch.randn(n, generator=gen) * mag
        sp = _specials()
        k = min(n, sp.numel())
        # rotate so that small sizes see different specials and the scalar tail of the larger ones holds specials too
        g[:k] = sp.roll(-n)[:k]
        if n > 2 * sp.numel():
            g[-sp.numel():] = sp
        _INPUT[n] = g
    return _INPUT[n]


def _same_bf16(got, want, what):
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions differ"
    gb, wb = got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]
    bad = (gb != wb).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} elements differ, first at {int(bad[0])}: {int(gb[bad[0]]) & 0xffff:#06x} vs {int(wb[bad[0]]) & 0xffff:#06x}"


@pytest.mark.parametrize("scale", [1.0, 0.5, 0.125])
@pytest.mark.parametrize("n", SIZES)
def test_pack_and_unpack_match_torch_bit_for_bit(n, scale):
    from vmg_amd import hip
    lib = hip.lib()
    g = _input(n)
    want = (g * scale).to(torch.bfloat16)
    pad = 24  # guard elements behind the buffers: a store past n would show
    g_dev = torch.zeros(n + pad, dtype=torch.float32, device="cuda")
    g_dev[:n] = g.cuda()
    out = torch.full((n + pad,), 3.0, dtype=torch.bfloat16, device="cuda")
    hip.check(lib.vmg_grad_pack_bf16(g_dev.data_ptr(), out.data_ptr(), n, scale, hip.stream_ptr()), "vmg_grad_pack_bf16")
    got = out.cpu()
    _same_bf16(got[:n], want, f"pack n={n} scale={scale}")
    assert bool((got[n:] == 3.0).all()), "pack wrote past n"
    assert torch.equal(g_dev[:n].cpu().view(torch.int32), g.view(torch.int32)), "pack changed its input"

    back = torch.full((n + pad,), 7.0, dtype=torch.float32, device="cuda")
    hip.check(lib.vmg_grad_unpack_bf16(out.data_ptr(), back.data_ptr(), n, hip.stream_ptr()), "vmg_grad_unpack_bf16")
    b = back.cpu()
    wf = want.float()
    nan = torch.isnan(wf)
    assert torch.equal(torch.isnan(b[:n]), nan)
    assert torch.equal(b[:n].view(torch.int32)[~nan], wf.view(torch.int32)[~nan]), f"unpack n={n}"
    assert bool((b[n:] == 7.0).all()), "unpack wrote past n"


def test_the_inputs_hold_what_they_should():
    """The generated vectors really contain the edge values (a test of the test: no GPU work)."""
    g = _input(4096 + 3)
    bits = g.view(torch.int32)
    assert torch.isnan(g).any() and torch.isinf(g).any() and (g == torch.finfo(torch.float32).max).any()
    assert ((g != 0) & (g.abs() < torch.finfo(torch.float32).tiny)).any()            # fp32 denormals
    assert ((g == 0) & (bits < 0)).any() and ((g == 0) & (bits == 0)).any()          # both zeros
    tie = (bits & 0xffff) == 0x8000
    assert (tie & ((bits >> 16) & 1 == 0)).any() and (tie & ((bits >> 16) & 1 == 1)).any()  # ties, both parities of the kept bit
    assert (g[-8:] != 0).any()
    assert torch.isinf(torch.tensor([torch.finfo(torch.float32).max]).to(torch.bfloat16)).all()  # torch rounds the largest fp32 to inf


def test_wrappers_and_refusals():
    from vmg_amd import hip
    from vmg_amd import kernels as K
    lib = hip.lib()
    g = torch.randn(64, device="cuda")
    out = torch.full((64,), 3.0, dtype=torch.bfloat16, device="cuda")
    s = hip.stream_ptr()
    # misaligned pointers and n = 0: an error code, a message, nothing launched (the buffers keep their contents)
    assert lib.vmg_grad_pack_bf16(g.data_ptr() + 4, out.data_ptr(), 8, 1.0, s) != 0
    assert b"16-byte" in lib.vmg_last_error()
    assert lib.vmg_grad_pack_bf16(g.data_ptr(), out.data_ptr() + 4, 8, 1.0, s) != 0
    assert lib.vmg_grad_pack_bf16(g.data_ptr(), out.data_ptr(), 0, 1.0, s) != 0
    assert lib.vmg_grad_unpack_bf16(out.data_ptr() + 4, g.data_ptr(), 8, s) != 0
    assert b"16-byte" in lib.vmg_last_error()
    assert lib.vmg_grad_unpack_bf16(out.data_ptr(), g.data_ptr() + 4, 8, s) != 0
    assert lib.vmg_grad_unpack_bf16(out.data_ptr(), g.data_ptr(), 0, s) != 0
    g0 = g.clone()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and torch.equal(g, g0)
    # the Python wrappers
    K.grad_pack_bf16(g, out, 0.5)
    assert torch.equal(out, (g * 0.5).to(torch.bfloat16))
    back = torch.empty_like(g)
    K.grad_unpack_bf16(out, back)
    assert torch.equal(back, out.float())
    with pytest.raises(hip.HipError):
        K.grad_pack_bf16(g, out[:32], 1.0)
    with pytest.raises(hip.HipError):
        K.grad_pack_bf16(g.double(), out, 1.0)
    with pytest.raises(hip.HipError):
        K.grad_unpack_bf16(out.cpu(), back)
