"""Which kernel serves which weight-gradient call, and with which grid: vmg_conv_wgrad_plan, the pure host function behind every entry
point of csrc/conv_wgrad.hip, on a machine without a GPU.

The expected values below were RECORDED from the dispatch this function replaced (the commit before it: the kernel id it reported next to
each launch, and the grid, splits and reduce blocks it passed to that launch), never from vmg_conv_wgrad_plan itself.  A row is
(name, (entry, dtype, ks, nprob, npairs, N, H, W, x_ps, Cin, dy_ps, Cout, align, workspace, 3x3 variant),
 (kernel, co blocks, ci blocks, K splits, workgroups, slabs?, reduce blocks) or None where the entry fails)."""
import pytest
import torch

from tests import test_wgrad_kernels_gpu as G
from tests import wgrad_ref as WR

PLAIN, WS, MULTI = 0, 1, 2  # include/vmg_hip.h VMG_WGRAD_ENTRY_*
X16, DY16, DY2 = 1, 2, 4    # VMG_WGRAD_ALIGN_*
BF16, F32 = torch.bfloat16, torch.float32


def _lib():
    from vmg_amd import hip
    return hip, hip.lib()


def _ws_bytes(lib, ws):
    return {"none": 0, "64K": 64 << 10, "1M-4": (1 << 20) - 4, "1M": 1 << 20, "full": lib.vmg_conv_wgrad_ws_bytes()}[ws]


def _plan(entry, dtype, ks, nprob, npairs, N, H, W, x_ps, Cin, dy_ps, Cout, align=X16 | DY16 | DY2, ws="full", It=None, o0=0, i0=0):
    """The plan's integers, or None where the entry rejects the call or (multi entries) its large-tile kernel does not apply."""
    import ctypes
    hip, lib = _lib()
    out = (ctypes.c_int * 7)()
    code = {BF16: hip.BF16, F32: hip.F32}.get(dtype, dtype)
    rc = lib.vmg_conv_wgrad_plan(entry, code, ks, nprob, npairs, N, H, W, x_ps, Cin, dy_ps, Cout, Cin + i0 if It is None else It, o0, i0, align,
                                 _ws_bytes(lib, ws), out)
    assert rc in (0, -1)
    return tuple(out) if rc == 0 and out[0] else None


@pytest.fixture
def variant():
    """Sets vmg_conv_wgrad3_variant for a test; the previous value is restored."""
    _, lib = _lib()
    prev = lib.vmg_conv_wgrad3_variant(-1)
    yield lib.vmg_conv_wgrad3_variant
    lib.vmg_conv_wgrad3_variant(prev)


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) every case of the GPU test reaches the kernel the GPU test expects (strides and alignment as tests/test_wgrad_kernels_gpu._Problem
#     makes them: x_ps / dy_ps None = the 8-rounded channel count + 8, offsets 0 = 16-byte aligned; 16 pairs per launch)
# ------------------------------------------------------------------------------------------------------------------------------------
def _ps(c, given):
    return G._c8(c) + 8 if given is None else given


def _launch_pairs(P):
    return sorted({min(16, P - s) for s in range(0, P, 16)})


@pytest.mark.parametrize("case", G.W3_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gpu_cases_large_tile_3x3(case, variant):
    hip, _ = _lib()
    N, H, W, Ci, Co, P = case
    seed = G.W3_CASES.index(case)
    x_ps, dy_ps = _ps(Ci, None if seed % 2 else Ci), _ps(Co, None if seed % 3 else Co)
    for v, kind in ((0, hip.WGRAD_3), (1, hip.WGRAD_3B)):
        variant(v)
        for n in _launch_pairs(P):
            assert _plan(WS, BF16, 3, 1, n, N, H, W, x_ps, Ci, dy_ps, Co)[0] == hip.wgrad_kernel_id(kind), (v, n)


@pytest.mark.parametrize("case", G.L2_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gpu_cases_large_tile_1x1(case):
    hip, _ = _lib()
    N, H, W, Ci, Co, P = case
    seed = 100 + G.L2_CASES.index(case)
    x_ps, dy_ps = _ps(Ci, None if seed % 2 else Ci), _ps(Co, None if seed % 3 else Co)
    assert _plan(WS, BF16, 1, 1, P, N, H, W, x_ps, Ci, dy_ps, Co)[0] == hip.wgrad_kernel_id(hip.WGRAD_L2)


@pytest.mark.parametrize("case", G.W7_CASES, ids=lambda c: "-".join(map(str, c)))
def test_gpu_cases_tap_row(case):
    hip, _ = _lib()
    ks, h, W, Ci, Co, P, dense = case
    seed = 200 + G.W7_CASES.index(case)
    x_ps, dy_ps = _ps(Ci, None if seed % 2 else Ci), _ps(Co, Co if dense else None)
    assert _plan(WS, BF16, ks, 1, P, 1 + seed % 2, G._w7_height(ks, h), W, x_ps, Ci, dy_ps, Co)[0] == G._w7_kernel(hip, ks, Co)


@pytest.mark.parametrize("case", G.V1_CASES, ids=lambda c: f"{'bf16' if c[0] == BF16 else 'fp32'}-ks{c[1]}-" + "x".join(map(str, c[2])))
def test_gpu_cases_general_kernel(case):
    hip, _ = _lib()
    dtype, ks, (N, H, W, Ci, Co) = case
    seed = 300 + G.V1_CASES.index(case)
    vpl = 8 if dtype == BF16 else 4
    x_ps, dy_ps = ((c + vpl - 1) // vpl * vpl + (vpl if seed % 2 else 0) for c in (Ci, Co))
    for align in (X16 | DY16 | DY2, DY2, 0):  # (the general kernel takes any alignment: test_general_kernel_element_loads)
        assert _plan(PLAIN, dtype, ks, 1, 1, N, H, W, x_ps, Ci, dy_ps, Co, align=align)[0] == G._v1_kernel(hip, dtype, ks, Ci, Co)


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) one row on each side of every threshold of the dispatch
# ------------------------------------------------------------------------------------------------------------------------------------
THRESHOLDS = [
    ('1x1 63 units', (1, 1, 1, 1, 1, 1, 1, 2016, 144, 144, 144, 144, 7, 'full', 1), (16843523, 3, 3, 1, 9, 0, 0)),
    ('1x1 64 units', (1, 1, 1, 1, 1, 1, 1, 2048, 144, 144, 144, 144, 7, 'full', 1), (67108864, 1, 1, 8, 8, 1, 360)),
    ('1x1 63 units in 3 pairs of 21', (1, 1, 1, 1, 3, 1, 1, 672, 144, 144, 144, 144, 7, 'full', 1), (16843523, 3, 3, 1, 9, 0, 0)),
    ('1x1 66 units in 3 pairs of 22', (1, 1, 1, 1, 3, 1, 1, 673, 144, 144, 144, 144, 7, 'full', 1), (67108864, 1, 1, 8, 8, 1, 360)),
    ('1x1 slabs do not fit 64 KiB', (1, 1, 1, 1, 1, 1, 1, 2048, 144, 144, 144, 144, 7, '64K', 1), (16843523, 3, 3, 2, 18, 0, 0)),
    ('1x1 slabs fit 1 MiB', (1, 1, 1, 1, 1, 1, 1, 2048, 144, 144, 144, 144, 7, '1M', 1), (67108864, 1, 1, 8, 8, 1, 360)),
    ('1x1 no workspace', (1, 1, 1, 1, 1, 1, 1, 2048, 144, 144, 144, 144, 7, 'none', 1), (16843523, 3, 3, 2, 18, 0, 0)),
    ('1x1 plain entry', (0, 1, 1, 1, 1, 1, 1, 2048, 144, 144, 144, 144, 7, 'full', 1), (16843523, 3, 3, 2, 18, 0, 0)),
    ('1x1 Cin 150 in a stride of 152', (1, 1, 1, 1, 1, 1, 1, 2048, 152, 150, 144, 144, 7, 'full', 1), (16843523, 3, 4, 2, 24, 0, 0)),
    ('1x1 x stride 150', (1, 1, 1, 1, 1, 1, 1, 2048, 150, 144, 144, 144, 7, 'full', 1), (16843523, 3, 3, 2, 18, 0, 0)),
    ('1x1 dy stride 147', (1, 1, 1, 1, 1, 1, 1, 2048, 144, 144, 147, 144, 7, 'full', 1), (16843523, 3, 3, 2, 18, 0, 0)),
    ('1x1 x unaligned', (1, 1, 1, 1, 1, 1, 1, 2048, 144, 144, 144, 144, 6, 'full', 1), (16843523, 3, 3, 2, 18, 0, 0)),
    ('1x1 dy 2-byte aligned', (1, 1, 1, 1, 1, 1, 1, 2048, 144, 144, 144, 144, 5, 'full', 1), (16843523, 3, 3, 2, 18, 0, 0)),
    ('1x1 fp32', (1, 0, 1, 1, 1, 1, 1, 2048, 144, 144, 144, 144, 7, 'full', 1), (16843523, 3, 3, 2, 18, 0, 0)),
    ('3x3 Cout 16', (1, 1, 3, 1, 1, 1, 64, 32, 64, 64, 16, 16, 7, 'full', 1), (83952384, 4, 1, 4, 16, 1, 160)),
    ('3x3 Cout 17', (1, 1, 3, 1, 1, 1, 64, 32, 64, 64, 24, 17, 7, 'full', 1), (50331648, 1, 2, 8, 16, 1, 2304)),
    ('7x7 Cout 16', (1, 1, 7, 1, 1, 1, 64, 32, 8, 8, 16, 16, 7, 'full', 1), (83953408, 1, 1, 8, 8, 1, 200)),
    ('7x7 Cout 17', (1, 1, 7, 1, 1, 1, 64, 32, 8, 8, 24, 17, 7, 'full', 1), (84018944, 1, 1, 8, 8, 1, 400)),
    ('7x7 Cout 32', (1, 1, 7, 1, 1, 1, 64, 32, 8, 8, 32, 32, 7, 'full', 1), (84018944, 1, 1, 8, 8, 1, 400)),
    ('7x7 Cout 33', (1, 1, 7, 1, 1, 1, 64, 32, 8, 8, 40, 33, 7, 'full', 1), (84150016, 1, 1, 8, 8, 1, 800)),
    ('7x7 Cout 64', (1, 1, 7, 1, 1, 1, 64, 32, 8, 8, 64, 64, 7, 'full', 1), (84150016, 1, 1, 8, 8, 1, 800)),
    ('7x7 Cout 65', (1, 1, 7, 1, 1, 1, 64, 32, 8, 8, 72, 65, 7, 'full', 1), (17236225, 5, 1, 2, 10, 1, 246)),
    ('7x7 dense dy of 2 channels', (1, 1, 7, 1, 1, 1, 64, 32, 16, 16, 2, 2, 7, 'full', 1), (83953408, 1, 1, 8, 8, 1, 200)),
    ('7x7 dy 2-byte aligned', (1, 1, 7, 1, 1, 1, 64, 32, 16, 16, 8, 2, 5, 'full', 1), (83953408, 1, 1, 8, 8, 1, 200)),
    ('7x7 dy on an odd byte', (1, 1, 7, 1, 1, 1, 64, 32, 16, 16, 8, 2, 1, 'full', 1), (17236225, 1, 1, 2, 2, 1, 50)),
    ('7x7 x unaligned', (1, 1, 7, 1, 1, 1, 64, 32, 16, 16, 8, 2, 6, 'full', 1), (17236225, 1, 1, 2, 2, 1, 50)),
    ('7x7 Cin 3 in a stride of 8', (1, 1, 7, 1, 1, 1, 64, 32, 8, 3, 8, 2, 7, 'full', 1), (17236225, 1, 1, 2, 2, 1, 50)),
    ('7x7 x stride 19', (1, 1, 7, 1, 1, 1, 64, 32, 19, 16, 8, 2, 7, 'full', 1), (17236225, 1, 1, 2, 2, 1, 50)),
    ('7x7 fp32', (1, 0, 7, 1, 1, 1, 64, 32, 16, 16, 8, 2, 7, 'full', 1), (17236225, 1, 1, 2, 2, 1, 50)),
    ('7x7 2^30 - 2^15 units', (1, 1, 7, 1, 16, 32767, 256, 1024, 8, 8, 8, 2, 7, 'full', 1), (83953408, 1, 1, 512, 512, 1, 200)),
    ('7x7 2^30 units', (1, 1, 7, 1, 16, 32768, 256, 1024, 8, 8, 8, 2, 7, 'full', 1), (17236225, 1, 1, 1024, 1024, 1, 50)),
    ('3x3 2^30 - 2^15 units', (1, 1, 3, 1, 16, 32767, 512, 1024, 8, 8, 8, 2, 7, 'full', 1), (83952384, 1, 1, 512, 512, 1, 40)),
    ('3x3 2^30 units', (1, 1, 3, 1, 16, 32768, 512, 1024, 8, 8, 8, 2, 7, 'full', 1), (16974081, 1, 1, 1024, 1024, 0, 0)),
    ('7x7 3 ci blocks, no slab in 64 KiB', (1, 1, 7, 1, 1, 1, 64, 32, 40, 40, 16, 16, 7, '64K', 1), (17236225, 1, 3, 2, 6, 0, 0)),
    ('7x7 1 ci block, a slab in 64 KiB', (1, 1, 7, 1, 1, 1, 64, 32, 8, 8, 16, 16, 7, '64K', 1), (83953408, 1, 1, 1, 1, 1, 200)),
    ('7x7 3 ci blocks, 1 MiB', (1, 1, 7, 1, 1, 1, 64, 32, 40, 40, 16, 16, 7, '1M', 1), (83953408, 3, 1, 6, 18, 1, 600)),
    ('7x7 9 ci blocks of CT 4: no slab in 1 MiB, and no split of the general kernel either', (1, 1, 7, 1, 1, 48, 64, 64, 144, 144, 64, 64, 7, '1M', 1), (17236225, 4, 9, 1, 36, 0, 0)),
    ('7x7 Cout 72, 1 MiB - 4', (1, 1, 7, 1, 2, 1, 5, 33, 8, 8, 72, 72, 7, '1M-4', 1), (17236225, 5, 1, 1, 5, 0, 0)),
    ('7x7 Cout 72, 1 MiB', (1, 1, 7, 1, 2, 1, 5, 33, 8, 8, 72, 72, 7, '1M', 1), (17236225, 5, 1, 1, 5, 1, 246)),
    ('7x7 Cout 72, full', (1, 1, 7, 1, 2, 1, 5, 33, 8, 8, 72, 72, 7, 'full', 1), (17236225, 5, 1, 1, 5, 1, 246)),
    ('7x7 288 x 150, no split in 1 MiB', (1, 1, 7, 1, 1, 1, 64, 32, 152, 150, 288, 288, 7, '1M', 1), (17236225, 18, 10, 1, 180, 0, 0)),
    ('7x7 288 x 150, full', (1, 1, 7, 1, 1, 1, 64, 32, 152, 150, 288, 288, 7, 'full', 1), (17236225, 18, 10, 2, 360, 1, 4096)),
    ('7x7 Cout 72, 20 tiles: 1 MiB holds one split', (1, 1, 7, 1, 1, 48, 64, 64, 64, 64, 72, 72, 7, '1M', 1), (17236225, 5, 4, 1, 20, 1, 982)),
    ('7x7 plain entry', (0, 1, 7, 1, 1, 1, 64, 32, 8, 8, 16, 16, 7, 'full', 1), (17236225, 1, 1, 2, 2, 0, 0)),
    ('3x3 144 x 144', (1, 1, 3, 1, 1, 1, 64, 32, 144, 144, 144, 144, 7, 'full', 1), (50331648, 1, 3, 8, 24, 1, 3456)),
    ('3x3 144 x 144 variant 0', (1, 1, 3, 1, 1, 1, 64, 32, 144, 144, 144, 144, 7, 'full', 0), (33554432, 1, 3, 8, 24, 1, 3456)),
    ('3x3 slabs do not fit 64 KiB', (1, 1, 3, 1, 1, 1, 64, 32, 144, 144, 144, 144, 7, '64K', 1), (16974593, 3, 9, 2, 54, 0, 0)),
    ('3x3 slabs do not fit 1 MiB', (1, 1, 3, 1, 1, 1, 64, 32, 144, 144, 144, 144, 7, '1M', 1), (16974593, 3, 9, 2, 54, 0, 0)),
    ('3x3 stem: Cin 3 in a stride of 8', (1, 1, 3, 1, 1, 1, 64, 32, 8, 3, 144, 144, 7, 'full', 1), (50331648, 1, 1, 8, 8, 1, 1152)),
    ('3x3 dense Cin 3', (1, 1, 3, 1, 1, 1, 64, 32, 3, 3, 144, 144, 7, 'full', 1), (16974593, 3, 1, 2, 6, 0, 0)),
    ('3x3 Cin 150 in a stride of 152', (1, 1, 3, 1, 1, 1, 64, 32, 152, 150, 144, 144, 7, 'full', 1), (50331648, 1, 4, 8, 32, 1, 4608)),
    ('3x3 x stride 150', (1, 1, 3, 1, 1, 1, 64, 32, 150, 144, 144, 144, 7, 'full', 1), (16974593, 3, 9, 2, 54, 0, 0)),
    ('3x3 x unaligned', (1, 1, 3, 1, 1, 1, 64, 32, 144, 144, 144, 144, 6, 'full', 1), (16974593, 3, 9, 2, 54, 0, 0)),
    ('3x3 dy 2-byte aligned', (1, 1, 3, 1, 1, 1, 64, 32, 144, 144, 144, 144, 5, 'full', 1), (16974593, 3, 9, 2, 54, 0, 0)),
    ('3x3 fp32', (1, 0, 3, 1, 1, 1, 64, 32, 144, 144, 144, 144, 7, 'full', 1), (16974593, 3, 9, 2, 54, 0, 0)),
    ('3x3 reach below 2^31', (1, 1, 3, 1, 1, 1, 6896, 1024, 152, 144, 152, 144, 7, 'full', 1), (50331648, 1, 3, 85, 255, 1, 3456)),
    ('3x3 reach above 2^31', (1, 1, 3, 1, 1, 1, 6897, 1024, 152, 144, 152, 144, 7, 'full', 1), (33554432, 1, 3, 85, 255, 1, 3456)),
    ('3x3 Cout 16, Cin 63, no workspace', (1, 1, 3, 1, 1, 1, 64, 32, 64, 63, 16, 16, 7, 'none', 1), (16974081, 1, 4, 2, 8, 0, 0)),
    ('3x3 Cout 16, Cin 64, no workspace', (1, 1, 3, 1, 1, 1, 64, 32, 64, 64, 16, 16, 7, 'none', 1), (16974084, 1, 1, 2, 2, 0, 0)),
    ('3x3 Cout 17, Cin 64, no workspace', (1, 1, 3, 1, 1, 1, 64, 32, 64, 64, 24, 17, 7, 'none', 1), (16974593, 1, 4, 2, 8, 0, 0)),
    ('3x3 fp32 Cout 16', (0, 0, 3, 1, 1, 1, 64, 32, 64, 64, 16, 16, 7, 'full', 1), (16974593, 1, 4, 2, 8, 0, 0)),
    ('1x1 K splits bounded by U / 32', (0, 1, 1, 1, 1, 1, 1, 2060, 40, 40, 56, 56, 7, 'full', 1), (16843523, 2, 1, 2, 4, 0, 0)),
    ('3x3 16 pairs', (0, 1, 3, 1, 16, 8, 64, 64, 144, 144, 144, 144, 7, 'full', 1), (16974593, 3, 9, 37, 999, 0, 0)),
    ('multi 3x3 x 8', (2, 1, 3, 8, 2, 1, 3, 33, 64, 56, 160, 152, 7, 'full', 1), (50331648, 2, 2, 1, 32, 1, 4608)),
    ('multi 3x3 x 8 variant 0', (2, 1, 3, 8, 2, 1, 3, 33, 64, 56, 160, 152, 7, 'full', 0), (33554432, 2, 2, 1, 32, 1, 4608)),
    ('multi 3x3 Cout 16', (2, 1, 3, 2, 1, 1, 64, 32, 64, 64, 16, 16, 7, 'full', 1), (50331648, 1, 2, 8, 32, 1, 2304)),
    ('multi 3x3 64 KiB', (2, 1, 3, 2, 1, 1, 64, 32, 64, 64, 16, 16, 7, '64K', 1), None),
    ('multi 3x3 dense Cin 3', (2, 1, 3, 2, 1, 1, 64, 32, 3, 3, 144, 144, 7, 'full', 1), None),
    ('multi 3x3 x unaligned', (2, 1, 3, 2, 1, 1, 64, 32, 64, 64, 16, 16, 6, 'full', 1), None),
    ('multi 3x3 reach above 2^31', (2, 1, 3, 2, 1, 1, 6897, 1024, 152, 144, 152, 144, 7, 'full', 1), (33554432, 1, 3, 42, 252, 1, 3456)),
    ('multi 1x1 x 8', (2, 1, 1, 8, 2, 1, 1, 2049, 144, 136, 160, 152, 7, 'full', 1), (67108864, 2, 1, 16, 256, 1, 720)),
    ('multi 1x1 63 units', (2, 1, 1, 8, 1, 1, 1, 2016, 144, 144, 144, 144, 7, 'full', 1), None),
    ('multi 1x1 64 units', (2, 1, 1, 8, 1, 1, 1, 2048, 144, 144, 144, 144, 7, 'full', 1), (67108864, 1, 1, 8, 64, 1, 360)),
    ('multi 1x1 64 KiB', (2, 1, 1, 8, 1, 1, 1, 2048, 144, 144, 144, 144, 7, '64K', 1), None),
    ('multi 1x1 Cin 150', (2, 1, 1, 2, 1, 1, 1, 2048, 152, 150, 144, 144, 7, 'full', 1), None),
    ('multi 1x1 x stride 150', (2, 1, 1, 2, 1, 1, 1, 2048, 150, 144, 144, 144, 7, 'full', 1), None),
]


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) the shapes of a train step.  Default bench step (4 clips x 7 frames x 64 x 64, 144 channels): problems, pairs, pixels and channels as
#     profiles/r04_e_wgrad_in_step.txt lists them for the recurrent chain (30 problems x 7 pairs on 8 x 64 x 64 pixels) and the TAB stages
#     (28 frames); SPyNet's five 7x7 convs on 48 frame pairs per pyramid level as in tools/bench_spy_wgrad.py; conv_last on the 28 HR frames.
#     "full:" rows: --workload train_full (1 clip, 112 channels), the same layers on a quarter of the frames.
# ------------------------------------------------------------------------------------------------------------------------------------
BENCH = [
    ('chain 3x3 144 -> 144, 8 per launch', (2, 1, 3, 8, 7, 8, 64, 64, 144, 144, 144, 144, 7, 'full', 1), (50331648, 1, 3, 10, 240, 1, 3456)),
    ('chain 3x3 144 -> 144, the last 6 of 30', (2, 1, 3, 6, 7, 8, 64, 64, 144, 144, 144, 144, 7, 'full', 1), (50331648, 1, 3, 14, 252, 1, 3456)),
    ('chain 3x3 144 -> 144, alone', (1, 1, 3, 1, 7, 8, 64, 64, 144, 144, 144, 144, 7, 'full', 1), (50331648, 1, 3, 85, 255, 1, 3456)),
    ('mixer 1x1 144 -> 144 x 8, 64 x 64', (2, 1, 1, 8, 1, 28, 64, 64, 144, 144, 144, 144, 7, 'full', 1), (67108864, 1, 1, 64, 512, 1, 360)),
    ('mixer 1x1 144 -> 144 x 8, 32 x 32', (2, 1, 1, 8, 1, 28, 32, 32, 144, 144, 144, 144, 7, 'full', 1), (67108864, 1, 1, 64, 512, 1, 360)),
    ('mixer 1x1 288 -> 144 x 4, 64 x 64', (2, 1, 1, 4, 1, 28, 64, 64, 288, 288, 144, 144, 7, 'full', 1), (67108864, 1, 2, 64, 512, 1, 720)),
    ('mixer 1x1 144 -> 144 x 4, 32 x 32', (2, 1, 1, 4, 1, 28, 32, 32, 144, 144, 144, 144, 7, 'full', 1), (67108864, 1, 1, 112, 448, 1, 360)),
    ('3x3 144 -> 288 x 4, 64 x 64', (2, 1, 3, 4, 1, 28, 64, 64, 144, 144, 288, 288, 7, 'full', 1), (50331648, 2, 3, 10, 240, 1, 6912)),
    ('3x3 144 -> 144 x 5, 32 x 32', (2, 1, 3, 5, 1, 28, 32, 32, 144, 144, 144, 144, 7, 'full', 1), (50331648, 1, 3, 17, 255, 1, 3456)),
    ('conv_last 3x3 64 -> 3, dense dy', (1, 1, 3, 1, 1, 28, 256, 256, 64, 64, 3, 3, 7, 'full', 1), (83952384, 4, 1, 128, 512, 1, 160)),
    ('conv_last 3x3 64 -> 3, dy padded to 8', (1, 1, 3, 1, 1, 28, 256, 256, 64, 64, 8, 3, 7, 'full', 1), (83952384, 4, 1, 128, 512, 1, 160)),
    ('SPyNet 7x7 8 -> 32 at 64 x 64', (1, 1, 7, 1, 1, 48, 64, 64, 8, 8, 32, 32, 7, 'full', 1), (84018944, 1, 1, 512, 512, 1, 400)),
    ('SPyNet 7x7 32 -> 64 at 64 x 64', (1, 1, 7, 1, 1, 48, 64, 64, 32, 32, 64, 64, 7, 'full', 1), (84150016, 2, 1, 230, 460, 1, 1600)),
    ('SPyNet 7x7 64 -> 32 at 64 x 64', (1, 1, 7, 1, 1, 48, 64, 64, 64, 64, 32, 32, 7, 'full', 1), (84018944, 4, 1, 128, 512, 1, 1600)),
    ('SPyNet 7x7 32 -> 16 at 64 x 64', (1, 1, 7, 1, 1, 48, 64, 64, 32, 32, 16, 16, 7, 'full', 1), (83953408, 2, 1, 256, 512, 1, 400)),
    ('SPyNet 7x7 16 -> 2 at 64 x 64', (1, 1, 7, 1, 1, 48, 64, 64, 16, 16, 2, 2, 7, 'full', 1), (83953408, 1, 1, 512, 512, 1, 200)),
    ('SPyNet 7x7 8 -> 32 at 16 x 16', (1, 1, 7, 1, 1, 48, 16, 16, 8, 8, 32, 32, 7, 'full', 1), (84018944, 1, 1, 96, 96, 1, 400)),
    ('SPyNet 7x7 32 -> 64 at 16 x 16', (1, 1, 7, 1, 1, 48, 16, 16, 32, 32, 64, 64, 7, 'full', 1), (84150016, 2, 1, 96, 192, 1, 1600)),
    ('SPyNet 7x7 64 -> 32 at 16 x 16', (1, 1, 7, 1, 1, 48, 16, 16, 64, 64, 32, 32, 7, 'full', 1), (84018944, 4, 1, 96, 384, 1, 1600)),
    ('SPyNet 7x7 32 -> 16 at 16 x 16', (1, 1, 7, 1, 1, 48, 16, 16, 32, 32, 16, 16, 7, 'full', 1), (83953408, 2, 1, 96, 192, 1, 400)),
    ('SPyNet 7x7 16 -> 2 at 16 x 16', (1, 1, 7, 1, 1, 48, 16, 16, 16, 16, 2, 2, 7, 'full', 1), (83953408, 1, 1, 96, 96, 1, 200)),
    ('SPyNet 7x7 8 -> 32 at 2 x 2', (1, 1, 7, 1, 1, 48, 2, 2, 8, 8, 32, 32, 7, 'full', 1), (84018944, 1, 1, 24, 24, 1, 400)),
    ('SPyNet 7x7 32 -> 64 at 2 x 2', (1, 1, 7, 1, 1, 48, 2, 2, 32, 32, 64, 64, 7, 'full', 1), (84150016, 2, 1, 24, 48, 1, 1600)),
    ('SPyNet 7x7 64 -> 32 at 2 x 2', (1, 1, 7, 1, 1, 48, 2, 2, 64, 64, 32, 32, 7, 'full', 1), (84018944, 4, 1, 24, 96, 1, 1600)),
    ('SPyNet 7x7 32 -> 16 at 2 x 2', (1, 1, 7, 1, 1, 48, 2, 2, 32, 32, 16, 16, 7, 'full', 1), (83953408, 2, 1, 24, 48, 1, 400)),
    ('SPyNet 7x7 16 -> 2 at 2 x 2', (1, 1, 7, 1, 1, 48, 2, 2, 16, 16, 2, 2, 7, 'full', 1), (83953408, 1, 1, 24, 24, 1, 200)),
    ('full: chain 3x3 112 -> 112, 8 per launch', (2, 1, 3, 8, 7, 2, 64, 64, 112, 112, 112, 112, 7, 'full', 1), (50331648, 1, 3, 10, 240, 1, 3456)),
    ('full: mixer 1x1 112 -> 112 x 8, 64 x 64', (2, 1, 1, 8, 1, 7, 64, 64, 112, 112, 112, 112, 7, 'full', 1), (67108864, 1, 1, 64, 512, 1, 360)),
    ('full: conv_last 3x3 64 -> 3', (1, 1, 3, 1, 1, 7, 256, 256, 64, 64, 3, 3, 7, 'full', 1), (83952384, 4, 1, 128, 512, 1, 160)),
    ('full: SPyNet 7x7 32 -> 64 at 64 x 64', (1, 1, 7, 1, 1, 12, 64, 64, 32, 32, 64, 64, 7, 'full', 1), (84150016, 2, 1, 192, 384, 1, 1600)),
]


def _check_row(row, variant):
    name, args, want = row
    entry, code, *dims, align, ws, v = args
    variant(v)
    assert _plan(entry, code, *dims, align=align, ws=ws) == want, name


@pytest.mark.parametrize("row", THRESHOLDS, ids=lambda r: r[0])
def test_thresholds(row, variant):
    _check_row(row, variant)


@pytest.mark.parametrize("row", BENCH, ids=lambda r: r[0])
def test_train_step_shapes(row, variant):
    _check_row(row, variant)


def test_hard_errors_are_the_same_for_every_entry():
    ok = dict(dtype=BF16, ks=3, nprob=1, npairs=1, N=1, H=8, W=33, x_ps=48, Cin=48, dy_ps=144, Cout=144)
    bad = [dict(ks=5), dict(dtype=2), dict(npairs=0), dict(npairs=17), dict(N=0), dict(H=0), dict(W=0), dict(x_ps=40), dict(dy_ps=136), dict(It=40), dict(o0=-1),
           dict(i0=-1), dict(i0=8, It=48)]
    for entry in (PLAIN, WS, MULTI):
        assert _plan(entry, **ok) is not None
        for b in bad:
            assert _plan(entry, **{**ok, **b}) is None, (entry, b)
    assert _plan(PLAIN, **{**ok, "nprob": 2}) is None and _plan(MULTI, **{**ok, "nprob": 8}) is not None and _plan(MULTI, **{**ok, "nprob": 9}) is None


# ------------------------------------------------------------------------------------------------------------------------------------
# (d) kernels.conv_wgrad3_multi_ok(x, dy, ks) implies that the multi entry takes the operands
# ------------------------------------------------------------------------------------------------------------------------------------
def _operand(M, C, ps, off):
    return WR.embed(torch.zeros(1, 1, M, C, dtype=BF16), ps, 0, offset=off)


OK_ROWS = [(args[2],) + args[8:13] for _, args, _ in THRESHOLDS if args[1] == 1 and args[2] in (1, 3) and args[12] & DY2] + [
    (3, 150, 144, 144, 144, 7), (3, 150, 72, 150, 72, 7),  # a channel slice of a 150-wide tensor
    (3, 3, 3, 144, 144, 7), (1, 3, 3, 144, 144, 7),        # dense 3 channels
    (3, 8, 3, 24, 17, 7), (3, 64, 64, 16, 16, 7), (1, 152, 152, 8, 8, 7), (1, 144, 144, 152, 150, 7)]


@pytest.mark.parametrize("row", sorted(set(OK_ROWS)), ids=lambda r: "-".join(map(str, r)))
def test_multi_ok_implies_the_large_tile_kernel(row):
    from vmg_amd import kernels as K
    hip, _ = _lib()
    ks, x_ps, Cin, dy_ps, Cout, align = row
    M = 2048
    x, dy = _operand(M, Cin, x_ps, 0 if align & X16 else 1), _operand(M, Cout, dy_ps, 0 if align & DY16 else 1)
    assert (x.data_ptr() % 16 == 0) == bool(align & X16) and (dy.data_ptr() % 16 == 0) == bool(align & DY16)
    for src, d in ((x, dy), (x.float(), dy), (x, dy.float())):
        if K.conv_wgrad3_multi_ok(src, d, ks):
            assert src.dtype == d.dtype == BF16
            for nprob in (1, 8):
                p = _plan(MULTI, BF16, ks, nprob, 1, 1, 1, M, x_ps, Cin, dy_ps, Cout, align=align)
                assert p is not None and p[0] >> 24 in (hip.WGRAD_3, hip.WGRAD_3B, hip.WGRAD_L2), (row, nprob, p)
    assert not K.conv_wgrad3_multi_ok(x, dy, 7)


def test_multi_ok_accepts_what_the_step_passes():
    """Dense 144-channel operands, the padded stem input, 2 048 pixels for a Linear: the predicate must not turn these away."""
    from vmg_amd import kernels as K
    a, b8, s3 = _operand(2048, 144, 144, 0), _operand(2048, 144, 152, 0), _operand(2048, 3, 8, 0)
    assert K.conv_wgrad3_multi_ok(a, a, 3) and K.conv_wgrad3_multi_ok(a, b8, 1) and K.conv_wgrad3_multi_ok(s3, a, 3)
    assert not K.conv_wgrad3_multi_ok(_operand(2047, 144, 144, 0), _operand(2047, 144, 144, 0), 1)
