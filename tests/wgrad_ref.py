"""Reference of the OPERATION behind vmg_conv_wgrad* (include/vmg_hip.h), spelled the slow obvious way in fp64, and the inputs that make
a comparison with it EXACT: torch and numpy only, nothing of vmg_amd.

    dW[o][i][ky][kx] = sum_pairs sum_{n,y,x} dY[n,y,x,o] * X[n, y+ky-ks//2, x+kx-ks//2, i]       db[o] = sum_pairs sum_{n,y,x} dY[n,y,x,o]

The kernels multiply bf16 / fp32 values exactly into fp32 and add in fp32, each in an order of its own (waves, LDS and global float atomics,
K slabs, a reduce kernel).  With every operand value k * 2^-s, k a small integer, every product is an integer multiple of 2^-(sx+sy), and as
long as the sum of the products' magnitudes stays below 2^24 of those units every partial sum in ANY order is an fp32 number: the result has
no rounding at all and must equal the fp64 reference bit for bit."""
import numpy as np
import torch
import torch.nn.functional as F

# family -> (largest |k|, s): values k * 2^-s.  "full" uses every mantissa bit of a bf16 (255 = 0b11111111), "small" allows long sums.
FAMILIES = {"full": (255, 7), "small": (8, 2)}
# largest |integer| of an initial dW / db value that assert_exact accounts for
INIT_MAX = {"full": 1, "small": 8}


def wgrad_ref(xs, dys, ks):
    """xs[p] (N, H, W, Cin), dys[p] (N, H, W, Cout) channels-last -> (dW (Cout, Cin, ks, ks), db (Cout,)) in fp64, summed over the pairs."""
    pad = ks // 2
    N, H, W, Cin = xs[0].shape
    Cout = dys[0].shape[-1]
    dW = torch.zeros(Cout, Cin, ks, ks, dtype=torch.float64)
    db = torch.zeros(Cout, dtype=torch.float64)
    for x, dy in zip(xs, dys):
        assert tuple(x.shape) == (N, H, W, Cin) and tuple(dy.shape) == (N, H, W, Cout)
        x, dy = x.double(), dy.double()
        xpad = F.pad(x, (0, 0, pad, pad, pad, pad))
        for ky in range(ks):
            for kx in range(ks):
                dW[:, :, ky, kx] += torch.einsum("nhwo,nhwi->oi", dy, xpad[:, ky:ky + H, kx:kx + W])
        db += dy.sum((0, 1, 2))
    return dW, db


def exact_values(shape, seed, family):
    """Dense seeded fp32 values k * 2^-s of the family (every one also a bf16 number), k uniform in [-kmax, kmax]."""
    kmax, s = FAMILIES[family]
    k = torch.randint(-kmax, kmax + 1, tuple(shape), generator=torch.Generator().manual_seed(seed))
    return k.float() / float(2 ** s)


def exact_init(shape, seed, family):
    """Integer-valued fp32 initial gradient within the family's INIT_MAX."""
    m = INIT_MAX[family]
    return torch.randint(-m, m + 1, tuple(shape), generator=torch.Generator().manual_seed(seed)).float()


def assert_exact(family, terms, init_max=None):
    """The invariant: with `terms` products per output element (pixels * pairs), operands of the family, an integer initial value up to
    init_max and a scale in {1, 0.5, -0.25}, init + scale * (any partial sum) is an fp32 number.  A partial sum is an integer below
    kmax^2 * terms in units of 2^-2s; scaled by a power of two it keeps that integer.  The initial value is at most init_max * 2^(2s+2)
    in units of the finest grid, 2^-(2s+2) (scale -0.25).  Their sum below 2^24 bounds the integer of every intermediate value for every
    scale (conservatively for 1 and 0.5, whose grids are coarser), so each fits the 24-bit significand."""
    kmax, s = FAMILIES[family]
    init_max = INIT_MAX[family] if init_max is None else init_max
    assert init_max <= INIT_MAX[family]
    total = kmax * kmax * terms + init_max * 2 ** (2 * s + 2)
    assert total < 2 ** 24, f"family {family!r} is not exact at {terms} terms: {total} >= 2^24"


def embed(t, pix_stride, guard, offset=0, device=None):
    """Place the channels-last tensor t (..., C) into a larger NaN-filled allocation and return a view of t's shape whose pixel stride is
    pix_stride elements and whose first element lies 16-byte aligned (+ `offset` elements, to make an unaligned operand).  At least `guard`
    pixels of NaN lie before and after the view.  Inside a pixel's stride, channels [C, C8) -- C8 = C rounded up to 8, the channels the
    kernels document as "computed and dropped" -- hold finite junk, channels [C8, pix_stride) NaN.  The allocation is made on `device`."""
    C = t.shape[-1]
    M = t.numel() // C
    assert pix_stride >= C and guard >= 0 and offset >= 0
    es = t.element_size()
    front = guard * pix_stride
    front += (-front * es % 16) // es  # (es divides 16: the view starts on a 16-byte boundary of the aligned allocation)
    total = front + offset + M * pix_stride + guard * pix_stride
    flat = torch.full((total,), float("nan"), dtype=t.dtype)
    body = flat[front + offset: front + offset + M * pix_stride].view(M, pix_stride)
    body[:, :C] = t.reshape(M, C)
    c8 = min((C + 7) // 8 * 8, pix_stride)
    if c8 > C:
        junk = torch.randint(-64, 65, (M, c8 - C), generator=torch.Generator().manual_seed(M * 131 + C)).to(t.dtype)
        body[:, C:c8] = junk + 0.5
    if device is not None:
        flat = flat.to(device)
    assert flat.data_ptr() % 16 == 0
    lead = tuple(t.shape[:-1])
    strides = []
    acc = pix_stride
    for d in reversed(lead):
        strides.append(acc)
        acc *= d
    view = flat.as_strided(lead + (C,), tuple(reversed(strides)) + (1,), front + offset)
    assert view.data_ptr() % 16 == (offset * es) % 16
    return view


def embed_outside(view):
    """Every element of the allocation behind an embed() view that is not one of the view's own elements, as one flat tensor (for tests of
    embed itself), and the number of junk (finite) elements among them."""
    C, ps = view.shape[-1], view.stride(-2) if view.dim() > 1 else view.shape[-1]
    M = view.numel() // C
    base = view._base if view._base is not None else view
    flat = base.reshape(-1)
    mask = torch.ones(flat.numel(), dtype=torch.bool)
    idx = (view.storage_offset() + torch.arange(M)[:, None] * ps + torch.arange(C)[None, :]).reshape(-1)
    mask[idx] = False
    return flat[mask]


def first_mismatch(got, want):
    """(number of differing elements, index of the first, got there, want there) of two equal-shaped tensors; NaN differs from everything."""
    bad = ~(got == want)
    n = int(bad.sum())
    if n == 0:
        return 0, None, None, None
    i = int(torch.nonzero(bad.reshape(-1))[0])
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(got.shape)))
    return n, idx, float(got[idx]), float(want[idx])
