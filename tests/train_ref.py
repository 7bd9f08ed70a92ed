"""Plain references of the kernels that end a training step: csrc/optim.hip (adamw_flat_kernel, grad_sumsq_kernel, grad_clip_scale_kernel)
and csrc/loss.hip (lap_even_blur_kernel, lap_fwd_kernel, lap_bwd_even_kernel, lap_bwd_kernel).  Torch and NumPy only, written from the
operations' definitions; tests/test_train_ref.py pins each against an independent one (torch.optim.AdamW, torch.nn.utils.clip_grad_norm_,
the oracle's loss and autograd).  Everything is fp64 and runs on whatever device its tensor arguments live on, so the few cases past the
kernels' grid caps can be evaluated where their inputs are.

Next to every value the reference returns the magnitudes S that a rounding-error bound scales with, and the *_bounds functions turn them
into per-element bounds  c * 2^-24 * S  with c counted from the kernel's fp32 operations (one rounding of at most 2^-24 relative per
operation; a contraction into a fused multiply-add only removes roundings).  ORDER2 covers the products of those terms (every c * 2^-24
here is below 1e-4, so the second-order part is below 1e-4 of the first)."""
import math

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24           # unit roundoff of fp32
DENORM = 2.0 ** -149     # the smallest fp32 denormal
MIN_NORMAL = 2.0 ** -126
ORDER2 = 1.001


def bits(t):
    return t.contiguous().view(torch.int32)


def f32(v):
    """A host double as the kernel receives it through a `float` argument or an fp32 tensor, widened again."""
    return float(np.float32(v))


# ================================================================================================ AdamW
def adamw_step_ref(p, g, m, v, lr, wd, b1, b2, eps, t):
    """One torch.optim.AdamW step (no amsgrad, no maximize) from the given state, fp64, step count t >= 1 AFTER the increment:
        p *= 1 - lr wd;  m += (1 - b1)(g - m);  v = b2 v + (1 - b2) g^2;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
    with bc1 = 1 - b1^t, bc2 = 1 - b2^t.  p, g, m, v: the fp32 values (any float tensor; widened here).  -> (p, m, v, mags): the new
    state and the intermediate magnitudes adamw_bounds needs."""
    p, g, m, v = (a.to(F64) for a in (p, g, m, v))
    bc1, sq = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
    decay, step = 1.0 - lr * wd, lr / bc1
    q = p * decay
    mo = m + (1.0 - b1) * (g - m)
    g2 = g * g
    vo = b2 * v + (1.0 - b2) * g2
    root = vo.sqrt()
    den = root / sq + eps
    ratio = mo / den
    upd = step * ratio
    pn = q - upd
    mags = dict(p=p.abs(), q=q.abs(), gm=(g - m).abs(), mo=mo.abs(), v=v, g2=g2, vo=vo, root=root, den=den, ratio=ratio.abs(), upd=upd.abs(),
                pn=pn.abs(), lr=lr, wd=wd, b1=b1, b2=b2, eps=eps, sq=sq, step=abs(step), decay=abs(decay))
    return pn, mo, vo, mags


def one_minus_kappa(b):
    """|fl32(1 - fl32(b)) - (1 - b)| / (1 - b) in units of U: how far the kernel's fp32 `1 - b` is from the host's."""
    return abs(float(np.float32(1.0) - np.float32(b)) - (1.0 - b)) / (1.0 - b) / U


def adamw_bounds(k):
    """Per-element bounds (Bp, Bm, Bv) on |kernel - adamw_step_ref| for adamw_flat_kernel, from the magnitudes `k` of adamw_step_ref.

    The kernel receives fl32 of the host's doubles: b1, b2, eps as arguments, (lr, wd, bc1, sqrt(bc2)) as a `hyper` row; each is off by up
    to U relative.  It forms c = 1 - b in fp32 from the rounded b, which magnifies b's rounding by b / (1 - b) (99 for b2 = 0.99): instead
    of that worst case the bound takes the ACTUAL relative distance kappa of fl32(1 - fl32(b)) from 1 - b, a property of the number format
    (0.10 U for b1 = 0.9, 16 U for b2 = 0.99), in units of U.
      m = M + c1 (G - M):        c1 [kappa1], the subtraction, the product: (kappa1 + 2) U (1 - b1)|g - m|;  the sum: U |m'|.
      v = b2 V + c2 (G G):       b2 and its product: 2 U b2 v;  c2 [kappa2], the square, the product: (kappa2 + 2) U (1 - b2) g^2;
                                 the sum: U v'.  Where g^2 is below the smallest normal fp32 the products round to a multiple of DENORM
                                 (absolute error up to DENORM / 2 each, the later one scaled by 1 - b2 < 1; sums of denormals are exact):
                                 one DENORM in all.
      root = sqrtf(v'):          |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= min(Bv / (sqrt(b) + sqrt(max(b - Bv, 0))), sqrt(Bv)), and
                                 U root for sqrtf (correctly rounded).
      den = root / sq + eps:     sq and the division: 2 U root / sq;  eps: U eps;  the sum: U den.
      ratio = m' / den:          Bm / den + |ratio| Bden / den + U |ratio|.
      step = lr / bc1:           3 U (two roundings of inputs, one division);  upd = step ratio: one more.
      q = P decay:               decay = 1 - lr wd is off by 3 U lr wd + U decay;  the product: U |q|.
      p' = q - upd:              U |p'|."""
    k1, k2 = one_minus_kappa(k["b1"]), one_minus_kappa(k["b2"])
    Bm = U * ((k1 + 2.0) * (1.0 - k["b1"]) * k["gm"] + k["mo"])
    floor = torch.where(k["g2"] < MIN_NORMAL, torch.full_like(k["g2"], DENORM), torch.zeros_like(k["g2"]))
    Bv = U * (2.0 * k["b2"] * k["v"] + (k2 + 2.0) * (1.0 - k["b2"]) * k["g2"] + k["vo"]) + floor
    Broot = torch.minimum(Bv / (k["root"] + (k["vo"] - Bv).clamp_min(0).sqrt()).clamp_min(1e-300), Bv.sqrt()) + U * k["root"]
    Bden = Broot / k["sq"] + U * (2.0 * k["root"] / k["sq"] + k["eps"] + k["den"])
    Bratio = Bm / k["den"] + k["ratio"] * Bden / k["den"] + U * k["ratio"]
    Bupd = k["step"] * Bratio + 4.0 * U * k["upd"]
    Bp = k["p"] * U * (3.0 * k["lr"] * k["wd"] + k["decay"]) + U * k["q"] + Bupd + U * k["pn"]
    return Bp * ORDER2, Bm * ORDER2, Bv * ORDER2


# ================================================================================================ gradient clipping
CLIP_BLOCKS = 1024  # csrc/optim.hip


def clip_coef_ref(norm32, max_norm):
    """clamp(max_norm / (norm + 1e-6), max=1) in float32 arithmetic from an fp32 norm: one addition, one correctly rounded division, and a
    cap that leaves NaN as it is.  -> np.float32."""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else c


def clip_ref(g, max_norm, norm32=None):
    """torch.nn.utils.clip_grad_norm_(g, max_norm, norm_type=2) on one flat fp32 gradient.  -> (norm, coef, scaled): the fp64 total norm
    (a 0-dim fp64 tensor on g's device), the np.float32 coefficient computed from `norm32` (default: the fp64 norm rounded to fp32), and
    fl32(g * coef), which for coef == 1 is g itself, bit for bit."""
    norm = g.to(F64).square().sum().sqrt()
    coef = clip_coef_ref(float(norm) if norm32 is None else norm32, max_norm)
    scaled = g * torch.tensor(float(coef), dtype=F32, device=g.device)  # one fp32 product per element
    return norm, coef, scaled


def clip_norm_bound(n, norm):
    """Bound on |norm_out[0] - norm| for grad_sumsq_kernel + grad_clip_scale_kernel on n elements.

    A lane adds, per trip, x^2 + y^2 + z^2 + w^2 of one float4 to an fp32 run: each square one rounding, three additions inside the float4, one
    into the run, and a run holds at most 64 trips before it is moved to a double.  A block owns per = ceil(n4 / 1024) float4, a lane at most
    ceil(per / 256) of them.  All terms are non-negative, so the sum of squares is off by at most (1 + 3 + min(trips, 64)) U relative;
    everything above (the runs, the waves, the 1024 partials, the n % 4 tail) is added in double, a few thousand roundings of 2^-53.  A square
    below the smallest normal fp32 is off by up to DENORM / 2 absolutely: n DENORM / 2 in all.  sqrt halves the relative error
    (|sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b))); the conversion to float adds U."""
    n4 = n // 4
    per = -(-n4 // CLIP_BLOCKS)
    trips = -(-per // 256)
    c = 1 + 3 + min(trips, 64)
    if norm == 0.0:
        return 0.0
    Bsumsq = (c * U + 4096 * 2.0 ** -53) * norm * norm + 0.5 * n * DENORM
    return (Bsumsq / (norm + math.sqrt(max(norm * norm - Bsumsq, 0.0))) + U * norm) * ORDER2


# ================================================================================================ Laplacian pyramid of the loss
TAPS = tuple(float(np.float32(t)) for t in (0.05, 0.25, 0.4, 0.25, 0.05))  # the fp32 taps (what the kernels and the oracle's kernel tensor hold)


def blur_matrix(n, device="cpu", taps=TAPS):
    """G_n: the n x n matrix of the 1-D five-tap blur with replicate padding, G[t, clamp(t + e)] += k(e), e = -2 .. 2."""
    G = np.zeros((n, n), dtype=np.float64)
    for t in range(n):
        for e in range(-2, 3):
            G[t, min(max(t + e, 0), n - 1)] += taps[e + 2]
    return torch.from_numpy(G).to(device)


def even_matrix(n, device="cpu"):
    """Z_n: keep the even positions, times 2 (per axis: 4 for both), zero the odd ones."""
    z = np.zeros(n, dtype=np.float64)
    z[::2] = 2.0
    return torch.diag(torch.from_numpy(z)).to(device)


def _two(My, Mx, v):
    """My v Mx^T on the last two axes (one axis after the other)."""
    return torch.matmul(torch.matmul(My, v), Mx.transpose(0, 1))


class Pyramid:
    """The matrices of one image size (H, W) and the operators of the loss built from them; v is (planes, H, W) fp64.
        down(v) = Z G v G^T Z      (the blurred image times 4 at (even, even), zero elsewhere; [::2, ::2] of it is the kernels' a1)
        lap(v)  = v - G down(v) G^T
    and the adjoints by transposing the SAME matrices:
        lap_t(w)  = w - G^T Z (G^T w G) Z G   ([::2, ::2] of Z (G^T w G) Z is the kernels' u).
    Every entry of G and Z is non-negative, so the same products applied to |v| are the sums of absolute terms."""

    def __init__(self, H, W, device="cpu"):
        self.H, self.W = H, W
        self.Gy, self.Gx = blur_matrix(H, device), blur_matrix(W, device)
        self.Zy, self.Zx = even_matrix(H, device), even_matrix(W, device)
        self.GyT, self.GxT = self.Gy.transpose(0, 1).contiguous(), self.Gx.transpose(0, 1).contiguous()

    def blur(self, v):
        return _two(self.Gy, self.Gx, v)

    def blur_t(self, w):
        return _two(self.GyT, self.GxT, w)

    def stuff(self, v):
        return _two(self.Zy, self.Zx, v)

    def lap(self, v):
        return v - self.blur(self.stuff(self.blur(v)))

    def lap_t(self, w):
        return w - self.blur_t(self.stuff(self.blur_t(w)))


def lap_fwd_ref(x, y, eps, pyr=None):
    """Forward of the loss kernels on (planes, H, W): d = x - y, a1 = 4 (G d) at even positions (quarter size), ld = lap(d), and the two sums
    sum sqrt(d^2 + eps), sum sqrt(ld^2 + eps).  -> dict with the values and the sums of absolute terms: S_a1 = 4 (G |d|) at even positions,
    S_gz = G z[|a1|] (the second blur's terms), S_gz2 = G z[S_a1] (what an error of a1 relative to S_a1 becomes in ld)."""
    pyr = pyr or Pyramid(x.shape[-2], x.shape[-1], x.device)
    d = x.to(F64) - y.to(F64)
    A = pyr.stuff(pyr.blur(d))
    SA = pyr.stuff(pyr.blur(d.abs()))
    gz = pyr.blur(A)
    ld = d - gz
    t1, t2 = (d * d + eps).sqrt(), (ld * ld + eps).sqrt()
    return dict(d=d, a1=A[..., ::2, ::2].contiguous(), S_a1=SA[..., ::2, ::2].contiguous(), gz=gz, S_gz=pyr.blur(A.abs()), S_gz2=pyr.blur(SA),
                ld=ld, sum1=t1.sum(), sum2=t2.sum(), pyr=pyr)


def lap_fwd_bounds(r, trips):
    """Bounds for lap_even_blur_kernel and lap_fwd_kernel from lap_fwd_ref's dict; `trips` = grid-stride trips of a lane of lap_fwd_kernel.
      a1:   v = x - y [1], per row five products [1] summed from 0 [4 additions], five row sums times a tap [1] summed [4], times 4 (exact):
            11 U S_a1.
      ld:   the second blur reads the kernel's a1 (off by 11 U S_a1 -> 11 U S_gz2 after the blur) and does the same product-and-sum per
            axis [5 + 5] on its own terms: 10 U S_gz;  d = x - y: U |d|;  the subtraction: U |ld|.
      sums: sqrt(. + eps) has slope <= 1 in its argument's root, so a term moves by at most the error of d (U |d|) or of ld (B_ld), plus its
            own operations: the square and the sum [2] halved by the root, the root [1]: 2 U of the term.  A term then passes through the
            lane's run (`trips` additions) and eight levels of the block's tree: (trips + 8) U of the sum of terms."""
    B_a1 = 11.0 * U * r["S_a1"] * ORDER2
    B_ld = U * (r["d"].abs() + r["ld"].abs() + 10.0 * r["S_gz"] + 11.0 * r["S_gz2"]) * ORDER2
    B_sum1 = (U * r["d"].abs().sum() + (2.0 + trips + 8.0) * U * r["sum1"]) * ORDER2
    B_sum2 = (B_ld.sum() + (2.0 + trips + 8.0) * U * r["sum2"]) * ORDER2
    return dict(a1=B_a1, ld=B_ld, sum1=B_sum1, sum2=B_sum2)


def lap_bwd_ref(x, y, ld, eps, gs1, gs2, pyr=None):
    """Backward of the loss kernels FROM A GIVEN ld (the forward kernel's fp32 output: w has slope up to 1 / sqrt(eps) at ld = 0, so only a
    reference that starts from the same ld can be compared tightly):
        w = ld / sqrt(ld^2 + eps);  u = 4 (G^T w G) at even positions (quarter size);  dx = gs1 d / sqrt(d^2 + eps) + gs2 (w - G^T z[u] G)
    with the transposes of the forward's matrices.  -> dict with the values and S_u = 4 (G^T |w| G) at even positions, S_t = G^T z[|u|] G,
    S_t2 = G^T z[S_u] G."""
    pyr = pyr or Pyramid(x.shape[-2], x.shape[-1], x.device)
    d = x.to(F64) - y.to(F64)
    ld = ld.to(F64)
    w = ld / (ld * ld + eps).sqrt()
    Uf = pyr.stuff(pyr.blur_t(w))        # 4 (G^T w) at (even, even), zero elsewhere
    SU = pyr.stuff(pyr.blur_t(w.abs()))
    t = pyr.blur_t(Uf)
    f1 = d / (d * d + eps).sqrt()
    dx = gs1 * f1 + gs2 * (w - t)
    return dict(w=w, u=Uf[..., ::2, ::2].contiguous(), S_u=SU[..., ::2, ::2].contiguous(), t=t, S_t=pyr.blur_t(Uf.abs()), S_t2=pyr.blur_t(SU),
                f1=f1, dx=dx, gs1=gs1, gs2=gs2)


def lap_bwd_bounds(r):
    """Bounds for lap_bwd_even_kernel and lap_bwd_kernel from lap_bwd_ref's dict.
      w:    the square and the sum [2] halved by the root, the root [1], the division [1]: 3 U |w|.
      u:    the adjoint weight of an edge target is a sum of up to three taps [2 additions]; per axis weight [2], product [1], up to five
            terms summed from 0 [4]: 7 per axis, 14 for both, on terms that carry w's 3: 17 U S_u (times 4: exact).
      t:    reads the kernel's u (17 U S_u -> 17 U S_t2) and does the same weights, products and sums: 14 U S_t.
      dx:   d = x - y [1] (a RELATIVE change of d moves d / sqrt(d^2 + eps) by no more than the same relative amount), then as w [3], times
            gs1 [1]: 5 U |gs1 f1|;  gs2 ((w - t)): w [3 U |w|], t [above], the subtraction and the product [2 U |w - t|];  the sum: U |dx|."""
    B_u = 17.0 * U * r["S_u"] * ORDER2
    B_t = U * (14.0 * r["S_t"] + 17.0 * r["S_t2"])
    wt = (r["w"] - r["t"]).abs()
    B_dx = (5.0 * U * abs(r["gs1"]) * r["f1"].abs() + abs(r["gs2"]) * (3.0 * U * r["w"].abs() + B_t + 2.0 * U * wt) + U * r["dx"].abs()) * ORDER2
    return dict(u=B_u, dx=B_dx)


def loss_ref(x, y, eps, aux_ratio):
    """The loss value mean sqrt(d^2 + eps) + aux_ratio * mean sqrt(lap(d)^2 + eps) on (B, T, 3, H, W), through the matrices."""
    H, W = x.shape[-2:]
    r = lap_fwd_ref(x.reshape(-1, H, W), y.reshape(-1, H, W), eps)
    return (r["sum1"] + aux_ratio * r["sum2"]) / x.numel()


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements (0 / 0 counts as 0: an exact result under a zero bound)."""
    err = (got.to(F64) - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0
