"""Reference of the OPERATIONS behind csrc/ltam.hip (trajectory window attention, forward and backward) and csrc/warp.hip (bilinear / border
flow warp forward and backward, nearest location advection, flow smoothing), spelled the slow obvious way.  Plain module: numpy and torch
only, neither the package nor the oracle (tests/test_traj_ref.py pins it against the oracle and against fp32 F.grid_sample).

Sampling POSITIONS are part of the operations' definition and are float32: the coordinates are computed in float32, one rounding per step,
in the order flow_warp + F.grid_sample(align_corners=True) take them
    g = x + flow;   gn = 2 g / max(size - 1, 1) - 1;   i = ((gn + 1) / 2) (size - 1)
then clamped (border) or rounded half-to-even with zeros padding (the attention's gather).  Everything that touches VALUES -- bilinear
weights, norms, logits, softmax, every sum -- is float64.

The small functions below (decay_powers, rpe_term, round_index, pad_index, norm_groups, border_grad, bilinear_weights) each hold one
convention of the operation; tests/test_traj_ref.py patches them one at a time to build deliberately wrong variants.

Every backward also returns, on request, the SCALE of each gradient element: the sum of the absolute values of the addends the reference
summed into it.  A kernel that adds the same terms in fp32 in another order is off by a small multiple of 2^-24 of that scale."""
import numpy as np
import torch

F32 = np.float32
EPS = 1e-12


# ------------------------------------------------------------------------------------------------------------------ positions (float32)
def unnorm_coord(pos, size):
    """float32 pixel positions -> float32 sample coordinates, through the normalised grid and back (align_corners=True)."""
    pos = np.asarray(pos, dtype=F32)
    gn = (F32(2.0) * pos) / F32(max(size - 1, 1)) - F32(1.0)
    return ((gn + F32(1.0)) / F32(2.0)) * F32(size - 1)


def round_index(v):
    """std::nearbyint in the default rounding mode: half to even."""
    return np.rint(v)


def pad_index(xn, yn, h, w):
    """The attention's gather pads with ZEROS: a rounded position outside the map has no source (-1)."""
    ok = (xn >= 0) & (xn <= w - 1) & (yn >= 0) & (yn <= h - 1)
    return np.where(ok, yn * w + xn, -1).astype(np.int64)


def ltam_gather_index(loc, h, w):
    """loc (n, 2t, h, w) float32 tracked positions, x then y per key-frame -> (n, t, h, w) int64 source pixel y * w + x, or -1."""
    loc = np.asarray(loc, dtype=F32)
    n, t2 = loc.shape[:2]
    lx, ly = loc[:, 0::2], loc[:, 1::2]
    with np.errstate(invalid="ignore"):
        xn, yn = round_index(unnorm_coord(lx, w)), round_index(unnorm_coord(ly, h))
        return pad_index(xn, yn, h, w)


def border_grad(v, hi):
    """clip_coordinates_set_grad: the gradient of the clamp is 0 AT and beyond the borders."""
    return ((v > 0) & (v < hi)).astype(np.float64)


def warp_coords(flow, h, w):
    """flow (n, h, w, 2) float32 -> clamped float32 sample coordinates ix, iy (n, h, w) and the clamp's gradient factors."""
    flow = np.asarray(flow, dtype=F32)
    ix = unnorm_coord(np.arange(w, dtype=F32)[None, None, :] + flow[..., 0], w)
    iy = unnorm_coord(np.arange(h, dtype=F32)[None, :, None] + flow[..., 1], h)
    gmx, gmy = border_grad(ix, F32(w - 1)), border_grad(iy, F32(h - 1))
    return np.clip(ix, F32(0), F32(w - 1)), np.clip(iy, F32(0), F32(h - 1)), gmx, gmy


def bilinear_weights(tx, ty):
    """nw, ne, sw, se: x runs west -> east with tx, y north -> south with ty."""
    return (1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty


# ------------------------------------------------------------------------------------------------------------------ flow warp
def _corners(flow, h, w):
    ix, iy, gmx, gmy = warp_coords(flow, h, w)
    x0, y0 = np.floor(ix), np.floor(iy)
    tx, ty = torch.from_numpy(ix.astype(np.float64) - x0), torch.from_numpy(iy.astype(np.float64) - y0)
    x0, y0 = torch.from_numpy(x0.astype(np.int64)), torch.from_numpy(y0.astype(np.int64))
    wts = bilinear_weights(tx, ty)
    # d weight / d ix, d weight / d iy per corner
    sx = (-(1 - ty), (1 - ty), -ty, ty)
    sy = (-(1 - tx), -tx, (1 - tx), tx)
    cs = []
    for (dy, dx), wt, gx, gy in zip(((0, 0), (0, 1), (1, 0), (1, 1)), wts, sx, sy):
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        cs.append((torch.where(ok, yy * w + xx, torch.zeros_like(yy)), ok.double(), wt, gx, gy))
    return cs, torch.from_numpy(gmx), torch.from_numpy(gmy)


def _rows(x, idx):
    """x (n, h*w, c), idx (n, h, w) -> the rows x[n, idx] as (n, h, w, c)."""
    n, hw, c = x.shape
    return torch.gather(x, 1, idx.reshape(n, -1, 1).expand(n, idx[0].numel(), c)).reshape(idx.shape + (c,))


def warp_bilinear_reference(x, flow):
    """x (n, h, w, c), flow (n, h, w, 2) float32 pixel offsets -> bilinear sample with border padding, float64."""
    n, h, w, c = x.shape
    x = x.double().reshape(n, h * w, c)
    cs, _, _ = _corners(flow.detach().float().numpy(), h, w)
    out = torch.zeros((n, h, w, c), dtype=torch.float64)
    for idx, ok, wt, _, _ in cs:
        out += _rows(x, idx) * (ok * wt)[..., None]
    return out


def warp_bilinear_reference_backward(x, flow, dy, with_scales=False):
    """-> dx (n, h, w, c), dflow (n, h, w, 2) [, {name: sum of |addends| per element}]."""
    n, h, w, c = x.shape
    x, dy = x.double().reshape(n, h * w, c), dy.double()
    cs, gmx, gmy = _corners(flow.detach().float().numpy(), h, w)
    dx, sdx = torch.zeros_like(x), torch.zeros_like(x)
    df, sdf = torch.zeros((n, h, w, 2), dtype=torch.float64), torch.zeros((n, h, w, 2), dtype=torch.float64)
    for idx, ok, wt, gx, gy in cs:
        add = dy * (ok * wt)[..., None]
        ii = idx.reshape(n, -1, 1).expand(n, h * w, c)
        dx.scatter_add_(1, ii, add.reshape(n, h * w, c))
        sdx.scatter_add_(1, ii, add.abs().reshape(n, h * w, c))
        xv = _rows(x, idx) * dy * ok[..., None]
        df[..., 0] += xv.sum(-1) * gx
        df[..., 1] += xv.sum(-1) * gy
        sdf[..., 0] += xv.abs().sum(-1) * gx.abs()
        sdf[..., 1] += xv.abs().sum(-1) * gy.abs()
    df[..., 0] *= gmx
    df[..., 1] *= gmy
    sdf[..., 0] *= gmx
    sdf[..., 1] *= gmy
    dx, sdx = dx.reshape(n, h, w, c), sdx.reshape(n, h, w, c)
    return (dx, df, dict(dx=sdx, dflow=sdf)) if with_scales else (dx, df)


def warp_nearest_reference(loc, flow):
    """loc (n, k2, h, w) planes advected by flow (n, h, w, 2): nearest sample (half to even) with border padding.  Copies, so any dtype."""
    n, k2, h, w = loc.shape
    ix, iy, _, _ = warp_coords(flow.detach().float().numpy(), h, w)
    idx = torch.from_numpy((round_index(iy) * w + round_index(ix)).astype(np.int64))  # (n, h, w)
    return torch.gather(loc.reshape(n, k2, h * w), 2, idx.reshape(n, 1, h * w).expand(n, k2, h * w)).reshape(n, k2, h, w)


# ------------------------------------------------------------------------------------------------------------------ flow smoothing
def flow_smooth_reference(x, r):
    """x (planes, H, W) numpy: reflect-pad right / bottom to a multiple of r, r x r mean, spread over the block, crop.  float64."""
    x = np.asarray(x, dtype=np.float64)
    p, H, W = x.shape
    hf, wf = -(-H // r) * r, -(-W // r) * r
    xp = np.pad(x, ((0, 0), (0, hf - H), (0, wf - W)), mode="reflect")
    m = xp.reshape(p, hf // r, r, wf // r, r).mean(axis=(2, 4))
    return np.repeat(np.repeat(m, r, axis=1), r, axis=2)[:, :H, :W]


def flow_smooth_reference_backward(g, r):
    """The adjoint, step by step backwards: crop -> zero-extend, spread -> block sum, mean -> / r^2, reflect-pad -> fold the padding back."""
    g = np.asarray(g, dtype=np.float64)
    p, H, W = g.shape
    hf, wf = -(-H // r) * r, -(-W // r) * r
    gp = np.zeros((p, hf, wf))
    gp[:, :H, :W] = g
    m = gp.reshape(p, hf // r, r, wf // r, r).sum(axis=(2, 4)) / (r * r)
    d = np.repeat(np.repeat(m, r, axis=1), r, axis=2)
    for k in range(W, wf):
        d[:, :, 2 * (W - 1) - k] += d[:, :, k]
    d = d[:, :, :W]
    for k in range(H, hf):
        d[:, 2 * (H - 1) - k] += d[:, k]
    return d[:, :H]


# ------------------------------------------------------------------------------------------------------------------ trajectory attention
def decay_powers(decay, t):
    """(heads, t): key-frame j of t (0 = the oldest) carries decay^(t - j)."""
    return torch.stack([decay ** (t - j) for j in range(t)], 1)


def rpe_term(rpe):
    """(heads, query position, key position), positions row-major inside the wh x ww window."""
    return rpe


def norm_groups(heads):
    """L2 normalisation runs over ALL channels, before the head split: one group."""
    return 1


def _normalise(x, heads):
    """x (..., c) -> x / max(||x||, eps) and the clamped norm, per norm group."""
    g = norm_groups(heads)
    xs = x.reshape(x.shape[:-1] + (g, x.shape[-1] // g))
    nr = xs.norm(dim=-1, keepdim=True).clamp_min(EPS)
    return (xs / nr).reshape(x.shape), nr


def _normalise_backward(xn, nr, dxn, heads):
    """Gradient through x / max(||x||, eps) [, and the sum of |addends|]: the projection off xn where the norm is its own, 1 / eps where clamped."""
    g = norm_groups(heads)
    shp = xn.shape
    xs, ds = xn.reshape(shp[:-1] + (g, shp[-1] // g)), dxn.reshape(shp[:-1] + (g, shp[-1] // g))
    free = (nr > EPS).double()
    return ((ds - free * xs * (xs * ds).sum(-1, keepdim=True)) / nr).reshape(shp)


def _normalise_backward_scale(xn, nr, adxn, heads):
    g = norm_groups(heads)
    shp = xn.shape
    xs, ds = xn.abs().reshape(shp[:-1] + (g, shp[-1] // g)), adxn.reshape(shp[:-1] + (g, shp[-1] // g))
    free = (nr > EPS).double()
    return ((ds + free * xs * (xs * ds).sum(-1, keepdim=True)) / nr).reshape(shp)


def _windows(z, wh, ww, heads):
    """(n, [t,] h, w, c) -> (n, h/wh, w/ww, heads, [t,] wh*ww, d)"""
    if z.dim() == 4:
        n, h, w, c = z.shape
        z = z.reshape(n, h // wh, wh, w // ww, ww, heads, c // heads).permute(0, 1, 3, 5, 2, 4, 6)
        return z.reshape(n, h // wh, w // ww, heads, wh * ww, c // heads)
    n, t, h, w, c = z.shape
    z = z.reshape(n, t, h // wh, wh, w // ww, ww, heads, c // heads).permute(0, 2, 4, 6, 1, 3, 5, 7)
    return z.reshape(n, h // wh, w // ww, heads, t, wh * ww, c // heads)


def _unwindows(z, wh, ww):
    """the inverse of _windows"""
    if z.dim() == 6:
        n, Y, X, heads, wq, d = z.shape
        return z.reshape(n, Y, X, heads, wh, ww, d).permute(0, 1, 4, 2, 5, 3, 6).reshape(n, Y * wh, X * ww, heads * d)
    n, Y, X, heads, t, wq, d = z.shape
    return z.reshape(n, Y, X, heads, t, wh, ww, d).permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(n, t, Y * wh, X * ww, heads * d)


def _gathered(frames, idx):
    """frames: t tensors (n, h, w, c); idx (n, t, h, w) -> (n, t, h, w, c), zero rows where idx < 0."""
    n, t, h, w = idx.shape
    src = torch.stack([f.double() for f in frames], 1).reshape(n * t, h * w, -1)
    rows = _rows(src, idx.clamp_min(0).reshape(n * t, h, w))
    return (rows * (idx >= 0).double().reshape(n * t, h, w, 1)).reshape(n, t, h, w, -1)


def _ltam_logits(q, keys, vals, loc, rpe, decay, wh, ww, scale):
    n, h, w, c = q.shape
    heads, t = rpe.shape[0], len(keys)
    idx = torch.from_numpy(ltam_gather_index(loc.detach().float().numpy(), h, w))
    qn, qnr = _normalise(q.double(), heads)
    kn, knr = _normalise(_gathered(keys, idx), heads)
    v = _gathered(vals, idx)
    qw, kw, vw = _windows(qn, wh, ww, heads), _windows(kn, wh, ww, heads), _windows(v, wh, ww, heads)
    pw = decay_powers(decay.double().reshape(-1), t)  # (heads, t)
    logits = scale * torch.einsum("nyxhqd,nyxhjkd->nyxhqjk", qw, kw) + pw[:, None, :, None] * rpe_term(rpe.double())[:, :, None, :]
    return dict(idx=idx, qn=qn, qnr=qnr, kn=kn, knr=knr, qw=qw, kw=kw, vw=vw, pw=pw, logits=logits, heads=heads, t=t)


def _per_head(z, wh, ww):
    """(n, Y, X, heads, wq) -> (n, h, w, heads)"""
    n, Y, X, heads, wq = z.shape
    return z.reshape(n, Y, X, heads, wh, ww).permute(0, 1, 4, 2, 5, 3).reshape(n, Y * wh, X * ww, heads)


def _to_windows_per_head(z, wh, ww):
    """(n, h, w, heads) -> (n, Y, X, heads, wq)"""
    n, h, w, heads = z.shape
    return z.reshape(n, h // wh, wh, w // ww, ww, heads).permute(0, 1, 3, 5, 2, 4).reshape(n, h // wh, w // ww, heads, wh * ww)


def ltam_reference(q, keys, vals, loc, rpe, decay, wh, ww, scale):
    """q (n, h, w, c); keys / vals: t tensors of q's shape, oldest key-frame first; loc (n, 2t, h, w) float32; rpe (heads, wh*ww, wh*ww);
    decay (heads).  -> out (n, h, w, c), lse (n, h, w, heads) natural-log logsumexp of every query's t * wh*ww logits.  float64."""
    s = _ltam_logits(q, keys, vals, loc, rpe, decay, wh, ww, scale)
    lg = s["logits"]
    lse = torch.logsumexp(lg.flatten(-2), -1)  # (n, Y, X, heads, wq)
    p = torch.exp(lg - lse[..., None, None])
    out = torch.einsum("nyxhqjk,nyxhjkd->nyxhqd", p, s["vw"])
    return _unwindows(out, wh, ww), _per_head(lse, wh, ww)


def ltam_reference_backward(q, keys, vals, loc, rpe, decay, wh, ww, scale, out_for_delta, dout, lse=None, with_scales=False):
    """-> dq, [dk_j], [dv_j], drpe [, scales].  The probabilities are exp(logit - lse) with the GIVEN lse (the reference's own when None) and
    the softmax Jacobian's delta = <dout, out_for_delta> per (pixel, head): what a backward kernel that is handed out and lse computes."""
    n, h, w, c = q.shape
    s = _ltam_logits(q, keys, vals, loc, rpe, decay, wh, ww, scale)
    heads, t, idx = s["heads"], s["t"], s["idx"]
    if lse is None:
        lse_w = torch.logsumexp(s["logits"].flatten(-2), -1)
    else:
        lse_w = _to_windows_per_head(lse.double(), wh, ww)
    p = torch.exp(s["logits"] - lse_w[..., None, None])  # n y x h q j k
    gw = _windows(dout.double(), wh, ww, heads)  # n y x h q d
    ow = _windows(out_for_delta.double(), wh, ww, heads)
    delta = (gw * ow).sum(-1)  # n y x h q
    dp = torch.einsum("nyxhqd,nyxhjkd->nyxhqjk", gw, s["vw"])
    ds = p * (dp - delta[..., None, None])
    pw = s["pw"]
    drpe_qk = torch.einsum("nyxhqjk,hj->hqk", ds, pw)
    sc_rpe = torch.einsum("nyxhqjk,hj->hqk", ds.abs(), pw.abs())
    if rpe_term(rpe) is not rpe:  # (a wrong variant that transposes the table transposes its gradient back)
        drpe_qk, sc_rpe = rpe_term(drpe_qk), rpe_term(sc_rpe)
    dv_g = torch.einsum("nyxhqjk,nyxhqd->nyxhjkd", p, gw)
    sc_dv_g = torch.einsum("nyxhqjk,nyxhqd->nyxhjkd", p, gw.abs())
    dqn = scale * torch.einsum("nyxhqjk,nyxhjkd->nyxhqd", ds, s["kw"])
    dkn = scale * torch.einsum("nyxhqjk,nyxhqd->nyxhjkd", ds, s["qw"])
    sc_dkn = scale * torch.einsum("nyxhqjk,nyxhqd->nyxhjkd", ds.abs(), s["qw"].abs())
    dq = _normalise_backward(s["qn"], s["qnr"], _unwindows(dqn, wh, ww), heads)
    dk_g = _normalise_backward(s["kn"], s["knr"], _unwindows(dkn, wh, ww), heads)  # (n, t, h, w, c)
    sc_dk_g = _normalise_backward_scale(s["kn"], s["knr"], _unwindows(sc_dkn, wh, ww), heads)
    dv_g, sc_dv_g = _unwindows(dv_g, wh, ww), _unwindows(sc_dv_g, wh, ww)

    def scatter(rows):  # (n, t, h, w, c) rows back to their gather sources
        ok = (idx >= 0).double()[..., None]
        ii = idx.clamp_min(0).reshape(n, t, h * w, 1).expand(n, t, h * w, c)
        acc = torch.zeros((n, t, h * w, c), dtype=torch.float64)
        acc.scatter_add_(2, ii, (rows * ok).reshape(n, t, h * w, c))
        return [acc[:, j].reshape(n, h, w, c) for j in range(t)]

    dk, dv = scatter(dk_g), scatter(dv_g)
    if not with_scales:
        return dq, dk, dv, drpe_qk
    return dq, dk, dv, drpe_qk, dict(dk=scatter(sc_dk_g), dv=scatter(sc_dv_g), drpe=sc_rpe)
