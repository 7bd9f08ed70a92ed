"""Reference of the OPERATION behind the max-mode kernels of csrc/ltam.hip (hard trajectory attention, LTAM_multi_head.forward_max of the
reference, en_field=False, if_ia=False), spelled the slow obvious way in float64.  Plain module: numpy and torch only (the gather positions come
from tests/traj_ref.py, which holds that convention for the window mode too).

Per pixel p and key-frame j: s_j the nearest-neighbour source (float32 positions, zeros padding), K_j = keys[j][s_j] or the zero row;
qn = q / max(||q||, eps), kn_j = K_j / max(||K_j||, eps) over ALL c channels; per head g: score[g][j] = <qn_g, kn_{j,g}>,
idx[g] = the FIRST j of maximal score, out_g = score[g][idx[g]] * vals[idx[g]][s]_g.

The backward takes idx as a constant.  It also returns, on request, the sum of the absolute values of the addends summed into every element of
dk and dv (the scale a kernel that adds the same terms in fp32 in another order is off by a small multiple of 2^-24 of).  An element of dv is
sc * dout_d with sc = sum_d' qn_d' kn_d' a D-term dot product, i.e. the sum of the D addends qn_d' kn_d' dout_d: its scale is
(sum_d' |qn_d' kn_d'|) |dout_d|, not |sc dout_d| -- where the score nearly cancels, an fp32 dot product is off by 2^-24 of the former, whatever the
latter.  Likewise gs = sum_d dout_d V_d inside a dk row: the scale of (dkn - kn <kn, dkn>) / ||K|| uses sum |dout_d V_d| for |gs| and
(sum |dout_d V_d|)(sum |qn_d kn_d|) for |<kn, dkn>| = |gs sc|.  (The standard bound of a floating-point dot product, gamma_D sum |x_i y_i|.)"""
import torch

from tests import traj_ref as TR

EPS = 1e-12
HEADS = 4


def _gather(frames, sidx):
    """frames: t tensors (n,h,w,c); sidx (n,t,h,w) source pixel or -1 -> (n,t,h,w,c) float64, zero rows without a source."""
    n, t, h, w = sidx.shape
    out = torch.zeros((n, t, h, w, frames[0].shape[-1]), dtype=torch.float64)
    for j in range(t):
        src = frames[j].double().reshape(n, h * w, -1)
        for b in range(n):
            rows = src[b][sidx[b, j].clamp_min(0).reshape(-1)].reshape(h, w, -1)
            out[b, j] = rows * (sidx[b, j] >= 0).double()[..., None]
    return out


def _normalise(x):
    nr = x.norm(dim=-1, keepdim=True).clamp_min(EPS)
    return x / nr, nr


def first_maximum(table):
    """table (..., t, heads) -> (...,heads) the smallest j attaining the maximum over t."""
    t = table.shape[-2]
    mx = table.max(dim=-2, keepdim=True).values
    js = torch.arange(t).reshape((1,) * (table.dim() - 2) + (t, 1)).expand_as(table)
    return torch.where(table == mx, js, torch.full_like(js, t)).min(dim=-2).values


def _select(rows, idx):
    """rows (n,t,h,w,X); idx (n,h,w,heads) -> (n,h,w,heads,X): key-frame idx[g]'s row for every head."""
    n, t, h, w, X = rows.shape
    ii = idx.long().permute(0, 3, 1, 2)[..., None].expand(n, idx.shape[-1], h, w, X)  # n g h w X
    return torch.gather(rows, 1, ii).permute(0, 2, 3, 1, 4)


def forward(q, keys, vals, loc, heads=HEADS, idx=None):
    """-> out (n,h,w,c), idx (n,h,w,heads) int64, score (n,h,w,heads), table (n,h,w,t,heads).  idx= overrides the argmax."""
    n, h, w, c = q.shape
    t, D = len(keys), c // heads
    sidx = torch.from_numpy(TR.ltam_gather_index(loc.detach().float().numpy(), h, w))
    qn, _ = _normalise(q.double())
    kn, _ = _normalise(_gather(keys, sidx))
    v = _gather(vals, sidx)
    table = (qn.reshape(n, 1, h, w, heads, D) * kn.reshape(n, t, h, w, heads, D)).sum(-1).permute(0, 2, 3, 1, 4)
    if idx is None:
        idx = first_maximum(table)
    idx = idx.long()
    score = torch.gather(table, 3, idx[:, :, :, None, :]).squeeze(3)
    vsel = _select(v, idx).reshape(n, h, w, heads, heads, D)  # [.., g, g', D]: head g's key-frame, slice g'
    vown = torch.stack([vsel[:, :, :, g, g] for g in range(heads)], 3)
    out = (score[..., None] * vown).reshape(n, h, w, c)
    return out, idx, score, table


def backward(q, keys, vals, loc, idx, dout, heads=HEADS, with_scales=False):
    """-> dq, [dk_j], [dv_j] [, dict(dk=[...], dv=[...]) sums of |addends|].  idx is the selection, a constant."""
    n, h, w, c = q.shape
    t, D = len(keys), c // heads
    idx = idx.long()
    sidx = torch.from_numpy(TR.ltam_gather_index(loc.detach().float().numpy(), h, w))
    qn, qnr = _normalise(q.double())
    kn, knr = _normalise(_gather(keys, sidx))
    v = _gather(vals, sidx)
    g_out = dout.double().reshape(n, h, w, heads, D)
    qh = qn.reshape(n, h, w, heads, D)
    kn_sel = _select(kn, idx)        # n h w g c: the full normalised key row of head g's key-frame
    knr_sel = _select(knr, idx)      # n h w g 1
    v_sel = _select(v, idx).reshape(n, h, w, heads, heads, D)
    s_sel = torch.gather(sidx.permute(0, 2, 3, 1), 3, idx)  # n h w g: the source pixel of head g's key-frame

    dk = torch.zeros((n, t, h * w, c), dtype=torch.float64)
    dv = torch.zeros_like(dk)
    sdk, sdv = torch.zeros_like(dk), torch.zeros_like(dk)
    dqn = torch.zeros((n, h, w, heads, D), dtype=torch.float64)
    bb = torch.arange(n).reshape(n, 1, 1).expand(n, h, w)
    for g in range(heads):
        kg = kn_sel[:, :, :, g]                                   # n h w c
        sc = (qh[:, :, :, g] * kg.reshape(n, h, w, heads, D)[:, :, :, g]).sum(-1)
        gs = (g_out[:, :, :, g] * v_sel[:, :, :, g, g]).sum(-1)
        dqn[:, :, :, g] = gs[..., None] * kg.reshape(n, h, w, heads, D)[:, :, :, g]
        dkn = torch.zeros((n, h, w, heads, D), dtype=torch.float64)
        dkn[:, :, :, g] = gs[..., None] * qh[:, :, :, g]
        dkn = dkn.reshape(n, h, w, c)
        nr = knr_sel[:, :, :, g]
        free = (nr > EPS).double()
        row = (dkn - free * kg * (kg * dkn).sum(-1, keepdim=True)) / nr          # dense over all c channels
        # the addends, down to the scalar products the operation sums: sc = sum_d qn_d kn_d and gs = sum_d dout_d V_d are D-term dot products
        asc = (qh[:, :, :, g] * kg.reshape(n, h, w, heads, D)[:, :, :, g]).abs().sum(-1)
        ags = (g_out[:, :, :, g] * v_sel[:, :, :, g, g]).abs().sum(-1)
        adkn = torch.zeros((n, h, w, heads, D), dtype=torch.float64)
        adkn[:, :, :, g] = ags[..., None] * qh[:, :, :, g].abs()
        srow = (adkn.reshape(n, h, w, c) + free * kg.abs() * (ags * asc)[..., None]) / nr
        vrow = torch.zeros((n, h, w, heads, D), dtype=torch.float64)
        vrow[:, :, :, g] = sc[..., None] * g_out[:, :, :, g]
        vrow = vrow.reshape(n, h, w, c)
        ok = s_sel[:, :, :, g] >= 0
        where = (bb[ok], idx[:, :, :, g][ok], s_sel[:, :, :, g][ok])
        dk.index_put_(where, row[ok], accumulate=True)
        sdk.index_put_(where, srow[ok], accumulate=True)
        dv.index_put_(where, vrow[ok], accumulate=True)
        svrow = torch.zeros((n, h, w, heads, D), dtype=torch.float64)
        svrow[:, :, :, g] = asc[..., None] * g_out[:, :, :, g].abs()
        sdv.index_put_(where, svrow.reshape(n, h, w, c)[ok], accumulate=True)
    dqn = dqn.reshape(n, h, w, c)
    free = (qnr > EPS).double()
    dq = (dqn - free * qn * (qn * dqn).sum(-1, keepdim=True)) / qnr

    def frames(a):
        return [a[:, j].reshape(n, h, w, c) for j in range(t)]

    if not with_scales:
        return dq, frames(dk), frames(dv)
    return dq, frames(dk), frames(dv), dict(dk=frames(sdk), dv=frames(sdv))


def torch_forward(q, keys, vals, loc, heads=HEADS):
    """The same forward out of differentiable torch operations (in the inputs' dtype, autograd through it): what backward() is pinned against.
    F.normalize's clamp and torch.max's first-maximum rule are the reference's own."""
    import torch.nn.functional as F
    n, h, w, c = q.shape
    t, D = len(keys), c // heads
    sidx = torch.from_numpy(TR.ltam_gather_index(loc.detach().float().numpy(), h, w))  # n t h w
    ok = (sidx >= 0).to(q.dtype)[..., None]
    flat = sidx.clamp_min(0).reshape(n, t, h * w, 1).expand(n, t, h * w, c)
    K = torch.gather(torch.stack(keys, 1).reshape(n, t, h * w, c), 2, flat).reshape(n, t, h, w, c) * ok
    V = torch.gather(torch.stack(vals, 1).reshape(n, t, h * w, c), 2, flat).reshape(n, t, h, w, c) * ok
    qn = F.normalize(q, dim=-1).reshape(n, 1, h, w, heads, D)
    kn = F.normalize(K, dim=-1).reshape(n, t, h, w, heads, D)
    table = (qn * kn).sum(-1)  # n t h w g
    sc, idx = torch.max(table, dim=1)
    vsel = torch.gather(V.reshape(n, t, h, w, heads, D), 1, idx[:, None, :, :, :, None].expand(n, 1, h, w, heads, D)).squeeze(1)
    return (sc[..., None] * vsel).reshape(n, h, w, c), idx
