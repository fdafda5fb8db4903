"""An fp64 numpy restatement of K46's three backward formulas for the tests (cocosnet_amd/csrc/plane_pair.hip and
gather_patches_subcell_bwd_off_kernel of gather_warp.hip), built on tests/match_refine_case.py's forward restatement, and the same
formulas in torch ops of any dtype and device: the fp32 arm the GPU tests measure the kernels' error against, and the fp64 function
torch.autograd differentiates to check the restatement itself.

With W = (2 r + 1)^2 slots, slot e = (dy + r)(2 r + 1) + (dx + r), p the window softmax and o = (sum p dx, sum p dy) NOT limited:
    ds[i, e]  = p_e ((dx_e - o_x) doff_x + (dy_e - o_y) doff_y), 0 for a slot outside the key grid
    dq[i]     = inv_t sum_e ds[i, e] k[j_e]
    dk[j]     = inv_t sum over the pairs (i, e) with j_e = j of ds[i, e] q[i]
    doff[cell] = sum over the cell's C down^2 pixels of dout * (d out / d off_x, d out / d off_y), where with t = off down,
                 p = base + floor(t), f = t - floor(t) per axis:  d out / d off_x = down ((1 - fy)(v01 - v00) + fy (v11 - v10)),
                 d out / d off_y = down (bottom - top), each 0 where that axis is clamped (p < 0 or p >= side - 1)
"""
import numpy as np
import torch

import match_refine_case as mc


def slot(dx, dy, r):
    return (dy + r) * (2 * r + 1) + dx + r


# ---------------------------------------------------------------------------------------------------------------- numpy, fp64
def refine_bwd(qv, kv, idx, kgrid, r, inv_t, doff):
    """(ds [B,Nq,W], dq [B,Nq,256], dk [B,Nk,256]) fp64 from the operand-plane values qv [B,Nq,256], kv [B,Nk,256], the centre table
    idx [B,Nq] (any integers) and the incoming gradient doff [B,Nq,2] of the offset"""
    qv, kv, doff = (np.asarray(t, dtype=np.float64) for t in (qv, kv, doff))
    B, Nq, _ = qv.shape
    ds, dq, dk = np.zeros((B, Nq, (2 * r + 1) ** 2)), np.zeros_like(qv), np.zeros_like(kv)
    for b in range(B):
        for i in range(Nq):
            keys, dx, dy = (np.array(v) for v in zip(*mc.window(idx[b, i], kgrid, r)))
            s = inv_t * (kv[b, keys] @ qv[b, i])
            p = np.exp(s - s.max())
            p /= p.sum()
            ox, oy = (p * dx).sum(), (p * dy).sum()
            d = p * ((dx - ox) * doff[b, i, 0] + (dy - oy) * doff[b, i, 1])
            ds[b, i, slot(dx, dy, r)] = d
            dq[b, i] = inv_t * (d @ kv[b, keys])
            np.add.at(dk[b], keys, inv_t * d[:, None] * qv[b, i][None, :])
    return ds, dq, dk


def _axis(off, base, down, side):
    """(p0, f, clamped) of one axis: the integer / fraction decomposition of the sample position (off, base broadcastable)"""
    t = off * down
    ti = np.floor(t)
    p = base + ti.astype(np.int64)
    clamped = (p < 0) | (p >= side - 1)
    return np.clip(p, 0, side - 1), np.where(clamped, 0.0, t - ti), clamped


def gather_bwd_off(img, idx, off, dout, grid, kgrid, down):
    """doff [B,fh fw,2] fp64: img [Be,C,hk down,wk down] (Be = B or 1), idx [B,fh fw] (any integers), off [B,fh fw,2], dout
    [B,C,fh down,fw down]"""
    (fh, fw), (hk, wk) = grid, kgrid
    img, off, dout = (np.asarray(t, dtype=np.float64) for t in (img, off, dout))
    B, C = off.shape[0], img.shape[1]
    Hr, Wr = hk * down, wk * down
    j = np.clip(np.asarray(idx, dtype=np.int64).reshape(B, fh, fw), 0, hk * wk - 1)
    off = off.reshape(B, fh, fw, 2)
    up = lambda t: np.repeat(np.repeat(t, down, axis=1), down, axis=2)                    # cell -> its down x down pixels
    ry, rx = np.arange(fh * down).reshape(1, -1, 1) % down, np.arange(fw * down).reshape(1, 1, -1) % down
    x0, fx, xc = _axis(up(off[..., 0]), up(j % wk) * down + rx, down, Wr)
    y0, fy, yc = _axis(up(off[..., 1]), up(j // wk) * down + ry, down, Hr)
    x1, y1 = np.minimum(x0 + 1, Wr - 1), np.minimum(y0 + 1, Hr - 1)
    doff = np.zeros((B, fh, fw, 2))
    for b in range(B):
        src = img[b if img.shape[0] == B else 0]
        v00, v01, v10, v11 = src[:, y0[b], x0[b]], src[:, y0[b], x1[b]], src[:, y1[b], x0[b]], src[:, y1[b], x1[b]]
        top, bottom = v00 + fx[b] * (v01 - v00), v10 + fx[b] * (v11 - v10)
        sx = np.where(xc[b], 0.0, down * ((1 - fy[b]) * (v01 - v00) + fy[b] * (v11 - v10)))
        sy = np.where(yc[b], 0.0, down * (bottom - top))
        cells = lambda t: (dout[b] * t).reshape(C, fh, down, fw, down).sum(axis=(0, 2, 4))
        doff[b, ..., 0], doff[b, ..., 1] = cells(sx), cells(sy)
    return doff.reshape(B, fh * fw, 2)


# ---------------------------------------------------------------------------------------------------------------- torch, any dtype
def t_window(idx, kgrid, r):
    """(keys [B,Nq,W] int64 — the centre where a slot lies outside the grid —, inside [B,Nq,W] bool, dx [W], dy [W]) of an integer
    centre table idx [B,Nq] on its device"""
    hk, wk = kgrid
    c = idx.long().clamp(0, hk * wk - 1)
    d = torch.arange(-r, r + 1, device=idx.device)
    dy, dx = d.repeat_interleave(2 * r + 1), d.repeat(2 * r + 1)
    ky, kx = torch.div(c, wk, rounding_mode="floor").unsqueeze(-1) + dy, (c % wk).unsqueeze(-1) + dx
    inside = (ky >= 0) & (ky < hk) & (kx >= 0) & (kx < wk)
    return torch.where(inside, ky * wk + kx, c.unsqueeze(-1)), inside, dx, dy


def _t_softmax(qv, kv, idx, kgrid, r, inv_t):
    keys, inside, dx, dy = t_window(idx, kgrid, r)
    B, Nq, W = keys.shape
    kk = torch.stack([kv[b][keys[b].reshape(-1)].reshape(Nq, W, -1) for b in range(B)])      # [B,Nq,W,256]
    s = (inv_t * torch.einsum("bic,biwc->biw", qv, kk)).masked_fill(~inside, float("-inf"))
    p = torch.softmax(s, dim=-1)
    dx, dy = dx.to(qv.dtype), dy.to(qv.dtype)
    return keys, kk, p, dx, dy, torch.stack(((p * dx).sum(-1), (p * dy).sum(-1)), dim=-1)


def t_refine_off(qv, kv, idx, kgrid, r, inv_t):
    """off [B,Nq,2] (not limited) from qv [B,Nq,256], kv [B,Nk,256] in their dtype: differentiable torch ops"""
    return _t_softmax(qv, kv, idx, kgrid, r, inv_t)[-1]


def t_refine_bwd(qv, kv, idx, kgrid, r, inv_t, doff):
    """refine_bwd's three formulas in the dtype and on the device of qv (the fp32 arm of the GPU tests)"""
    keys, kk, p, dx, dy, o = _t_softmax(qv, kv, idx, kgrid, r, inv_t)
    ds = p * ((dx - o[..., :1]) * doff[..., :1] + (dy - o[..., 1:]) * doff[..., 1:])
    dq = inv_t * torch.einsum("biw,biwc->bic", ds, kk)
    dk = torch.zeros_like(kv)
    for b in range(kv.shape[0]):
        dk[b].index_add_(0, keys[b].reshape(-1), (inv_t * ds[b].unsqueeze(-1) * qv[b].unsqueeze(1)).reshape(-1, qv.shape[-1]))
    return ds, dq, dk


def _t_axis(off, base, down, side):
    t = off * down
    ti = torch.floor(t.detach())
    p = base + ti.long()
    clamped = (p < 0) | (p >= side - 1)
    return p.clamp(0, side - 1), torch.where(clamped, torch.zeros_like(t), t - ti), clamped


def _t_samples(img, idx, off, grid, kgrid, down):
    (fh, fw), (hk, wk) = grid, kgrid
    B = off.shape[0]
    Hr, Wr = hk * down, wk * down
    j = idx.long().reshape(B, fh, fw).clamp(0, hk * wk - 1)
    off = off.reshape(B, fh, fw, 2)
    up = lambda t: t.repeat_interleave(down, dim=1).repeat_interleave(down, dim=2)
    ry = (torch.arange(fh * down, device=off.device) % down).view(1, -1, 1)
    rx = (torch.arange(fw * down, device=off.device) % down).view(1, 1, -1)
    x0, fx, xc = _t_axis(up(off[..., 0]), up(j % wk) * down + rx, down, Wr)
    y0, fy, yc = _t_axis(up(off[..., 1]), up(torch.div(j, wk, rounding_mode="floor")) * down + ry, down, Hr)
    x1, y1 = (x0 + 1).clamp(max=Wr - 1), (y0 + 1).clamp(max=Hr - 1)
    pick = lambda yy, xx: torch.stack([img[b if img.shape[0] == B else 0][:, yy[b], xx[b]] for b in range(B)])
    return pick(y0, x0), pick(y0, x1), pick(y1, x0), pick(y1, x1), fx.unsqueeze(1), fy.unsqueeze(1), xc.unsqueeze(1), yc.unsqueeze(1)


def t_gather_subcell(img, idx, off, grid, kgrid, down):
    """out [B,C,fh down,fw down] in off's dtype: differentiable in off (the floor and the clamp are constants, as in the kernel)"""
    v00, v01, v10, v11, fx, fy, _, _ = _t_samples(img, idx, off, grid, kgrid, down)
    top, bottom = v00 + fx * (v01 - v00), v10 + fx * (v11 - v10)
    return top + fy * (bottom - top)


def t_gather_bwd_off(img, idx, off, dout, grid, kgrid, down):
    """gather_bwd_off's formula in the dtype and on the device of off (the fp32 arm of the GPU tests)"""
    (fh, fw), B, C = grid, off.shape[0], img.shape[1]
    v00, v01, v10, v11, fx, fy, xc, yc = _t_samples(img, idx, off.detach(), grid, kgrid, down)
    top, bottom = v00 + fx * (v01 - v00), v10 + fx * (v11 - v10)
    zero = torch.zeros_like(top)
    sx = torch.where(xc, zero, down * ((1 - fy) * (v01 - v00) + fy * (v11 - v10)))
    sy = torch.where(yc, zero, down * (bottom - top))
    cells = lambda t: (dout * t).reshape(B, C, fh, down, fw, down).sum(dim=(1, 3, 5)).reshape(B, fh * fw)
    return torch.stack((cells(sx), cells(sy)), dim=-1)


def away_from_kinks(off, down, margin=1e-3):
    """offsets [.., 2] whose off * down lies within `margin` of an integer are moved to that integer + margin * 2 (no case is left
    out: the bilinear sample has a kink there, and the two sides' slopes differ)"""
    t = off.double() * down
    near = (t - t.round()).abs() < margin
    return torch.where(near, (t.round() + 2 * margin) / down, off.double()).to(off.dtype)
