"""A numpy fp64 restatement of K44 for the tests (cocosnet_amd/csrc/plane_pair.hip and gather_patches_subcell_kernel of
gather_warp.hip): which keys are in a query's window, the window softmax and its expected offset, and the bilinear gather at the
sub-cell position.

    window(j, r)    the keys (yk + dy, xk + dx), |dy|, |dx| <= r, inside the hk x wk grid, around j clamped into [0, hk wk);
                    dy ascending outside, dx ascending inside; a position outside the grid is left out
    refine          s = inv_t <q, k> over the window;  m = max s;  lse_win = m + log sum exp(s - m);  p = exp(s - lse_win);
                    off = (sum p dx, sum p dy)
    gather          pixel (Y, X) of cell (Y // down, X // down):  sx = (xk + off_x) down + X % down clamped into [0, Wr - 1],
                    x0 = floor(sx), fx = sx - x0, x1 = min(x0 + 1, Wr - 1), y likewise;  top = v00 + fx (v01 - v00),
                    bottom = v10 + fx (v11 - v10), out = top + fy (bottom - top)
"""
import numpy as np


def window(j, kgrid, r):
    """[(key, dx, dy)] of the window around key j (any integer: clamped), in visiting order"""
    hk, wk = kgrid
    j = min(max(int(j), 0), hk * wk - 1)
    yk, xk = divmod(j, wk)
    return [((yk + dy) * wk + xk + dx, dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1)
            if 0 <= yk + dy < hk and 0 <= xk + dx < wk]


def softargmax(s, dx, dy):
    """(off_x, off_y, lse_win) of window scores s with offsets dx, dy (1-d arrays in visiting order)"""
    s = np.asarray(s, dtype=np.float64)
    m = s.max()
    lse = m + np.log(np.exp(s - m).sum())
    p = np.exp(s - lse)
    r = max(np.abs(dx).max(), np.abs(dy).max())      # (the kernel limits by its radius; a rounded sum passes neither)
    return float(np.clip((p * dx).sum(), -r, r)), float(np.clip((p * dy).sum(), -r, r)), float(lse)


def refine(qv, kv, idx, kgrid, r, inv_t):
    """(off [B,Nq,2], lse_win [B,Nq]) fp64 from the operand-plane values qv [B,Nq,256], kv [B,Nk,256] (patchmatch_case.plane_values)
    and the centre table idx [B,Nq] (any integers)"""
    B, Nq, _ = qv.shape
    off, lse = np.zeros((B, Nq, 2)), np.zeros((B, Nq))
    for b in range(B):
        for i in range(Nq):
            keys, dx, dy = (np.array(v) for v in zip(*window(idx[b, i], kgrid, r)))
            off[b, i, 0], off[b, i, 1], lse[b, i] = softargmax(inv_t * (kv[b, keys] @ qv[b, i]), dx, dy)
    return off, lse


def gather_subcell(img, idx, off, grid, kgrid, down):
    """out [B,C,fh down,fw down] fp64: img [Be,C,hk down,wk down] (Be = B or 1), idx [B,fh fw] (any integers), off [B,fh fw,2]"""
    (fh, fw), (hk, wk) = grid, kgrid
    img, off = np.asarray(img, dtype=np.float64), np.asarray(off, dtype=np.float64)
    B = off.shape[0]
    Hr, Wr = hk * down, wk * down
    j = np.clip(np.asarray(idx, dtype=np.int64).reshape(B, fh, fw), 0, hk * wk - 1)
    off = off.reshape(B, fh, fw, 2)
    up = lambda t: np.repeat(np.repeat(t, down, axis=1), down, axis=2)                    # cell -> its down x down pixels
    ry, rx = np.arange(fh * down).reshape(1, -1, 1) % down, np.arange(fw * down).reshape(1, 1, -1) % down
    sx = np.clip((up(j % wk) + up(off[..., 0])) * down + rx, 0, Wr - 1)
    sy = np.clip((up(j // wk) + up(off[..., 1])) * down + ry, 0, Hr - 1)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = (sx - x0)[:, None], (sy - y0)[:, None]
    x1, y1 = np.minimum(x0 + 1, Wr - 1), np.minimum(y0 + 1, Hr - 1)
    out = np.zeros((B, img.shape[1], fh * down, fw * down))
    for b in range(B):
        src = img[b if img.shape[0] == B else 0]
        v00, v01, v10, v11 = src[:, y0[b], x0[b]], src[:, y0[b], x1[b]], src[:, y1[b], x0[b]], src[:, y1[b], x1[b]]
        top, bottom = v00 + fx[b] * (v01 - v00), v10 + fx[b] * (v11 - v10)
        out[b] = top + fy[b] * (bottom - top)
    return out
