"""The mutual match (K48) restated in torch, for the tests: fp64 logits L = inv_t * q^T k, row and column argmax with the lowest index
among equal values, logsumexp, the round trip of the two index maps and Chebyshev distances on rectangular grids.  Plain tensor code on
whatever device its inputs live on; tested on hand-made cases in tests/test_match_mutual_cpu.py."""
import torch


def logits(q, k, inv_t):
    """q [B,C,Nq], k [B,C,Nk] -> L [B,Nq,Nk] fp64"""
    return inv_t * torch.einsum("bci,bcj->bij", q.double(), k.double())


def argmax_lowest(L, dim):
    """(max, index) along `dim`; among equal maxima the LOWEST index (torch.max does not promise one)"""
    m = L.max(dim=dim, keepdim=True).values
    n = L.shape[dim]
    shape = [1] * L.dim()
    shape[dim] = n
    ar = torch.arange(n, device=L.device).view(shape).expand_as(L)
    idx = torch.where(L == m, ar, torch.full_like(ar, n)).min(dim=dim).values
    return m.squeeze(dim), idx


def readout(L):
    """L [B,Nq,Nk] -> ((row_idx [B,Nq], row_max, row_lse), (col_idx [B,Nk], col_max, col_lse))"""
    rm, ri = argmax_lowest(L, 2)
    cm, ci = argmax_lowest(L, 1)
    return (ri, rm, torch.logsumexp(L, dim=2)), (ci, cm, torch.logsumexp(L, dim=1))


def chebyshev(a, b, w):
    """cells between the flat positions a and b (y * w + x) of a grid of width w: max(|dx|, |dy|)"""
    ax, ay = a % w, torch.div(a, w, rounding_mode="floor")
    bx, by = b % w, torch.div(b, w, rounding_mode="floor")
    return torch.maximum((ax - bx).abs(), (ay - by).abs())


def round_trip(row_idx, col_idx, qgrid, kgrid):
    """row_idx [B,hq*wq] (positions of the kgrid), col_idx [B,hk*wk] (positions of the qgrid), any integers (clamped into range) ->
    (q_back, q_dist, k_back, k_dist) int64: q_back = col_idx[row_idx], q_dist its Chebyshev distance from the position itself on the
    qgrid; k_back = row_idx[col_idx], k_dist on the kgrid"""
    (hq, wq), (hk, wk) = qgrid, kgrid
    Nq, Nk = hq * wq, hk * wk
    r = row_idx.long().clamp(0, Nk - 1)
    c = col_idx.long().clamp(0, Nq - 1)
    q_back = c.gather(1, r)
    k_back = r.gather(1, c)
    iq = torch.arange(Nq, device=r.device).unsqueeze(0).expand_as(q_back)
    ik = torch.arange(Nk, device=r.device).unsqueeze(0).expand_as(k_back)
    return q_back, chebyshev(q_back, iq, wq), k_back, chebyshev(k_back, ik, wk)
