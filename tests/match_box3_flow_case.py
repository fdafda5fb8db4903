"""The arbiter of K52 (ops.box3_soft_match_offset) and the data its tests share.  The arbiter is the literal restatement:
F.unfold(kernel_size=3, padding=1) of theta and phi, centre over the 2304 entries, divide by (norm + ops.NORM_EPS), dot — the
match_kernel-3 logit — then K44's window rules (membership on 2-D coordinates, dy ascending outside, dx ascending inside, a key outside
the grid left out), the soft-argmax and the limit to [-r, r].  It is written in torch ops of any dtype and device, so it is the fp64
reference that autograd differentiates and, run in fp32 on the device, the arm the kernels' error is measured against.  It shares no
code with the kernels' tap formulation: the unfolded vectors come from tests/box3_sparse_case.py, the window from
tests/match_flow_case.py (which restates tests/match_refine_case.py's `window` in torch ops).

`arbiter` takes theta and phi alone: its gradients are TOTAL derivatives.  `arbiter_stats` takes the statistics (mu, a), (nu, b) as
arguments of their own, as the op does — R is still the product of the raw unfolded vectors — so each of the op's six gradients has a
reference; with the statistics of box3_sparse_case.stats the two agree (tests/test_match_box3_flow_cpu.py)."""
import torch
import torch.nn.functional as F

import box3_sparse_case as bc
import match_flow_case as fc

features = bc.features


def _soft_argmax(z, inside, dx, dy, r):
    """(off [B,Nq,2], lse_win [B,Nq], p [B,Nq,W]) of window logits z [B,Nq,W]; the limit passes the gradient through unchanged"""
    z = z.masked_fill(~inside, float("-inf"))
    lse = torch.logsumexp(z, dim=-1)
    p = torch.exp(z - lse.unsqueeze(-1))
    dx, dy = dx.to(z.dtype), dy.to(z.dtype)
    off = torch.stack(((p * dx).sum(-1), (p * dy).sum(-1)), dim=-1)
    return off + (off.clamp(-r, r) - off).detach(), lse, p


def arbiter(theta, phi, idx, r, inv_rt, parts=False):
    """theta [B,C,fh,fw], phi [B,C,gh,gw] in one dtype, idx [B,fh*fw] any integers -> (off [B,Nq,2], lse_win [B,Nq])
    (`parts`: also p [B,Nq,W] and inside [B,Nq,W])"""
    keys, inside, dx, dy = fc.t_window(idx, tuple(phi.shape[2:]), r)
    z = inv_rt * torch.einsum("bci,biwc->biw", bc.unit_unfolded(theta), bc.gather(bc.unit_unfolded(phi), keys))
    off, lse, p = _soft_argmax(z, inside, dx, dy, r)
    return (off, lse, p, inside) if parts else (off, lse)


def arbiter_stats(theta, phi, mu, a, nu, b, idx, r, inv_rt):
    """the same with the statistics as arguments: z = inv_rt a_p b_q (<unfold(theta)[:,p], unfold(phi)[:,q]> - 9 C mu_p nu_q)"""
    keys, inside, dx, dy = fc.t_window(idx, tuple(phi.shape[2:]), r)
    uq, uk = F.unfold(theta, kernel_size=3, padding=1), F.unfold(phi, kernel_size=3, padding=1)
    R = torch.einsum("bci,biwc->biw", uq, bc.gather(uk, keys))
    pick = lambda t: torch.stack([t[n][keys[n]] for n in range(t.shape[0])])      # [B,Nk] -> [B,Nq,W]
    c = R - uq.shape[1] * mu.unsqueeze(-1) * pick(nu)
    off, lse, _ = _soft_argmax(inv_rt * a.unsqueeze(-1) * pick(b) * c, inside, dx, dy, r)
    return off, lse


def centre_table(B, grid, kgrid, seed):
    """idx [B,Nq] int64.  Batch 0: the four corners, the four edges, the interior and out-of-range entries on both sides (clamped by the
    op onto the first and the last key) in front of random centres.  The last batch: ONE centre all its queries share, key 0 — the
    longest serial list, and every key further than the window from the corner lies in nobody's window."""
    (fh, fw), (gh, gw) = grid, kgrid
    Nq, Nk = fh * fw, gh * gw
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, Nk, (B, Nq), generator=g)
    fixed = [-1, Nk, 0, Nk - 1, gw - 1, Nk - gw, 10 ** 9, -(2 ** 31),      # out of range (clamped) and the corners: in the smallest table too
             gw // 2, Nk - 1 - gw // 2, gw * (gh // 2), gw * (gh // 2) + gw - 1, (gh // 2) * gw + gw // 2][:Nq]
    idx[0, :len(fixed)] = torch.tensor(fixed)
    idx[B - 1] = 0
    return idx


def touched(idx, kgrid, r, reach=0):
    """[B,Nk] bool: the keys inside some query's window, widened by `reach` cells (1: the keys a tap of a window key reaches)"""
    gh, gw = kgrid
    keys, inside, _, _ = fc.t_window(idx, kgrid, r + reach)
    out = torch.zeros(idx.shape[0], gh * gw, dtype=torch.bool)
    for n in range(idx.shape[0]):
        out[n, keys[n][inside[n]]] = True
    return out
