"""K50 arbiter: a torch fp64 restatement of the biased top-k readout, the log-domain Sinkhorn iteration over the correlation, the
masses of the transport plan and the k-sparse warp with detached potentials.  Device-agnostic (the CPU tests run it on the CPU, the GPU
tests on the inputs' device); nothing here calls the library.

Notation: L [B,Nq,Nk] = inv_t <qn_i, kn_j> (fp64), mu = 1 / Nq, nu = 1 / Nk, g^0 = 0 and for t = 1..iters
    f_i = tau (log mu - log sum_j exp(L_ij + g_j)),    g_j = tau (log nu - log sum_i exp(L_ij + f_i))
P_ij = exp(L_ij + f_i + g_j) is the plan, softmax_j(L_ij + g_j) its row-conditional form."""
import math

import torch

NEG_INF = float("-inf")


def logits(qn, kn, inv_t):
    """qn [B,C,Nq], kn [B or 1,C,Nk] -> L [B,Nq,Nk] fp64"""
    return torch.matmul(qn.double().transpose(1, 2), kn.double()) * inv_t


def logsumexp(z, dim=-1):
    """log sum exp along `dim`; a slice of -inf alone gives -inf (no NaN)"""
    m = z.amax(dim=dim, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    return (torch.log(torch.exp(z - m).sum(dim=dim)) + m.squeeze(dim))


def biased_topk(L, bias, k):
    """z = L + bias[:, None, :] -> (idx int64 [B,Nq,k], val [B,Nq,k], lse [B,Nq], z): z descending, the LOWER index first among equal
    values (a stable descending sort keeps equal elements in their original order)"""
    z = L + bias.double().unsqueeze(1)
    val, idx = torch.sort(z, dim=-1, descending=True, stable=True)
    return idx[..., :k], val[..., :k], logsumexp(z), z


def decided(z, k, e):
    """bool [B,Nq,k]: the ranks of the top-k of z whose value lies more than 2 e away from both neighbours in the sorted row — two
    values each known to within e cannot trade places across such a gap, so the index of that rank is determined by the values"""
    s = torch.sort(z, dim=-1, descending=True, stable=True).values[..., :k + 1]
    if s.shape[-1] < k + 1:
        s = torch.cat((s, torch.full_like(s[..., :1], NEG_INF)), -1)
    gap = s[..., :-1] - s[..., 1:]                      # gap[r]: between rank r and rank r + 1
    gap = torch.where(torch.isnan(gap), torch.zeros_like(gap), gap)      # -inf next to -inf: undecided
    above = torch.cat((torch.full_like(gap[..., :1], float("inf")), gap[..., :-1]), -1)
    return (gap > 2 * e) & (above > 2 * e)


def sinkhorn(L, iters, tau=1.0):
    """-> (f [B,Nq], g [B,Nk], row_lse [B,Nq] = log sum_j exp(L_ij + g_j) against the final g)"""
    B, Nq, Nk = L.shape
    log_mu, log_nu = -math.log(Nq), -math.log(Nk)
    g = torch.zeros(B, Nk, dtype=torch.float64, device=L.device)
    for _ in range(iters):
        f = tau * (log_mu - logsumexp(L + g.unsqueeze(1), -1))
        g = tau * (log_nu - logsumexp(L + f.unsqueeze(2), 1))
    return f, g, logsumexp(L + g.unsqueeze(1), -1)


def masses(L, f, g):
    """(match_mass [B,Nq], key_mass [B,Nk]): the row and column sums of the plan over mu and nu — 1 where the marginal is met"""
    B, Nq, Nk = L.shape
    logp = L + f.unsqueeze(2) + g.unsqueeze(1)
    return torch.exp(logsumexp(logp, -1) + math.log(Nq)), torch.exp(logsumexp(logp, 1) + math.log(Nk))


def sparse_warp(qn, kn, v, g, inv_t, k, idx=None):
    """The k-sparse warp over the plan's rows with DETACHED potentials: candidates = top-k of z = L + g (no gradient; `idx` [B,Nq,k]
    given: those), w = softmax_r(L[i, j_r] + g[j_r]), out [B,Cv,Nq] = sum_r w_r v[:, j_r].  qn, kn, v fp64, possibly requiring
    gradients; g is detached here.  -> (out, w, idx)"""
    L = logits(qn, kn, inv_t)
    g = g.detach().double()
    if idx is None:
        idx = biased_topk(L.detach(), g, k)[0]
    s = L.gather(2, idx) + g.unsqueeze(1).expand(-1, L.shape[1], -1).gather(2, idx)
    w = torch.softmax(s, dim=-1)
    B, Nq, kk = idx.shape
    picked = v.double().gather(2, idx.reshape(B, 1, Nq * kk).expand(-1, v.shape[1], -1)).reshape(B, v.shape[1], Nq, kk)
    return (picked * w.unsqueeze(1)).sum(-1), w, idx


# ---- the inputs of the biased-readout tests ---------------------------------------------------------------------------------------
BIAS_SIGMA = 5.0
BIAS_EXCLUDED = 0.10


def make_bias(B, Nk, seed):
    """fp32 [B,Nk] ~ N(0, 5^2) with about 10 % of the entries -inf (CPU tensor)"""
    g = torch.Generator().manual_seed(seed)
    bias = torch.randn(B, Nk, generator=g) * BIAS_SIGMA
    bias[torch.rand(B, Nk, generator=g) < BIAS_EXCLUDED] = NEG_INF
    return bias


def bias_seed(Nq, Nk, shared):
    return 50 + 3 * Nq + Nk + (1000 if shared else 0)


def unit(x):
    x = x.double()
    return (x / x.norm(dim=1, keepdim=True)).float().contiguous()


def readout_case(B, Nq, Nk):
    """(q [B,256,Nq], k [B,256,Nk]) fp32 unit-norm columns on the CPU: tests/test_gpu_match.py's inputs (same seeds)"""
    rn = lambda n, seed: torch.randn(B, 256, n, generator=torch.Generator().manual_seed(seed))
    return unit(rn(Nq, Nq)), unit(rn(Nk, 1000 + Nk))


# ---- the planted collapse ---------------------------------------------------------------------------------------------------------
PLANT_A = 1.2
PLANT_NK = 64


def planted(B=3, Nk=PLANT_NK, a=PLANT_A, seed=5):
    """Keys: near-orthogonal unit vectors (the first Nk axes of the 256, each with noise of norm ~0.05), key 0 the hub h.  Queries
    i < Nk - 1: unit(k_pi(i) + a h) for a permutation pi of the keys 1..Nk-1; the query that pads Nq = Nk - 1 to a multiple of 4 is h
    itself.  With a > 1 every row's largest plain logit is the hub's; the balanced plan cannot give the hub more than its share.
    -> (q [B,256,Nq], k [B,256,Nk] fp32 on the CPU, pi [B,Nq] int64 with pi[:, -1] = 0)"""
    gen = torch.Generator().manual_seed(seed)
    Nq = Nk - 1 + (-(Nk - 1)) % 4
    assert Nq == Nk, "the pad query takes the hub: one pad row"
    keys = torch.eye(256, dtype=torch.float64)[:, :Nk].unsqueeze(0) + 0.05 / 16 * torch.randn(B, 256, Nk, generator=gen).double()
    keys = keys / keys.norm(dim=1, keepdim=True)
    pi = torch.stack([torch.cat((1 + torch.randperm(Nk - 1, generator=gen), torch.zeros(1, dtype=torch.int64))) for _ in range(B)])
    own = keys.gather(2, pi.unsqueeze(1).expand(-1, 256, -1))
    q = own + a * keys[:, :, :1]
    q[:, :, -1] = keys[:, :, 0]
    return unit(q), keys.float().contiguous(), pi
