"""The fp64 restatement of the label-restricted match readout (K47), shared by tests/test_match_labels_cpu.py and
tests/test_gpu_match_labels.py.  Plain torch on whatever device its arguments live on; nothing here calls the library.

    allowed(i, j) = q_label[i] < 0 or q_label[i] == k_label[j]
    L = inv_t * qn^T kn with the disallowed entries -inf; top-k by (value descending, index ascending); logsumexp over the row."""
import torch
import torch.nn.functional as F


def allowed(q_label, k_label):
    """bool [B,Nq,Nk]; k_label [1,Nk] (a shared key set) broadcasts"""
    q, k = q_label.long().unsqueeze(2), k_label.long().unsqueeze(1)
    return (q < 0) | (q == k)


def masked_logits(q, k, q_label, k_label, inv_t):
    """fp64 [B,Nq,Nk] from unit-norm columns q [B,C,Nq], k [B or 1,C,Nk]"""
    L = inv_t * torch.einsum("bci,bcj->bij", q.double(), k.double().expand(q.shape[0], -1, -1))
    return L.masked_fill(~allowed(q_label, k_label), float("-inf"))


def topk_by_value_then_index(L, k):
    """(idx int64 [..,k], val [..,k]) of the rows of L: value descending and, among equal values, index ascending (a stable sort of
    the negated row).  -inf entries come last, lowest index first."""
    order = torch.sort(-L, dim=-1, stable=True).indices[..., :k]
    return order, L.gather(-1, order)


def logsumexp(L):
    """the row log-sum-exp; -inf (not NaN) for a row of -inf"""
    m = L.max(dim=-1, keepdim=True).values
    safe = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    return (safe + torch.log(torch.exp(L - safe).sum(-1, keepdim=True))).squeeze(-1)


def fallback(q_label, k_label, k):
    """(effective query labels int64 [B,Nq], restricted bool [B,Nq]): a position keeps its label only if it is non-negative and the other
    side holds at least k positions of that label in the same sample; otherwise it becomes -1.  Written with loops on purpose."""
    q_label, k_label = q_label.long().cpu(), k_label.long().cpu()
    B, Nq = q_label.shape
    eff, restricted = torch.full((B, Nq), -1, dtype=torch.int64), torch.zeros(B, Nq, dtype=torch.bool)
    for b in range(B):
        keys = k_label[b].tolist()
        count = {}
        for lab in keys:
            if lab >= 0:
                count[lab] = count.get(lab, 0) + 1
        for i, lab in enumerate(q_label[b].tolist()):
            if lab >= 0 and count.get(lab, 0) >= k:
                eff[b, i], restricted[b, i] = lab, True
    return eff, restricted


def cell_labels(seg, down):
    """int64 [B,h,w]: per down x down cell the class with the largest pixel count, the lowest class among equal counts (counted, not
    averaged: integers)"""
    B, nc, H, W = seg.shape
    counts = F.avg_pool2d(seg.double(), down, divisor_override=1).round().long()      # [B,nc,h,w] pixel counts
    best = counts.max(dim=1, keepdim=True).values
    classes = torch.arange(nc, device=seg.device).view(1, nc, 1, 1).expand_as(counts)
    return torch.where(counts == best, classes, torch.full_like(classes, nc)).min(dim=1).values
