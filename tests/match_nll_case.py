"""The trainable match readout (K49) restated in torch, for the tests: logits L = inv_t * q^T k from the fp32-rounded operands in a chosen
dtype (fp64: the reference; fp32 on the device: the yardstick arm), logsumexp over both axes, the gather of the target's logit and of
its column lse, and autograd for the gradients.  Plain tensor code on whatever device its inputs live on; the numbers of a hand-made
case are worked out in tests/test_match_nll_cpu.py.

Metrics and bound are tests/accuracy_case.py's: rel_max and rel_slice against fp64, E_kernel <= FACTOR * max(E_fp32, eps) with FACTOR = 4,
at most EXCLUDED_MAX of the positions left out of rel_slice (asserted on the reference).  The gradient tensors carry the suite's floor
for dq / dk (accuracy_case.FLOORS): a planted target makes inv_t (sum_j p_ij k_j - k_t) vanish by cancellation, and such a gradient is
judged on the operands' scale."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy_case as ac  # noqa: E402

rel_max, rel_slice, FACTOR = ac.rel_max, ac.rel_slice, ac.FACTOR
INV_T = ac.INV_T
B = 2
#: partial query and key tiles, a last tile of 4 keys, two and four query blocks with a last block of 4 queries, one tile of 8
SHAPES = [(64, 64), (132, 68), (36, 260), (256, 128), (388, 132), (8, 8)]
#: sigma of the semi regime (k = q + sigma * noise before the normalisation), accuracy_case's where it has the shape; (388, 132) takes
#: (384, 384)'s.  (8, 8) has no semi case, as there.
SEMI_SIGMA = {**ac.SEMI_SIGMA, (388, 132): 8.0}
SEMI_SIGMA.pop((384, 384))
PEAKED_SIGMA = 0.05
GRAD_FLOOR = ac.FLOORS["dq"]
#: (36, 260), corr_pair_nll: a sample's 36 queries name at most 36 of its 260 keys, and a key nobody names and nobody weights has no
#: gradient to speak of — a third of the key columns of the fp64 reference lie below SLICE_MIN, whatever the seed.  Nothing is left out
#: for that: dk is judged in two parts (judge(split=...)), the named columns under both metrics within the 5 % cap, the unnamed ones
#: under rel_max among themselves, where the row-softmax term is the whole gradient.
EXCLUDED_SPLIT = {("corr_pair_nll", 36, 260): "dk"}


#: The peaked regime (sigma = 0.05: every softmax row one-hot) and the fp32 lse.  The backward forms p = exp(s - lse) from the forward's lse, an
#: fp32 number of magnitude inv_t, and whatever that number is off by is a RELATIVE error of every p of its row (column): no backward
#: that takes the lse vectors as fp32 inputs can do better.  torch's fp32 arm is exact there by coincidence — in a one-hot row logsumexp
#: returns the row maximum itself, x_max - lse is exactly 0, p exactly 1, E_fp32 ~ eps — so 4 x E_fp32 measures that coincidence, not fp32
#: arithmetic (measured on an MI355X, profiles/k49_match_nll.txt: the kernel at 45 x .. 6900 x the arm on (64, 64), 7 x .. 45 x on (132, 68)).
#: The peaked cases are therefore judged after an ALLOWANCE derived from the forward's recorded tolerance, not by measured factors:
#: the lse of the readout kernels is within LSE_TOL = 4 x 9.70e-6 at inv_t = 100 (tests/test_gpu_match.py), i.e. within
#: delta(inv_t) = LSE_TOL inv_t / 100 at a magnitude of inv_t, so element (c, i) of a gradient may be off by
#:     D[c,i] = delta inv_t sum_j (|g_row_i| p_ij + |g_col_j| c_ij) |k_cj|          (lse_allowance; p / c the fp64 row / column softmax)
#: and what is left of |x - ref| after D is held to the class rule, 4 x max(E_fp32, eps), under rel_max AND rel_slice, at every shape.
#: tests/test_match_nll_cpu.py shows in numpy, for every (inv_t, shape, tensor, metric), what a lost lo plane measures against this rule.
#: the readout's recorded tolerance of an lse at inv_t = 100 (tests/test_gpu_match.py: TOL = 4 * 9.70e-6)
LSE_TOL = 4 * 9.70e-6


def planted_bound(inv_t, k, g_r, g_c):
    """A planted target makes inv_t (g_r + g_c) (sum_j p_ij k_j - k_t) vanish by cancellation: what is left is the error of sum_j p_ij,
    i.e. of the two lse vectors (each within LSE_TOL), times inv_t max|g_r + g_c| max|k| — an ABSOLUTE bound on dq and dk, derived from
    the forward's tolerance (fp32's own one-hot rows cancel exactly: its error of 1e-35 is no yardstick)"""
    return float(inv_t * 2 * LSE_TOL * (g_r.abs() + g_c.abs()).max() * k.abs().max())


def lse_delta(inv_t):
    return LSE_TOL * inv_t / 100.0


def lse_allowance(q, k, g_row, g_col, inv_t):
    """{"dq": D [B,C,Nq], "dk": D [B,C,Nk]} fp64: what an lse vector that is off by lse_delta(inv_t) may move each gradient element by
    (first order; g_row [B,Nq] / g_col [B,Nk] are the gradients that reach row_lse / col_lse, None = 0)"""
    L = logits(q, k, inv_t)
    w = torch.zeros_like(L)
    if g_row is not None:
        w = w + g_row.double().abs().unsqueeze(2) * torch.softmax(L, dim=2)
    if g_col is not None:
        w = w + g_col.double().abs().unsqueeze(1) * torch.softmax(L, dim=1)
    f = lse_delta(inv_t) * inv_t
    return {"dq": f * torch.einsum("bij,bcj->bci", w, k.double().abs()), "dk": f * torch.einsum("bij,bci->bcj", w, q.double().abs())}


def nll_lse_grads(target, g_r, g_c, Nk):
    """the gradients corr_pair_nll's upstream (g_r, g_c) [B,Nq] sends to (row_lse [B,Nq], col_lse [B,Nk]): g_r on the supervised
    positions, g_c summed over the queries that name a key"""
    sup = target >= 0
    zero = torch.zeros_like(g_r)
    g_col = torch.zeros(g_r.shape[0], Nk, dtype=g_r.dtype, device=g_r.device)
    g_col.scatter_add_(1, target.clamp(min=0).long(), torch.where(sup, g_c, zero))
    return torch.where(sup, g_r, zero), g_col


def discount(x, ref, allowance):
    """x with the allowance taken off its error, elementwise: ref + sign(x - ref) max(|x - ref| - D, 0)"""
    d = torch.as_tensor(ac._np64(x)) - torch.as_tensor(ac._np64(ref))
    return torch.as_tensor(ac._np64(ref)) + torch.sign(d) * (d.abs() - torch.as_tensor(ac._np64(allowance))).clamp(min=0)


def cases():
    return [(Nq, Nk, r) for Nq, Nk in SHAPES for r in (("diffuse", "semi") if (Nq, Nk) in SEMI_SIGMA else ("diffuse",))]


def make_qk(Nq, Nk, regime, sigma=None):
    """(qn [B,256,Nq], kn [B,256,Nk]) fp32 CPU tensors: accuracy_case.make_qkv's operands (centred, unit columns, fp32-rounded);
    regime "peaked" is semi with sigma = PEAKED_SIGMA (every row one-hot on its own index)"""
    if regime == "peaked":
        regime, sigma = "semi", PEAKED_SIGMA
    if regime == "semi" and sigma is None:
        sigma = SEMI_SIGMA[(Nq, Nk)]
    q, k, _, _ = ac.make_qkv(B, Nq, Nk, 1, regime, sigma=sigma)
    return torch.from_numpy(q).float(), torch.from_numpy(k).float()


def upstream(Nq, Nk, seed=49):
    """random upstream gradients: (g_row [B,Nq], g_col [B,Nk]) for corr_lse, (g_r, g_c) both [B,Nq] for corr_pair_nll"""
    g = torch.Generator().manual_seed(seed + 3 * Nq + Nk)
    return (torch.randn(B, Nq, generator=g), torch.randn(B, Nk, generator=g)), (torch.randn(B, Nq, generator=g), torch.randn(B, Nq, generator=g))


def targets(Nq, Nk, seed=7, unsupervised=0.25):
    """random targets in [0, Nk), a share of them negative"""
    g = torch.Generator().manual_seed(seed + Nq + 5 * Nk)
    t = torch.randint(0, Nk, (B, Nq), generator=g)
    t[torch.rand(B, Nq, generator=g) < unsupervised] = -1
    return t


def logits(q, k, inv_t, dtype=torch.float64):
    """q [B,C,Nq], k [B,C,Nk] -> L [B,Nq,Nk]"""
    return inv_t * torch.einsum("bci,bcj->bij", q.to(dtype), k.to(dtype))


def lse_pair(q, k, inv_t, dtype=torch.float64):
    L = logits(q, k, inv_t, dtype)
    return torch.logsumexp(L, dim=2), torch.logsumexp(L, dim=1)


def pair_nll(q, k, target, inv_t, dtype=torch.float64):
    """(row_nll, col_nll) [B,Nq]; 0 where target < 0"""
    L = logits(q, k, inv_t, dtype)
    sup = target >= 0
    t = target.clamp(min=0).long()
    s = L.gather(2, t.unsqueeze(2)).squeeze(2)
    zero = torch.zeros_like(s)
    return (torch.where(sup, torch.logsumexp(L, dim=2) - s, zero),
            torch.where(sup, torch.logsumexp(L, dim=1).gather(1, t) - s, zero))


def restate(q, k, inv_t, ups, target=None, dtype=torch.float64):
    """outputs and gradients of sum(up_0 * out_0) + sum(up_1 * out_1) in `dtype` (fp32: run under accuracy_case.plain_fp32 on the
    device) -> {"out0", "out1", "dq", "dk"}; an upstream entry may be None"""
    q = q.detach().clone().to(dtype).requires_grad_(True)
    k = k.detach().clone().to(dtype).requires_grad_(True)
    with ac.plain_fp32():
        outs = lse_pair(q, k, inv_t, dtype) if target is None else pair_nll(q, k, target, inv_t, dtype)
        loss = sum((o * u.to(dtype)).sum() for o, u in zip(outs, ups) if u is not None)
        loss.backward()
    return {"out0": outs[0].detach(), "out1": outs[1].detach(), "dq": q.grad, "dk": k.grad}


def _columns(x, mask):
    """x [B,C,N], mask [B,N] -> [1,C,M]: the selected positions of all samples side by side"""
    x = torch.as_tensor(ac._np64(x))
    return x.permute(1, 0, 2)[:, torch.as_tensor(mask).cpu()].unsqueeze(0)


def judge(kernel, shape, regime, got, arm, ref, factor=FACTOR, slices=True, allow=None, split=None):
    """accuracy_case.Judge over dq and dk (got / arm / ref: dicts as restate's) -> the Judge, rows printed.
    slices   True / False / a set of tensor names: which tensors are judged under rel_slice as well as rel_max.  A tensor is left to
             rel_max alone only where the TARGETS leave whole positions without a gradient (negative targets; one key all queries name)
    allow    lse_allowance's dict: taken off the kernel's error first (the peaked regime; the arm is judged as it is)
    split    {tensor: mask [B,N]}: the tensor is judged in two parts — the positions of the mask under both metrics, the others under
             rel_max (the key columns no query names at (36, 260): a third of them vanish in the reference, see EXCLUDED_SPLIT)"""
    j = ac.Judge(kernel, "ops", shape, regime)
    parts = []
    for t in ("dq", "dk"):
        if got.get(t) is None:
            continue
        x = got[t] if allow is None else discount(got[t], ref[t], allow[t])
        per_slice = slices if isinstance(slices, bool) else t in slices
        if split is not None and t in split:
            m = torch.as_tensor(split[t]).bool()
            parts.append((t + "[named]", _columns(x, m), _columns(arm[t], m), _columns(ref[t], m), per_slice))
            parts.append((t + "[unnamed]", _columns(x, ~m), _columns(arm[t], ~m), _columns(ref[t], ~m), False))
        else:
            parts.append((t, x, arm[t], ref[t], per_slice))
    for name, x, a, r, per_slice in parts:
        if per_slice:
            j.add(name, x, a, r, floor=GRAD_FLOOR, factor=factor, excluded=ac.EXCLUDED_MAX)
        else:
            ek, ea = rel_max(x, r, GRAD_FLOOR), rel_max(a, r, GRAD_FLOOR)
            j.rows.append((name, "rel_max", ek, ea, factor))
            print(f"{j.head} {name} rel_max {ek:.3e} {ea:.3e} {ek / max(ea, ac.FP32_EPS):.2f}", flush=True)
    return j


def excluded_shares(ref):
    """share of the positions rel_slice would leave out, per gradient tensor of a reference"""
    return {t: ac.excluded_share(ref[t]) for t in ("dq", "dk")}


# ---- what a lost lo plane costs (numpy, fp64 arithmetic with ONE operand of ONE product rounded to its f16 hi plane) ---------------
def lost_plane_dq(q, k, g_row, g_col, inv_t, which):
    """dq [B,C,Nq] of sum g_row row_lse + sum g_col col_lse with `which` in {"k_lo_qk", "k_lo_wk", "w_lo"} dropped (None: nothing)"""
    q, k, a, b = (np.asarray(t, dtype=np.float64) for t in (q, k, g_row, g_col))
    kq = ac.hi_plane(k, 16.0) if which == "k_lo_qk" else k
    L = inv_t * np.einsum("bci,bcj->bij", q, kq)
    L0 = inv_t * np.einsum("bci,bcj->bij", q, k)
    lse = lambda x, ax: np.log(np.exp(x - x.max(axis=ax, keepdims=True)).sum(axis=ax, keepdims=True)) + x.max(axis=ax, keepdims=True)
    # the lse vectors are the forward's (whole planes): only the recomputed S carries the loss
    w = a[:, :, None] * np.exp(L - lse(L0, 2)) + b[:, None, :] * np.exp(L - lse(L0, 1))
    if which == "w_lo":
        w = ac.hi_plane(w, 2.0 ** 14 / (np.abs(a).max() + np.abs(b).max()))
    kv = ac.hi_plane(k, 16.0) if which == "k_lo_wk" else k
    return inv_t * np.einsum("bij,bcj->bci", w, kv)
