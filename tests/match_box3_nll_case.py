"""The fp64 arbiter of K53 (ops.box3_lse, ops.box3_pair_logits, hot_path.correspondence_nll_box3) and the data its tests share.  The
arbiter is the literal restatement: F.unfold(kernel_size=3, padding=1) of theta and phi, centre over the 2304 entries, divide by
(norm + ops.NORM_EPS), dot, times 1 / temperature, torch.logsumexp over each axis, gather at the target — gradients from autograd.  It
shares no code with the kernels' box / tap formulations."""
import torch
import torch.nn.functional as F

INV_T = 100.0


def unit_unfolded(x):
    """x [B,C,h,w] -> [B,9C,h*w]: the zero-padded 3x3-unfolded vectors, centred over their 9C entries and divided by (norm + eps)"""
    from cocosnet_amd import ops
    u = F.unfold(x, kernel_size=3, padding=1)
    u = u - u.mean(dim=1, keepdim=True)
    return u / (u.norm(dim=1, keepdim=True) + ops.NORM_EPS)


def stats(x):
    """(mu, a) [B,h*w] as ops.unfold3_stats defines them, in the dtype of x, with autograd"""
    from cocosnet_amd import ops
    u = F.unfold(x, kernel_size=3, padding=1)
    mu = u.mean(dim=1)
    return mu, 1.0 / ((u - mu.unsqueeze(1)).norm(dim=1) + ops.NORM_EPS)


def logits(theta, phi, inv_t=INV_T):
    """z [B,Nq,Nk] in the dtype of the inputs"""
    return inv_t * torch.einsum("bci,bcj->bij", unit_unfolded(theta), unit_unfolded(phi))


def arbiter(theta, phi, target, inv_t=INV_T, weight=None, symmetric=True):
    """theta, phi [B,C,h,w] in one dtype, target [B,h,w] or [B,N] integers below Nk (negative: unsupervised) -> the dictionary of
    hot_path.correspondence_nll_box3 with flat [B,N] entries (and z_t)"""
    z = logits(theta, phi, inv_t)
    B, Nq, Nk = z.shape
    t = target.reshape(B, Nq).long()
    sup = t >= 0
    row_lse, col_lse = torch.logsumexp(z, dim=2), torch.logsumexp(z, dim=1)
    tc = t.clamp_min(0)
    z_t = torch.gather(z, 2, tc.unsqueeze(2)).squeeze(2)
    zero = torch.zeros((), dtype=z.dtype)
    row_nll = torch.where(sup, row_lse - z_t, zero)
    col_nll = torch.where(sup, torch.gather(col_lse, 1, tc) - z_t, zero)
    w = sup.to(z.dtype) if weight is None else torch.where(sup, weight.reshape(B, Nq).to(z.dtype), zero)
    per = row_nll + col_nll if symmetric else row_nll
    loss = (w * per).sum() / w.sum().clamp_min(torch.finfo(torch.float32).tiny)
    return {"match_nll": row_nll, "back_nll": col_nll, "match_lse": row_lse, "back_lse": col_lse, "z_t": torch.where(sup, z_t, zero),
            "loss_match": loss}


# ---- the case generators ------------------------------------------------------------------------------------------------------------
def diffuse(B, grid, seed, C=256):
    """(theta, phi) fp32 on the host: independent noise with a common offset (the kc mu nu term of the logit matters) — flat rows"""
    g = torch.Generator().manual_seed(seed)
    theta, phi = torch.randn(B, C, *grid, generator=g), torch.randn(B, C, *grid, generator=g)
    return (theta + 0.1).contiguous(), (phi - 0.05).contiguous()


def peaked(B, grid, seed, C=256, noise=0.05):
    """phi = theta permuted along the positions plus a little noise: every row and column of the logits has one dominant entry.
    -> (theta, phi, perm) with perm [N] the exemplar position of content position i"""
    g = torch.Generator().manual_seed(seed)
    theta = torch.randn(B, C, *grid, generator=g)
    N = grid[0] * grid[1]
    perm = torch.randperm(N, generator=g)
    phi = torch.empty(B, C, N)
    phi[:, :, perm] = theta.reshape(B, C, N)
    phi = phi.reshape(B, C, *grid) + noise * torch.randn(B, C, *grid, generator=g)
    return theta.contiguous(), phi.contiguous(), perm


def identical(B, grid, seed, C=256):
    """theta == phi: the planted permutation is the identity and match_target_prob -> 1 at inv_t = 100"""
    g = torch.Generator().manual_seed(seed)
    theta = torch.randn(B, C, *grid, generator=g).contiguous()
    return theta, theta.clone()


def targets(B, grid, seed, kind="mixed"):
    """target [B,h,w] int64: "all_negative"; "mixed": random positions with every fifth cell unsupervised, repeats (every third cell
    names key 0 of its sample: a hub) and the last key named; "identity": t_i = i"""
    N = grid[0] * grid[1]
    g = torch.Generator().manual_seed(seed)
    if kind == "all_negative":
        return torch.full((B, *grid), -1, dtype=torch.int64)
    if kind == "identity":
        return torch.arange(N).repeat(B, 1).reshape(B, *grid)
    t = torch.randint(0, N, (B, N), generator=g)
    t[:, 0::3] = 0
    t[:, 1::5] = -1
    t[:, 2] = N - 1
    t[:, 4] = -7
    return t.reshape(B, *grid)


def weights(B, grid, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(B, *grid, generator=g) * 2.0
    w[:, 0, 0::7] = 0.0
    return w


# ---- the peaked regime: what the readout's lse tolerance allows a gradient element -------------------------------------------------
def lse_gradients(target, weight, symmetric):
    """(g_row [B,N], g_col [B,N]) fp64: the gradients loss_match sends to row_lse and col_lse — w_i / sum w on the supervised cells,
    and its sum over the cells that name a key (0 unless symmetric)"""
    B = target.shape[0]
    t = target.reshape(B, -1).long()
    sup = t >= 0
    w = sup.double() if weight is None else torch.where(sup, weight.reshape(B, -1).double(), torch.zeros((), dtype=torch.float64, device=t.device))
    g_row = w / w.sum().clamp_min(torch.finfo(torch.float32).tiny)
    g_col = torch.zeros_like(g_row)
    if symmetric:
        g_col.scatter_add_(1, t.clamp_min(0), g_row)
    return g_row, g_col


def _allow_side(x, other, w_t, wz, mu, a, nu_other):
    """sum over the pairs (p, q) of |w_pq| |d z_pq / d x[c,m]| for x = the side whose positions index the ROWS of w_t / wz:
    the tap term (R is bilinear: its derivative with |other| in the other slot), the mean term and the norm term (see lse_allowance)"""
    B, C, h, w = x.shape
    xr = x.detach().clone().requires_grad_(True)
    r = torch.einsum("bkp,bkq->bpq", F.unfold(xr, 3, padding=1), F.unfold(other.abs(), 3, padding=1))
    (a1,) = torch.autograd.grad((w_t * r).sum(), xr)
    box = lambda s: F.avg_pool2d(s.reshape(B, 1, h, w), 3, stride=1, padding=1, divisor_override=1)
    a2 = box((w_t * nu_other.abs().unsqueeze(1)).sum(2))
    rp = F.pad((a * a * wz.sum(2)).reshape(B, 1, h, w), (1, 1, 1, 1))
    mp = F.pad(mu.reshape(B, 1, h, w), (1, 1, 1, 1))
    a3 = torch.zeros_like(x)
    for dy in range(3):
        for dx in range(3):
            a3 = a3 + rp[:, :, dy:dy + h, dx:dx + w] * (x - mp[:, :, dy:dy + h, dx:dx + w]).abs()
    return a1 + a2 + a3


def lse_allowance(theta, phi, g_row, g_col, inv_t, delta):
    """{"dtheta", "dphi"} fp64: what lse vectors that are off by `delta` (the readout's recorded tolerance at this temperature) may move
    each gradient element by, to first order.  The backward forms w_pq = g exp(z_pq - lse) from the forward's lse: an lse off by delta
    is a RELATIVE error delta of every w of its row (column), so element (c, m) moves by at most
        delta sum_pq (|g_row_p| P_pq + |g_col_q| C_pq) |d z_pq / d theta[c,m]|                (P / C: the fp64 row / column softmax)
    with z_pq = inv_t a_p b_q (R_pq - kc mu_p nu_q) and, for m = p + d a tap of p inside the grid,
        |d z_pq / d theta[c,m]| <= inv_t a_p b_q |phi[c,q+d]|  +  inv_t a_p b_q |nu_q|  +  |z_pq| a_p^2 |theta[c,m] - mu_p|
    (through R, through mu_p = mean, through a_p = 1 / norm); phi likewise with the roles exchanged."""
    z = logits(theta, phi, inv_t)
    wabs = g_row.abs().unsqueeze(2) * torch.softmax(z, dim=2) + g_col.abs().unsqueeze(1) * torch.softmax(z, dim=1)
    (mu, a), (nu, b) = stats(theta), stats(phi)
    w_t = wabs * inv_t * a.unsqueeze(2) * b.unsqueeze(1)
    wz = wabs * z.abs()
    tr = lambda m: m.transpose(1, 2)
    return {"dtheta": delta * _allow_side(theta, phi, w_t, wz, mu, a, nu), "dphi": delta * _allow_side(phi, theta, tr(w_t), tr(wz), nu, b, mu)}
