"""The fp64 arbiter of K51 (ops.box3_sparse_softmax_warp) and the data its tests share.  The arbiter is the literal restatement:
F.unfold(kernel_size=3, padding=1) of theta and phi, centre over the 2304 entries, divide by (norm + ops.NORM_EPS), gather the k logits
per query from the clamped idx, softmax, blend — gradients from autograd.  It shares no code with the kernels' tap formulation
(`tap_R` below is that formulation on the host, written with loops over 2-D coordinates, and is checked against the unfolded product
in tests/test_box3_sparse_cpu.py)."""
import torch
import torch.nn.functional as F


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


def gather(t, idx):
    """t [B,C,Nk], idx [B,Nq,k] int64 in range -> [B,Nq,k,C]"""
    return torch.stack([t[b].t()[idx[b]] for b in range(t.shape[0])])


def arbiter(theta, phi, v, idx, inv_t, weights=False):
    """theta [B,C,fh,fw], phi [B,C,gh,gw], v [B,Cv,gh*gw] in one dtype (fp64 in every test), idx [B,fh*fw,k] any integers
    -> out [B,Cv,fh*fw] (and w [B,fh*fw,k])"""
    Nk = phi.shape[2] * phi.shape[3]
    j = idx.long().clamp(0, Nk - 1)
    z = inv_t * torch.einsum("bci,birc->bir", unit_unfolded(theta), gather(unit_unfolded(phi), j))
    w = torch.softmax(z, dim=-1)
    out = torch.einsum("bir,birc->bci", w, gather(v, j))
    return (out, w) if weights else out


def dense(theta, phi, v, inv_t):
    """the dense route in the dtype of the inputs: unfold, centre, normalise, all logits, softmax over every key, matmul"""
    z = inv_t * torch.einsum("bci,bcj->bij", unit_unfolded(theta), unit_unfolded(phi))
    return torch.einsum("bij,bcj->bci", torch.softmax(z, dim=-1), v)


def tap_R(theta, phi):
    """R [B,Nq,Nk] by the kernels' rule, with loops over 2-D coordinates: the sum over the taps d in {-1,0,1}^2 with p+d inside the
    content grid AND q+d inside the exemplar grid of <theta[:,p+d], phi[:,q+d]>"""
    B, _, fh, fw = theta.shape
    gh, gw = phi.shape[2:]
    R = torch.zeros(B, fh * fw, gh * gw, dtype=theta.dtype)
    for py in range(fh):
        for px in range(fw):
            for qy in range(gh):
                for qx in range(gw):
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            if 0 <= py + dy < fh and 0 <= px + dx < fw and 0 <= qy + dy < gh and 0 <= qx + dx < gw:
                                R[:, py * fw + px, qy * gw + qx] += (theta[:, :, py + dy, px + dx] * phi[:, :, qy + dy, qx + dx]).sum(1)
    return R


def features(B, grid, kgrid, seed, C=256):
    """(theta [B,C,*grid], phi [B,C,*kgrid]) fp32 on the host: random, with a few exemplar cells planted next to content cells (peaked
    rows next to diffuse ones) and a common offset (means that are not zero: the kc mu nu term of the logit matters)"""
    g = torch.Generator().manual_seed(seed)
    theta, phi = torch.randn(B, C, *grid, generator=g), torch.randn(B, C, *kgrid, generator=g)
    for n in range(3):
        (py, px), (qy, qx) = ((n * 5) % grid[0], (n * 3) % grid[1]), ((n * 7 + 1) % kgrid[0], (n * 2 + 1) % kgrid[1])
        phi[:, :, qy, qx] = 2.0 * theta[:, :, py, px] + 0.3 * torch.randn(B, C, generator=g)
    return (theta + 0.1).contiguous(), (phi - 0.05).contiguous()


def index_table(B, Nq, Nk, k, seed):
    """idx [B,Nq,k] int64, random, with: repeats inside rows, values below 0 and at or above Nk (clamped by the op: they land on the
    first and the last key, the corners of the grid), one key every query names (the last one, in rank 0; with k = 1 every second
    query, or the table would hold nothing else), candidates in the first and last row and column (keys 0 and Nk - 1), and — where
    the grid has more than two keys — one key that nobody names (key 1) -> (idx, hub, dead or None)"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(-2, Nk + 2, (B, Nq, k), generator=g)
    hub, dead = Nk - 1, (1 if Nk > 2 else None)
    if k > 1:
        idx[:, :, 0] = hub
        idx[:, 0::3, 1] = idx[:, 0::3, 0]            # a repeat inside every third row
        idx[:, 1::4, k - 1] = 0                      # the first key
    else:
        idx[:, 0::2, 0] = hub
        idx[:, 1::4, 0] = 0
    idx[0, 0, k - 1], idx[B - 1, Nq - 1, k - 1] = -7, Nk + 10 ** 9
    if dead is not None:
        idx[idx == dead] = 0
    return idx, hub, dead
