"""K54 case helper: the inputs, the bias and the bounds that tests/test_match_box3_transport_cpu.py (on the CPU, arbiter alone) and
tests/test_gpu_match_box3_transport.py (against the kernels) share.  Nothing here calls the library.

Arbiter: the fp64 box logit matrix of tests/test_gpu_match_box3.py (`_arbiter`: unfold -> centre -> normalise -> matmul, times INV_T),
fed to tests/transport_case.py's biased_topk / sinkhorn / masses / decided — those take any L.  Both are imported, not restated.

Bound (K50's rule on this route's recorded figure): an element z' = z + bias of the kernel is tt + bias / a_n, one fma, times a_n; its
error is the unbiased readout's (TOL of tests/test_gpu_match_box3.py = 4 E_BOX, recorded at |z| <= INV_T) grown with the magnitude of
the number it now holds:
    lse_bound(bias) = TOL * (INV_T + max |finite bias|) / INV_T
bounds val and lse of one launch.  A potential after n half-steps has gone through n such launches, each feeding the next through an
affine map of slope tau <= 1: n * lse_bound.  An index is held to the arbiter's wherever the arbiter's value at that rank is more than
2 * lse_bound away from both sorted neighbours; at most EXCUSED_MAX of the ranks may be excused this way."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transport_case as tc  # noqa: E402
from test_gpu_match_box3 import INV_T, KC, TOL, _arbiter  # noqa: E402,F401

#: (h, w, B): tpr = 2 at 256 keys; tpr = 4; 5120 keys — the chunk ring and the restaging of the third plane
GRIDS = [(4, 64, 2), (2, 128, 2), (40, 128, 1)]
GRID_IDS = [f"{h}x{w}" for h, w, _ in GRIDS]
EXCUSED_MAX = 0.01
NEG_INF = float("-inf")


def inputs(h, w, B):
    """(theta, phi) fp32 [B,256,h,w] on the CPU: tests/test_gpu_match_box3.py's `_case` inputs, value for value (same seeds, the same
    CPU generator) — phi carries a weak shifted copy of theta under noise"""
    rn = lambda seed: torch.randn(B, 256, h, w, generator=torch.Generator().manual_seed(seed))
    theta = rn(100 * h + w) + 0.1
    phi = 0.3 * theta.roll((1, 7), (2, 3)) + rn(100 * h + w + 1) - 0.05
    return theta, phi


def bias_for(h, w, B, transposed):
    """fp32 [B,N] on the CPU: transport_case.make_bias (N(0, 5^2), about 10 % -inf), one seed per grid and direction"""
    N = h * w
    return tc.make_bias(B, N, tc.bias_seed(N, N, transposed))


def lse_bound(bias, tol=TOL, inv_t=INV_T):
    fin = bias[torch.isfinite(bias)]
    return tol * (inv_t + (float(fin.abs().max()) if fin.numel() else 0.0)) / inv_t


def directed(L, transposed):
    """the logits of the direction read: rows of L, or of its transpose"""
    return L.transpose(1, 2) if transposed else L


def excused_share(L, bias, k):
    """the share of the top-k ranks of L + bias whose index the arbiter's values do not decide at lse_bound(bias)"""
    z = tc.biased_topk(L, bias, 1)[3]
    return 1.0 - tc.decided(z, k, lse_bound(bias)).double().mean().item()


# ---- the planted collapse on the box route ----------------------------------------------------------------------------------------
PLANT_A = 2.0
PLANT_HUB = (1, 20)
PLANT_MIN_SHARE = 0.45      # every interior row of a 4-row grid: 2 * 62 of 256 positions = 0.484
PLANT_MAX_LOAD = 8


def planted(h=4, w=64, B=2, a=PLANT_A, seed=3):
    """(theta, phi, hub) on the CPU.  phi is noise except for the 3x3 neighbourhood of the hub cell, which holds one zero-mean vector S
    in all nine cells: the hub's unfolded patch is S nine times.  theta is phi rolled by (1, 7) — every content position has a partner
    of its own — plus a * S in every cell, so the patch of every INTERIOR content position has its largest component along the hub's
    patch and its plain argmax is the hub (border positions, whose patches are zero-padded, pick other cells of the neighbourhood: the
    share that collapses onto the one hub is the interior share, 0.484 of a 4 x 64 grid).  Balanced transport cannot give the hub
    more than its 1 / N."""
    g = torch.Generator().manual_seed(seed)
    phi = torch.randn(B, 256, h, w, generator=g)
    S = torch.randn(256, generator=g)
    S = S - S.mean()
    hy, hx = PLANT_HUB
    phi[:, :, hy - 1:hy + 2, hx - 1:hx + 2] = S.view(1, 256, 1, 1) + 0.05 * torch.randn(B, 256, 3, 3, generator=g)
    theta = phi.roll((1, 7), (2, 3)) + a * S.view(1, 256, 1, 1)
    return theta.contiguous(), phi.contiguous(), hy * w + hx


def loads(idx, Nk):
    """rows served per key, per sample: [B,Nk] from the best key per row idx [B,N]"""
    return torch.stack([torch.bincount(r.reshape(-1).long(), minlength=Nk) for r in idx])


def hub_share(L, hub, margin=1.0):
    """per sample the share of the rows whose plain argmax is the hub by more than `margin` over the runner-up (thousands of times the
    kernels' error: no arithmetic flavour decides otherwise)"""
    top = L.sort(-1, descending=True).values
    return ((L.argmax(-1) == hub) & (top[..., 0] - top[..., 1] > margin)).double().mean(-1)
