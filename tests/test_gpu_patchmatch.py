"""K43 on the GPU: ops.patchmatch_step / patchmatch_topk, hot_path.correspondence_sparse(search="patchmatch") and
NoVGGCorrespondence.sparse_warp(search="patchmatch").

The reference is tests/patchmatch_case.py: the candidate pool of every query restated in integer numpy (exact) and fp64 scores from the
values of the operand planes the kernel reads.  Tolerance on a score: tests/test_gpu_parity.py's OUT_TOL times inv_t (|<q, k>| <= 1, so
inv_t is the scale of the logits).  Selection is judged by criteria that hold under near-ties: every returned key is in the pool, the
keys are distinct, the scores are the pairs' scores, they do not increase, and the last one is not below the pool's k-th best by more
than that tolerance.

This file sorts before tests/test_gpu_red_zones.py: its red-zone case (below) has run when that file's "every entry point was reached"
audit counts the `cocos_patchmatch_step_f16x3` literal of cocosnet_amd/ops.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patchmatch_case as pc  # noqa: E402
import test_gpu_red_zones as rz  # noqa: E402
from test_gpu_parity import OUT_TOL, rel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INV_T = 100.0
TOL = OUT_TOL * INV_T
B = 2
QGRID = (8, 12)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _unit(x):
    x = x.double()
    return (x / x.norm(dim=1, keepdim=True)).float().contiguous()


_CASES = {}


def _case(kgrid):
    """(qn, kn, planes, qv, kv): unit-norm columns on the device — every key a noisy copy of some query, so the scores of a pool spread
    from near inv_t down to noise — their operand planes and the fp64 values of those planes.  Made once per key grid, never written."""
    from cocosnet_amd import ops
    if kgrid not in _CASES:
        Nq, Nk = QGRID[0] * QGRID[1], kgrid[0] * kgrid[1]
        g = _gen(100 + Nk)
        q = _unit(torch.randn(B, 256, Nq, generator=g))
        src = torch.randint(0, Nq, (B, Nk), generator=g)
        noise = torch.rand(B, 1, Nk, generator=g) * 2.0
        k = _unit(torch.stack([q[b][:, src[b]] for b in range(B)]) + noise * torch.randn(B, 256, Nk, generator=g) / 16.0)
        q, k = q.to(DEV), k.to(DEV)
        planes = ops.OperandPlanes()
        with torch.no_grad():
            qv = pc.plane_values(*planes.get(q, True, ops.SPLIT_OPERAND_SCALE), ops.SPLIT_OPERAND_SCALE)
            kv = pc.plane_values(*planes.get(k, True, ops.SPLIT_OPERAND_SCALE), ops.SPLIT_OPERAND_SCALE)
        _CASES[kgrid] = (q, k, planes, qv, kv)
    return _CASES[kgrid]


def _judge(tag, idx, val, cand, qv, kv, k):
    """the five criteria of one step, for every query"""
    idx, val = idx.cpu().numpy().astype(np.int64), val.cpu().numpy()
    assert idx.shape == val.shape == cand.shape[:2] + (k,) and np.isfinite(val).all(), tag
    member = (idx[:, :, :, None] == cand[:, :, None, :]).any(axis=3)
    assert member.all(), (tag, "a returned key is not in the pool", np.argwhere(~member)[:4])
    sc = pc.scores(qv, kv, cand, INV_T)
    kth, count = pc.kth_best_distinct(cand, sc, k)
    full = count >= k
    srt = np.sort(idx, axis=2)
    distinct = (np.diff(srt, axis=2) > 0).all(axis=2) if k > 1 else np.ones_like(full)
    assert distinct[full].all(), (tag, "repeated keys although the pool holds k distinct ones")
    err = np.abs(val - pc.scores(qv, kv, idx, INV_T)).max()
    slack = (kth - val[:, :, k - 1])[full].max() if full.any() else -np.inf
    print(f"[patchmatch] {tag}: max |val - fp64| {err:.3e}  max (k-th best - val[k-1]) {slack:.3e}  (tolerance {TOL:.1e}); "
          f"pools below k distinct keys: {int((~full).sum())}")
    assert err <= TOL, (tag, err)
    assert (np.diff(val, axis=2) <= 0).all(), (tag, "val increases along the ranks")
    assert slack <= TOL, (tag, slack)
    for b, i in np.argwhere(~full):      # a short pool: its distinct keys, then the last pair repeated
        c = count[b, i]
        assert len(set(idx[b, i, :c])) == c and (idx[b, i, c:] == idx[b, i, c - 1]).all() and (val[b, i, c:] == val[b, i, c - 1]).all(), tag


# ---------------------------------------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("k", [1, 3, 4, 8])
@pytest.mark.parametrize("kgrid", [(8, 12), (6, 8)])
def test_one_step_against_the_restatement(kgrid, k):
    from cocosnet_amd import ops
    qn, kn, planes, qv, kv = _case(kgrid)
    Nq, Nk = QGRID[0] * QGRID[1], kgrid[0] * kgrid[1]
    grids = (QGRID, kgrid)
    table = torch.randint(0, Nk, (B, Nq, k), generator=_gen(7 * k + Nk))
    table[:, 1, 0], table[:, 2, k - 1], table[0, 5, 0], table[1, Nq - 1, 0] = -1, Nk, 10 ** 9, -(2 ** 31)      # out of range: clamped
    table[:, 9, :] = table[:, 9, :1]                                                                             # a row of one key
    for stride in (1, 2):
        for S in (0, 3):
            for it, t in enumerate((table, None)):
                seed = 11 + stride
                idx, val = ops.patchmatch_step(qn, kn, None if t is None else t.to(DEV), grids, INV_T, k, stride, S, 4, seed, it, planes)
                assert idx.dtype == torch.int32 and val.dtype == torch.float32
                cand = pc.pool(None if t is None else t.numpy(), B, grids, k, stride, S, 4, seed, it)
                _judge(f"key {kgrid} k={k} stride={stride} S={S} {'table' if t is not None else 'random init'}", idx, val, cand, qv, kv, k)


def test_tie_order():
    """key rows that are bitwise copies of one another: wherever both reach the top k, the lower index comes first, with equal bits"""
    from cocosnet_amd import ops
    kgrid = (6, 8)
    qn, kn, _, _, _ = _case(kgrid)
    Nq, Nk, k = QGRID[0] * QGRID[1], 48, 3
    kn = kn.clone()
    pairs = [(3, 40), (17, 18), (0, 47)]
    for lo, hi in pairs:
        kn[:, :, hi] = kn[:, :, lo]
    table = torch.zeros(B, Nq, k, dtype=torch.int64)
    for i in range(Nq):
        lo, hi = pairs[i % 3]
        table[:, i] = torch.tensor([hi, lo, (i * 5) % Nk])      # the copy with the HIGHER index first in the own list
    # stride 16 leaves no neighbour inside the 8 x 12 grid: the pool is the own list, both copies are always in the top 3; stride 1
    # adds the neighbours' candidates, which may push a copy out — judged wherever both stayed
    for stride in (16, 1):
        idx, val = ops.patchmatch_step(qn, kn, table.to(DEV), (QGRID, kgrid), INV_T, k, stride, 0, 0, 0, 0)
        idx, bits = idx.cpu().numpy(), val.cpu().numpy().view(np.int32)
        seen = 0
        for b in range(B):
            for i in range(Nq):
                row = idx[b, i].tolist()
                for lo, hi in pairs:
                    if lo in row and hi in row:
                        seen += 1
                        assert row.index(lo) + 1 == row.index(hi), (stride, b, i, row)
                        assert bits[b, i, row.index(lo)] == bits[b, i, row.index(hi)], (stride, b, i)
        assert seen >= (B * Nq if stride == 16 else 1), (stride, seen)


def test_short_pool_repeats_its_last_pair():
    """rows of one key, no neighbour inside the grid (stride 16), no search: a pool of ONE distinct key for k = 3 — the key once, then
    repeated with its score; with two radii of search around it the pool grows again"""
    from cocosnet_amd import ops
    kgrid = (6, 8)
    qn, kn, planes, qv, kv = _case(kgrid)
    Nq, k = QGRID[0] * QGRID[1], 3
    table = torch.randint(0, 48, (B, Nq, 1), generator=_gen(9)).expand(B, Nq, k).contiguous()
    for S in (0, 2):
        idx, val = ops.patchmatch_step(qn, kn, table.to(DEV), (QGRID, kgrid), INV_T, k, 16, S, 1, 0, 0, planes)
        cand = pc.pool(table.numpy(), B, (QGRID, kgrid), k, 16, S, 1, 0, 0)
        _judge(f"short pool S={S}", idx, val, cand, qv, kv, k)
        if S == 0:
            assert torch.equal(idx.cpu().long(), table) and bool((val[:, :, 1:] == val[:, :, :1]).all())


def test_propagation_is_exact():
    """the key planes are the query planes moved by (+2, -3) (copied rows: query (y, x) has its copy at key (y - 2, x + 3)), no search,
    stride 1, k = 1; the table is right in column x = 0 only and names one fixed wrong key elsewhere.  After t launches a query whose
    copy lies inside the key grid is right exactly when x <= t.  The copy scores inv_t, random unit vectors score about inv_t / 16: no
    tolerance is involved.  (The wrong key (7, 0) shifted along any path is the copy of a position outside the query grid.)"""
    from cocosnet_amd import ops
    h, w = QGRID
    g = _gen(3)
    q = _unit(torch.randn(B, 256, h * w, generator=g))
    kn = _unit(torch.randn(B, 256, h * w, generator=g))
    true = torch.full((h, w), -1, dtype=torch.int64)
    for y in range(h):
        for x in range(w):
            if y - 2 >= 0 and x + 3 < w:
                true[y, x] = (y - 2) * w + x + 3
                kn[:, :, true[y, x]] = q[:, :, y * w + x]
    wrong = 7 * w
    table = torch.full((h, w), wrong, dtype=torch.int64)
    table[:, 0] = torch.where(true[:, 0] >= 0, true[:, 0], table[:, 0])
    idx = table.reshape(1, h * w, 1).expand(B, -1, -1).contiguous().to(DEV)
    q, kn = q.to(DEV), kn.to(DEV)
    planes = ops.OperandPlanes()
    inside = (true >= 0)
    xs = torch.arange(w).view(1, w).expand(h, w)
    for t in (1, 2, 3):
        idx, val = ops.patchmatch_step(q, kn, idx, (QGRID, QGRID), INV_T, 1, 1, 0, 0, 0, t - 1, planes)
        got = idx.cpu().reshape(B, h, w).to(torch.int64)
        for b in range(B):
            right = got[b] == true
            assert torch.equal(right[inside], (xs <= t)[inside]), (t, b, right.int())
        assert float(val.cpu().reshape(B, h, w)[:, inside & (xs <= t)].min()) > 0.99 * INV_T


def test_scores_never_decrease_over_iterations():
    """four iterations from the random initialisation: the best and the k-th score of every query never decrease, bitwise (the own
    candidates are always in the pool, they are distinct, and a pair's score is a pure function of the pair)"""
    from cocosnet_amd import ops
    kgrid, k = (8, 12), 4
    qn, kn, planes, _, _ = _case(kgrid)
    idx, prev = None, None
    for it, stride in enumerate((1, 2, 1, 1)):
        idx, val = ops.patchmatch_step(qn, kn, idx, (QGRID, kgrid), INV_T, k, stride, 2, 6, 5, it, planes)
        if prev is not None:
            assert bool((val[:, :, 0] >= prev[:, :, 0]).all()) and bool((val[:, :, k - 1] >= prev[:, :, k - 1]).all()), it
        prev = val
    assert bool(torch.isfinite(prev).all())


def test_reproducible_and_seeded():
    from cocosnet_amd import ops
    kgrid = (6, 8)
    qn, kn, planes, _, _ = _case(kgrid)
    run = lambda seed: ops.patchmatch_topk(qn, kn, INV_T, 4, (QGRID, kgrid), "random", (1, 2, 1), (2, 3), seed, planes)
    a, b, c = run(1), run(1), run(2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert not torch.equal(a[0], c[0])
    assert a[0].shape == a[1].shape == (B, QGRID[0] * QGRID[1], 4) and int(a[0].min()) >= 0 and int(a[0].max()) < 48


def test_values_are_the_logits_of_the_sparse_warp():
    """softmax(val) against the weights ops.sparse_softmax_warp forms for the same index table on the same planes"""
    from cocosnet_amd import ops
    kgrid = (6, 8)
    qn, kn, planes, _, _ = _case(kgrid)
    for k in (1, 3, 8):
        idx, val = ops.patchmatch_topk(qn, kn, INV_T, k, (QGRID, kgrid), "random", (1, 1), (1, 2), 3, planes)
        v = torch.randn(B, 5, 48, generator=_gen(k)).to(DEV)
        with torch.no_grad():
            _, w = ops.sparse_softmax_warp(qn, kn, v, idx, INV_T, planes, return_weights=True)
        err = rel(torch.softmax(val, dim=-1), w.cpu().numpy())
        print(f"[patchmatch] k={k}: softmax(val) against K42's weights: rel {err:.3e}")
        assert err < OUT_TOL, (k, err)


# ---------------------------------------------------------------------------------------------------------------- hot path and module
def test_coarse_initialisation_expands_the_half_grid_candidates():
    """every fine query (y, x) starts from the candidates of coarse query (y / 2, x / 2), each moved to the fine key
    (2 ky + y % 2, 2 kx + x % 2); grids the half-grid readout does not take start from "random" """
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import _flat, _patchmatch_coarse_init
    g = _gen(21)
    theta, phi = torch.randn(2, 256, 8, 8, generator=g).to(DEV), torch.randn(2, 256, 8, 12, generator=g).to(DEV)
    with torch.no_grad():
        init = _patchmatch_coarse_init(theta, phi, INV_T, 3)
        pl = ops.OperandPlanes()
        pool = lambda t: _flat(torch.nn.functional.avg_pool2d(t, 2))
        qc, kc = ops.center_l2norm_planes(pool(theta), 1, pl, want_chan=False), ops.center_l2norm_planes(pool(phi), 1, pl, want_chan=False)
        coarse = ops.corr_topk(qc, kc, INV_T, 3, pl)[0].cpu().numpy()
    assert init.shape == (2, 64, 3) and init.dtype == torch.int64
    init = init.cpu().numpy()
    for y in range(8):
        for x in range(8):
            c = coarse[:, (y // 2) * 4 + x // 2]                      # [B,3] on the 4 x 6 half key grid
            want = (2 * (c // 6) + y % 2) * 12 + 2 * (c % 6) + x % 2
            assert np.array_equal(init[:, y * 8 + x], want), (y, x)
    with torch.no_grad():
        assert _patchmatch_coarse_init(theta[:, :, :6, :6], phi[:, :, :6, :6], INV_T, 3) == "random"      # 3 x 3: 9 positions
        assert _patchmatch_coarse_init(theta[:, :, :7], phi, INV_T, 3) == "random"                          # an odd side
        assert _patchmatch_coarse_init(theta[:, :, :4, :4], phi[:, :, :4, :4], INV_T, 5) == "random"        # 4 half-grid keys < k


@pytest.mark.parametrize("fh", [8, 6])
def test_correspondence_sparse_patchmatch(fh):
    """8 x 8: the coarse start; 6 x 6: the random start.  Same keys and shapes as the dense selector, indices in range, weights that sum
    to one, gradients at theta and phi; the warp is K42's on the returned candidates (its own tests judge its values)"""
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse
    g = _gen(40 + fh)
    theta = torch.randn(2, 256, fh, fh, generator=g).to(DEV).requires_grad_(True)
    phi = torch.randn(2, 256, fh, fh, generator=g).to(DEV).requires_grad_(True)
    ref_img = (torch.rand(2, 3, 4 * fh, 4 * fh, generator=g) * 2 - 1).to(DEV)
    onehot = lambda: torch.zeros(2, 5, 4 * fh, 4 * fh).scatter_(1, torch.randint(0, 5, (2, 1, 4 * fh, 4 * fh), generator=g), 1.0).to(DEV)
    seg, ref_seg = onehot(), onehot()
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4, warp_mask_losstype="direct")
    dense = correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, 0.01, 4)
    out = correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, 0.01, 4, search="patchmatch")
    assert set(out) == set(dense) and all(out[n].shape == dense[n].shape and out[n].dtype == dense[n].dtype for n in out)
    assert int(out["match_index"].min()) >= 0 and int(out["match_index"].max()) < fh * fh
    assert float(out["match_weight"].sum(1).sub(1).abs().max()) < 1e-5
    (out["warp_out"].square().sum() + out["warp_mask"].square().sum()).backward()
    for t in (theta, phi):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0
    again = correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, 0.01, 4, search="patchmatch")
    assert all(torch.equal(out[n], again[n]) for n in out)
    explicit = correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, 0.01, 4, search="dense")
    assert all(torch.equal(dense[n], explicit[n]) for n in dense)


def test_module_sparse_warp_patchmatch():
    """NoVGGCorrespondence.sparse_warp(search="patchmatch", topk=4) at a 64 x 64 crop (a 16 x 16 grid): the keys and shapes of the dense
    selector, indices in range, finite gradients at theta, phi and the exemplar image; search="dense" is the call without the argument,
    bit for bit"""
    from test_gpu_exemplar import _module_case
    net, ref_img, real, seg, ref_seg = _module_case("ade20k_options", 64, 2, 2, match_kernel=1)
    with torch.no_grad():
        omitted = net.sparse_warp(ref_img, real, seg, ref_seg, topk=4)
        dense = net.sparse_warp(ref_img, real, seg, ref_seg, topk=4, search="dense")
    assert set(omitted) == set(dense) and all(torch.equal(omitted[n], dense[n]) for n in dense)
    ref_img = ref_img.clone().requires_grad_(True)
    out = net.sparse_warp(ref_img, real, seg, ref_seg, topk=4, search="patchmatch")
    assert set(out) == set(dense) and all(out[n].shape == dense[n].shape and out[n].dtype == dense[n].dtype for n in out)
    assert out["match_index"].shape == (2, 4, 16, 16) and int(out["match_index"].min()) >= 0 and int(out["match_index"].max()) < 256
    assert all(bool(torch.isfinite(out[n]).all()) for n in ("warp_out", "warp_mask", "match_weight"))
    (out["warp_out"].square().sum() + out["warp_mask"].square().sum()).backward()
    for t in (net.theta.weight, net.phi.weight, ref_img):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- red zones
# The case joins tests/test_gpu_red_zones.py's table at import time, as tests/test_gpu_sparse_warp.py's does.
def _rz_patchmatch(c):
    from cocosnet_amd import ops
    q, k = c.data(rz.unit(2, 256, 35, 51)), c.data(rz.unit(2, 256, 18, 52))
    idx = torch.randint(-2, 21, (2, 35, 3), generator=torch.Generator().manual_seed(53))      # odd sizes, out-of-range entries
    grids = ((5, 7), (3, 6))
    first = ops.patchmatch_step(q, k, c.data(idx), grids, 100.0, 3, 1, 2, 3, 0, 0)
    second = ops.patchmatch_step(q, k, None, grids, 100.0, 3, 2, 1, 1, 0, 1)
    return [*first, *second]


RZ_CASES = {"patchmatch_step-2x5x7-3x6-k3": _rz_patchmatch}
for _name, _body in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_step_inside_red_zones(name, monkeypatch):
    """two steps (a table with out-of-range entries, the random initialisation) under tests/guarded_alloc.guarded: no guard byte changes,
    every returned score is finite (a read outside a buffer, or of one nobody wrote, carries the guard's NaN)"""
    rz.test_red_zones(name, monkeypatch)
    assert "cocos_patchmatch_step_f16x3" in set(rz.COVERAGE[name][0])
