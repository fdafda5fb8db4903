"""K44 on the GPU: ops.match_refine, ops.gather_patches_subcell, hot_path.correspondence_match(refine=r) and
NoVGGCorrespondence.match(refine=r).

The reference is tests/match_refine_case.py: window membership, window softmax, expected offset and bilinear gather restated in fp64
numpy, the scores from the values of the operand planes the kernel reads (tests/patchmatch_case.plane_values).  Bounds:
    lse_win   2e-4 inv_t: the score bound of the split-precision kernels (tests/test_gpu_parity.OUT_TOL; |<q, k>| <= 1, so inv_t is the
              scale of the logits)
    off       2 r (2e-4 inv_t): a softmax moves by at most twice a uniform bound on its logits' error, times the largest |dx|
    gather    1e-6 of max |reference|: three fp32 lerps of O(1) values

This file sorts before tests/test_gpu_red_zones.py: its red-zone cases (below) have run when that file's "every entry point was reached"
audit counts the `cocos_match_refine_f16x3` and `cocos_gather_patches_subcell` literals of cocosnet_amd/ops.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_refine_case as mc  # noqa: E402
import patchmatch_case as pc  # noqa: E402
import test_gpu_red_zones as rz  # noqa: E402
from test_gpu_parity import OUT_TOL, rel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
B = 2
QGRID = (5, 7)
NQ = QGRID[0] * QGRID[1]
KGRIDS = [(3, 6), (8, 8)]


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
    """(qn, kn, planes, qv, kv, idx): unit-norm columns on the device — every key a noisy copy of some query, so the scores of a window
    spread from near inv_t down to noise — their operand planes, the fp64 values of those planes and the centre table: random keys,
    the four corners, edges, the interior and out-of-range entries.  Made once per key grid, never written."""
    from cocosnet_amd import ops
    if kgrid not in _CASES:
        hk, wk = kgrid
        Nk = hk * wk
        g = _gen(200 + Nk)
        q = _unit(torch.randn(B, 256, NQ, generator=g))
        src = torch.randint(0, NQ, (B, Nk), generator=g)
        noise = torch.rand(B, 1, Nk, generator=g) * 2.0
        k = _unit(torch.stack([q[b][:, src[b]] for b in range(B)]) + noise * torch.randn(B, 256, Nk, generator=g) / 16.0)
        q, k = q.to(DEV), k.to(DEV)
        planes = ops.OperandPlanes()
        with torch.no_grad():
            qv = pc.plane_values(*planes.get(q, True, ops.SPLIT_OPERAND_SCALE), ops.SPLIT_OPERAND_SCALE)
            kv = pc.plane_values(*planes.get(k, True, ops.SPLIT_OPERAND_SCALE), ops.SPLIT_OPERAND_SCALE)
        idx = torch.randint(0, Nk, (B, NQ), generator=g)
        fixed = [0, wk - 1, Nk - wk, Nk - 1,                        # the corners
                 wk // 2, Nk - 1 - wk // 2, wk, 2 * wk - 1,         # the four edges
                 wk + 1, (hk // 2) * wk + wk // 2,                  # the interior
                 -1, Nk, 10 ** 9, -(2 ** 31)]                       # out of range: clamped
        idx[0, :len(fixed)] = torch.tensor(fixed)
        idx[1, NQ - len(fixed):] = torch.tensor(fixed)
        _CASES[kgrid] = (q, k, planes, qv, kv, idx)
    return _CASES[kgrid]


# ---------------------------------------------------------------------------------------------------------------- the refinement
@pytest.mark.parametrize("inv_t", [10.0, 100.0])
@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("kgrid", KGRIDS)
def test_refine_against_the_restatement(kgrid, r, inv_t):
    from cocosnet_amd import ops
    qn, kn, planes, qv, kv, idx = _case(kgrid)
    off, lse = ops.match_refine(qn, kn, idx.to(DEV), kgrid, inv_t, r, planes)
    assert off.shape == (B, NQ, 2) and lse.shape == (B, NQ) and off.dtype == lse.dtype == torch.float32
    want_off, want_lse = mc.refine(qv, kv, idx.numpy(), kgrid, r, inv_t)
    off, lse = off.double().cpu().numpy(), lse.double().cpu().numpy()
    e_lse, e_off = np.abs(lse - want_lse).max(), np.abs(off - want_off).max()
    tol = OUT_TOL * inv_t
    print(f"[match_refine] key {kgrid} r={r} inv_t={inv_t:g}: max |lse_win - fp64| {e_lse:.3e} (bound {tol:.1e})  "
          f"max |off - fp64| {e_off:.3e} (bound {2 * r * tol:.1e})  max |off| {np.abs(off).max():.3f}")
    assert np.isfinite(off).all() and np.isfinite(lse).all()
    assert e_lse <= tol, (kgrid, r, inv_t, e_lse)
    assert e_off <= 2 * r * tol, (kgrid, r, inv_t, e_off)
    assert np.abs(off).max() <= r
    # a window cut by the border cannot point across it: the corner (0, 0) has no negative offset, the corner (hk - 1, wk - 1) no positive one
    assert (off[0, 0] >= 0).all() and (off[0, 3] <= 0).all()
    int32 = ops.match_refine(qn, kn, idx.clamp(-(2 ** 31), 2 ** 31 - 1).to(torch.int32).to(DEV), kgrid, inv_t, r, planes)
    assert np.array_equal(int32[0].double().cpu().numpy(), off) and np.array_equal(int32[1].double().cpu().numpy(), lse)


@pytest.mark.parametrize("kgrid", KGRIDS)
def test_window_scores_are_the_scores_of_the_match_family(kgrid):
    """inv_t = 100, the 3 x 3 window: the nine scores come from ops.patchmatch_step (k = 1, no neighbour inside the query grid at
    stride 2^20, no search: the pool of a query is its one candidate, val the logit of that pair — K42's, bit for bit).  lse_win and
    off against the fp64 soft-argmax of those fp32 scores.  With equal score bits what is left is the window softmax's own rounding:
    below |lse| < 128 the final sum rounds by at most 2^-18 = 3.8e-6, the sum of at most 49 exponentials and its logarithm add less than
    64 eps = 7.6e-6 — bound 2e-5 on lse_win, and (as for the scores) 2 r times it on off."""
    from cocosnet_amd import ops
    hk, wk = kgrid
    qn, kn, planes, _, _, idx = _case(kgrid)
    inv_t, r = 100.0, 1
    centre = idx.clamp(0, hk * wk - 1)
    yk, xk = centre // wk, centre % wk
    scores, inside, dxs, dys = [], [], [], []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ok = (yk + dy >= 0) & (yk + dy < hk) & (xk + dx >= 0) & (xk + dx < wk)
            key = torch.where(ok, (yk + dy) * wk + xk + dx, centre)
            got, val = ops.patchmatch_step(qn, kn, key.reshape(B, NQ, 1).to(DEV), (QGRID, kgrid), inv_t, 1, 2 ** 20, 0, 0, 0, 0, planes)
            assert torch.equal(got.cpu().long().reshape(B, NQ), key)
            scores.append(val.reshape(B, NQ).double().cpu().numpy())
            inside.append(ok.numpy())
            dxs.append(dx)
            dys.append(dy)
    off, lse = (t.double().cpu().numpy() for t in ops.match_refine(qn, kn, idx.to(DEV), kgrid, inv_t, r, planes))
    scores, inside = np.stack(scores, axis=2), np.stack(inside, axis=2)
    e_lse = e_off = 0.0
    for b in range(B):
        for i in range(NQ):
            keep = inside[b, i]
            ox, oy, want = mc.softargmax(scores[b, i][keep], np.array(dxs)[keep], np.array(dys)[keep])
            e_lse = max(e_lse, abs(lse[b, i] - want))
            e_off = max(e_off, abs(off[b, i, 0] - ox), abs(off[b, i, 1] - oy))
    print(f"[match_refine] key {kgrid}: against the soft-argmax of patchmatch_step's scores: lse_win {e_lse:.3e} (bound 2e-5)  "
          f"off {e_off:.3e} (bound {2 * r * 2e-5:.0e})")
    assert np.abs(lse).max() < 128
    assert e_lse <= 2e-5 and e_off <= 2 * r * 2e-5


def test_two_runs_are_bitwise_equal():
    from cocosnet_amd import ops
    qn, kn, planes, _, _, idx = _case((8, 8))
    img = (torch.rand(B, 3, 16, 16, generator=_gen(8)) * 2 - 1).to(DEV)
    for r in (1, 3):
        a = ops.match_refine(qn, kn, idx.to(DEV), (8, 8), 100.0, r, planes)
        b = ops.match_refine(qn, kn, idx.to(DEV), (8, 8), 100.0, r)            # planes made again from the tensors
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
        wa, wb = (ops.gather_patches_subcell(img, idx.to(DEV), a[0], QGRID, (8, 8), 2) for _ in range(2))
        assert torch.equal(wa.view(torch.int32), wb.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- the gather
def _gather_inputs(kgrid, down, Be, seed):
    hk, wk = kgrid
    g = _gen(seed)
    img = torch.rand(Be, 3, hk * down, wk * down, generator=g) * 2 - 1
    idx = torch.randint(0, hk * wk, (B, NQ), generator=g)
    idx[0, 0], idx[0, 1], idx[1, 2], idx[1, 3], idx[1, 4], idx[0, NQ - 1] = -1, hk * wk, 10 ** 9, -(2 ** 31), 0, hk * wk - 1
    return img, idx, g


@pytest.mark.parametrize("Be", [B, 1])
@pytest.mark.parametrize("down", [2, 4])
def test_zero_offset_is_the_hard_warp(down, Be):
    """off == 0: gather_patches' copy, bit for bit (ops.gather_patches has one grid for both sides: 5 x 7 here)"""
    from cocosnet_amd import ops
    img, idx, _ = _gather_inputs(QGRID, down, Be, 30 + down)
    img, idx = img.to(DEV), idx.to(DEV)
    hard = ops.gather_patches(img, idx, *QGRID, down)
    sub = ops.gather_patches_subcell(img, idx, torch.zeros(B, NQ, 2, device=DEV), QGRID, QGRID, down)
    assert sub.shape == hard.shape == (B, 3, QGRID[0] * down, QGRID[1] * down)
    assert torch.equal(sub.view(torch.int32), hard.view(torch.int32))


@pytest.mark.parametrize("Be", [B, 1])
@pytest.mark.parametrize("down", [2, 4])
@pytest.mark.parametrize("kgrid", [(3, 6), (5, 7)])
def test_random_offsets_against_the_restatement(kgrid, down, Be):
    """C = 3, odd grids, offsets in (-3, 3), among them ones that leave the image (clamped): within 1e-6 of max |reference| — the
    kernel splits the sample position into an integer pixel and an exact fraction (off * down is exact for these power-of-two
    `down`), so what is left is the three fp32 lerps of O(1) values.  Any fp32 offset, and (an extra) the same offsets rounded to the
    2^-8 lattice."""
    from cocosnet_amd import ops
    img, idx, g = _gather_inputs(kgrid, down, Be, 40 + down + kgrid[0])
    anyoff = (torch.rand(B, NQ, 2, generator=g) * 2 - 1) * 2.99      # (the lattice rounds by at most 2^-9: still inside (-3, 3))
    lattice = torch.round(anyoff * 256) / 256
    for tag, off, tol in (("any fp32", anyoff, 1e-6), ("2^-8 lattice", lattice, 1e-6)):
        assert float(off.abs().max()) < 3
        out = ops.gather_patches_subcell(img.to(DEV), idx.to(DEV), off.to(DEV), QGRID, kgrid, down)
        want = mc.gather_subcell(img.numpy(), idx.numpy(), off.numpy(), QGRID, kgrid, down)
        err = rel(out, want)
        print(f"[gather_patches_subcell] key {kgrid} down={down} Be={Be} offsets {tag}: rel {err:.3e} (bound {tol:.0e})")
        assert out.shape == (B, 3, QGRID[0] * down, QGRID[1] * down) and err <= tol, (tag, err)


# ---------------------------------------------------------------------------------------------------------------- hot path and module
def test_module_match_refine():
    """NoVGGCorrespondence.match(refine=r) at a 64 x 64 crop (a 16 x 16 grid), B = 2: the new keys and their shapes, match_index and
    every other key of refine = 0 bit for bit, match_xy_sub - match_xy == match_offset, |match_offset| <= r, warp_sub next to an
    unchanged warp_hard, both directions, a refinement temperature of its own"""
    from test_gpu_exemplar import _module_case
    net, ref_img, _, seg, ref_seg = _module_case("ade20k_options", 64, 2, 2, match_kernel=1)
    base = net.match(ref_img, seg, ref_seg, hard_warp=True)
    assert not {"match_offset", "match_xy_sub", "match_window_prob", "warp_sub"} & set(base)
    explicit = net.match(ref_img, seg, ref_seg, hard_warp=True, refine=0)
    assert set(explicit) == set(base) and all(torch.equal(explicit[n], base[n]) for n in base)
    for r in (1, 2, 3):
        out = net.match(ref_img, seg, ref_seg, hard_warp=True, refine=r)
        assert set(out) == set(base) | {"match_offset", "match_xy_sub", "match_window_prob", "warp_sub"}
        assert all(torch.equal(out[n], base[n]) for n in base)                       # match_index, warp_hard, ...: untouched
        assert out["match_offset"].shape == out["match_xy_sub"].shape == (2, 2, 16, 16) and out["match_window_prob"].shape == (2, 16, 16)
        assert out["match_offset"].dtype == out["match_xy_sub"].dtype == torch.float32 and out["warp_sub"].shape == (2, 3, 64, 64)
        # match_xy_sub is match_xy + match_offset in fp32, bit for bit; taking match_xy off again returns match_offset up to the one
        # rounding of that sum: half an ulp of a position below 32 (16 cells + 3) = 2^-20
        assert torch.equal(out["match_xy_sub"], out["match_xy"].float() + out["match_offset"])
        assert float((out["match_xy_sub"] - out["match_xy"].float() - out["match_offset"]).abs().max()) <= 2.0 ** -20
        assert float(out["match_offset"].abs().max()) <= r and all(bool(torch.isfinite(out[n]).all()) for n in out)
        wp = out["match_window_prob"]
        # the window holds the match and no more than everything; the readout (K36a) and the window (K44) form their logits in
        # different arithmetic, each within OUT_TOL inv_t of the true one: a factor exp(2 OUT_TOL inv_t) between the two
        slack = float(np.exp(2 * OUT_TOL * 100.0))
        assert bool((wp * slack >= out["match_prob"]).all()) and float(wp.max()) <= slack
        assert float(out["warp_sub"].abs().max()) <= float(ref_img.abs().max()) * (1 + 1e-6)      # a convex combination of exemplar pixels
        assert not torch.equal(out["warp_sub"], out["warp_hard"])
    cols0 = net.match(ref_img, seg, ref_seg, direction="cols")
    cols = net.match(ref_img, seg, ref_seg, direction="cols", refine=1)
    assert all(torch.equal(cols[n], cols0[n]) for n in cols0) and "warp_sub" not in cols
    assert cols["match_offset"].shape == (2, 2, 16, 16) and float(cols["match_offset"].abs().max()) <= 1
    assert not torch.equal(cols["match_offset"], out["match_offset"])
    # the operands are exchanged: the window around an exemplar position's best content position holds that match, scored from the
    # exemplar position's side (with the content positions asking, the centre's score would be another pair's)
    assert bool((cols["match_window_prob"] * slack >= cols["match_prob"]).all()) and float(cols["match_window_prob"].max()) <= slack
    sharp = net.match(ref_img, seg, ref_seg, refine=1, refine_temperature=1e-4)      # a window softmax that is nearly hard
    soft = net.match(ref_img, seg, ref_seg, refine=1, refine_temperature=0.01)
    one = net.match(ref_img, seg, ref_seg, refine=1)
    assert torch.equal(soft["match_offset"], one["match_offset"]) and torch.equal(soft["match_window_prob"], one["match_window_prob"])
    assert float(sharp["match_offset"].abs().mean()) < float(soft["match_offset"].abs().mean())


def test_hot_path_refusals_that_need_the_tensors():
    """an exemplar grid the fused readout does not take (Nk % 4 != 0): refine > 0 is refused, nothing falls back"""
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match
    g = _gen(60)
    theta, phi = torch.randn(2, 256, 4, 4, generator=g).to(DEV), torch.randn(2, 256, 3, 3, generator=g).to(DEV)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    with pytest.raises(ValueError, match="refine=1"):
        correspondence_match(theta, phi, cfg, refine=1)


# ---------------------------------------------------------------------------------------------------------------- red zones
# The cases join tests/test_gpu_red_zones.py's table at import time, as tests/test_gpu_patchmatch.py's does.
def _rz_table(seed):
    return torch.randint(-2, 21, (2, 35), generator=torch.Generator().manual_seed(seed))      # 18 keys: out-of-range entries on both sides


def _rz_match_refine(c):
    from cocosnet_amd import ops
    q, k = c.data(rz.unit(2, 256, 35, 61)), c.data(rz.unit(2, 256, 18, 62))
    return [*ops.match_refine(q, k, c.data(_rz_table(63)), (3, 6), 100.0, 2)]


def _rz_gather_subcell(c):
    from cocosnet_amd import ops
    img, off = c.data(rz.uni(2, 3, 6, 12, seed=64)), c.data(rz.uni(2, 35, 2, seed=65) * 2.5)
    return ops.gather_patches_subcell(img, c.data(_rz_table(66)), off, (5, 7), (3, 6), 2)


RZ_CASES = {"match_refine-2x5x7-3x6-r2": (_rz_match_refine, "cocos_match_refine_f16x3"),
            "gather_patches_subcell-2x3x5x7-d2": (_rz_gather_subcell, "cocos_gather_patches_subcell")}
for _name, (_body, _) in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_inside_red_zones(name, monkeypatch):
    """both kernels on odd sizes with out-of-range centres under tests/guarded_alloc.guarded: no guard byte changes, every returned
    value is finite (a read outside a buffer, or of one nobody wrote, carries the guard's NaN)"""
    rz.test_red_zones(name, monkeypatch)
    assert RZ_CASES[name][1] in set(rz.COVERAGE[name][0])
