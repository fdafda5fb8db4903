"""K55 on the GPU: the label-restricted readout of the match_kernel-3 logits (ops.box3_topk_labelled, the LABELS instantiations of
box3_topk_kernel), hot_path.correspondence_match_box3 / correspondence_sparse_box3(restrict=) and the module's match_box3 /
sparse_warp_box3(restrict=).

Arbiter: the fp64 box logit matrix of tests/test_gpu_match_box3.py (`_case` / `_arbiter`), masked with match_labels_case.allowed and
judged with that file's rule under its bound TOL = 4 * E_BOX (imported).  Ranks a row cannot fill (fewer than k allowed keys) are judged
on their own: val = -inf exactly, the index in range, lse over what is allowed (-inf for an empty row).

(The file name sorts before test_gpu_red_zones.py: its red-zone case is registered before that file's audit counts the entry points.)"""
import gc
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_labels_case as lc  # noqa: E402
import test_gpu_match_box3 as mb  # noqa: E402
import test_gpu_match_box3_topk as mtk  # noqa: E402
import test_gpu_red_zones as rz  # noqa: E402
from test_gpu_match_box3 import DEV, INV_T, KC, TOL, _block, _case  # noqa: E402

pytestmark = pytest.mark.gpu
ENTRY = "cocos_box3_topk_labels_f16x3"
NEG_INF = float("-inf")
GRIDS = [(4, 64, 2), (2, 128, 2), (40, 128, 1)]      # the two tile widths at 256 positions; 5120 keys: the chunk ring, both boundaries
GRID_IDS = [f"{h}x{w}" for h, w, _ in GRIDS]
GRID = dict(argnames="h,w,B", argvalues=GRIDS, ids=GRID_IDS)
DIRS = dict(argnames="transposed", argvalues=[False, True], ids=["rows", "transposed"])
LOW = -128 * math.log(2)      # a natural-unit logit below this has a reference under -128 in log2 units: 2^(0 - r) overflows


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def _labelled(opnd, ql, kl, h, w, k, transposed):
    """ql / kl: the labels of the PROBLEM's queries and keys (after the exchange when transposed)"""
    from cocosnet_amd import ops
    t, mu, a, nu, b = opnd
    if transposed:
        mu, a, nu, b = nu, b, mu, a
    return ops.box3_topk_labelled(t, mu, a, nu, b, ql.to(DEV), kl.to(DEV), h, w, KC, INV_T, k, transposed=transposed)


def _plain(opnd, h, w, k, transposed):
    from cocosnet_amd import ops
    t, mu, a, nu, b = opnd
    if transposed:
        mu, a, nu, b = nu, b, mu, a
    return ops.box3_topk(t, mu, a, nu, b, h, w, KC, INV_T, k, transposed=transposed)


def _directed(L, transposed):
    return L.transpose(1, 2) if transposed else L


def _mask(L, ql, kl):
    return L.masked_fill(~lc.allowed(ql.to(L.device), kl.to(L.device)), NEG_INF)


def _judge(tag, idx, val, lse, Lm, exact_idx=False):
    """every row of (idx [B,N,k] int32, val, lse) against the masked fp64 matrix Lm [B,N,Nk] under test_gpu_match_box3's rule and TOL:
    the picked entry as good as the arbiter's rank, val the picked entry, lse the masked log-sum-exp; short rows on their own"""
    Nk, k = Lm.shape[-1], idx.shape[-1]
    assert idx.dtype == torch.int32 and val.dtype == lse.dtype == torch.float32, tag
    assert idx.shape == val.shape == Lm.shape[:-1] + (k,) and lse.shape == Lm.shape[:-1], tag
    assert not bool(torch.isnan(val).any()) and not bool(torch.isnan(lse).any()), f"{tag}: NaN"
    assert int(idx.min()) >= 0 and int(idx.max()) < Nk, (tag, int(idx.min()), int(idx.max()))
    n_allowed = torch.isfinite(Lm).sum(-1)
    full = torch.arange(k, device=Lm.device).expand_as(idx) < n_allowed.unsqueeze(-1)
    a_idx, want = lc.topk_by_value_then_index(Lm, k)
    picked = Lm.gather(-1, idx.long())
    assert bool(torch.isfinite(picked[full]).all()), f"{tag}: a disallowed key was returned"
    assert bool(torch.isfinite(val[full]).all()), f"{tag}: val is not finite on a rank the row can fill"
    assert bool((val[~full] == NEG_INF).all()), f"{tag}: a rank beyond the allowed keys does not hold -inf"
    srt = torch.where(full, idx.long(), Nk + torch.arange(k, device=Lm.device).expand_as(idx)).sort(-1).values
    assert bool((srt[..., 1:] != srt[..., :-1]).all()), f"{tag}: a row returns one key twice"
    assert bool((val[..., :-1] >= val[..., 1:]).all()), f"{tag}: val is not non-increasing"
    has = n_allowed > 0
    assert bool((lse[~has] == NEG_INF).all()), f"{tag}: an empty row's lse is not -inf"
    assert bool(torch.isfinite(lse[has]).all()), f"{tag}: lse is not finite on a row with an allowed key"
    z = lambda x: x.abs().max().item() if x.numel() else 0.0
    e_val = z((val.double() - picked)[full])
    e_pick = (want - picked)[full].max().item() if bool(full.any()) else 0.0
    e_lse = z((lse.double() - lc.logsumexp(Lm))[has])
    print(f"[box3-labels] {tag}: |val - L[idx]| = {e_val:.3e}  max_r sort(L)[r] - L[idx[r]] = {e_pick:.3e}  |lse - logsumexp L| = {e_lse:.3e}  "
          f"(tol {TOL:.2e}; short rows {int((n_allowed < k).sum())}, empty {int((~has).sum())})")
    assert e_val <= TOL, (tag, e_val)
    assert e_pick <= TOL, (tag, e_pick)
    assert e_lse <= TOL, (tag, e_lse)
    if exact_idx:
        assert torch.equal(idx.long()[full], a_idx[full]), f"{tag}: idx is not the arbiter's (value descending, index ascending)"


def _rand_labels(B, N, classes, seed):
    return torch.randint(0, classes, (B, N), generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------- A: bitwise identity
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize(**DIRS)
@pytest.mark.parametrize(**GRID)
def test_nothing_restricted_is_the_unlabelled_entry_bitwise(h, w, B, transposed, k):
    """every query label negative (whatever the keys carry), and one label everywhere: no select fires, so all three outputs are
    cocos_box3_topk_f16x3's bits (k = 1: cocos_box3_match_f16x3's)"""
    opnd, N = _case(h, w, B)[2], h * w
    want = _plain(opnd, h, w, k, transposed)
    neg = -1 - _rand_labels(B, N, 5, 1)
    one = torch.full((B, N), 3, dtype=torch.int64)
    for tag, ql, kl in (("negative", neg, _rand_labels(B, N, 3, 2)), ("one label int64", one, one), ("one label int32", one.int(), one.int())):
        got = _labelled(opnd, ql, kl, h, w, k, transposed)
        for x, y, what in zip(got, want, ("idx", "val", "lse")):
            assert torch.equal(x, y), f"{tag}: {what} differs from cocos_box3_topk_f16x3"
    if k == 1:
        i1, m1, l1 = mb._match(opnd, h, w, transposed)
        assert torch.equal(got[0][..., 0], i1) and torch.equal(got[1][..., 0], m1) and torch.equal(got[2], l1)


# ---------------------------------------------------------------------------------------------------------------- B: random labels
_MASKED = {}


def _masked_case(h, w, B, transposed):
    """(ql, kl, masked L as the direction sees it): made once per grid and direction, never written"""
    key = (h, w, transposed)
    if key not in _MASKED:
        N = h * w
        ql, kl = _rand_labels(B, N, 3, 10 * h + transposed), _rand_labels(B, N, 3, 10 * h + 5 + transposed)
        _MASKED[key] = (ql, kl, _mask(_directed(_case(h, w, B)[3], transposed), ql, kl))
    return _MASKED[key]


@pytest.mark.parametrize("k", [1, 2, 3, 4, 8])
@pytest.mark.parametrize(**DIRS)
@pytest.mark.parametrize(**GRID)
def test_random_labels_every_query(h, w, B, transposed, k):
    opnd = _case(h, w, B)[2]
    ql, kl, Lm = _masked_case(h, w, B, transposed)
    _judge(f"random labels ({h},{w}) {'transposed' if transposed else 'rows'} k={k}", *_labelled(opnd, ql, kl, h, w, k, transposed), Lm)


# ---------------------------------------------------------------------------------------------------------------- C: rows that start low
def _low_case(h, w, B):
    """a synthetic blocked T with a = b = 1, mu = nu = 0: the box logit is 100 * ybox(M).  M is non-zero only for (key in the LAST grid
    row, query in the FIRST): there the y box has one term, -(0.9296875 + j / 1024), j in 0..15 — exact in fp32, logits in
    [-94.5, -92.9] — and every other logit is 0.  -> (M [B,key,query], z64 [B,query,key])"""
    N = h * w
    g = torch.Generator().manual_seed(55 + h)
    M = torch.zeros(B, N, N)
    M[:, N - w:, :w] = -(0.9296875 + torch.randint(0, 16, (B, w, w), generator=g) / 1024.0)
    M = M.to(DEV)
    zero, one = torch.zeros(B, N, device=DEV), torch.ones(B, N, device=DEV)
    return M, mtk._z64(M, zero, one, zero, one, w), (zero, one, zero, one)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("half", [None, 0, 1], ids=["both-halves", "half0", "half1"])
@pytest.mark.parametrize(**DIRS)
@pytest.mark.parametrize(**GRID)
def test_masked_rows_whose_first_allowed_logit_lies_below_the_overflow_line(h, w, B, transposed, half, k):
    """The queries of the first grid row carry label 1; label 1 on the keys sits in the last grid row only, so every 32-key tile in
    front of it is FULLY masked for them and the first maximum they meet is below -128 in log2 units (their foreign keys have the
    logit 0: a leaked mask would win every rank).  `half` None: both half-waves hold allowed keys — the rescale at the first move of
    the maximum, in the tile loop.  `half` = 0 / 1: the allowed keys are 8g + 4*half + e of those tiles only, so the other half-wave
    ends with m = -inf, l = 0 — the two exponents of the half-wave merge.  Every other query carries label 0 and ranges over the
    ordinary keys."""
    from cocosnet_amd import ops
    N = h * w
    M, z, (zero, one, _, _) = _low_case(h, w, B)
    ql = torch.zeros(B, N, dtype=torch.int64)
    ql[:, :w] = 1
    kl = torch.zeros(B, N, dtype=torch.int64)
    last = torch.arange(N - w, N)
    kl[:, last] = 1 if half is None else torch.where(((last >> 2) & 1) == half, 1, 2)
    Lm = _mask(z, ql, kl)
    planted = Lm[:, :w]
    assert bool(torch.isfinite(planted).any(-1).all()) and planted[torch.isfinite(planted)].max().item() < LOW, "the plant is not low enough"
    assert int(torch.isfinite(planted[:, :, :N - w]).sum()) == 0      # no allowed key in an earlier tile, in either half-wave
    t = _block(M.transpose(1, 2).contiguous() if transposed else M)
    got = ops.box3_topk_labelled(t, zero, one, zero, one, ql.to(DEV), kl.to(DEV), h, w, KC, INV_T, k, transposed=transposed)
    assert bool(torch.isfinite(got[2][:, :w]).all()) and bool(torch.isfinite(got[1][:, :w]).all())
    _judge(f"low start ({h},{w}) {'transposed' if transposed else 'rows'} half={half} k={k}", *got, Lm)


# ---------------------------------------------------------------------------------------------------------------- D: positions
def _position_sets(N):
    keys = torch.arange(N)
    sets = {"first-tile": keys < 32, "last-four": keys >= N - 4, "half0-of-every-tile": ((keys >> 2) & 1) == 0,
            "half1-of-every-tile": ((keys >> 2) & 1) == 1}
    if N > 4096:
        sets["second-chunk"] = (keys >= 2048) & (keys < 4096)
    return sets


@pytest.mark.parametrize(**DIRS)
@pytest.mark.parametrize(**GRID)
def test_allowed_keys_in_chosen_positions(h, w, B, transposed):
    """label 1 on every query; on the keys only in the first tile / the last four keys / one half-wave's keys of every tile / the
    second chunk of the ring"""
    opnd, N = _case(h, w, B)[2], h * w
    L = _directed(_case(h, w, B)[3], transposed)
    ql = torch.ones(B, N, dtype=torch.int32)
    for name, where in _position_sets(N).items():
        kl = where.to(torch.int32).expand(B, N).contiguous()
        _judge(f"{name} ({h},{w}) {'transposed' if transposed else 'rows'}", *_labelled(opnd, ql, kl, h, w, 4, transposed), _mask(L, ql, kl))


# ---------------------------------------------------------------------------------------------------------------- E: short rows
@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize(**DIRS)
@pytest.mark.parametrize("h,w,B", [GRIDS[0], GRIDS[2]], ids=[GRID_IDS[0], GRID_IDS[2]])
def test_rows_with_exactly_k_fewer_than_k_and_no_allowed_keys(h, w, B, transposed, k):
    """label 5 sits on exactly k keys, label 6 on k - 1, label 7 on none (and label 8 is out of int32's range before the clamp)"""
    opnd, N = _case(h, w, B)[2], h * w
    g = torch.Generator().manual_seed(77 + k)
    kl = torch.zeros(B, N, dtype=torch.int64)
    for b in range(B):
        at = torch.randperm(N, generator=g)
        kl[b, at[:k]] = 5
        kl[b, at[k:2 * k - 1]] = 6
    ql = torch.tensor([5, 6, 7, 0, 2 ** 40], dtype=torch.int64)[torch.randint(0, 5, (B, N), generator=g)]
    got = _labelled(opnd, ql, kl, h, w, k, transposed)
    Lm = _mask(_directed(_case(h, w, B)[3], transposed), ql, kl)
    empty = (ql.to(DEV) == 7) | (ql.to(DEV) == 2 ** 40) | ((ql.to(DEV) == 6) & (k == 1))
    assert bool((got[2][empty] == NEG_INF).all()) and bool((got[1][empty] == NEG_INF).all()) and int(empty.sum()) > 0
    _judge(f"short rows ({h},{w}) {'transposed' if transposed else 'rows'} k={k}", *got, Lm)


# ---------------------------------------------------------------------------------------------------------------- F: ties
SPARSE = {256: [5, 31, 32, 36, 127, 128, 200, 255], 5120: [5, 2047, 2048, 2052, 4095, 4096, 5000, 5119]}


@pytest.mark.parametrize(**DIRS)
@pytest.mark.parametrize("h,w", [(4, 64), (40, 128)], ids=["4x64", "40x128"])
def test_equal_logits_under_one_label_resolve_to_the_lower_index(h, w, transposed):
    """T = 0, mu = nu = 0: every logit is 0.  Key labels q % 3, except eight scattered keys (both sides of every tile, half-wave and
    chunk boundary) with label 200: a query returns the k lowest indices of ITS label — through the register scan, the tile loop,
    the half-wave merge and across chunks — and never an equal logit under a foreign label"""
    from cocosnet_amd import ops
    B, N = 1, h * w
    z, one = torch.zeros(B, N, device=DEV), torch.ones(B, N, device=DEV)
    kl = (torch.arange(N) % 3).expand(B, N).clone()
    kl[:, SPARSE[N]] = 200
    ql = torch.tensor([0, 1, 2, 200])[_rand_labels(B, N, 4, 3)]
    t = torch.zeros(B * N * N, device=DEV)
    Lm = _mask(torch.zeros(B, N, N, dtype=torch.float64, device=DEV), ql, kl)
    for k in (1, 4, 8):
        idx, val, lse = ops.box3_topk_labelled(t, z, one, z, one, ql.to(DEV), kl.to(DEV), h, w, KC, INV_T, k, transposed=transposed)
        assert bool((val == 0).all())
        _judge(f"ties ({h},{w}) {'transposed' if transposed else 'rows'} k={k}", idx, val, lse, Lm, exact_idx=True)
    rows200 = (ql == 200)[0].nonzero()[:, 0].to(DEV)
    assert idx[0, rows200].long().tolist() == [SPARSE[N]] * len(rows200)


# ---------------------------------------------------------------------------------------------------------------- G: hot path, module
def _blocky_seg(B, nc, crop, cell, seed, absent=(), rare=None):
    """one-hot [B,nc,crop,crop] of `cell`-pixel blocks of random classes; `absent` classes never occur, `rare` occurs in two cells"""
    g = torch.Generator().manual_seed(seed)
    n = crop // cell
    pool = torch.tensor([c for c in range(nc) if c not in absent and c != rare])
    lab = pool[torch.randint(0, len(pool), (B, n, n), generator=g)]
    lab = lab.repeat_interleave(cell, 1).repeat_interleave(cell, 2)
    if rare is not None:
        lab[:, :4, :8] = rare      # two 4 x 4 feature cells at down = 4
    return torch.zeros(B, nc, crop, crop).scatter_(1, lab.unsqueeze(1), 1.0).to(DEV)


_MODULE = {}


def _module():
    """crop 256 at down 4: a 64 x 64 grid, B = 2, 7 classes in blocks of 32 pixels; class 6 is rare on the exemplar (two cells: fewer
    than topk = 4) and class 5 absent from it; made once, never written"""
    if not _MODULE:
        from test_gpu_exemplar import _module_case
        net, ref_img, real, _, _ = _module_case("ade20k_options", 256, 2, 2, match_kernel=3)
        seg = _blocky_seg(2, 7, 256, 32, 551)
        ref_seg = _blocky_seg(2, 7, 256, 32, 552, absent=(5,), rare=6)
        with torch.no_grad():
            corr = net(ref_img, real, seg, ref_seg, return_corr=True).double()
        _MODULE["case"] = (net, ref_img, real, seg, ref_seg, corr)
    return _MODULE["case"]


def _as_rows(out, k):
    """(idx int32 [B,N,k], val [B,N,k], lse [B,N]) of a module result; val = lse + log prob"""
    B = out["match_lse"].shape[0]
    lse = out["match_lse"].reshape(B, -1)
    idx, prob = out["match_index"], out["match_prob"]
    if k == 1:
        idx, prob = idx.unsqueeze(1), prob.unsqueeze(1)
    idx, prob = (x.reshape(B, k, -1).permute(0, 2, 1).contiguous() for x in (idx, prob))
    return idx.to(torch.int32), prob, lse


def _judge_module(tag, out, corr, q_eff, kl, k):
    """index and lse under _judge's rule; prob = exp(logit - lse) under test_gpu_match_box3's prob bound"""
    idx, prob, lse = _as_rows(out, k)
    Lm = _mask(corr, q_eff, kl)
    picked = Lm.gather(-1, idx.long())
    want = Lm.topk(k, dim=-1).values
    assert bool(torch.isfinite(picked).all()), f"{tag}: a disallowed position was returned"
    e_pick = (want - picked).max().item()
    e_lse = (lse.double() - lc.logsumexp(Lm)).abs().max().item()
    e_p = ((prob.double() - torch.exp(picked - lc.logsumexp(Lm).unsqueeze(-1))).abs() / torch.exp(picked - lc.logsumexp(Lm).unsqueeze(-1))).max().item()
    print(f"[box3-labels] {tag}: max_r sort(L)[r] - L[idx[r]] = {e_pick:.3e}  |lse - logsumexp| = {e_lse:.3e}  rel |prob| = {e_p:.3e}")
    assert e_pick <= TOL and e_lse <= TOL, (tag, e_pick, e_lse)
    assert e_p <= math.expm1(2 * TOL) + 4 * mb.FP32_EPS * (1 + corr.abs().max().item()), (tag, e_p)


@pytest.mark.parametrize("k", [1, 4])
def test_module_match_box3_against_the_masked_matrix(k):
    net, ref_img, real, seg, ref_seg, corr = _module()
    ql, kl = lc.cell_labels(seg, 4).reshape(2, -1), lc.cell_labels(ref_seg, 4).reshape(2, -1)
    rows = net.match_box3(ref_img, seg, ref_seg, topk=k, hard_warp=True)
    cols = net.match_box3(ref_img, seg, ref_seg, topk=k, direction="cols")
    assert set(rows) >= {"match_index", "match_xy", "match_prob", "match_lse", "match_restricted", "warp_hard"}
    assert rows["match_index"].shape == ((2, 64, 64) if k == 1 else (2, k, 64, 64)) and not any(v.requires_grad for v in rows.values())
    for tag, out, c, q, kk in (("rows", rows, corr, ql, kl), ("cols", cols, corr.transpose(1, 2), kl, ql)):
        eff, restricted = lc.fallback(q, kk, k)
        assert torch.equal(out["match_restricted"].reshape(2, -1).cpu(), restricted), tag
        _judge_module(f"module {tag} k={k}", out, c, eff.to(DEV), kk, k)
    restricted = rows["match_restricted"].reshape(2, -1)
    assert bool((ql[~restricted] == 5).logical_or(ql[~restricted] == 6).all()) and 0 < int((~restricted).sum()) < restricted.numel()
    if k == 4:      # the rare class has two cells: restricted at topk = 1, a fall-back at topk = 4
        assert not bool(restricted[ql == 6].any())
    first = rows["match_index"] if k == 1 else rows["match_index"][:, 0]
    assert torch.equal(rows["warp_hard"], mb._gather_reference(ref_img, first.reshape(2, -1), 64, 64, net.opt.down))
    if k > 1:
        assert "warp_topk" in rows and bool(torch.isfinite(rows["warp_topk"]).all())
    # an explicit pair: "the left half takes from the right half", any int64 ids, negative = unrestricted
    qp = torch.full((2, 64, 64), 7_000_000_000, dtype=torch.int64, device=DEV)
    qp[:, :, 40:] = -3
    kp = torch.full((2, 64, 64), 11, dtype=torch.int64, device=DEV)
    kp[:, :, 32:] = 7_000_000_000
    pair = net.match_box3(ref_img, seg, ref_seg, topk=k, restrict=(qp, kp))
    eff, restricted = lc.fallback(qp.reshape(2, -1), kp.reshape(2, -1), k)
    assert torch.equal(pair["match_restricted"].reshape(2, -1).cpu(), restricted)
    _judge_module(f"module pair k={k}", pair, corr, eff.to(DEV), kp.reshape(2, -1), k)
    picked_x = (pair["match_index"] % 64).reshape(2, -1, 64, 64)
    assert bool((picked_x[:, :, :, :40] >= 32).all())
    # restrict=None is match() bit for bit
    plain, same = net.match(ref_img, seg, ref_seg, topk=k, hard_warp=True), net.match_box3(ref_img, seg, ref_seg, topk=k, hard_warp=True, restrict=None)
    assert set(plain) == set(same) and all(torch.equal(plain[n], same[n]) for n in plain)


def test_hot_path_restrict_none_and_boxed_corr_method():
    from cocosnet_amd.hot_path import HotPathConfig, _BoxedCorr, correspondence_match, correspondence_match_box3, restrict_fallback
    h, w, B = 4, 64, 2
    theta, phi, opnd, _ = _case(h, w, B)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    for k in (1, 4):
        for direction in ("rows", "cols"):
            x = correspondence_match(theta, phi, cfg, 1.0 / INV_T, direction=direction, topk=k)
            y = correspondence_match_box3(theta, phi, cfg, 1.0 / INV_T, direction=direction, topk=k)
            assert type(x) is type(y) and all(torch.equal(getattr(x, n), getattr(y, n)) for n in ("index", "prob", "lse")) and y.restricted is None
    corr = _BoxedCorr(theta, phi, INV_T)
    ql, kl = _rand_labels(B, h * w, 3, 31).to(DEV), _rand_labels(B, h * w, 3, 32).to(DEV)
    for transposed in (False, True):
        q, kk = (kl, ql) if transposed else (ql, kl)
        got = corr.match_labelled(not transposed, q.int(), kk.int(), 4)
        assert all(torch.equal(a, b) for a, b in zip(got, _labelled(opnd, q, kk, h, w, 4, transposed)))
    # the function on a pair, both directions: the op on restrict_fallback's labels
    for direction, (q, kk) in (("rows", (ql, kl)), ("cols", (kl, ql))):
        m = correspondence_match_box3(theta, phi, cfg, 1.0 / INV_T, direction=direction, topk=4, restrict=(ql.reshape(B, h, w), kl.reshape(B, h, w)))
        q_eff, k_eff, restricted = restrict_fallback(q, kk, 4)
        idx, val, lse = _labelled(opnd, q_eff, k_eff, h, w, 4, direction == "cols")
        assert torch.equal(m.index, idx.long().permute(0, 2, 1).reshape(B, 4, h, w)) and torch.equal(m.lse.reshape(B, -1), lse)
        assert torch.equal(m.restricted.reshape(B, -1), restricted)


# ---------------------------------------------------------------------------------------------------------------- H: sparse warp
def _record_calls(monkeypatch):
    """the launch spy of tests/test_gpu_match_launch_trace.py: every entry point that goes through _lib.call, in order"""
    from cocosnet_amd import _lib
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


@pytest.mark.parametrize("h,w", [(4, 64), (2, 128)], ids=["4x64", "2x128"])
def test_sparse_box3_with_restrict_against_fp64(h, w, monkeypatch):
    """selection = correspondence_match_box3's restricted top-4; warp_out, warp_mask, the weights and the gradients to theta, phi and
    (through the op) the values against fp64 on those indices, under K51's bounds; restrict=None is the route as it was, outputs and
    launch sequence"""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match_box3, correspondence_sparse_box3
    from test_gpu_match_box3_sparse import GRAD_TOL, OUT_TOL, rel
    B, k, N = 2, 4, h * w
    theta0, phi0, _, _ = _case(h, w, B)
    g = torch.Generator().manual_seed(61 + h)
    ref_img = (torch.rand(B, 3, 4 * h, 4 * w, generator=g) * 2 - 1).to(DEV)
    seg, ref_seg = _blocky_seg(B, 7, 4 * w, 16, 70 + h)[:, :, :4 * h], _blocky_seg(B, 7, 4 * w, 16, 71 + h, absent=(5,))[:, :, :4 * h]
    seg, ref_seg = seg.contiguous(), ref_seg.contiguous()
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4, warp_mask_losstype="direct")
    theta, phi = theta0.clone().requires_grad_(True), phi0.clone().requires_grad_(True)
    out = correspondence_sparse_box3(theta, phi, ref_img, seg, ref_seg, cfg, 1.0 / INV_T, k, restrict="label")
    assert set(out) == {"warp_out", "warp_mask", "match_index", "match_weight", "match_restricted"}
    m = correspondence_match_box3(theta0, phi0, cfg, 1.0 / INV_T, topk=k, restrict="label", seg_map=seg, ref_seg_map=ref_seg)
    assert torch.equal(out["match_index"], m.index) and torch.equal(out["match_restricted"], m.restricted)
    assert out["match_restricted"].dtype == torch.bool and 0 < int(out["match_restricted"].sum())
    ql, kl = lc.cell_labels(seg, 4).reshape(B, -1), lc.cell_labels(ref_seg, 4).reshape(B, -1)
    idx = out["match_index"].permute(0, 2, 3, 1).reshape(B, N, k)
    same = kl.gather(1, idx.reshape(B, -1)).reshape(B, N, k) == ql.unsqueeze(-1)
    assert bool(same[out["match_restricted"].reshape(B, N)].all())
    gen = torch.Generator().manual_seed(5)
    g_out, g_mask = torch.randn(out["warp_out"].shape, generator=gen).to(DEV), torch.randn(out["warp_mask"].shape, generator=gen).to(DEV)
    ((out["warp_out"] * g_out).sum() + (out["warp_mask"] * g_mask).sum()).backward()
    th64, ph64 = theta0.double().requires_grad_(True), phi0.double().requires_grad_(True)
    vals = torch.cat([F.avg_pool2d(ref_img.double(), 4).reshape(B, 3, -1),
                      F.interpolate(ref_seg.double(), scale_factor=0.25, mode="nearest").reshape(B, ref_seg.shape[1], -1)], 1).requires_grad_(True)
    w64 = torch.softmax(mb._arbiter(th64, ph64).gather(2, idx), -1)
    picked = vals.gather(2, idx.reshape(B, 1, N * k).expand(-1, vals.shape[1], -1)).reshape(B, vals.shape[1], N, k)
    o = (picked * w64.unsqueeze(1)).sum(-1)
    warp_r = F.interpolate(o[:, :3].reshape(B, 3, h, w), scale_factor=4, mode="nearest")
    mask_r = o[:, 3:].reshape(B, -1, h, w)
    ((warp_r * g_out.double()).sum() + (mask_r * g_mask.double()).sum()).backward()
    errs = {"warp_out": rel(out["warp_out"], warp_r.detach().cpu().numpy()), "warp_mask": rel(out["warp_mask"], mask_r.detach().cpu().numpy()),
            "match_weight": rel(out["match_weight"].permute(0, 2, 3, 1).reshape(B, N, k), w64.detach().cpu().numpy()),
            "d theta": rel(theta.grad, th64.grad.cpu().numpy()), "d phi": rel(phi.grad, ph64.grad.cpu().numpy())}
    # the values' gradient: the op on the route's own indices (the route makes its values without a graph)
    with torch.no_grad():
        (mu, a), (nu, b) = ops.unfold3_stats(theta0, KC), ops.unfold3_stats(phi0, KC)
    v32 = vals.detach().float().contiguous().requires_grad_(True)
    o32 = ops.box3_sparse_softmax_warp(theta0, phi0, mu, a, nu, b, v32, idx, INV_T)
    g_o = torch.randn(o32.shape, generator=gen).to(DEV)
    (o32 * g_o).sum().backward()
    v64 = vals.detach().clone().requires_grad_(True)
    p64 = v64.gather(2, idx.reshape(B, 1, N * k).expand(-1, v64.shape[1], -1)).reshape(B, v64.shape[1], N, k)
    ((p64 * w64.detach().unsqueeze(1)).sum(-1) * g_o.double()).sum().backward()
    errs["d v"] = rel(v32.grad, v64.grad.cpu().numpy())
    print(f"[box3-labels] sparse_box3(restrict) ({h},{w}): " + "  ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    assert all(e < (GRAD_TOL if n.startswith("d ") else OUT_TOL) for n, e in errs.items()), errs
    # restrict=None: today's outputs and today's launch sequence
    names = _record_calls(monkeypatch)
    x = correspondence_sparse_box3(theta0, phi0, ref_img, seg, ref_seg, cfg, 1.0 / INV_T, k)
    first, n0 = list(names), len(names)
    y = correspondence_sparse_box3(theta0, phi0, ref_img, seg, ref_seg, cfg, 1.0 / INV_T, k, restrict=None)
    assert names[n0:] == first and ENTRY not in first and "cocos_box3_topk_f16x3" in first
    assert set(x) == set(y) and all(torch.equal(x[n], y[n]) for n in x)
    n1 = len(names)
    correspondence_sparse_box3(theta0, phi0, ref_img, seg, ref_seg, cfg, 1.0 / INV_T, k, restrict="label")
    assert names[n1:].count(ENTRY) == 1 and names[n1:].count("cocos_box3_corr_xbox_f16x3") == 1 and "cocos_box3_topk_f16x3" not in names[n1:]


def test_module_sparse_warp_box3_with_restrict():
    net, ref_img, real, seg, ref_seg, _ = _module()
    sp = net.sparse_warp_box3(ref_img, real, seg, ref_seg, topk=4, restrict="label")
    m = net.match_box3(ref_img, seg, ref_seg, topk=4)
    assert {"warp_out", "match_index", "match_weight", "match_restricted"} <= set(sp)
    assert torch.equal(sp["match_index"], m["match_index"]) and torch.equal(sp["match_restricted"], m["match_restricted"])
    assert float(sp["match_weight"].sum(1).sub(1).abs().max()) < 1e-5 and bool(torch.isfinite(sp["warp_out"]).all())
    sp["warp_out"].square().sum().backward()
    for p in (net.theta.weight, net.phi.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    net.zero_grad(set_to_none=True)


# ---------------------------------------------------------------------------------------------------------------- I: memory, reproducibility
def test_restricted_route_keeps_one_hw_by_hw_tensor_and_repeats_bitwise():
    """B = 1, 64 x 64: the peak above the live bytes is under twice one T (64 MiB: K54's margin), nothing HW x HW stays after return,
    and two runs agree bit for bit"""
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match_box3
    g = torch.Generator().manual_seed(9)
    theta = (torch.randn(1, 256, 64, 64, generator=g) + 0.1).to(DEV)
    phi = (0.3 * theta.cpu().roll((1, 7), (2, 3)) + torch.randn(1, 256, 64, 64, generator=g)).to(DEV)
    seg, ref_seg = _blocky_seg(1, 7, 256, 32, 91), _blocky_seg(1, 7, 256, 32, 92)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    kw = dict(topk=4, restrict="label", seg_map=seg, ref_seg_map=ref_seg)
    one_t = 4096 * 4096 * 4
    first = correspondence_match_box3(theta, phi, cfg, 0.01, **kw)      # (warm: the library's own lazily made buffers)
    rz._clear_pools()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = correspondence_match_box3(theta, phi, cfg, 0.01, **kw)
    torch.cuda.synchronize()
    held, peak = torch.cuda.memory_allocated() - before, torch.cuda.max_memory_allocated() - before
    print(f"[box3-labels] memory: peak above live {peak / 2**20:.1f} MiB (one T = {one_t / 2**20:.0f} MiB), held after return {held / 2**20:.2f} MiB")
    assert peak < 2 * one_t, peak
    assert held < one_t // 8, held
    for n in ("index", "prob", "logit", "lse", "restricted"):
        assert torch.equal(getattr(first, n), getattr(res, n)), n


# ---------------------------------------------------------------------------------------------------------------- J: guards
def test_labelled_readout_hands_over_live_buffers_only(monkeypatch):
    import test_gpu_live_buffers as lb
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match_box3
    h, w, B = 4, 64, 2
    theta, phi, opnd, _ = _case(h, w, B)
    ql, kl = _rand_labels(B, h * w, 3, 41), _rand_labels(B, h * w, 3, 42)
    guard = lb._Guard(monkeypatch)
    _labelled(opnd, ql, kl, h, w, 4, False)
    _labelled(opnd, kl, ql, h, w, 1, True)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    for direction in ("rows", "cols"):
        correspondence_match_box3(theta, phi, cfg, 0.01, direction=direction, topk=2, restrict=(ql.reshape(B, h, w).to(DEV), kl.reshape(B, h, w).to(DEV)))
    guard.check(4, 4 * 10)      # four labelled launches, ten device pointers each (and the route's own launches around them)


def _rz_box3_labels(c):
    """both directions of the labelled readout at k = 1, 3 and 8 with labels and outputs between red zones; the label VALUES are
    out-of-range and negative (they are compared, never used as an index)"""
    from cocosnet_amd import ops
    B, h, w = 2, 4, 64
    th = c.data(rz.rnd(B, 256, h, w, seed=81) + 0.15)
    ph = c.data(0.05 * rz.rnd(B, 256, h, w, seed=81).roll((1, 5), (2, 3)) + rz.rnd(B, 256, h, w, seed=82) - 0.1)
    g = torch.Generator().manual_seed(83)
    values = torch.tensor([2 ** 31 - 1, -(2 ** 31), -1, 1 << 20, 1 << 20, 99999], dtype=torch.int64)
    ql = c.data(values[torch.randint(0, 6, (B, h * w), generator=g)].to(torch.int32).to(DEV))
    kl = c.data(values[torch.randint(0, 6, (B, h * w), generator=g)].to(torch.int32).to(DEV))
    with torch.no_grad():
        (mu, a), (nu, b) = ops.unfold3_stats(th, KC), ops.unfold3_stats(ph, KC)
        t = ops.box3_corr_xbox(th, ph)
    out = []
    for k in (1, 3, 8):
        out += list(ops.box3_topk_labelled(t, mu, a, nu, b, ql, kl, h, w, KC, 100.0, k))
        out += list(ops.box3_topk_labelled(t, nu, b, mu, a, kl, ql, h, w, KC, 100.0, k, transposed=True))
    return out


RZ_CASES = {"box3_topk_labelled-2x4x64-k1+k3+k8+transposed": _rz_box3_labels}
for _name, _body in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_the_new_op_inside_red_zones(name, monkeypatch):
    rz.test_red_zones(name, monkeypatch)
    assert ENTRY in set(rz.COVERAGE[name][0])
