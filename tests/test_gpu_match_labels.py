"""K47 label-restricted match readout on the GPU: the LABELS instantiations of the fused scan (cocos_corr_topk_labels_f16x3),
`hot_path.correspondence_match / correspondence_sparse(restrict=...)` and `NoVGGCorrespondence.match / sparse_warp(restrict=...)`.

Arbiter: tests/match_labels_case.py — the fp64 matrix L = inv_t * qn^T kn with the disallowed entries -inf.  Tolerance and argument
are tests/test_gpu_match.py's and tests/test_gpu_match_topk.py's (INV_T, TOL and _judge imported, not restated): the mask changes no
logit, it only removes elements, so every allowed logit of the kernel is within its element error e <= TOL of the arbiter's and the
order-statistic argument holds among the allowed elements of a row.  _judge is run wherever every row holds at least k allowed keys (it
subtracts picked values, which must be finite); `_judge_masked` below states the same three conditions for rows of any length and adds
the row semantics of short and empty rows.  The file name sorts before test_gpu_red_zones.py: its red-zone case has run when that
file's "every entry point was reached" audit is collected."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_labels_case as lc  # noqa: E402
import test_gpu_match_topk as tt  # noqa: E402
import test_gpu_red_zones as rz  # noqa: E402
from test_gpu_match import DEV, FP32_EPS, INV_T, TOL, _gather_reference, _module, _planes, _randn, _unit  # noqa: E402
from test_gpu_match_topk import TIE_PAIRS, _distinct, _judge  # noqa: E402
from test_gpu_parity import GRAD_TOL, rel  # noqa: E402

pytestmark = pytest.mark.gpu
ENTRY = "cocos_corr_topk_labels_f16x3"
B = 2
SHAPES = [(36, 260), (132, 68), (36, 8)]      # four 64-key stages + a 4-key tail; two query blocks (the second partial), a stage + a tail; k = 8 = Nk
KS = [1, 2, 3, 4, 8]
NEG_INF = float("-inf")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


_CASES = {}


def _case(Nq, Nk):
    """(q [B,256,Nq], k [B,256,Nk]) unit-norm columns: made once per shape, shared by the tests, never written"""
    if (Nq, Nk) not in _CASES:
        _CASES[(Nq, Nk)] = (_unit(_randn(B, 256, Nq, seed=Nq)), _unit(_randn(B, 256, Nk, seed=1000 + Nk)))
    return _CASES[(Nq, Nk)]


def _i32(t):
    return t.to(device=DEV, dtype=torch.int32).contiguous()


def _labelled(q, k, ql, kl, shared, kk):
    from cocosnet_amd import ops
    return ops._corr_topk_labels_planes(*_planes(q), *_planes(k[:1].contiguous() if shared else k), _i32(ql), _i32(kl[:1] if shared else kl), INV_T, kk)


def _arbiter(q, k, ql, kl, shared):
    return lc.masked_logits(q, k[:1] if shared else k, ql.to(DEV), (kl[:1] if shared else kl).to(DEV), INV_T)


def _judge_masked(tag, idx, val, lse, L, ql=None, kl=None, check=True):
    """the row semantics of the issue on rows of any length, against the masked fp64 matrix L [B,Nq,Nk]; check=False (the tie cases, as
    tests/test_gpu_match_topk.py judges its own): semantics, range, order and distinctness, the three figures printed only"""
    Nk, k = L.shape[-1], idx.shape[-1]
    n_allowed = torch.isfinite(L).sum(-1)                                          # [B,Nq]
    rank = torch.arange(k, device=DEV).view(1, 1, k)
    have = rank < n_allowed.unsqueeze(-1)                                          # ranks that exist
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and idx.shape == val.shape == L.shape[:-1] + (k,), tag
    assert not bool(torch.isnan(val).any()) and not bool(torch.isnan(lse).any()), f"{tag}: NaN"
    assert int(idx.min()) >= 0 and int(idx.max()) < Nk, (tag, int(idx.min()), int(idx.max()))
    assert torch.equal(val == NEG_INF, ~have), f"{tag}: val is -inf on other ranks than the missing ones"
    assert torch.equal(lse == NEG_INF, n_allowed == 0), f"{tag}: lse is -inf on other rows than the empty ones"
    picked = L.gather(-1, idx.long())
    assert bool(torch.isfinite(picked[have]).all()), f"{tag}: a disallowed key was returned"
    want = L.sort(dim=-1, descending=True).values[..., :k]
    e_val = (val.double() - picked)[have].abs().max().item() if bool(have.any()) else 0.0
    e_pick = (want - picked)[have].max().item() if bool(have.any()) else 0.0
    rows = n_allowed > 0
    e_lse = (lse.double() - lc.logsumexp(L))[rows].abs().max().item() if bool(rows.any()) else 0.0
    print(f"[labels] {tag}: |val - L[idx]| = {e_val:.3e}  max_r sort(L)[r] - L[idx[r]] = {e_pick:.3e}  |lse - logsumexp L| = {e_lse:.3e}  "
          f"(tol {TOL:.1e}; rows short {int((n_allowed < k).sum())} empty {int((~rows).sum())})")
    # order and distinctness among the ranks that exist (a missing rank repeats a clamped index)
    a, b_ = val[..., :-1], val[..., 1:]
    ok = (a > b_) | ((a == b_) & (idx[..., :-1] < idx[..., 1:])) | ~have[..., 1:]
    assert bool(ok.all()), f"{tag}: val is not non-increasing with ascending indices among equals"
    spread = torch.where(have, idx.long(), Nk + rank.expand_as(idx))
    assert _distinct(spread), f"{tag}: a row returns one key twice"
    if check:
        assert e_val <= TOL and e_pick <= TOL and e_lse <= TOL, (tag, e_val, e_pick, e_lse)
    if ql is not None:      # every returned key of a restricted row carries the row's label
        got = (kl.to(DEV).expand(L.shape[0], -1) if kl.shape[0] == 1 else kl.to(DEV)).long().gather(1, idx.long().reshape(L.shape[0], -1)).reshape(idx.shape)
        q_ = ql.to(DEV).long().unsqueeze(-1)
        assert bool(((got == q_) | (q_ < 0) | ~have).all()), f"{tag}: k_label[idx] != q_label"
    if bool((n_allowed >= k).all()):      # every row is full: the imported conditions, word for word
        _judge(tag, idx, val, lse, L, check=check)


def _run(tag, Nq, Nk, k, shared, ql, kl):
    q, kn = _case(Nq, Nk)
    idx, val, lse = _labelled(q, kn, ql, kl, shared, k)
    _judge_masked(f"{tag} ({Nq},{Nk}) k={k} {'shared' if shared else 'dense'}", idx, val, lse, _arbiter(q, kn, ql, kl, shared), ql, kl[:1] if shared else kl)
    return idx, val, lse


GRID = dict(argnames="Nq,Nk,k,shared", argvalues=[(Nq, Nk, k, s) for Nq, Nk in SHAPES for k in KS for s in (False, True)],
            ids=[f"{Nq}x{Nk}-k{k}-{'shared' if s else 'dense'}" for Nq, Nk in SHAPES for k in KS for s in (False, True)])


# ---------------------------------------------------------------------------------------------------------------- pattern 1
@pytest.mark.parametrize(**GRID)
def test_nothing_restricted_is_the_unlabelled_kernel_bitwise(Nq, Nk, k, shared):
    from cocosnet_amd import ops
    q, kn = _case(Nq, Nk)
    want = ops._corr_topk_planes(*_planes(q), *_planes(kn[:1].contiguous() if shared else kn), INV_T, k)
    g = torch.Generator().manual_seed(Nq + Nk + k)
    one = (torch.full((B, Nq), 5), torch.full((B, Nk), 5))
    free = (torch.full((B, Nq), -1), torch.randint(-3, 4, (B, Nk), generator=g))
    neg = (torch.randint(-2 ** 31, 0, (B, Nq), generator=g), torch.randint(-3, 4, (B, Nk), generator=g))
    for name, (ql, kl) in (("one label", one), ("all queries -1", free), ("any negative query label", neg)):
        got = _labelled(q, kn, ql, kl, shared, k)
        for a, b_, what in zip(got, want, ("idx", "val", "lse")):
            assert torch.equal(a, b_), f"{name}: {what} differs from cocos_corr_topk_f16x3"


# ---------------------------------------------------------------------------------------------------------------- pattern 2
@pytest.mark.parametrize(**GRID)
def test_random_labels(Nq, Nk, k, shared):
    """three random labels, each with at least 8 keys (Nk = 8 has room for one such label)"""
    nlab = min(3, Nk // 8)
    g = torch.Generator().manual_seed(7 * Nq + Nk)
    kl = torch.randint(0, nlab, (B, Nk), generator=g)
    for b in range(B):
        kl[b, torch.randperm(Nk, generator=g)[:8 * nlab]] = torch.arange(nlab).repeat(8)      # at least 8 keys of every label
    ql = torch.randint(0, nlab, (B, Nq), generator=g)
    assert all(int((kl[b] == lab).sum()) >= 8 for b in range(B) for lab in range(nlab))
    idx, _, _ = _run("random labels", Nq, Nk, k, shared, ql, kl)
    kls = (kl[:1].expand(B, -1) if shared else kl).to(DEV)
    assert torch.equal(kls.gather(1, idx.long().reshape(B, -1)).reshape(idx.shape), ql.to(DEV).unsqueeze(-1).expand_as(idx))


# ---------------------------------------------------------------------------------------------------------------- pattern 3
@pytest.mark.parametrize(**GRID)
def test_allowed_keys_in_the_first_stage_only_and_in_the_tail_only(Nq, Nk, k, shared):
    """even queries: label 1, whose keys lie in the first stage only — the state must survive the masked stages after it; odd queries:
    label 2, whose keys are the last four only — the state is (-inf, 0) through every stage before the last one, in wave group 0 and,
    for the whole scan, in wave group 1 and (Nk = 260) in both half-waves' merges.  Rows of label 2 are short when k = 8."""
    first = min(64, Nk - 4)
    kl = torch.zeros(B, Nk, dtype=torch.int64)
    kl[:, :first], kl[:, Nk - 4:] = 1, 2
    if Nk > 68:
        kl[:, 64:Nk - 4] = 3                      # a label nobody asks for
    ql = torch.ones(B, Nq, dtype=torch.int64)
    ql[:, 1::2] = 2
    idx, val, lse = _run("first stage / tail", Nq, Nk, k, shared, ql, kl)
    assert int(idx[:, 0::2].max()) < first and bool(torch.isfinite(lse).all())
    assert int(idx[:, 1::2, :min(k, 4)].min()) >= Nk - 4
    assert bool(torch.isfinite(val[:, 0::2]).all()) == (k <= first)


# ---------------------------------------------------------------------------------------------------------------- pattern 4
@pytest.mark.parametrize(**GRID)
def test_half_of_a_wave_has_no_key_in_a_tile(Nq, Nk, k, shared):
    """queries 0..15 of the first wave carry label 1, queries 16..31 label 2; one 32-key tile (keys 32..63; at Nk = 8 keys 0..3) holds
    keys of label 2 only, the other keys alternate: the lanes of one wave are masked differently inside one tile"""
    lo, hi = (32, 64) if Nk >= 64 else (0, 4)
    kl = 1 + (torch.arange(Nk) % 2).expand(B, -1).clone()
    kl[:, lo:hi] = 2
    ql = torch.ones(B, Nq, dtype=torch.int64)
    ql[:, 16:32] = 2
    idx, val, _ = _run("per-lane mask", Nq, Nk, k, shared, ql, kl)
    in_tile = (idx >= lo) & (idx < hi) & torch.isfinite(val)      # (a missing rank of a short row holds a clamped index)
    assert not bool(in_tile[:, :16].any())


# ---------------------------------------------------------------------------------------------------------------- pattern 5
@pytest.mark.parametrize(**GRID)
def test_short_and_empty_rows(Nq, Nk, k, shared):
    """label 10 has exactly k keys, label 11 k - 1 (as many as are left at Nk = 8), label 12 none: val is -inf exactly on the missing
    ranks, lse -inf exactly on the empty rows, every idx in range, no NaN (all asserted by _judge_masked from the arbiter's counts)"""
    g = torch.Generator().manual_seed(Nq + 3 * Nk + k)
    kl = torch.zeros(B, Nk, dtype=torch.int64)
    for b in range(B):
        p = torch.randperm(Nk, generator=g)
        kl[b, p[:k]], kl[b, p[k:2 * k - 1]] = 10, 11
    ql = torch.tensor([10, 11, 12, 0])[torch.arange(Nq) % 4].expand(B, -1).clone()
    ql[:, -1] = -1
    idx, val, lse = _run("short rows", Nq, Nk, k, shared, ql, kl)
    n11 = int((kl[0] == 11).sum())
    assert bool(torch.isfinite(val[:, 0::4]).all())                                 # exactly k keys: a full row
    assert bool((val[0, 1::4, n11:] == NEG_INF).all()) and bool(torch.isfinite(val[0, 1::4, :n11]).all())
    assert bool((lse[:, 2:Nq - 1:4] == NEG_INF).all()) and bool((val[:, 2:Nq - 1:4] == NEG_INF).all())
    if n11:
        assert bool(torch.isfinite(lse[0, 1::4]).all())


# ---------------------------------------------------------------------------------------------------------------- pattern 6
@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("shared", [False, True], ids=["dense", "shared"])
def test_equal_logits_under_labels(shared, k):
    """tests/test_gpu_match_topk.py's TIE_PAIRS: keys a < b are both copies of query i.  One label everywhere: a comes first (and b second).
    With a under a foreign label: b is returned and a is not."""
    Nq, Nk = 36, 260
    q, kn = _case(Nq, Nk)
    kn = (kn[:1].expand(B, -1, -1) if shared else kn).clone()
    src = q[:1].expand(B, -1, -1) if shared else q
    for i, (a, b_) in enumerate(TIE_PAIRS):
        kn[:, :, a] = src[:, :, i]
        kn[:, :, b_] = src[:, :, i]
    kn = kn.contiguous()
    ql, same = torch.ones(B, Nq, dtype=torch.int64), torch.ones(B, Nk, dtype=torch.int64)
    foreign = same.clone()
    foreign[:, [a for a, _ in TIE_PAIRS]] = 2
    samples = [0] if shared else range(B)
    idx, val, lse = _labelled(q, kn, ql, same, shared, k)
    idx_f, val_f, lse_f = _labelled(q, kn, ql, foreign, shared, k)
    _judge_masked(f"ties same label k={k}", idx, val, lse, _arbiter(q, kn, ql, same, shared), check=False)
    _judge_masked(f"ties foreign label k={k}", idx_f, val_f, lse_f, _arbiter(q, kn, ql, foreign, shared), ql, foreign[:1] if shared else foreign, check=False)
    for s_ in samples:
        for i, (a, b_) in enumerate(TIE_PAIRS):
            assert idx[s_, i, :2].tolist() == [a, b_][:k], (s_, i, idx[s_, i].tolist())
            assert int(idx_f[s_, i, 0]) == b_ and a not in idx_f[s_, i].tolist(), (s_, i, idx_f[s_, i].tolist())
            assert val_f[s_, i, 0] == val[s_, i, 0]


def test_public_op_takes_int64_labels_and_handles():
    """ops.corr_topk_labelled on fp32 columns with int64 labels is the planes call on the narrowed labels, bitwise; forward only"""
    from cocosnet_amd import ops
    q, kn = _case(132, 68)
    g = torch.Generator().manual_seed(3)
    ql, kl = torch.randint(-1, 3, (B, 132), generator=g), torch.randint(-1, 3, (B, 68), generator=g)
    got = ops.corr_topk_labelled(q, kn, ql.to(DEV), kl.to(DEV), INV_T, 3)
    want = _labelled(q, kn, ql, kl, False, 3)
    assert all(torch.equal(a, b_) for a, b_ in zip(got, want))
    assert not any(t.requires_grad for t in ops.corr_topk_labelled(q.clone().requires_grad_(True), kn, ql.to(DEV), kl.to(DEV), INV_T, 3))
    with pytest.raises(ops._lib.CocosHipError, match="no CPU fallback"):
        ops.corr_topk_labelled(q, kn, ql, kl.to(DEV), INV_T, 3)


# ---------------------------------------------------------------------------------------------------------------- hot path and module
K_MOD = 4
_MOD = {}


def _mod():
    """(net, ref_img, real, seg, ref_seg, corr): the module tests' smallest case (crop 64, 7 classes, a 16 x 16 grid) and the matrix
    forward(return_corr=True) returns for it — made once, never written"""
    if not _MOD:
        net, ref_img, real, seg, ref_seg = _module("ade20k_options", 1)
        with torch.no_grad():
            corr = net(ref_img, real, seg, ref_seg, return_corr=True)
        _MOD["case"] = (net, ref_img, real, seg, ref_seg, corr)
    return _MOD["case"]


def _check_module_masked(tag, out, corr, ql, kl, k):
    """tests/test_gpu_match_topk.py::_check_module's acceptance rule (gap <= TOL, |lse| <= TOL, the relative bound on match_prob) against
    the restatement applied to the matrix `corr` [B,N,Nk]: the fallback rule, then the mask.  (That function cannot be called on the
    masked matrix itself: its bound on match_prob scales with max |corr|, which the -inf entries make infinite — the bound is formed
    from the unmasked matrix here.)  -> the restatement's restricted mask"""
    import math
    Bm, N, Nk = corr.shape
    eff, restricted = lc.fallback(ql, kl, k)
    Ld = corr.double().masked_fill(~lc.allowed(eff.to(DEV), kl.to(DEV)), NEG_INF)
    topk = out["match_index"].dim() == 4
    flat = (lambda t: t.reshape(Bm, k, -1).transpose(1, 2)) if topk else (lambda t: t.reshape(Bm, -1, 1))
    idx, prob = flat(out["match_index"]), flat(out["match_prob"]).double()
    assert out["match_index"].dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < Nk and _distinct(idx), tag
    picked = Ld.gather(2, idx)
    assert bool(torch.isfinite(picked).all()), f"{tag}: a disallowed position was returned"
    want = Ld.sort(dim=2, descending=True).values[..., :k]
    gap = (want - picked).max().item()
    lse_want = lc.logsumexp(Ld)
    e_lse = (out["match_lse"].reshape(Bm, -1).double() - lse_want).abs().max().item()
    want_p = torch.exp(picked - lse_want.unsqueeze(2))
    e_p = ((prob - want_p).abs() / want_p).max().item()
    print(f"[labels] {tag}: max_r sort(L)[r] - L[idx[r]] = {gap:.3e}  rel |prob - softmax| = {e_p:.3e}  |lse - logsumexp| = {e_lse:.3e}  "
          f"restricted {int(restricted.sum())} of {restricted.numel()}")
    assert gap <= TOL and e_lse <= TOL, (tag, gap, e_lse)
    assert e_p <= math.expm1(2 * TOL) + 4 * FP32_EPS * (1 + corr.abs().max().item()), (tag, e_p)
    assert bool((prob[..., :-1] >= prob[..., 1:]).all()), f"{tag}: match_prob is not non-increasing in the rank"
    got_r = out["match_restricted"]
    assert got_r.dtype == torch.bool and got_r.shape == out["match_lse"].shape
    assert torch.equal(got_r.reshape(Bm, -1).cpu(), restricted), f"{tag}: match_restricted is not the restatement's fallback mask"
    lab = kl.to(DEV).gather(1, idx.reshape(Bm, -1)).reshape(idx.shape)
    assert bool(((lab == ql.to(DEV).unsqueeze(-1)) | ~restricted.to(DEV).unsqueeze(-1)).all()), f"{tag}: a restricted position left its label"
    return restricted


def _cells(seg, ref_seg, down=4):
    return lc.cell_labels(seg, down).reshape(seg.shape[0], -1), lc.cell_labels(ref_seg, down).reshape(ref_seg.shape[0], -1)


@pytest.mark.parametrize("k", [1, K_MOD])
def test_module_match_restrict_label_against_return_corr(k, monkeypatch):
    net, ref_img, real, seg, ref_seg, corr = _mod()
    ql, kl = _cells(seg, ref_seg)
    spy = tt._Spy(monkeypatch)
    with torch.no_grad():
        rows = net.match(ref_img, seg, ref_seg, restrict="label", topk=k, hard_warp=True)
        took = spy.take()
        cols = net.match(ref_img, seg, ref_seg, restrict="label", topk=k, direction="cols")
        pair = net.match(ref_img, seg, ref_seg, restrict=(ql.reshape(2, 16, 16), kl.reshape(2, 16, 16)), topk=k, hard_warp=True)
        pair32 = net.match(ref_img, seg, ref_seg, restrict=(ql.reshape(2, 16, 16).int(), kl.reshape(2, 16, 16).int()), topk=k, direction="cols")
    assert ENTRY in took and not took & {"cocos_corr_topk_f16x3", "cocos_corr_match_f16x3", "cocos_row_topk_lse", "cocos_row_argmax_lse"}, sorted(took)
    _check_module_masked(f"module rows k={k}", rows, corr, ql, kl, k)
    _check_module_masked(f"module cols k={k}", cols, corr.transpose(1, 2), kl, ql, k)      # the transposed problem: labels swap with the operands
    want_keys = {"match_index", "match_xy", "match_prob", "match_lse", "match_restricted", "warp_hard"} | ({"warp_topk"} if k > 1 else set())
    assert set(rows) == want_keys and set(cols) == want_keys - {"warp_hard", "warp_topk"}
    for n in rows:
        assert torch.equal(rows[n], pair[n]), f"the explicit pair differs from 'label' in {n}"
    for n in cols:
        assert torch.equal(cols[n], pair32[n]), f"the explicit int32 pair differs from 'label' in {n} (cols)"
    first = rows["match_index"][:, 0] if k > 1 else rows["match_index"]
    assert torch.equal(rows["warp_hard"], _gather_reference(ref_img, first.reshape(2, -1), 16, 16, 4))
    assert not any(v.requires_grad for v in rows.values())


def test_module_match_fallback_mask_with_rare_and_absent_labels():
    """an explicit pair in which content region 98 has K_MOD - 1 exemplar positions, region 99 none and region 97 exactly K_MOD; some content
    positions unrestricted by a negative label"""
    net, ref_img, real, seg, ref_seg, corr = _mod()
    ql, kl = _cells(seg, ref_seg)
    ql, kl = ql.clone(), kl.clone()
    kl[:, :K_MOD - 1], kl[:, 100:100 + K_MOD] = 98, 97
    ql[:, 0:256:5], ql[:, 1:256:5], ql[:, 2:256:5], ql[:, 3:256:7] = 98, 99, 97, -4
    with torch.no_grad():
        out = net.match(ref_img, seg, ref_seg, restrict=(ql.reshape(2, 16, 16), kl.reshape(2, 16, 16)), topk=K_MOD)
    restricted = _check_module_masked("module fallback", out, corr, ql, kl, K_MOD)
    assert not bool(restricted[ql.cpu() == 98].any()) and not bool(restricted[ql.cpu() == 99].any()) and not bool(restricted[ql.cpu() < 0].any())
    assert bool(restricted[ql.cpu() == 97].all())
    assert bool(torch.isfinite(out["match_lse"]).all()) and bool(torch.isfinite(out["match_prob"]).all())


def _hot_case(seed):
    g = torch.Generator().manual_seed(seed)
    theta, phi = torch.randn(2, 256, 8, 8, generator=g).to(DEV), torch.randn(2, 256, 8, 8, generator=g).to(DEV)
    ref_img = (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).to(DEV)
    onehot = lambda: torch.zeros(2, 5, 32, 32).scatter_(1, torch.randint(0, 5, (2, 1, 32, 32), generator=g), 1.0).to(DEV)
    return theta, phi, ref_img, onehot(), onehot()


def _op_chain(theta, phi, ref_img, idx, k, v_grad=False):
    """correspondence_sparse's steps after the selection, from the ops: K1 planes, pooled values, K42, nearest up-sampling -> (warp, v);
    `v_grad`: the pooled values [B,3,Nk] are a leaf that asks for its gradient"""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import _flat
    planes = ops.OperandPlanes()
    qn, kn = ops.center_l2norm_planes(_flat(theta), 1, planes), ops.center_l2norm_planes(_flat(phi), 1, planes)
    with torch.no_grad():
        v = _flat(ops.warp_values(ref_img, None, 4)).clone()
    v.requires_grad_(v_grad)
    o = ops.sparse_softmax_warp(qn, kn, v, idx, 100.0, planes)
    return ops.upsample_nearest(o.reshape(2, 3, 8, 8), 4), v


@pytest.mark.parametrize("k", [1, K_MOD])
def test_correspondence_sparse_restrict_label(k):
    """crop 32, 5 classes, an 8 x 8 grid: the selection is correspondence_match(restrict="label")'s bit for bit, the warp is K42 on those
    indices bit for bit, and the gradients of theta and phi are within GRAD_TOL of the fp64 restatement on the same indices.  ref_img:
    correspondence_sparse pools the exemplar under no_grad (as without restrict), so the image itself gets no gradient on this route; the
    value gradient K42 owns is judged on the same chain built from the ops (bitwise the same warp), with the pooled exemplar as a leaf."""
    import test_gpu_sparse_warp as tsw
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match, correspondence_sparse
    theta0, phi0, ref_img, seg, ref_seg = _hot_case(50 + k)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    theta, phi = theta0.clone().requires_grad_(True), phi0.clone().requires_grad_(True)
    out = correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, 0.01, k, restrict="label")
    assert set(out) == {"warp_out", "match_index", "match_weight", "match_restricted"}
    m = correspondence_match(theta0, phi0, cfg, 0.01, topk=k, restrict="label", seg_map=seg, ref_seg_map=ref_seg)
    assert torch.equal(out["match_index"], m.index if k > 1 else m.index.unsqueeze(1)) and torch.equal(out["match_restricted"], m.restricted)
    ql, kl = _cells(seg, ref_seg)
    eff, restricted = lc.fallback(ql, kl, k)
    assert torch.equal(out["match_restricted"].reshape(2, -1).cpu(), restricted) and bool(restricted.any())
    idx = out["match_index"].permute(0, 2, 3, 1).reshape(2, 64, k)
    lab = kl.to(DEV).gather(1, idx.reshape(2, -1)).reshape(idx.shape)
    assert bool(((lab == ql.to(DEV).unsqueeze(-1)) | ~restricted.to(DEV).unsqueeze(-1)).all())
    th2, ph2 = theta0.clone().requires_grad_(True), phi0.clone().requires_grad_(True)
    warp2, vq = _op_chain(th2, ph2, ref_img, idx, k, v_grad=True)
    assert torch.equal(out["warp_out"], warp2), "warp_out is not ops.sparse_softmax_warp on the restricted indices"
    g_out = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(9)).to(DEV)
    (out["warp_out"] * g_out).sum().backward()
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in (theta, phi))
    if k == 1:      # w = 1: the logits carry no gradient
        assert float(theta.grad.abs().max()) == 0.0 and float(phi.grad.abs().max()) == 0.0
        return
    th64, ph64 = theta0.double().requires_grad_(True), phi0.double().requires_grad_(True)
    warp_r, _ = tsw._hot_ref(th64, ph64, ref_img, ref_seg, idx, 4, False, 100.0)
    (warp_r * g_out.double()).sum().backward()
    errs = {"d theta": rel(theta.grad, th64.grad.cpu().numpy()), "d phi": rel(phi.grad, ph64.grad.cpu().numpy())}
    # the value gradient: the same loss on the chain built from the ops, v [B,3,Nk] (the pooled exemplar) a leaf on both sides
    import torch.nn.functional as F
    from oracle.torch_ref import _unit_columns
    (warp2 * g_out).sum().backward()
    v64 = vq.detach().double().requires_grad_(True)
    o64 = tsw._ref(_unit_columns(theta0.double().reshape(2, 256, -1), True), _unit_columns(phi0.double().reshape(2, 256, -1), True), v64, idx, 100.0)
    (F.interpolate(o64.reshape(2, 3, 8, 8), scale_factor=4, mode="nearest") * g_out.double()).sum().backward()
    errs["d v"] = rel(vq.grad, v64.grad.cpu().numpy())
    assert torch.equal(th2.grad, theta.grad) and torch.equal(ph2.grad, phi.grad)
    print(f"[labels] correspondence_sparse restrict k={k}: " + "  ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    assert bool(torch.isfinite(vq.grad).all()) and all(e < GRAD_TOL for e in errs.values()), errs


def test_module_sparse_warp_restrict_label():
    net, ref_img, real, seg, ref_seg, _ = _mod()
    out = net.sparse_warp(ref_img, real, seg, ref_seg, topk=K_MOD, restrict="label")
    assert {"warp_out", "match_index", "match_weight", "match_restricted"} <= set(out)
    with torch.no_grad():
        m = net.match(ref_img, seg, ref_seg, topk=K_MOD, restrict="label")
    assert torch.equal(out["match_index"], m["match_index"]) and torch.equal(out["match_restricted"], m["match_restricted"])
    out["warp_out"].square().sum().backward()
    for p in (net.theta.weight, net.phi.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    net.zero_grad(set_to_none=True)


def test_restrict_none_is_the_unlabelled_route_bitwise(monkeypatch):
    """match and sparse_warp with restrict=None against the same calls without the keyword and against the unlabelled ops called
    directly, in one process: same keys, same bits, and the labelled entry point is never reached"""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, _flat, correspondence_match, correspondence_sparse
    net, ref_img, real, seg, ref_seg, _ = _mod()
    spy = tt._Spy(monkeypatch)
    with torch.no_grad():
        for kw in (dict(topk=1, hard_warp=True), dict(topk=K_MOD, hard_warp=True), dict(topk=K_MOD, direction="cols")):
            a, b_ = net.match(ref_img, seg, ref_seg, **kw), net.match(ref_img, seg, ref_seg, restrict=None, **kw)
            assert sorted(a) == sorted(b_) and "match_restricted" not in b_ and all(torch.equal(a[n], b_[n]) for n in a), kw
    sa, sb = net.sparse_warp(ref_img, real, seg, ref_seg, topk=K_MOD), net.sparse_warp(ref_img, real, seg, ref_seg, topk=K_MOD, restrict=None)
    assert sorted(sa) == sorted(sb) and "match_restricted" not in sb and all(torch.equal(sa[n], sb[n]) for n in sa)
    theta, phi, ref_img2, seg2, ref_seg2 = _hot_case(77)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    planes = ops.OperandPlanes()
    qn = ops.center_l2norm_planes(_flat(theta), 1, planes, want_chan=False)
    kn = ops.center_l2norm_planes(_flat(phi), 1, planes, want_chan=False)
    idx, val, lse = ops.corr_topk(qn, kn, 100.0, K_MOD, planes)
    m = correspondence_match(theta, phi, cfg, 0.01, topk=K_MOD, restrict=None)
    assert m.restricted is None and torch.equal(m.index, idx.long().reshape(2, 8, 8, K_MOD).permute(0, 3, 1, 2))
    assert torch.equal(m.lse, lse.reshape(2, 8, 8)) and torch.equal(m.logit, val.reshape(2, 8, 8, K_MOD).permute(0, 3, 1, 2))
    s = correspondence_sparse(theta, phi, ref_img2, seg2, ref_seg2, cfg, 0.01, K_MOD, restrict=None)
    assert set(s) == {"warp_out", "match_index", "match_weight"} and torch.equal(s["match_index"], m.index)
    assert torch.equal(s["warp_out"], _op_chain(theta, phi, ref_img2, idx, K_MOD)[0])
    assert ENTRY not in spy.take()


def test_fused_route_allocates_nothing_hw_by_hw():
    """test_gpu_match_topk's probe with restrict: B = 1, a 64 x 64 grid — the peak above the live memory stays below half of the matrix"""
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match
    N = 64 * 64
    theta, phi = _randn(1, 256, 64, 64, seed=21), _randn(1, 256, 64, 64, seed=22)
    lab = (torch.arange(N, device=DEV) // 600).reshape(1, 64, 64)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = correspondence_match(theta, phi, cfg, topk=4, restrict=(lab, lab))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"[labels] peak memory above live: {peak / 2 ** 20:.1f} MiB (the matrix: {N * N * 4 / 2 ** 20:.0f} MiB)")
    assert peak < N * N * 4 // 2 and bool(m.restricted.all())
    assert torch.equal(lab.reshape(1, 1, N).expand(-1, 4, -1), lab.reshape(1, N).gather(1, m.index.reshape(1, -1)).reshape(1, 4, N))


# ---------------------------------------------------------------------------------------------------------------- guards
def test_match_restrict_hands_over_live_buffers_only(monkeypatch):
    import test_gpu_live_buffers as lb
    net, ref_img, real, seg, ref_seg, _ = _mod()
    guard = lb._Guard(monkeypatch)
    with torch.no_grad():
        net.match(ref_img, seg, ref_seg, restrict="label", topk=K_MOD, hard_warp=True)
        net.match(ref_img, seg, ref_seg, restrict="label", direction="cols")
    guard.check(20, 75)


# ---- red zones: the case joins tests/test_gpu_red_zones.py's table at import time, so its coverage report and its "every entry point was
# ---- reached" audit count the K47 entry point too (as tests/test_gpu_match_topk.py does for K39).  Partial query / key tiles, k = 3 and
# ---- k = 8, labels out of any class range and negative on both sides: a read past q_label [B,Nq] or k_label [B,Nk] meets a guard's NaN
# ---- bits (an int that equals no label), a write past idx / val [B,Nq,k] lands in a guard
def _rz_corr_topk_labelled(c):
    from cocosnet_amd import ops
    q, k = c.data(rz.unit(2, 256, 132, 31)), c.data(rz.unit(2, 256, 68, 32))
    g = torch.Generator().manual_seed(45)
    ql, kl = torch.randint(0, 3, (2, 132), generator=g), torch.randint(0, 3, (2, 68), generator=g)
    ql[:, ::7], ql[:, 3::11], kl[:, ::5], kl[:, 2::9] = -1, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1
    ql, kl = c.data(ql.to(torch.int32)), c.data(kl)
    # (queries of a label no key carries have lse = -inf: only the unrestricted rows' outputs are returned for the finiteness check)
    free = (ql < 0).nonzero(as_tuple=True)
    outs = []
    for kk in (3, 8):
        idx, val, lse = ops.corr_topk_labelled(q, k, ql, kl, 100.0, kk)
        assert int(idx.min()) >= 0 and int(idx.max()) < 68
        outs += [idx, val[free], lse[free]]
    return outs


RZ_CASES = {"corr_topk_labelled-2x132x68-k3+k8": _rz_corr_topk_labelled}
for _name, _body in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_op_inside_red_zones(name, monkeypatch):
    rz.test_red_zones(name, monkeypatch)
    assert ENTRY in set(rz.COVERAGE[name][0])
