"""K39 top-k match readout on the GPU: the fused kernel (K39a, cocos_corr_topk_f16x3), the one-sweep reader of a materialised matrix
(K39b, cocos_row_topk_lse), the k-sparse warp (K39c, cocos_gather_blend_patches) and `NoVGGCorrespondence.match(topk=k)`.

Cases, arbiter and tolerance are tests/test_gpu_match.py's (imported, not restated): SHAPES plus (36, 8) for k = Nk, B = 3, INV_T = 100,
the fp64 arbiter L = inv_t * qn^T kn, TOL = 4 * E_FWD with E_FWD the forward kernel's own lse error.  That file argues that
`L[idx] >= max L - TOL` holds for a correct kernel whatever the gap to the runner-up; the argument is the same at every rank: each of
the kernel's logits is within its element error e <= TOL of the arbiter's, so the kernel's r-th largest logit is within e of the arbiter's
r-th largest (an order statistic moves by at most the largest element move), and the arbiter's value at the r-th pick is within e of that
again — `L[idx[r]] >= sort_desc(L)[r] - TOL` with nothing excluded and no assumption about gaps."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_match as tm  # noqa: E402
import test_gpu_red_zones as rz  # noqa: E402
from test_gpu_match import B, DEV, FP32_EPS, INV_T, TOL, _arbiter, _case, _gather_reference, _module, _planes, _randn, _rep, _unit  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = tm.SHAPES + [(36, 8)]      # (36, 8): k = 8 = Nk, every key is returned
KS = [1, 2, 3, 4, 8]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def _topk(q, k, shared, kk):
    from cocosnet_amd import ops
    return ops._corr_topk_planes(*_planes(q), *_planes(k[:1].contiguous() if shared else k), INV_T, kk)


def _ordered(val, idx):
    """val non-increasing along the last dim and, among bitwise-equal neighbours, the index ascending"""
    a, b = val[..., :-1], val[..., 1:]
    return bool(((a > b) | ((a == b) & (idx[..., :-1] < idx[..., 1:]))).all())


def _distinct(idx):
    s = idx.sort(dim=-1).values
    return bool((s[..., 1:] != s[..., :-1]).all())


def _judge(tag, idx, val, lse, L, tol=TOL, check=True):
    """conditions 1 of the issue, every row: idx [..,k] int32, val [..,k], lse [..] against the fp64 matrix L [.., Nk]"""
    Nk, k = L.shape[-1], idx.shape[-1]
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and idx.shape == val.shape == L.shape[:-1] + (k,), tag
    assert int(idx.min()) >= 0 and int(idx.max()) < Nk, (tag, int(idx.min()), int(idx.max()))
    assert _distinct(idx), f"{tag}: a row returns one key twice"
    picked = L.gather(-1, idx.long())
    want = L.sort(dim=-1, descending=True).values[..., :k]
    e_val = (val.double() - picked).abs().max().item()
    e_pick = (want - picked).max().item()
    e_lse = (lse.double() - torch.logsumexp(L, dim=-1)).abs().max().item()
    print(f"[topk] {tag}: |val - L[idx]| = {e_val:.3e}  max_r sort(L)[r] - L[idx[r]] = {e_pick:.3e}  |lse - logsumexp L| = {e_lse:.3e}  (tol {tol:.1e})")
    assert _ordered(val, idx), f"{tag}: val is not non-increasing with ascending indices among equals"
    if check:
        assert e_val <= tol, (tag, e_val)
        assert e_pick <= tol, (tag, e_pick)
        assert e_lse <= tol, (tag, e_lse)


# ---------------------------------------------------------------------------------------------------------------- K39a
@pytest.mark.parametrize("shared", [False, True], ids=["dense", "shared"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("Nq,Nk", SHAPES)
def test_random_inputs_every_query(Nq, Nk, k, shared):
    q, kn, L, Ls = _case(Nq, Nk)
    idx, val, lse = _topk(q, kn, shared, k)
    _judge(f"random ({Nq},{Nk}) k={k} {'shared' if shared else 'dense'}", idx, val, lse, Ls if shared else L)


@pytest.mark.parametrize("shared", [False, True], ids=["dense", "shared"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("Nq,Nk", SHAPES)
def test_rank_0_and_lse_are_k36a_bitwise(Nq, Nk, k, shared):
    q, kn, _, _ = _case(Nq, Nk)
    idx, val, lse = _topk(q, kn, shared, k)
    i1, m1, l1 = tm._match(q, kn, shared)
    assert torch.equal(idx[..., 0], i1) and torch.equal(val[..., 0], m1) and torch.equal(lse, l1)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shape", [(2, 37, 68), (1, 256, 260), (3, 7, 67), (2, 5, 8)])
def test_row_topk_lse(shape, k):
    """K39b against torch on the same fp32 matrix: values are elements of the row (bitwise), picks are exact, rank 0 and lse are K36b's bits.
    (3, 7, 67): rows that are not 16-byte aligned — the dword sweep; (2, 5, 8): k = 8 = Nk"""
    from cocosnet_amd import ops
    f = _randn(*shape, seed=shape[1] + shape[2]) * 3.0
    idx, val, lse = ops.row_topk_lse(f, k)
    i1, m1, l1 = ops.row_argmax_lse(f)
    assert torch.equal(idx[..., 0], i1) and torch.equal(val[..., 0], m1) and torch.equal(lse, l1)
    assert torch.equal(val, f.gather(2, idx.long())) and torch.equal(val, f.topk(k, dim=2).values)
    _judge(f"row_topk_lse {shape} k={k}", idx, val, lse, f.double(), tol=4 * FP32_EPS * (torch.logsumexp(f.double(), 2).abs().max().item() + 1))


def test_row_topk_lse_orders_equal_values_by_index():
    """the same value in many lanes, in one lane's 16-byte step and 256 apart (one lane's next step): ascending indices, no repeats"""
    from cocosnet_amd import ops
    f = _randn(2, 5, 516, seed=11)
    cols = [300, 13, 12, 269, 515, 40]
    f[:, :, cols] = 9.0
    f[0, 2, 3] = 9.5
    idx, val, _ = ops.row_topk_lse(f, 8)
    want = torch.tensor(sorted(cols), device=DEV, dtype=torch.int32)
    assert torch.equal(idx[1, :, :6], want.expand(5, -1)) and bool((val[1, :, :6] == 9.0).all())
    assert int(idx[0, 2, 0]) == 3 and torch.equal(idx[0, 2, 1:7], want)
    assert _distinct(idx) and _ordered(val, idx)
    g = f[:, :, :515].contiguous()                           # odd width: the dword sweep
    idx, val, _ = ops.row_topk_lse(g, 4)
    assert torch.equal(idx[1], torch.tensor(sorted(cols)[:4], device=DEV, dtype=torch.int32).expand(5, -1)) and _ordered(val, idx)


# ---- planted candidates
PLANT_TILE = [3, 6, 0, 5, 2, 7, 1, 4]      # rank r of every planted query sits in 32-key tile PLANT_TILE[r]


def _plant_position(i, r):
    """key index of rank r of planted query i: tile PLANT_TILE[r] (stage = tile // 2, wave group = tile % 2); the offset inside the tile
    is distinct over the 16 queries and flips bit 2 (the half-wave) between ranks"""
    return 32 * PLANT_TILE[r] + (2 * i + 5 * (r >> 1)) % 32


@pytest.mark.parametrize("shared", [False, True], ids=["dense", "shared"])
def test_planted_candidates_come_back_in_order(shared):
    Nq, Nk, nplant = 36, 260, 16
    q, kn, _, _ = _case(Nq, Nk)
    kn = (kn[:1].expand(B, -1, -1) if shared else kn).clone()
    pos = torch.tensor([[_plant_position(i, r) for r in range(8)] for i in range(nplant)])
    assert pos.unique().numel() == nplant * 8
    for i in range(nplant):
        tiles, off = pos[i] // 32, pos[i] % 32
        assert tiles.unique().numel() == 8 and (tiles // 2).unique().numel() == 4 and set((tiles % 2).tolist()) == {0, 1}
        assert set(((off >> 2) & 1).tolist()) == {0, 1}, "both half-waves"
    u = _randn(B, 256, nplant, 8, seed=77).double()
    qd = q[:, :, :nplant].double()
    if shared:      # one key set: planted from sample 0's queries, judged in sample 0
        qd, u = qd[:1].expand(B, -1, -1), u[:1].expand(B, -1, -1, -1)
    u = u - (u * qd.unsqueeze(3)).sum(1, keepdim=True) * qd.unsqueeze(3)
    u = u / u.norm(dim=1, keepdim=True)
    cos = (1.0 - 0.07 * torch.arange(8, device=DEV, dtype=torch.float64)).view(1, 1, 1, 8)
    planted = (cos * qd.unsqueeze(3) + (1 - cos * cos).sqrt() * u).float()          # [B,256,16,8], unit norm
    kn[:, :, pos.reshape(-1).to(DEV)] = planted.reshape(B, 256, -1)
    kn = kn.contiguous()
    L = _arbiter(q, kn)
    samples = [0] if shared else list(range(B))
    top9 = L[samples, :nplant].topk(9, dim=2)
    gaps = top9.values[..., :-1] - top9.values[..., 1:]
    print(f"[topk] planted {'shared' if shared else 'dense'}: smallest arbiter gap {gaps.min().item():.3f}")
    assert gaps.min().item() > 3.0, "the planted gaps (between ranks, and to the best random key) this test relies on"
    assert torch.equal(top9.indices[..., :8], pos.to(DEV).expand(len(samples), -1, -1))
    for k in (2, 4, 8):
        idx, val, lse = _topk(q, kn, shared, k)
        got = idx[samples, :nplant].long()
        assert torch.equal(got, pos.to(DEV)[:, :k].expand(len(samples), -1, -1)), f"k={k}: {int((got != pos.to(DEV)[:, :k]).sum())} planted ranks missed"
        _judge(f"planted k={k} {'shared' if shared else 'dense'}", idx, val, lse, L, check=False)


# ---- ties
TIE_PAIRS = [(1, 9), (2, 5), (3, 35), (70, 200), (100, 130), (44, 259)]


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("shared", [False, True], ids=["dense", "shared"])
def test_equal_logits_come_back_in_index_order(shared, k):
    """The pairs of test_gpu_match.test_equal_logits_return_the_lowest_index (one per merge level: a lane's registers, the two half-waves,
    the two wave groups, two stages of one wave, lower index in the odd-tile wave, the last tile of 4 keys), each a pair of copies of the
    query itself, and per query a SECOND tie below the maximum: two copies of another unit vector (cosine 0.8 with the query) at the
    pair's positions shifted by 16 and 48 keys — a tie that is decided at ranks 2 and 3 and crosses tiles the other way round."""
    Nq, Nk = 36, 260
    q, kn, _, _ = _case(Nq, Nk)
    kn = (kn[:1].expand(B, -1, -1) if shared else kn).clone()
    src = q[:1].expand(B, -1, -1) if shared else q
    second = []
    for i, (a, b) in enumerate(TIE_PAIRS):
        kn[:, :, a] = src[:, :, i]
        kn[:, :, b] = src[:, :, i]
        a2, b2 = (b + 48) % 256, (a + 16) % 256
        lo, hi = min(a2, b2), max(a2, b2)
        second.append((lo, hi))
        u = _randn(B, 256, seed=90 + i).double()
        qd = src[:, :, i].double()
        u = u - (u * qd).sum(1, keepdim=True) * qd
        v = (0.8 * qd + 0.6 * u / u.norm(dim=1, keepdim=True)).float()
        kn[:, :, lo] = v
        kn[:, :, hi] = v
    used = [p for pair in TIE_PAIRS + second for p in pair]
    assert len(set(used)) == len(used)
    kn = kn.contiguous()
    idx, val, lse = _topk(q, kn, shared, k)
    L = _arbiter(q, kn[:1].expand(B, -1, -1) if shared else kn)
    for s_ in ([0] if shared else range(B)):
        for i, ((a, b), (a2, b2)) in enumerate(zip(TIE_PAIRS, second)):
            row = L[s_, i]
            assert row[a] == row[b] == row.max() and row[a2] == row[b2] and (row > row[a2]).sum() == 2, "the arbiter's ties this test relies on"
            want = [a, b, a2, b2][:k]
            assert idx[s_, i, :len(want)].tolist() == want, (f"pairs {(a, b), (a2, b2)} sample {s_}", idx[s_, i].tolist())
            assert val[s_, i, 0] == val[s_, i, 1] and (k < 4 or val[s_, i, 2] == val[s_, i, 3])
    _judge(f"ties k={k} {'shared' if shared else 'dense'}", idx, val, lse, L, check=False)      # range, distinct, order; figures printed


# ---- padded keys
@pytest.mark.parametrize("shared", [False, True], ids=["dense", "shared"])
@pytest.mark.parametrize("Nk,k", [(36, 4), (36, 8), (260, 3), (260, 8), (8, 8)])
def test_all_negative_rows_never_return_a_padded_key(Nk, k, shared):
    """all-positive queries against all-negative keys: a zero-padded key of the last tile (logit 0) would head every list"""
    Nq = 36
    q, kn = _unit(_randn(B, 256, Nq, seed=3).abs() + 0.01), _unit(-_randn(B, 256, Nk, seed=4).abs() - 0.01)
    idx, val, lse = _topk(q, kn, shared, k)
    assert float(val.max()) < 0.0
    _judge(f"all-negative Nk={Nk} k={k} {'shared' if shared else 'dense'}", idx, val, lse, _arbiter(q, kn[:1].expand(B, -1, -1) if shared else kn))
    if k == Nk:
        assert torch.equal(idx.sort(dim=2).values, torch.arange(8, device=DEV, dtype=torch.int32).expand(B, Nq, -1))


def test_non_finite_input_keeps_the_indices_in_range():
    q, kn, _, _ = _case(36, 260)
    q = q.clone()
    q[0, :, 3] = float("nan")
    q[1, :, 5] = float("inf")
    idx, _, _ = _topk(q, kn, False, 8)
    assert int(idx.min()) >= 0 and int(idx.max()) < 260


# ---------------------------------------------------------------------------------------------------------------- K39c
def _blend_reference(img, idx, w, h, wg, down):
    """fp64: sum_r w_r * (torch gather of rank r), and sum_r |w_r * p_r| for the bound"""
    k = idx.shape[1]
    idx = idx.reshape(idx.shape[0], k, h * wg)
    up = lambda t: t.reshape(-1, 1, h, wg).double().repeat_interleave(down, 2).repeat_interleave(down, 3)
    terms = [up(w[:, r]) * _gather_reference(img.double(), idx[:, r], h, wg, down) for r in range(k)]
    return sum(terms), sum(t.abs() for t in terms)


@pytest.mark.parametrize("Be", [1, 2])
@pytest.mark.parametrize("down", [2, 4])
def test_blend_of_one_patch_with_weight_one_is_gather_patches_bitwise(down, Be):
    from cocosnet_amd import ops
    Bq, C, h, w = 2, 3, 5, 7
    img = _randn(Be, C, h * down, w * down, seed=down)
    idx = torch.randint(0, h * w, (Bq, 1, h, w), generator=torch.Generator().manual_seed(Be)).to(DEV)
    out = ops.gather_blend_patches(img, idx, torch.ones(Bq, 1, h, w, device=DEV), h, w, down)
    assert torch.equal(out, ops.gather_patches(img, idx[:, 0], h, w, down))
    assert torch.equal(out, _gather_reference(img, idx.reshape(Bq, -1), h, w, down))


@pytest.mark.parametrize("Be", [1, 2])
@pytest.mark.parametrize("down", [2, 4])
def test_blend_of_four_patches_against_fp64(down, Be):
    """fp32 products and k - 1 fused adds in a fixed order: k roundings of partial sums bounded by sum_r |w_r p_r| plus one for the first
    product — |out - fp64| <= (k + 1) 2^-24 sum_r |w_r p_r| elementwise"""
    from cocosnet_amd import ops
    Bq, C, h, w, k = 2, 3, 5, 7, 4
    img = _randn(Be, C, h * down, w * down, seed=10 + down)
    idx = torch.randint(0, h * w, (Bq, k, h, w), generator=torch.Generator().manual_seed(20 + Be)).to(DEV)
    wt = torch.softmax(_randn(Bq, k, h, w, seed=5) * 2, dim=1)
    out = ops.gather_blend_patches(img, idx.to(torch.int32), wt, h, w, down)
    want, mag = _blend_reference(img, idx, wt, h, w, down)
    err = (out.double() - want).abs()
    bound = (k + 1) * 2.0 ** -24 * mag
    print(f"[topk] blend down={down} Be={Be}: max |out - fp64| / bound = {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    assert torch.equal(out, ops.gather_blend_patches(img, idx.reshape(Bq, k, h * w), wt.reshape(Bq, k, h * w), h, w, down))


def test_blend_clamps_an_out_of_range_index():
    from cocosnet_amd import ops
    Bq, C, h, w, down, k = 2, 3, 5, 7, 4, 2
    img = _randn(1, C, h * down, w * down, seed=31)
    idx = torch.randint(0, h * w, (Bq, k, h, w), generator=torch.Generator().manual_seed(32)).to(DEV)
    bad = idx.clone()
    bad[0, 0, 0, 0], bad[1, 1, 2, 3], bad[0, 1, 4, 6] = -5, h * w, 2 ** 31 - 1
    wt = torch.softmax(_randn(Bq, k, h, w, seed=33), dim=1)
    idx[0, 0, 0, 0], idx[1, 1, 2, 3], idx[0, 1, 4, 6] = 0, h * w - 1, h * w - 1
    assert torch.equal(ops.gather_blend_patches(img, bad, wt, h, w, down), ops.gather_blend_patches(img, idx, wt, h, w, down))


# ---------------------------------------------------------------------------------------------------------------- the module
K_MOD = 4


class _Spy:
    """the entry points that went through _lib.call"""

    def __init__(self, monkeypatch):
        from cocosnet_amd import _lib
        self.names, real = [], _lib.call
        monkeypatch.setattr(_lib, "call", lambda name, *args: (self.names.append(name), real(name, *args))[1])

    def take(self):
        got, self.names[:] = set(self.names), []
        return got


def _check_module(tag, out, corr, exact):
    """conditions 1 on match(topk=k)'s dict against the matrix forward(return_corr=True) returned (rows: [B, N, Nk]); the logit itself is
    not in the dict: match_prob is judged against the softmax of the matrix at the picked columns, relative, as _check_against_corr does"""
    Bm, k = corr.shape[0], out["match_index"].shape[1]
    flat = lambda t: t.reshape(Bm, k, -1).transpose(1, 2)                      # [B,N,k]
    idx, prob = flat(out["match_index"]), flat(out["match_prob"]).double()
    Ld = corr.double()
    assert out["match_index"].dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < corr.shape[2] and _distinct(idx), tag
    picked = Ld.gather(2, idx)
    want = Ld.sort(dim=2, descending=True).values[..., :k]
    gap = (want - picked).max().item()
    lse_want = torch.logsumexp(Ld, dim=2)
    e_lse = (out["match_lse"].reshape(Bm, -1).double() - lse_want).abs().max().item()
    want_p = torch.exp(picked - lse_want.unsqueeze(2))
    e_p = ((prob - want_p).abs() / want_p).max().item()
    print(f"[topk] {tag}: max_r sort(corr)[r] - corr[idx[r]] = {gap:.3e}  rel |prob - softmax| = {e_p:.3e}  |lse - logsumexp corr| = {e_lse:.3e}")
    assert (gap == 0.0) if exact else (gap <= TOL), (tag, gap)
    assert e_lse <= TOL, (tag, e_lse)
    # prob = exp(logit - lse) with both within TOL of the matrix's: a factor exp(+-2 TOL); 4 eps for the fp32 exp and subtraction
    assert e_p <= math.expm1(2 * TOL) + 4 * FP32_EPS * (1 + corr.abs().max().item()), (tag, e_p)
    assert bool((prob[..., :-1] >= prob[..., 1:]).all()), f"{tag}: match_prob is not non-increasing in the rank"
    xy = out["match_xy"]
    gw = out["match_index"].shape[3]
    assert xy.shape == out["match_index"].shape[:2] + (2,) + out["match_index"].shape[2:]
    assert torch.equal(xy[:, :, 1] * gw + xy[:, :, 0], out["match_index"])
    assert out["match_lse"].shape == out["match_index"].shape[:1] + out["match_index"].shape[2:]


def _check_warp_topk(tag, net, ref_img, out_full, out_topk):
    """warp_topk against a torch gather-blend of the dict's own indices and weights.  blend="full": the weights ARE match_prob, the
    bound is K39c's.  blend="topk": softmax over the k logits = match_prob / sum_r match_prob; the module forms it from the logits
    and this check from match_prob, two fp32 paths whose subtractions (logit - lse, logit - max; |x| < 128: half an ulp is 2^-18)
    and exp / sum / divide steps (8 eps) move a weight by at most 4 * 2^-18 + 8 eps < 2e-5 relative: that much of sum_r |w_r p_r| is added."""
    idx = out_full["match_index"]
    Bm, k, fh, fw = idx.shape
    down = net.opt.down
    assert torch.equal(out_topk["match_index"], idx) and torch.equal(out_topk["match_prob"], out_full["match_prob"])
    assert torch.equal(out_full["warp_hard"], _gather_reference(ref_img, idx[:, 0].reshape(Bm, -1), fh, fw, down))
    assert torch.equal(out_full["warp_hard"], out_topk["warp_hard"])
    want, mag = _blend_reference(ref_img, idx, out_full["match_prob"], fh, fw, down)
    err, bound = (out_full["warp_topk"].double() - want).abs(), (k + 1) * 2.0 ** -24 * mag
    p = out_full["match_prob"].double()
    want_n, mag_n = _blend_reference(ref_img, idx, p / p.sum(1, keepdim=True), fh, fw, down)
    err_n, bound_n = (out_topk["warp_topk"].double() - want_n).abs(), ((k + 1) * 2.0 ** -24 + 2e-5) * mag_n
    print(f"[topk] {tag}: warp_topk full |err| / bound = {(err / bound).max().item():.3f}, topk |err| / bound = {(err_n / bound_n).max().item():.3f}")
    assert out_full["warp_topk"].shape == (Bm, 3, fh * down, fw * down) and (err <= bound).all() and (err_n <= bound_n).all()


@pytest.mark.parametrize("mk,fused", [(1, True), (3, True), (1, False), (3, False)], ids=["mk1", "mk3", "mk1-MATCH_FUSED_off", "mk3-MATCH_FUSED_off"])
def test_module_match_topk_against_return_corr(mk, fused, monkeypatch):
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "MATCH_FUSED", fused)
    net, ref_img, real, seg, ref_seg = _module("ade20k_options", mk)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        corr = net(ref_img, real, seg, ref_seg, return_corr=True)
        spy.take()
        rows = net.match(ref_img, seg, ref_seg, hard_warp=True, topk=K_MOD, blend="full")
        took = spy.take()
        rows_n = net.match(ref_img, seg, ref_seg, hard_warp=True, topk=K_MOD)
        cols = net.match(ref_img, seg, ref_seg, direction="cols", topk=K_MOD)
        one = net.match(ref_img, seg, ref_seg, hard_warp=True, topk=1)
        today = net.match(ref_img, seg, ref_seg, hard_warp=True)
    on_k39a = mk == 1 and fused
    assert ("cocos_corr_topk_f16x3" if on_k39a else "cocos_row_topk_lse") in took and "cocos_gather_blend_patches" in took, sorted(took)
    assert ("cocos_row_topk_lse" if on_k39a else "cocos_corr_topk_f16x3") not in took
    _check_module(f"mk{mk} fused={fused} rows", rows, corr, exact=not on_k39a)
    _check_module(f"mk{mk} fused={fused} cols", cols, corr.transpose(1, 2), exact=False)
    _check_warp_topk(f"mk{mk} fused={fused}", net, ref_img, rows, rows_n)
    assert not any(v.requires_grad for v in rows.values())
    # topk = 1 is today's dict: the same keys, shapes, dtypes — and values
    assert sorted(one) == sorted(today) == ["match_index", "match_lse", "match_prob", "match_xy", "warp_hard"]
    fh = fw = 16
    assert {n: (tuple(v.shape), v.dtype) for n, v in one.items()} == {
        "match_index": ((2, fh, fw), torch.int64), "match_xy": ((2, 2, fh, fw), torch.int64), "match_prob": ((2, fh, fw), torch.float32),
        "match_lse": ((2, fh, fw), torch.float32), "warp_hard": ((2, 3, 64, 64), torch.float32)}
    for n in today:
        assert torch.equal(one[n], today[n]), n
    # rank 0 of the top-k readout is the argmax readout, bit for bit
    assert torch.equal(rows["match_index"][:, 0], today["match_index"]) and torch.equal(rows["match_lse"], today["match_lse"])
    assert torch.equal(rows["match_prob"][:, 0], today["match_prob"]) and torch.equal(rows["warp_hard"], today["warp_hard"])


@pytest.mark.parametrize("Be", [1, 2])
@pytest.mark.parametrize("mk", [1, 3])
def test_module_match_topk_with_a_prepared_exemplar(mk, Be):
    from cocosnet_amd import inference
    net, ref_img, real, seg, ref_seg = _module("ade20k_options", mk, Be=Be)
    with torch.no_grad():
        corr = net(_rep(ref_img, 2), real, seg, _rep(ref_seg, 2), return_corr=True)
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
        for direction in ("rows", "cols"):
            c = corr if direction == "rows" else corr.transpose(1, 2)
            got = net.match(None, seg, None, exemplar=rec, direction=direction, hard_warp=direction == "rows", topk=K_MOD, blend="full")
            _check_module(f"record Be={Be} mk{mk} {direction}", got, c, exact=False)
            if direction == "rows":
                got_n = net.match(None, seg, None, exemplar=rec, hard_warp=True, topk=K_MOD, blend="topk")
                _check_warp_topk(f"record Be={Be} mk{mk}", net, ref_img, got, got_n)


def test_module_match_refuses_more_candidates_than_positions():
    net, ref_img, real, seg, ref_seg = _module("ade20k_options", 1, crop=8)      # a 2 x 2 grid: four positions
    with pytest.raises(ValueError, match="topk=5"):
        net.match(ref_img, seg, ref_seg, topk=5)


def test_fused_route_allocates_nothing_hw_by_hw(monkeypatch):
    """test_gpu_match's probe with topk = 4: B = 1, 64 x 64 grid — the peak above the live memory stays below half of the matrix on the
    fused match_kernel-1 route; with MATCH_FUSED off the same probe sees the matrix"""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, TopkMatchReadout, correspondence_match
    N = 64 * 64
    theta, phi = _randn(1, 256, 64, 64, seed=21), _randn(1, 256, 64, 64, seed=22)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    deltas = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "MATCH_FUSED", fused)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m = correspondence_match(theta, phi, cfg, topk=4)
        torch.cuda.synchronize()
        deltas[fused] = torch.cuda.max_memory_allocated() - base
        assert isinstance(m, TopkMatchReadout) and m.index.shape == (1, 4, 64, 64) and m.lse.shape == (1, 64, 64)
        assert m.xy().shape == (1, 4, 2, 64, 64) and m.grid == (64, 64)
        del m
    print(f"[topk] peak memory above live: fused {deltas[True] / 2**20:.1f} MiB, materialised {deltas[False] / 2**20:.1f} MiB")
    assert deltas[True] < N * N * 4 // 2
    assert deltas[False] >= N * N * 4


# ---------------------------------------------------------------------------------------------------------------- rejections
def test_rejections(hip_lib):
    from cocosnet_amd import _lib, ops
    one, f = ctypes.c_void_p(16), ctypes.c_float
    err = hip_lib.cocos_last_error_string
    call = lambda K, Nk, k, stride=0, qh=one: hip_lib.cocos_corr_topk_f16x3(qh, one, one, one, one, one, one, 1, K, 64, Nk, k, f(100.0), f(16.0), stride, None)
    assert call(256, 64, 0) == -1 and b"k=0" in err()
    assert call(256, 64, 9) == -1 and b"k=9" in err()
    assert call(256, 4, 8) == -1 and b"Nk=4" in err()
    assert call(128, 64, 4) == -2 and b"K == 256" in err()
    assert call(256, 66, 4) == -2 and b"cocos_row_topk_lse" in err()
    assert call(256, 64, 4, stride=64) == -1 and b"k_batch_stride" in err()
    assert call(256, 64, 4, qh=ctypes.c_void_p(24)) == -1 and b"aligned" in err()
    assert hip_lib.cocos_row_topk_lse(one, one, one, one, 1, 4, 3, 4, None) == -1 and b"Nk=3" in err()
    q, kn, _, _ = _case(36, 8)
    planes = (*_planes(q), *_planes(kn))
    for bad in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="k="):
            ops._corr_topk_planes(*planes, INV_T, bad)
        with pytest.raises(ValueError, match="k="):
            ops.row_topk_lse(_randn(1, 4, 8, seed=1), bad)
    q4 = _planes(_case(36, 260)[1][:, :, :4].contiguous())
    with pytest.raises(ValueError, match="k=5"):
        ops._corr_topk_planes(*_planes(q), *q4, INV_T, 5)                       # k > Nk = 4
    with pytest.raises(ValueError, match="k=5"):
        ops.row_topk_lse(_randn(1, 4, 4, seed=1), 5)
    with pytest.raises(_lib.CocosHipError, match="multiple of 4") as e:          # Nk % 4 != 0: the message names K39b
        ops.corr_topk(_unit(_randn(1, 256, 8, seed=2)), _unit(_randn(1, 256, 6, seed=3)), INV_T, 2)
    assert e.value.unsupported
    with pytest.raises(ValueError, match="do not fit"):
        ops.gather_blend_patches(_randn(1, 3, 8, 8, seed=1), torch.zeros(1, 9, 2, 2, dtype=torch.int32, device=DEV), torch.ones(1, 9, 2, 2, device=DEV), 2, 2, 4)


# ---- red zones: the cases join tests/test_gpu_red_zones.py's table at import time, so its coverage report and its "every entry point was
# ---- reached" audit count the K39 entry points too (as tests/test_gpu_match.py does for K36).  Partial query / key tiles and k = 3:
# ---- a write past idx[B,Nq,k] or val[B,Nq,k] lands in a guard
def _rz_corr_topk(c):
    from cocosnet_amd import ops
    q, k = c.data(rz.unit(2, 256, 132, 31)), c.data(rz.unit(2, 256, 68, 32))
    return list(ops.corr_topk(q, k, 100.0, 3)) + list(ops.corr_topk(q, k, 100.0, 8))


def _rz_row_topk_lse(c):
    from cocosnet_amd import ops
    return list(ops.row_topk_lse(c.data(rz.rnd(2, 37, 68, seed=33)), 3)) + list(ops.row_topk_lse(c.data(rz.rnd(1, 5, 67, seed=34)), 8))


def _rz_gather_blend_patches(c):
    from cocosnet_amd import ops
    idx = c.data(torch.randint(0, 35, (2, 3, 5, 7), generator=torch.Generator().manual_seed(35)).to(torch.int32))
    w = c.data(torch.softmax(rz.rnd(2, 3, 5, 7, seed=37), dim=1))
    return [ops.gather_blend_patches(c.data(rz.uni(1, 3, 20, 28, seed=36)), idx, w, 5, 7, 4)]


RZ_CASES = {"corr_topk-2x132x68-k3+k8": _rz_corr_topk, "row_topk_lse-2x37x68-k3+1x5x67-k8": _rz_row_topk_lse,
            "gather_blend_patches-2x3x20x28-down4-k3": _rz_gather_blend_patches}
for _name, _body in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_every_new_op_inside_red_zones(name, monkeypatch):
    rz.test_red_zones(name, monkeypatch)
    want = {"corr_topk": "cocos_corr_topk_f16x3", "row_topk_lse": "cocos_row_topk_lse", "gather_blend_patches": "cocos_gather_blend_patches"}[name.split("-")[0]]
    assert want in set(rz.COVERAGE[name][0])


# ---------------------------------------------------------------------------------------------------------------- the warp family
# The copy, the blend and the sub-cell pair share one translation unit (gather_warp.hip), one pixel decode and one clamped match: the
# copy is the unweighted instantiation of the blend kernel.  Small odd shapes: 2 x 3 channels, a 3 x 5 grid of 2 x 2 cells.
def _bits(t):
    return t.contiguous().view(torch.int32)


def _index_copy(img, idx, grid, kgrid, down):
    """The hard warp by indexing alone (no arithmetic touches a pixel): cell (y, x) of `grid` receives the cell idx[b, y, x] (clamped)
    of the `kgrid` exemplar."""
    (fh, fw), (hk, wk) = grid, kgrid
    Bq, (Be, C) = idx.shape[0], img.shape[:2]
    up = lambda t: t.repeat_interleave(down, 1).repeat_interleave(down, 2)
    j = idx.reshape(Bq, fh, fw).long().clamp(0, hk * wk - 1)
    sy = up(torch.div(j, wk, rounding_mode="floor")) * down + (torch.arange(fh * down, device=img.device) % down).view(1, -1, 1)
    sx = up(j % wk) * down + (torch.arange(fw * down, device=img.device) % down).view(1, 1, -1)
    b = torch.arange(Bq, device=img.device).view(-1, 1, 1, 1) * (1 if Be == Bq else 0)
    return img[b, torch.arange(C, device=img.device).view(1, -1, 1, 1), sy[:, None], sx[:, None]]


def _special_case(Be):
    """img with a NaN of a non-default payload, a negative NaN, a -0 and both infinities in cells that idx names — through -1 and h*w
    (clamped to the first and the last cell) in sample 0, directly in sample 1"""
    Bq, C, h, w, down = 2, 3, 3, 5, 2
    img = _randn(Be, C, h * down, w * down, seed=70 + Be)
    bits = _bits(img)
    for b in range(Be):
        bits[b, 0, 0, 1], bits[b, 1, 1, 0] = 0x7FC12345, -0x3FEDCB         # cell 0: quiet NaNs with payloads, + and - (0xFFC01235)
        bits[b, 2, 4, 9], bits[b, 0, 5, 8], bits[b, 1, 5, 9] = -(2 ** 31), 0x7F800000, -0x800000      # cell 14: -0, +inf, -inf
    idx = torch.randint(0, h * w, (Bq, h, w), generator=torch.Generator().manual_seed(71)).to(DEV)
    idx[0, 0, 0], idx[0, 1, 2], idx[1, 2, 4], idx[1, 0, 3] = -1, h * w, 0, h * w - 1
    return img, idx, (Bq, C, h, w, down)


@pytest.mark.parametrize("Be", [1, 2])
def test_copy_instantiation_moves_bits_and_blend_of_one_agrees_on_finite_pixels(Be):
    """img_batch_stride 0 (Be = 1) and dense (Be = 2): the copy equals the index gather on the int32 view — NaN payloads, -0 and the
    infinities included; the blend with k = 1 and w = 1 equals the copy at every finite pixel (1 * p is p there; a NaN's payload is
    not promised)."""
    from cocosnet_amd import ops
    img, idx, (Bq, C, h, w, down) = _special_case(Be)
    out = ops.gather_patches(img, idx, h, w, down)
    want = _index_copy(img, idx, (h, w), (h, w), down)
    assert int(torch.isnan(want).sum()) >= 4 and int(torch.isinf(want).sum()) >= 4 and int((_bits(want) == -(2 ** 31)).sum()) >= 2
    assert torch.equal(_bits(out), _bits(want))
    one = ops.gather_blend_patches(img, idx.reshape(Bq, 1, h, w), torch.ones(Bq, 1, h, w, device=DEV), h, w, down)
    finite = torch.isfinite(out)
    assert torch.equal(_bits(one)[finite], _bits(out)[finite]) and bool(torch.isnan(one[torch.isnan(out)]).all())
    assert torch.equal(one[torch.isinf(out)], out[torch.isinf(out)])


def _fma_f32(a, b, c):
    """fma(a, b, c) of fp32 numpy arrays, correctly rounded: the product is exact in fp64; its sum with c is split into hi + lo
    (two-sum), and where hi lies exactly half way between two fp32 numbers the sign of lo decides instead of the tie rule"""
    import numpy as np
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    hi = p + c
    t = hi - p
    lo = (p - (hi - t)) + (c - t)
    r = hi.astype(np.float32)
    other = np.nextafter(r, np.where(hi > r, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    tie = (np.abs(hi - r.astype(np.float64)) == np.abs(other.astype(np.float64) - hi)) & (lo != 0) & (hi != r)
    towards_other = (lo > 0) == (other > r)
    return np.where(tie & towards_other, other, r).astype(np.float32)


@pytest.mark.parametrize("Be", [1, 2])
def test_blend_of_three_patches_in_the_written_order_bitwise(Be):
    """acc = w_0 p_0 (one fp32 product), then acc = fma(w_r, p_r, acc), r = 1, 2: restated in numpy with every rounding where the
    kernel has it — bit for bit, so a changed order of the taps or a product rounded before its add shows"""
    import numpy as np
    from cocosnet_amd import ops
    Bq, C, h, w, down, k = 2, 3, 3, 5, 2, 3
    img = _randn(Be, C, h * down, w * down, seed=80 + Be)
    idx = torch.randint(0, h * w, (Bq, k, h, w), generator=torch.Generator().manual_seed(81)).to(DEV)
    idx[0, 1, 0, 0], idx[1, 2, 2, 4] = -1, h * w
    wt = torch.softmax(_randn(Bq, k, h, w, seed=82) * 2, dim=1)
    out = ops.gather_blend_patches(img, idx, wt, h, w, down)
    px = [_index_copy(img, idx[:, r], (h, w), (h, w), down).cpu().numpy() for r in range(k)]
    wr = [wt[:, r].reshape(Bq, 1, h, w).repeat_interleave(down, 2).repeat_interleave(down, 3).expand(-1, C, -1, -1).cpu().numpy() for r in range(k)]
    acc = (wr[0] * px[0]).astype(np.float32)
    for r in range(1, k):
        acc = _fma_f32(wr[r], px[r], acc)
    assert np.array_equal(out.cpu().numpy().view(np.int32), acc.view(np.int32))


def test_subcell_pair_on_two_grids_with_border_and_nan_offsets():
    """A 3 x 4 content grid against a 2 x 5 exemplar grid, down = 2; offsets 0, +-0.5 (exact pixel positions: the right derivative),
    one pushing past each border and one NaN.  off == 0 is the copy bit for bit; the forward against tests/match_refine_case.py within
    tests/test_gpu_match_refine.py's 1e-6, d off against tests/match_flow_case.py by tests/test_gpu_match_flow.py's 4 x rule; the NaN
    offset makes its own cell NaN (forward and gradient) and no other."""
    import numpy as np
    import match_flow_case as fc
    import match_refine_case as mc
    from cocosnet_amd import ops
    from test_gpu_match_flow import _judge
    from test_gpu_parity import rel
    grid, kgrid, down, C = (3, 4), (2, 5), 2, 3
    nq, nk = grid[0] * grid[1], kgrid[0] * kgrid[1]
    g = torch.Generator().manual_seed(90)
    for Be in (2, 1):
        img = torch.rand(Be, C, kgrid[0] * down, kgrid[1] * down, generator=g) * 2 - 1
        idx = torch.randint(0, nk, (2, nq), generator=g)
        off = torch.zeros(2, nq, 2)
        off[0, 1], off[0, 2], off[1, 3] = torch.tensor((0.5, -0.5)), torch.tensor((-0.5, 0.5)), torch.tensor((0.5, 0.5))
        idx[0, 4], idx[0, 5], idx[0, 6], idx[0, 7] = 0, kgrid[1] - 1, 0, nk - 1              # left, right, top, bottom
        off[0, 4], off[0, 5], off[0, 6], off[0, 7] = (torch.tensor(o) for o in ((-1.3, 0.3), (1.3, 0.3), (0.3, -1.3), (0.3, 1.3)))
        idx[1, 0], idx[1, 1] = -1, nk                                                          # clamped matches
        nan_cell = (1, 9)
        zero = ops.gather_patches_subcell(img.to(DEV), idx.to(DEV), torch.zeros(2, nq, 2, device=DEV), grid, kgrid, down)
        assert torch.equal(_bits(zero), _bits(_index_copy(img.to(DEV), idx.to(DEV), grid, kgrid, down)))
        dout = torch.randn(2, C, grid[0] * down, grid[1] * down, generator=g)
        with_nan = off.clone()
        with_nan[nan_cell] = float("nan")
        leaf = with_nan.to(DEV).requires_grad_(True)
        out = ops.subcell_warp(img.to(DEV), idx.to(DEV), leaf, grid, kgrid, down)
        out.backward(dout.to(DEV))
        assert torch.equal(_bits(out), _bits(ops.gather_patches_subcell(img.to(DEV), idx.to(DEV), with_nan.to(DEV), grid, kgrid, down)))
        # the NaN cell: its 2 x 2 pixels of every channel, its two gradients; then it is set aside (the arbiter is run without it)
        y, x = divmod(nan_cell[1], grid[1])
        cell = out[nan_cell[0], :, y * down:(y + 1) * down, x * down:(x + 1) * down]
        assert bool(torch.isnan(cell).all()) and int(torch.isnan(out).sum()) == cell.numel()
        assert bool(torch.isnan(leaf.grad[nan_cell]).all()) and int(torch.isnan(leaf.grad).sum()) == 2
        got, dgot = out.detach().clone(), leaf.grad.clone()
        got[nan_cell[0], :, y * down:(y + 1) * down, x * down:(x + 1) * down] = zero[nan_cell[0], :, y * down:(y + 1) * down, x * down:(x + 1) * down]
        want = mc.gather_subcell(img.numpy(), idx.numpy(), off.numpy(), grid, kgrid, down)
        err = rel(got, want)
        print(f"[warp family] sub-cell forward Be={Be}: rel {err:.3e} (bound 1e-06)")
        assert err <= 1e-6
        dwant = fc.gather_bwd_off(img.numpy(), idx.numpy(), off.numpy(), dout.numpy(), grid, kgrid, down)
        arm = fc.t_gather_bwd_off(img.to(DEV), idx.to(DEV), off.to(DEV), dout.to(DEV), grid, kgrid, down)
        dgot[nan_cell] = torch.from_numpy(dwant[nan_cell]).float().to(DEV)
        _judge(f"3x4 on 2x5 down=2 Be={Be}", "doff", dgot, arm, dwant)
        for cell_i, axis in ((4, 0), (5, 0), (6, 1), (7, 1)):
            assert float(leaf.grad[0, cell_i, axis]) == 0.0 and dwant[0, cell_i, axis] == 0.0
