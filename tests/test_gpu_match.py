"""K36 match readout on the GPU: the fused kernel (K36a, cocos_corr_match_f16x3), the one-sweep reader of a materialised matrix (K36b,
cocos_row_argmax_lse), the hard warp (K36c, cocos_gather_patches) and the module-level `NoVGGCorrespondence.match`.

The arbiter of K36a is torch fp64 on the device: L = inv_t * qn^T kn from the fp32 unit-norm inputs.

E_FWD / TOL.  E_FWD is the largest |lse - logsumexp L| of the forward kernel cocos_corr_softmax_warp_fwd_f16x3 (called with a one-channel
V: the same three-term f16 arithmetic) over the four shapes of this file, shared and dense keys — `test_forward_kernel_lse_error_is_what_tol_was_set_from`
measures it again on every run and prints it.  TOL = 4 * E_FWD: the factor allows for another accumulation and merge order.  Every query is
judged, none excluded; `L[idx] >= max L - TOL` holds for a correct kernel whatever the gap to the runner-up is."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded_alloc import guarded  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

#: measured on an MI355X with the inputs of `_case` below (inv_t = 100, B = 3): max |lse - logsumexp L| of the forward kernel over the
#: eight cases was 9.694e-06 (the (256,128) dense one; the others 6.8e-06 .. 8.9e-06).  E_FWD is that figure rounded up in its third digit;
#: TOL = 4 * E_FWD = 3.88e-05
E_FWD = 9.70e-6
TOL = 4 * E_FWD
INV_T = 100.0
B = 3
SHAPES = [(64, 64), (256, 128), (132, 68), (36, 260)]      # partial query / key tiles, several key stages, a last tile of 4 keys
FP32_EPS = torch.finfo(torch.float32).eps


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def _unit(x):
    """fp32 unit-norm columns of x [B,K,N] (normalised in fp64)"""
    x = x.double()
    return (x / x.norm(dim=1, keepdim=True)).float().contiguous()


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


_CASES = {}


def _case(Nq, Nk):
    """(q [B,256,Nq], k [B,256,Nk], L dense fp64, L shared fp64): made once per shape, shared by the tests, never written"""
    if (Nq, Nk) not in _CASES:
        q, k = _unit(_randn(B, 256, Nq, seed=Nq)), _unit(_randn(B, 256, Nk, seed=1000 + Nk))
        _CASES[(Nq, Nk)] = (q, k, _arbiter(q, k), _arbiter(q, k[:1].expand(B, -1, -1)))
    return _CASES[(Nq, Nk)]


def _arbiter(q, k):
    return INV_T * torch.einsum("bci,bcj->bij", q.double(), k.double())


def _planes(x):
    from cocosnet_amd import ops
    return ops.split_f16(x, True, ops.SPLIT_OPERAND_SCALE)


def _match(q, k, shared):
    from cocosnet_amd import ops
    return ops._corr_match_planes(*_planes(q), *_planes(k[:1].contiguous() if shared else k), INV_T)


def _judge(tag, idx, mx, lse, L, check=True):
    tol = TOL
    Nk = L.shape[2]
    assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) < Nk, tag
    Lmax = L.max(dim=2).values
    picked = L.gather(2, idx.long().unsqueeze(2)).squeeze(2)
    e_pick = (Lmax - picked).max().item()
    e_max = (mx.double() - Lmax).abs().max().item()
    e_lse = (lse.double() - torch.logsumexp(L, dim=2)).abs().max().item()
    print(f"[match] {tag}: max L - L[idx] = {e_pick:.3e}  |max_out - max L| = {e_max:.3e}  |lse_out - logsumexp L| = {e_lse:.3e}  (tol {tol:.1e})")
    if check:
        assert e_pick <= tol, (tag, e_pick)
        assert e_max <= tol, (tag, e_max)
        assert e_lse <= tol, (tag, e_lse)


# ---------------------------------------------------------------------------------------------------------------- K36a
def test_forward_kernel_lse_error_is_what_tol_was_set_from():
    """E_FWD measured again: cocos_corr_softmax_warp_fwd_f16x3, one-channel V, the four shapes, shared and dense keys.
    This ties the file to that kernel's arithmetic on purpose (E_FWD is the record the tolerance comes from, with a margin of 0.06 %): a
    change to the forward kernel's accumulation order that moves its lse error fails HERE — then measure E again and set E_FWD from it."""
    from cocosnet_amd import _lib, ops
    worst = 0.0
    for Nq, Nk in SHAPES:
        q, k, L, Ls = _case(Nq, Nk)
        for shared in (False, True):
            kk = k[:1].expand(B, -1, -1).contiguous() if shared else k
            v = torch.ones(B, 1, Nk, device=DEV)
            (qh, ql), (kh, kl), (vh, vl) = _planes(q), _planes(kk), ops.split_f16(v, False, 1.0)
            out = torch.empty(B, 1, Nq, device=DEV)
            lse = torch.empty(B, Nq, device=DEV)
            _lib.call("cocos_corr_softmax_warp_fwd_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(), vh.data_ptr(),
                      vl.data_ptr(), out.data_ptr(), lse.data_ptr(), None, None, None, B, 256, Nq, Nk, 1, INV_T, ops.SPLIT_OPERAND_SCALE,
                      None, None, torch.cuda.current_stream().cuda_stream)
            e = (lse.double() - torch.logsumexp(Ls if shared else L, dim=2)).abs().max().item()
            print(f"[match] forward kernel ({Nq},{Nk}) {'shared' if shared else 'dense'}: |lse - logsumexp L| = {e:.3e}")
            worst = max(worst, e)
    print(f"[match] E (forward kernel) = {worst:.3e}; the file's E_FWD = {E_FWD:.3e}, TOL = {TOL:.3e}")
    assert worst <= E_FWD, f"the forward kernel's lse error {worst:.3e} is above the E_FWD = {E_FWD:.3e} that TOL was set from"


@pytest.mark.parametrize("shared", [False, True], ids=["dense", "shared"])
@pytest.mark.parametrize("Nq,Nk", SHAPES)
def test_random_inputs_every_query(Nq, Nk, shared):
    q, k, L, Ls = _case(Nq, Nk)
    idx, mx, lse = _match(q, k, shared)
    _judge(f"random ({Nq},{Nk}) {'shared' if shared else 'dense'}", idx, mx, lse, Ls if shared else L)


@pytest.mark.parametrize("Nq,Nk", SHAPES)
def test_shared_and_dense_keys_agree_bitwise(Nq, Nk):
    q, k, _, _ = _case(Nq, Nk)
    a = _match(q, k[:1].expand(B, -1, -1).contiguous(), False)
    b = _match(q, k, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("shared", [False, True], ids=["dense", "shared"])
@pytest.mark.parametrize("Nq,Nk", [(64, 64), (260, 260), (132, 68)])
def test_planted_matches_are_found_exactly(Nq, Nk, shared):
    """keys = a random permutation of (the first Nk) queries: cosine 1 against <~ 0.35 for every other key, a logit gap above 60.  A
    permutation puts a winner on every key, so on every residue mod 32 and into the last tile of 4 keys (68 = 2 x 32 + 4, 260 = 8 x 32 + 4).
    Shared keys: the one key set is taken from sample 0 and sample b's queries are sample 0's rolled by b positions.
    What is asserted is the index, exactly, at every planted query.  max_out / lse_out are printed only: a planted logit is 100, three times
    the largest logit of the random cases E_FWD was measured on, and the three-term arithmetic's error grows with it (the fp32 accumulator
    holds 256 * cos: one ulp at cos = 1 is 1.2e-05 in logit units) — TOL judges the random cases, as measured."""
    q0 = _unit(_randn(B, 256, Nq, seed=7 + Nq))
    src = torch.randperm(Nk, generator=torch.Generator().manual_seed(Nk)).to(DEV)      # key j is query src[j]
    if shared:
        q = torch.stack([q0[0].roll(b, dims=1) for b in range(B)]).contiguous()
        k = q0[:1, :, src].contiguous().expand(B, -1, -1).contiguous()
        planted = torch.stack([(src + b) % Nq for b in range(B)])                       # [B,Nk]: the query of key j in sample b
    else:
        q, k = q0, q0[:, :, src].contiguous()
        planted = src.unsqueeze(0).expand(B, -1)
    idx, mx, lse = _match(q, k, shared)
    want = torch.arange(Nk, device=DEV, dtype=torch.int32).unsqueeze(0).expand(B, -1)
    got = idx.gather(1, planted)
    assert torch.equal(got, want), f"{int((got != want).sum())} planted matches missed"
    L = _arbiter(q, k)
    top2 = L.topk(2, dim=2).values.gather(1, planted.unsqueeze(2).expand(-1, -1, 2))      # of the planted queries
    assert (top2[..., 0] - top2[..., 1]).min().item() > 60.0, "the planted gap this test relies on"
    _judge(f"planted ({Nq},{Nk}) {'shared' if shared else 'dense'}", idx, mx, lse, L, check=False)


@pytest.mark.parametrize("shared", [False, True], ids=["dense", "shared"])
def test_equal_logits_return_the_lowest_index(shared):
    """Duplicated key columns give bitwise-equal logits (the same products in the same order).  Per query one pair of copies of the query
    itself (cosine 1: the row maximum), placed so that every level of the merge has to break the tie — a 64-key stage is an even and an
    odd 32-key tile (one wave each), a lane holds the keys of its tile whose offset has bit 2 equal to lane >> 5:
      (1, 9)      one lane's registers: the scan inside a tile            (2, 5)      the two half-waves of one tile
      (3, 35)     even and odd tile of one stage: the merge through LDS   (70, 200)   two stages of the same wave: the strict `>`
      (100, 130)  the LOWER index sits with the odd-tile wave, the higher one in a later stage of the even-tile wave
      (44, 259)   an odd tile against the last tile of 4 keys"""
    Nq, Nk = 36, 260
    pairs = [(1, 9), (2, 5), (3, 35), (70, 200), (100, 130), (44, 259)]
    q, k, _, _ = _case(Nq, Nk)
    k = (k[:1].expand(B, -1, -1) if shared else k).clone()
    for i, (a, b) in enumerate(pairs):
        src = q[0] if shared else q          # shared keys: the copies are of sample 0's queries, judged in sample 0
        k[:, :, a] = src[..., i] if shared else src[:, :, i]
        k[:, :, b] = k[:, :, a]
    idx, mx, lse = _match(q, k.contiguous(), shared)
    L = _arbiter(q, k)
    samples = [0] if shared else list(range(B))
    for i, (a, b) in enumerate(pairs):
        for s_ in samples:
            assert L[s_, i, a] == L[s_, i, b] == L[s_, i].max(), "the arbiter's tie this test relies on"
            assert int(idx[s_, i]) == a, (f"pair {(a, b)} sample {s_}", int(idx[s_, i]))
    _judge(f"ties {'shared' if shared else 'dense'}", idx, mx, lse, L, check=False)


@pytest.mark.parametrize("shared", [False, True], ids=["dense", "shared"])
def test_all_negative_rows_ignore_padded_keys(shared):
    """all-positive queries against all-negative keys, Nk = 68: a zero-padded key of the last tile (logit 0) would win every row and would
    dominate every sum"""
    Nq, Nk = 36, 68
    q, k = _unit(_randn(B, 256, Nq, seed=3).abs() + 0.01), _unit(-_randn(B, 256, Nk, seed=4).abs() - 0.01)
    idx, mx, lse = _match(q, k, shared)
    assert float(mx.max()) < 0.0
    _judge(f"all-negative {'shared' if shared else 'dense'}", idx, mx, lse, _arbiter(q, k[:1].expand(B, -1, -1) if shared else k))


def test_non_finite_input_keeps_the_index_in_range():
    q, k, _, _ = _case(36, 260)
    q = q.clone()
    q[0, :, 3] = float("nan")
    q[1, :, 5] = float("inf")
    idx, _, _ = _match(q, k, False)
    assert int(idx.min()) >= 0 and int(idx.max()) < 260


def test_rejections(hip_lib):
    one = ctypes.c_void_p(16)
    f = ctypes.c_float
    call = lambda K, Nk, stride: hip_lib.cocos_corr_match_f16x3(one, one, one, one, one, one, one, 1, K, 64, Nk, f(100.0), f(16.0), stride, None)
    assert call(128, 64, 0) == -2 and b"K == 256" in hip_lib.cocos_last_error_string()
    assert call(256, 66, 0) == -2 and b"multiple of 4" in hip_lib.cocos_last_error_string()
    assert call(256, 64, 64) == -1 and b"k_batch_stride" in hip_lib.cocos_last_error_string()
    assert hip_lib.cocos_corr_match_f16x3(one, one, one, None, one, one, one, 1, 256, 64, 64, f(100.0), f(16.0), 0, None) == -1


# ---------------------------------------------------------------------------------------------------------------- K36b
@pytest.mark.parametrize("shape", [(2, 37, 68), (1, 256, 260)])
def test_row_argmax_lse(shape):
    from cocosnet_amd import ops
    f = _randn(*shape, seed=shape[1]) * 3.0
    fd = f.double()
    top2 = fd.topk(2, dim=2).values
    assert (top2[..., 0] > top2[..., 1]).all(), "the arbiter's row maxima must be unique for an exact index comparison"
    idx, mx, lse = ops.row_argmax_lse(f)
    assert idx.dtype == torch.int32 and torch.equal(idx.long(), torch.argmax(f, dim=2))
    assert torch.equal(mx, f.max(dim=2).values)                                   # bitwise: an element of the row
    want = torch.logsumexp(fd, dim=2)
    err = (lse.double() - want).abs()
    bound = 4 * FP32_EPS * (want.abs() + 1)
    print(f"[match] row_argmax_lse {shape}: max |lse - fp64| = {err.max().item():.3e}, bound >= {bound.min().item():.3e}")
    assert (err <= bound).all(), (err.max().item(), bound.min().item())


def test_row_argmax_lse_duplicated_maximum_and_odd_width():
    from cocosnet_amd import ops
    f = _randn(2, 5, 68, seed=11)
    f[:, :, 40] = 9.0
    f[:, :, 13] = 9.0
    f[0, 2, 3] = 9.0
    idx, mx, _ = ops.row_argmax_lse(f)
    want = torch.full((2, 5), 13, device=DEV, dtype=torch.int32)
    want[0, 2] = 3
    assert torch.equal(idx, want) and bool((mx == 9.0).all())
    g = _randn(3, 7, 67, seed=12)                                                  # rows that are not 16-byte aligned: the dword sweep
    idx, mx, lse = ops.row_argmax_lse(g)
    assert torch.equal(idx.long(), torch.argmax(g, dim=2)) and torch.equal(mx, g.max(dim=2).values)
    want = torch.logsumexp(g.double(), dim=2)
    assert ((lse.double() - want).abs() <= 4 * FP32_EPS * (want.abs() + 1)).all()


# ---------------------------------------------------------------------------------------------------------------- K36c
def _gather_reference(img, idx, h, w, down):
    """torch.gather construction: patches as columns [B, C*down*down, h*w], gathered along the positions, folded back"""
    Bq, C = idx.shape[0], img.shape[1]
    cols = torch.nn.functional.unfold(img, down, stride=down)
    if cols.shape[0] != Bq:
        cols = cols.expand(Bq, -1, -1)
    got = cols.gather(2, idx.reshape(Bq, 1, h * w).long().expand(-1, cols.shape[1], -1))
    return torch.nn.functional.fold(got, (h * down, w * down), down, stride=down)


@pytest.mark.parametrize("Be", [1, 2])
@pytest.mark.parametrize("down", [2, 4])
def test_gather_patches_is_a_bitwise_copy(down, Be):
    from cocosnet_amd import ops
    Bq, C, h, w = 2, 3, 5, 7
    img = _randn(Be, C, h * down, w * down, seed=down)
    idx = torch.randint(0, h * w, (Bq, h * w), generator=torch.Generator().manual_seed(Be)).to(DEV)
    idx[:, :4] = torch.tensor([0, w - 1, (h - 1) * w, h * w - 1], device=DEV)      # the four corners of the grid
    for ix in (idx, idx.to(torch.int32).reshape(Bq, h, w)):
        out = ops.gather_patches(img, ix, h, w, down)
        assert torch.equal(out, _gather_reference(img, idx, h, w, down))


# ---------------------------------------------------------------------------------------------------------------- the module
def _module(options, mk, Be=2, crop=64):
    from test_gpu_exemplar import _module_case
    return _module_case(options, crop, 2, Be, match_kernel=mk)


def _rep(t, n):
    return t if t.shape[0] == n else t.expand(n, -1, -1, -1).contiguous()


def _check_against_corr(tag, out, corr, exact):
    """every position: corr[b, i, match_index] against the row maximum of the matrix forward(return_corr=True) returned"""
    idx = out["match_index"].reshape(corr.shape[0], -1)
    picked = corr.gather(2, idx.unsqueeze(2)).squeeze(2)
    cmax = corr.max(dim=2).values
    gap = (cmax - picked).max().item()
    want_p = torch.softmax(corr.double(), dim=2).max(dim=2).values
    got_p = out["match_prob"].reshape(corr.shape[0], -1).double()
    e_p = ((got_p - want_p).abs() / want_p).max().item()
    e_lse = (out["match_lse"].reshape(corr.shape[0], -1).double() - torch.logsumexp(corr.double(), dim=2)).abs().max().item()
    print(f"[match] {tag}: max corr - corr[idx] = {gap:.3e}  rel |prob - softmax max| = {e_p:.3e}  |lse - logsumexp corr| = {e_lse:.3e}")
    if exact:
        assert gap == 0.0, (tag, gap)
    else:
        assert gap <= TOL, (tag, gap)
    # prob = exp(max - lse) with both within TOL of the matrix's: a factor exp(+-2 TOL); 4 eps for the fp32 exp and subtraction
    assert e_p <= math.expm1(2 * TOL) + 4 * FP32_EPS * (1 + corr.abs().max().item()), (tag, e_p)
    xy = out["match_xy"]
    gw = out["match_index"].shape[2]
    assert torch.equal(xy[:, 1] * gw + xy[:, 0], out["match_index"])


@pytest.mark.parametrize("options,mk,fused", [("ade20k_options", 1, True), ("celebahq_edge_options", 1, True),
                                              ("ade20k_options", 3, True), ("celebahq_edge_options", 3, True),
                                              ("ade20k_options", 1, False)],
                         ids=["ade20k-mk1", "celebahq-mk1", "ade20k-mk3", "celebahq-mk3", "ade20k-mk1-MATCH_FUSED_off"])
def test_module_match_against_return_corr(options, mk, fused, monkeypatch):
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "MATCH_FUSED", fused)
    net, ref_img, real, seg, ref_seg = _module(options, mk)
    with torch.no_grad():
        before = net(ref_img, real, seg, ref_seg)
        corr = net(ref_img, real, seg, ref_seg, return_corr=True)
        rows = net.match(ref_img, seg, ref_seg, hard_warp=True)
        cols = net.match(ref_img, seg, ref_seg, direction="cols")
        after = net(ref_img, real, seg, ref_seg)
    materialised = mk == 3 or not fused
    _check_against_corr(f"{options} mk{mk} rows", rows, corr, exact=materialised)
    _check_against_corr(f"{options} mk{mk} cols", cols, corr.transpose(1, 2), exact=False)
    fh, fw = rows["match_index"].shape[1:]
    assert torch.equal(rows["warp_hard"], _gather_reference(ref_img, rows["match_index"].reshape(2, -1), fh, fw, net.opt.down))
    assert not any(v.requires_grad for v in rows.values())
    assert sorted(before) == sorted(after)
    for k in before:      # nothing is cached across calls
        assert torch.equal(before[k], after[k]), k


@pytest.mark.parametrize("Be", [1, 2])
@pytest.mark.parametrize("mk", [1, 3])
def test_module_match_with_a_prepared_exemplar(mk, Be):
    """match() with a record against forward(return_corr=True)'s matrix AND against the ordinary match(), index, prob and lse, both
    directions, with the bounds of _check_against_corr"""
    from cocosnet_amd import inference
    net, ref_img, real, seg, ref_seg = _module("ade20k_options", mk, Be=Be)
    with torch.no_grad():
        corr = net(_rep(ref_img, 2), real, seg, _rep(ref_seg, 2), return_corr=True)
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
        for direction in ("rows", "cols"):
            c = corr if direction == "rows" else corr.transpose(1, 2)
            plain = net.match(_rep(ref_img, 2), seg, _rep(ref_seg, 2), direction=direction)
            got = net.match(None, seg, None, exemplar=rec, direction=direction, hard_warp=direction == "rows")
            _check_against_corr(f"record Be={Be} mk{mk} {direction}", got, c, exact=False)
            pick = lambda o: c.gather(2, o["match_index"].reshape(2, -1).unsqueeze(2)).squeeze(2)
            d_idx = (pick(plain) - pick(got)).max().item()
            same = (got["match_index"] == plain["match_index"]).float().mean().item()
            rel = ((got["match_prob"].double() - plain["match_prob"].double()).abs() / plain["match_prob"].double()).max().item()
            d_lse = (got["match_lse"].double() - plain["match_lse"].double()).abs().max().item()
            print(f"[match] record Be={Be} mk{mk} {direction} against the ordinary match(): corr[idx_plain] - corr[idx_record] = {d_idx:.3e} "
                  f"(equal indices: {same:.4f})  rel |prob| = {rel:.3e}  |lse| = {d_lse:.3e}")
            assert d_idx <= TOL
            assert rel <= math.expm1(2 * TOL) + 4 * FP32_EPS * (1 + corr.abs().max().item())
            assert d_lse <= TOL
            if direction == "rows":
                fh, fw = got["match_index"].shape[1:]
                assert torch.equal(got["warp_hard"], _gather_reference(ref_img, got["match_index"].reshape(2, -1), fh, fw, net.opt.down))


def test_fused_route_allocates_nothing_hw_by_hw(monkeypatch):
    """B = 1, 64 x 64 grid: the peak above the live memory stays below half of the matrix (the four operand planes are 8 MiB); with
    MATCH_FUSED off the same probe sees the matrix"""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match
    N = 64 * 64
    theta, phi = _randn(1, 256, 64, 64, seed=21), _randn(1, 256, 64, 64, seed=22)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    deltas = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "MATCH_FUSED", fused)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m = correspondence_match(theta, phi, cfg)
        torch.cuda.synchronize()
        deltas[fused] = torch.cuda.max_memory_allocated() - base
        assert m.index.shape == (1, 64, 64)
        del m
    print(f"[match] peak memory above live: fused {deltas[True] / 2**20:.1f} MiB, materialised {deltas[False] / 2**20:.1f} MiB")
    assert deltas[True] < N * N * 4 // 2
    assert deltas[False] >= N * N * 4


# ---------------------------------------------------------------------------------------------------------------- guards
def test_match_inside_red_zones_reaches_the_three_entry_points(monkeypatch):
    from cocosnet_amd import ops
    net, ref_img, real, seg, ref_seg = _module("ade20k_options", 1)
    entries = set()
    for fused in (True, False):
        monkeypatch.setattr(ops, "MATCH_FUSED", fused)
        with guarded() as g:
            out = net.match(g.place(ref_img), g.place(seg), g.place(ref_seg), hard_warp=True)
            bad = g.check()
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(v).all()) for v in out.values() if v.is_floating_point())
        assert bad == [] and g.violations == [], g.report()
        assert ("cocos_corr_match_f16x3" if fused else "cocos_row_argmax_lse") in g.entries
        entries |= g.entries
    assert {"cocos_corr_match_f16x3", "cocos_row_argmax_lse", "cocos_gather_patches"} <= entries


def test_match_hands_over_live_buffers_only(monkeypatch):
    import test_gpu_live_buffers as lb
    from cocosnet_amd import ops
    net, ref_img, real, seg, ref_seg = _module("ade20k_options", 1)
    guard = lb._Guard(monkeypatch)
    for fused in (True, False):
        monkeypatch.setattr(ops, "MATCH_FUSED", fused)
        net.match(ref_img, seg, ref_seg, hard_warp=True)
        net.match(ref_img, seg, ref_seg, direction="cols")
    guard.check(40, 150)


# ---- red zones: the cases join tests/test_gpu_red_zones.py's table through its own helpers, so its coverage report and its "every
# ---- entry point was reached" audit count the K36 entry points too (as tests/test_gpu_label_conv.py does for K35)
import test_gpu_red_zones as rz  # noqa: E402


def _rz_corr_match(c):
    from cocosnet_amd import ops
    q, k = c.data(rz.unit(2, 256, 132, 31)), c.data(rz.unit(2, 256, 68, 32))
    return list(ops.corr_match(q, k, 100.0))


def _rz_row_argmax_lse(c):
    from cocosnet_amd import ops
    return list(ops.row_argmax_lse(c.data(rz.rnd(2, 37, 68, seed=33)))) + list(ops.row_argmax_lse(c.data(rz.rnd(1, 5, 67, seed=34))))


def _rz_gather_patches(c):
    from cocosnet_amd import ops
    idx = c.data(torch.randint(0, 35, (2, 35), generator=torch.Generator().manual_seed(35)).to(torch.int32))
    return [ops.gather_patches(c.data(rz.uni(1, 3, 20, 28, seed=36)), idx, 5, 7, 4)]


RZ_CASES = {"corr_match-2x132x68": _rz_corr_match, "row_argmax_lse-2x37x68+1x5x67": _rz_row_argmax_lse, "gather_patches-2x3x20x28-down4": _rz_gather_patches}
for _name, _body in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_every_new_op_inside_red_zones(name, monkeypatch):
    rz.test_red_zones(name, monkeypatch)
    want = {"corr_match": "cocos_corr_match_f16x3", "row_argmax_lse": "cocos_row_argmax_lse", "gather_patches": "cocos_gather_patches"}[name.split("-")[0]]
    assert want in set(rz.COVERAGE[name][0])
