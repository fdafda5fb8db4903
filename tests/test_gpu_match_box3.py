"""K37 on the GPU: the match readout of the fused match_kernel-3 family (cocos_box3_match_f16x3), `ops.box3_match`, `_BoxedCorr.match`
and the third route of `correspondence_match` / `NoVGGCorrespondence.match`.

The arbiter is torch fp64 on the device, the reference's own formulation (the way tests/test_gpu_mk3_sizes.py's oracle forms it):
F.unfold(k = 3, padding 1) -> centre over the 2304 entries -> / (norm + eps) -> matmul -> * inv_t  =  L64 [B,N,N].

E_BOX / TOL (the method of tests/test_gpu_match.py).  E_BOX is the largest |lse - logsumexp L64| of the EXISTING forward kernel
cocos_box3_softmax_warp_fwd_f16x3, called through the C ABI with a one-channel V on this file's five grids, both directions —
`test_forward_kernel_lse_error_is_what_tol_was_set_from` measures it again on every run.  TOL = 4 * E_BOX: K36's margin, for the
exact-maximum against lazy-rescale difference in summation order and box-to-box variation.  Every query is judged, none excluded."""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded_alloc import guarded  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

#: measured on an MI355X with the inputs of `_case` below (inv_t = 100): max |lse - logsumexp L64| of the forward kernel per grid, rows /
#: transposed: (4,64) 9.657e-06 / 9.048e-06, (8,64) 1.210e-05 / 9.835e-06, (2,128) 5.688e-06 / 5.328e-06, (6,128) 8.884e-06 / 9.498e-06,
#: (40,128) 1.312e-05 / 1.162e-05.  E_BOX is the largest of them, 1.3123e-05, rounded up in its third digit; TOL = 4 * E_BOX = 5.28e-05
E_BOX = 1.32e-5
TOL = 4 * E_BOX
INV_T = 100.0
KC = 2304.0
GRIDS = [(4, 64, 2), (8, 64, 2), (2, 128, 2), (6, 128, 2), (40, 128, 1)]      # (h, w, B); (40,128): Nk = 5120 > 4096, the chunk ring
GRID_IDS = [f"{h}x{w}" for h, w, _ in GRIDS]
FP32_EPS = torch.finfo(torch.float32).eps
EPS = sys.float_info.epsilon


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _arbiter(theta, phi):
    """L64[b,p,q] = inv_t * <U_p, V_q> of the unfolded, centred, normalised vectors (correspondence.py:276-291, :304) in fp64"""
    def unit(x):
        u = F.unfold(x.double(), kernel_size=3, padding=1)
        u = u - u.mean(dim=1, keepdim=True)
        return u / (torch.norm(u, 2, 1, keepdim=True) + EPS)
    return INV_T * torch.matmul(unit(theta).transpose(1, 2), unit(phi))


def _operands(theta, phi):
    """(T blocked, mu, a, nu, b) as _BoxedCorr obtains them"""
    from cocosnet_amd import ops
    with torch.no_grad():
        mu, a = ops.unfold3_stats(theta, KC)
        nu, b = ops.unfold3_stats(phi, KC)
        t = ops.box3_corr_xbox(theta, phi)
    return t, mu, a, nu, b


_CASES = {}


def _case(h, w, B):
    """(theta, phi, operands, L64): made once per grid, shared by the tests, never written.  phi carries a weak shifted copy of theta
    (3x3 neighbourhoods only discriminate when neighbouring positions differ) under noise: logits of a trained network's size"""
    if (h, w) not in _CASES:
        theta = _randn(B, 256, h, w, seed=100 * h + w) + 0.1
        phi = 0.3 * theta.roll((1, 7), (2, 3)) + _randn(B, 256, h, w, seed=100 * h + w + 1) - 0.05
        _CASES[(h, w)] = (theta, phi, _operands(theta, phi), _arbiter(theta, phi))
    return _CASES[(h, w)]


def _match(ops_tuple, h, w, transposed):
    from cocosnet_amd import ops
    t, mu, a, nu, b = ops_tuple
    if transposed:
        return ops.box3_match(t, nu, b, mu, a, h, w, KC, INV_T, transposed=True)
    return ops.box3_match(t, mu, a, nu, b, h, w, KC, INV_T)


def _forward_kernel_lse(ops_tuple, h, w, transposed):
    """row log-sum-exp of the EXISTING cocos_box3_softmax_warp_fwd_f16x3 through the C ABI, one-channel V of ones"""
    from cocosnet_amd import _lib, ops
    t, mu, a, nu, b = ops_tuple
    if transposed:
        mu, a, nu, b = nu, b, mu, a
    B, N = mu.shape
    vh, vl = ops.split_f16(torch.ones(B, 1, N, device=DEV), False, 1.0)
    out, lse = torch.empty(B, 1, N, device=DEV), torch.empty(B, N, device=DEV)
    _lib.call("cocos_box3_softmax_warp_fwd_f16x3", t.data_ptr(), mu.data_ptr(), a.data_ptr(), nu.data_ptr(), b.data_ptr(), vh.data_ptr(),
              vl.data_ptr(), out.data_ptr(), lse.data_ptr(), None, None, B, N, N, 1, h, w, KC, INV_T, 1 if transposed else 0,
              torch.cuda.current_stream().cuda_stream)
    return lse


def _judge(tag, idx, mx, lse, L, check=True, tol=None):
    tol = TOL if tol is None else tol
    Nk = L.shape[2]
    assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) < Nk, tag
    Lmax = L.max(dim=2).values
    picked = L.gather(2, idx.long().unsqueeze(2)).squeeze(2)
    e_pick = (Lmax - picked).max().item()
    e_max = (mx.double() - Lmax).abs().max().item()
    e_lse = (lse.double() - torch.logsumexp(L, dim=2)).abs().max().item()
    print(f"[match-box3] {tag}: max L - L[idx] = {e_pick:.3e}  |max_out - max L| = {e_max:.3e}  |lse_out - logsumexp L| = {e_lse:.3e}  "
          f"(tol {tol:.2e}; max |L| = {L.abs().max().item():.1f})")
    if check:
        assert e_pick <= tol, (tag, e_pick)
        assert e_max <= tol, (tag, e_max)
        assert e_lse <= tol, (tag, e_lse)


# ---------------------------------------------------------------------------------------------------------------- the kernel
def test_forward_kernel_lse_error_is_what_tol_was_set_from():
    """E_BOX measured again: cocos_box3_softmax_warp_fwd_f16x3, one-channel V, the five grids, rows and transposed.  This ties the file
    to that kernel's arithmetic on purpose: a change that moves its lse error fails HERE — then measure again and set E_BOX from it."""
    worst = 0.0
    for h, w, B in GRIDS:
        _, _, opnd, L = _case(h, w, B)
        for transposed in (False, True):
            lse = _forward_kernel_lse(opnd, h, w, transposed)
            e = (lse.double() - torch.logsumexp(L.transpose(1, 2) if transposed else L, dim=2)).abs().max().item()
            print(f"[match-box3] forward kernel ({h},{w}) {'transposed' if transposed else 'rows'}: |lse - logsumexp L64| = {e:.3e}")
            worst = max(worst, e)
    print(f"[match-box3] E (forward kernel) = {worst:.3e}; the file's E_BOX = {E_BOX:.3e}, TOL = {TOL:.3e}")
    assert worst <= E_BOX, f"the forward kernel's lse error {worst:.3e} is above the E_BOX = {E_BOX:.3e} that TOL was set from"


@pytest.mark.parametrize("transposed", [False, True], ids=["rows", "transposed"])
@pytest.mark.parametrize("h,w,B", GRIDS, ids=GRID_IDS)
def test_random_inputs_every_query(h, w, B, transposed):
    _, _, opnd, L = _case(h, w, B)
    idx, mx, lse = _match(opnd, h, w, transposed)
    k19 = _forward_kernel_lse(opnd, h, w, transposed)
    print(f"[match-box3] ({h},{w}) {'transposed' if transposed else 'rows'}: |lse_K37 - lse_K19| on the same T = {(lse - k19).abs().max().item():.3e}")
    _judge(f"random ({h},{w}) {'transposed' if transposed else 'rows'}", idx, mx, lse, L.transpose(1, 2) if transposed else L)


# ---- synthetic T: the layout documented in include/cocos_hip.h — [B][Nk/32][Nq/32] blocks of [g 0..3][lane 0..63][4 floats], registers
# ---- 4g..4g+3 of a lane = keys 8g + 4 (lane >> 5) + 0..3, lane & 31 = query
def _block(M):
    """M [B,Nk,Nq] (keys in the rows) -> the blocked 1-D tensor"""
    B, Nk, Nq = M.shape
    x = M.reshape(B, Nk // 32, 4, 2, 4, Nq // 32, 32)          # b, kt, g, h, e, qb, c
    return x.permute(0, 1, 5, 2, 3, 6, 4).contiguous().reshape(-1)      # b, kt, qb, g, h, c, e


def _unblock(t, B, Nk, Nq):
    x = t.reshape(B, Nk // 32, Nq // 32, 4, 2, 32, 4)          # b, kt, qb, g, h, c, e
    return x.permute(0, 1, 3, 4, 6, 2, 5).contiguous().reshape(B, Nk, Nq)


def _ybox64(M, w):
    """fp64 y box of the unblocked tensor: Y[k,q] = M[k-w,q-w] + M[k,q] + M[k+w,q+w], zero outside the grid"""
    M = M.double()
    Y = M.clone()
    Y[:, w:, w:] += M[:, :-w, :-w]
    Y[:, :-w, :-w] += M[:, w:, w:]
    return Y


def test_block_helper_inverts_and_matches_the_gemm_layout():
    """the helper is its own inverse, and unblocking the GEMM's T gives xbox(C): ybox of it * the statistics is L64 (loosely: the
    tight comparison is test_random_inputs_every_query; this pins the helper's index order to the kernel's)"""
    M = _randn(2, 64, 96, seed=5)
    assert torch.equal(_unblock(_block(M), 2, 64, 96), M)
    h, w, B = GRIDS[0]
    theta, phi, (t, mu, a, nu, b), L = _case(h, w, B)
    Y = _ybox64(_unblock(t, B, h * w, h * w), w).transpose(1, 2)      # [B, query, key]
    z = INV_T * a.double().unsqueeze(2) * b.double().unsqueeze(1) * (Y - KC * mu.double().unsqueeze(2) * nu.double().unsqueeze(1))
    assert (z - L).abs().max().item() < 1e-3


@pytest.mark.parametrize("h,w,B", [(4, 64, 2), (6, 128, 2), (40, 128, 1)], ids=["4x64", "6x128", "40x128"])
def test_synthetic_t_against_an_fp64_y_box(h, w, B):
    """random T, random positive a / b: K37 alone, without the GEMM.  Scales chosen so that the logits are of the size of the random cases
    E_BOX was measured on (|z| up to ~20)"""
    from cocosnet_amd import ops
    N = h * w
    M = _randn(B, N, N, seed=7 + h)                                  # keys in the rows
    u = lambda s: torch.rand(B, N, generator=torch.Generator().manual_seed(s)).to(DEV)
    a, b = 0.1 + 0.1 * u(1), 0.1 + 0.1 * u(2)
    mu, nu = 0.02 * _randn(B, N, seed=3), 0.02 * _randn(B, N, seed=4)
    Y = _ybox64(M, w).transpose(1, 2)                                # [B, query, key]
    z = INV_T * a.double().unsqueeze(2) * b.double().unsqueeze(1) * (Y - KC * mu.double().unsqueeze(2) * nu.double().unsqueeze(1))
    t = _block(M)
    _judge(f"synthetic ({h},{w}) rows", *ops.box3_match(t, mu, a, nu, b, h, w, KC, INV_T), z)
    # the same tensor read transposed: the roles of the two sides exchanged
    _judge(f"synthetic ({h},{w}) transposed", *ops.box3_match(t, nu, b, mu, a, h, w, KC, INV_T, transposed=True), z.transpose(1, 2))


@pytest.mark.parametrize("transposed", [False, True], ids=["rows", "transposed"])
@pytest.mark.parametrize("h,w", [(4, 64), (40, 128)], ids=["4x64", "40x128"])
def test_equal_logits_return_the_lowest_index(h, w, transposed):
    """T = 0, mu = nu = 0: every logit is 0 — index 0 everywhere (the lowest among equals through the register scan, the tile loop and
    the half-wave merge), max 0, lse = log Nk"""
    from cocosnet_amd import ops
    B, N = 1, h * w
    z, one = torch.zeros(B, N, device=DEV), torch.ones(B, N, device=DEV)
    idx, mx, lse = ops.box3_match(torch.zeros(B * N * N, device=DEV), z, one, z, one, h, w, KC, INV_T, transposed=transposed)
    assert int(idx.abs().max()) == 0
    assert bool((mx == 0).all())
    assert (lse.double() - math.log(N)).abs().max().item() <= TOL


@pytest.mark.parametrize("transposed", [False, True], ids=["rows", "transposed"])
def test_non_finite_t_keeps_the_index_in_range(transposed):
    from cocosnet_amd import ops
    h, w, B = 4, 64, 2
    N = h * w
    M = _randn(B, N, N, seed=11)
    M[0, 3, :] = float("nan")
    M[0, :, 5] = float("nan")
    M[1, 7, 9] = float("inf")
    M[1, 100, :] = float("-inf")
    M[1, :, 200] = float("inf")
    one, z = torch.full((B, N), 0.1, device=DEV), torch.zeros(B, N, device=DEV)
    idx, _, _ = ops.box3_match(_block(M), z, one, z, one, h, w, KC, INV_T, transposed=transposed)
    assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) < N
    idx, _, _ = ops.box3_match(torch.full((B * N * N,), float("nan"), device=DEV), z, one, z, one, h, w, KC, INV_T, transposed=transposed)
    assert int(idx.min()) >= 0 and int(idx.max()) < N


@pytest.mark.parametrize("h,w,B", GRIDS, ids=GRID_IDS)
def test_identical_sides_match_themselves_exactly(h, w, B):
    """phi = theta: cosine 1 on the diagonal — idx == arange(N) at EVERY position, border included, in both directions"""
    theta = _case(h, w, B)[0]
    opnd = _operands(theta, theta.clone())
    want = torch.arange(h * w, device=DEV, dtype=torch.int32).unsqueeze(0).expand(B, -1)
    for transposed in (False, True):
        idx, _, _ = _match(opnd, h, w, transposed)
        assert torch.equal(idx, want), (transposed, int((idx != want).sum()))


@pytest.mark.parametrize("h,w,r", [(8, 64, 3), (6, 128, 2)], ids=["8x64-roll3", "6x128-roll2"])
def test_rolled_exemplar_is_found_exactly(h, w, r):
    """phi = torch.roll(theta, r, dims=2): phi[y] = theta[y - r], so content position (y, x) has its twin at exemplar position (y + r, x).
    Asserted set, fixed by geometry: the 3x3 neighbourhood of (y, x) lies inside the grid (1 <= y <= h - 2, 1 <= x <= w - 2) and so does
    that of its image without straddling the wrap seam between exemplar rows r - 1 and r (y + r <= h - 2; y >= 1 keeps it above the seam):
    1 <= y <= h - 2 - r, 1 <= x <= w - 2.  There the two unfolded vectors are equal (cosine 1) and the index is the rolled position —
    rows: idx[y w + x] = (y + r) w + x; transposed: the exemplar position (y + r, x) finds (y, x)."""
    B = 2
    theta = _case(h, w, B)[0]
    opnd = _operands(theta, torch.roll(theta, r, dims=2).contiguous())
    ys, xs = torch.meshgrid(torch.arange(1, h - 1 - r, device=DEV), torch.arange(1, w - 1, device=DEV), indexing="ij")
    src, dst = (ys * w + xs).reshape(-1), ((ys + r) * w + xs).reshape(-1)
    assert src.numel() == (h - 2 - r) * (w - 2) > 0
    idx, _, _ = _match(opnd, h, w, False)
    assert torch.equal(idx[:, src].long(), dst.unsqueeze(0).expand(B, -1))
    idx, _, _ = _match(opnd, h, w, True)
    assert torch.equal(idx[:, dst].long(), src.unsqueeze(0).expand(B, -1))


def test_rejections(hip_lib):
    """a 16-wide grid, Nq != Nk, an unknown flag bit — with real buffers; nothing is launched and the outputs keep their fill"""
    N = 256
    f = ctypes.c_float
    t, s = torch.zeros(N * N, device=DEV), torch.ones(N, device=DEV)
    idx = torch.full((N,), -7, device=DEV, dtype=torch.int32)
    mx, lse = torch.full((N,), -7.0, device=DEV), torch.full((N,), -7.0, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    call = lambda Nq, Nk, h, w, flags: hip_lib.cocos_box3_match_f16x3(p(t), p(s), p(s), p(s), p(s), p(idx), p(mx), p(lse), 1, Nq, Nk, h, w,
                                                                     f(KC), f(INV_T), flags, None)
    assert call(256, 256, 16, 16, 0) == -2 and b"64- or 128-wide" in hip_lib.cocos_last_error_string()
    assert call(256, 128, 4, 64, 0) == -2
    assert call(256, 256, 4, 64, 2) == -1 and b"flags" in hip_lib.cocos_last_error_string()
    assert call(256, 256, 4, 64, 8) == -1
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((mx == -7.0).all()) and bool((lse == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------- the module
def _module(options, Be=2):
    from test_gpu_exemplar import _module_case
    return _module_case(options, 256, 2, Be, match_kernel=3)      # crop 256 at down 4: a 64 x 64 grid, B = 2


def _rep(t, n):
    return t if t.shape[0] == n else t.expand(n, -1, -1, -1).contiguous()


def _gather_reference(img, idx, h, w, down):
    """torch.gather construction: patches as columns [B, C*down*down, h*w], gathered along the positions, folded back"""
    Bq = idx.shape[0]
    cols = F.unfold(img, down, stride=down)
    if cols.shape[0] != Bq:
        cols = cols.expand(Bq, -1, -1)
    got = cols.gather(2, idx.reshape(Bq, 1, h * w).long().expand(-1, cols.shape[1], -1))
    return F.fold(got, (h * down, w * down), down, stride=down)


def _check_against_corr(tag, out, corr):
    """the bounds of tests/test_gpu_match.py's _check_against_corr with this file's TOL and exact=False: every position, corr[b, i,
    match_index] against the row maximum of the matrix forward(return_corr=True) returned; prob; xy"""
    idx = out["match_index"].reshape(corr.shape[0], -1)
    picked = corr.gather(2, idx.unsqueeze(2)).squeeze(2)
    gap = (corr.max(dim=2).values - picked).max().item()
    want_p = torch.softmax(corr.double(), dim=2).max(dim=2).values
    got_p = out["match_prob"].reshape(corr.shape[0], -1).double()
    e_p = ((got_p - want_p).abs() / want_p).max().item()
    e_lse = (out["match_lse"].reshape(corr.shape[0], -1).double() - torch.logsumexp(corr.double(), dim=2)).abs().max().item()
    print(f"[match-box3] {tag}: max corr - corr[idx] = {gap:.3e}  rel |prob - softmax max| = {e_p:.3e}  |lse - logsumexp corr| = {e_lse:.3e}")
    assert gap <= TOL, (tag, gap)
    assert e_p <= math.expm1(2 * TOL) + 4 * FP32_EPS * (1 + corr.abs().max().item()), (tag, e_p)
    xy = out["match_xy"]
    gw = out["match_index"].shape[2]
    assert torch.equal(xy[:, 1] * gw + xy[:, 0], out["match_index"])


def _compare_readouts(tag, got, plain, c, corr_absmax):
    """two readouts of the same matrix c: the picked entries, prob and lse within the bounds of _check_against_corr"""
    pick = lambda o: c.gather(2, o["match_index"].reshape(c.shape[0], -1).unsqueeze(2)).squeeze(2)
    d_idx = (pick(plain) - pick(got)).max().item()
    same = (got["match_index"] == plain["match_index"]).float().mean().item()
    rel = ((got["match_prob"].double() - plain["match_prob"].double()).abs() / plain["match_prob"].double()).max().item()
    d_lse = (got["match_lse"].double() - plain["match_lse"].double()).abs().max().item()
    print(f"[match-box3] {tag}: corr[idx_other] - corr[idx] = {d_idx:.3e} (equal indices: {same:.4f})  rel |prob| = {rel:.3e}  |lse| = {d_lse:.3e}")
    assert d_idx <= TOL, (tag, d_idx)
    assert rel <= math.expm1(2 * TOL) + 4 * FP32_EPS * (1 + corr_absmax), (tag, rel)
    assert d_lse <= TOL, (tag, d_lse)


class _Spy:
    """the entry points that went through _lib.call"""

    def __init__(self, monkeypatch):
        from cocosnet_amd import _lib
        self.names, real = [], _lib.call
        monkeypatch.setattr(_lib, "call", lambda name, *args: (self.names.append(name), real(name, *args))[1])

    def take(self):
        got, self.names[:] = set(self.names), []
        return got


@pytest.mark.parametrize("options", ["ade20k_options", "celebahq_edge_options"])
def test_module_match_on_the_new_route(options, monkeypatch):
    from cocosnet_amd import ops
    net, ref_img, real, seg, ref_seg = _module(options)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        before = net(ref_img, real, seg, ref_seg)
        corr = net(ref_img, real, seg, ref_seg, return_corr=True)
        spy.take()
        rows = net.match(ref_img, seg, ref_seg, hard_warp=True)
        cols = net.match(ref_img, seg, ref_seg, direction="cols")
        new = spy.take()
        monkeypatch.setattr(ops, "MATCH_FUSED", False)
        rows0 = net.match(ref_img, seg, ref_seg, hard_warp=True)
        cols0 = net.match(ref_img, seg, ref_seg, direction="cols")
        old = spy.take()
        monkeypatch.setattr(ops, "MATCH_FUSED", True)
        after = net(ref_img, real, seg, ref_seg)
    assert rows["match_index"].shape == (2, 64, 64)
    assert "cocos_box3_match_f16x3" in new and "cocos_box3_corr_xbox_f16x3" in new and "cocos_row_argmax_lse" not in new, sorted(new)
    assert "cocos_row_argmax_lse" in old and "cocos_box3_match_f16x3" not in old, sorted(old)
    amax = corr.abs().max().item()
    _check_against_corr(f"{options} rows", rows, corr)
    _check_against_corr(f"{options} cols", cols, corr.transpose(1, 2))
    _compare_readouts(f"{options} rows against MATCH_FUSED off", rows, rows0, corr, amax)
    _compare_readouts(f"{options} cols against MATCH_FUSED off", cols, cols0, corr.transpose(1, 2), amax)
    for o in (rows, rows0):
        assert torch.equal(o["warp_hard"], _gather_reference(ref_img, o["match_index"].reshape(2, -1), 64, 64, net.opt.down))
    assert not any(v.requires_grad for v in rows.values())
    assert sorted(before) == sorted(after)
    for k in before:      # nothing is cached across calls
        assert torch.equal(before[k], after[k]), k


@pytest.mark.parametrize("Be", [1, 2])
def test_module_match_with_a_prepared_exemplar(Be, monkeypatch):
    """match() with a record on the new route (the record's key planes and statistics: the key side is not recomputed) against
    forward(return_corr=True)'s matrix AND against the ordinary match(), both directions"""
    from cocosnet_amd import inference
    net, ref_img, real, seg, ref_seg = _module("ade20k_options", Be=Be)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        corr = net(_rep(ref_img, 2), real, seg, _rep(ref_seg, 2), return_corr=True)
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
        for direction in ("rows", "cols"):
            c = corr if direction == "rows" else corr.transpose(1, 2)
            plain = net.match(_rep(ref_img, 2), seg, _rep(ref_seg, 2), direction=direction)
            spy.take()
            got = net.match(None, seg, None, exemplar=rec, direction=direction, hard_warp=direction == "rows")
            assert "cocos_box3_match_f16x3" in spy.take()
            _check_against_corr(f"record Be={Be} {direction}", got, c)
            _compare_readouts(f"record Be={Be} {direction} against the ordinary match()", got, plain, c, corr.abs().max().item())
            if direction == "rows":
                assert torch.equal(got["warp_hard"], _gather_reference(ref_img, got["match_index"].reshape(2, -1), 64, 64, net.opt.down))


def test_new_route_allocates_one_hw_by_hw_tensor(monkeypatch):
    """B = 1, 64 x 64 grid, N = 4096: the peak above the live memory stays below 1.5 matrices on the new route (one T, the operand
    planes and the statistics); with MATCH_FUSED off c_raw and the logits are live together: at least two"""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match
    N = 64 * 64
    theta, phi = _randn(1, 256, 64, 64, seed=21), _randn(1, 256, 64, 64, seed=22)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    deltas = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "MATCH_FUSED", fused)
        for direction in ("rows", "cols"):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            m = correspondence_match(theta, phi, cfg, direction=direction)
            torch.cuda.synchronize()
            deltas[(fused, direction)] = torch.cuda.max_memory_allocated() - base
            assert m.index.shape == (1, 64, 64)
            del m
    print("[match-box3] peak memory above live: " + ", ".join(f"{'new' if f else 'materialised'} {d} {v / 2**20:.1f} MiB" for (f, d), v in deltas.items()))
    for direction in ("rows", "cols"):
        assert deltas[(True, direction)] < 1.5 * N * N * 4
        assert deltas[(False, direction)] >= 2 * N * N * 4


def test_other_match_kernel3_shapes_keep_the_materialised_chain(monkeypatch):
    """a 16-wide grid, COCOS_PRECISION=fp32 and MATCH_FUSED = False stay on K3 -> K6 -> K36b"""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    spy = _Spy(monkeypatch)
    small = (_randn(1, 256, 16, 16, seed=31), _randn(1, 256, 16, 16, seed=32))
    wide = (_randn(1, 256, 4, 64, seed=33), _randn(1, 256, 4, 64, seed=34))
    correspondence_match(*small, cfg)
    assert "cocos_row_argmax_lse" in spy.take()
    correspondence_match(*wide, cfg)
    assert "cocos_box3_match_f16x3" in spy.take()
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    correspondence_match(*wide, cfg)
    assert "cocos_box3_match_f16x3" not in spy.take()
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    monkeypatch.setattr(ops, "MATCH_FUSED", False)
    correspondence_match(*wide, cfg)
    assert "cocos_box3_match_f16x3" not in spy.take()
    monkeypatch.setattr(ops, "MATCH_FUSED", True)
    correspondence_match(*wide, HotPathConfig(match_kernel=3, PONO_C=False, down=4))
    assert "cocos_box3_match_f16x3" not in spy.take()


# ---------------------------------------------------------------------------------------------------------------- guards
def test_match_inside_red_zones_reaches_the_entry_point():
    net, ref_img, real, seg, ref_seg = _module("ade20k_options")
    entries = set()
    for direction in ("rows", "cols"):
        with guarded() as g:
            out = net.match(g.place(ref_img), g.place(seg), g.place(ref_seg), direction=direction, hard_warp=direction == "rows")
            bad = g.check()
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(v).all()) for v in out.values() if v.is_floating_point())
        assert bad == [] and g.violations == [], g.report()
        assert "cocos_box3_match_f16x3" in g.entries
        entries |= g.entries
    assert {"cocos_box3_match_f16x3", "cocos_box3_corr_xbox_f16x3", "cocos_gather_patches"} <= entries


def test_match_hands_over_live_buffers_only(monkeypatch):
    import test_gpu_live_buffers as lb
    net, ref_img, real, seg, ref_seg = _module("ade20k_options")
    guard = lb._Guard(monkeypatch)
    net.match(ref_img, seg, ref_seg, hard_warp=True)
    net.match(ref_img, seg, ref_seg, direction="cols")
    guard.check(20, 75)


# ---- red zones: the case joins tests/test_gpu_red_zones.py's table through its own helper, so its coverage report and its "every entry
# ---- point was reached" audit count the K37 entry point too (as tests/test_gpu_match.py does for K36)
import test_gpu_red_zones as rz  # noqa: E402


def _rz_box3_match(c):
    from cocosnet_amd import ops
    B, h, w = 2, 4, 64
    th = c.data(rz.rnd(B, 256, h, w, seed=71) + 0.15)
    ph = c.data(0.05 * rz.rnd(B, 256, h, w, seed=71).roll((1, 5), (2, 3)) + rz.rnd(B, 256, h, w, seed=72) - 0.1)
    with torch.no_grad():
        (mu, a), (nu, b) = ops.unfold3_stats(th, KC), ops.unfold3_stats(ph, KC)
        t = ops.box3_corr_xbox(th, ph)
    return list(ops.box3_match(t, mu, a, nu, b, h, w, KC, 100.0)) + list(ops.box3_match(t, nu, b, mu, a, h, w, KC, 100.0, transposed=True))


RZ_CASES = {"box3_match-2x4x64+transposed": _rz_box3_match}
for _name, _body in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_the_new_op_inside_red_zones(name, monkeypatch):
    rz.test_red_zones(name, monkeypatch)
    assert "cocos_box3_match_f16x3" in set(rz.COVERAGE[name][0])
