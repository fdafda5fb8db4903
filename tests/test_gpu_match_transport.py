"""K50 on the GPU: the BIAS instantiations of the fused scan (cocos_corr_topk_bias_f16x3), the biased forward of the k-sparse warp
(cocos_sparse_softmax_warp_bias_fwd_f16x3), ops.corr_sinkhorn, hot_path.correspondence_transport / correspondence_sparse(transport=...)
and NoVGGCorrespondence.transport_match / sparse_warp(transport=...).

Arbiter: tests/transport_case.py (torch fp64).  Bounds.  An element z = s + bias of the kernel is the raw accumulator plus the bias in
raw units, one fma, times the natural-unit scale: its error is the unbiased readout's element error (TOL of tests/test_gpu_match.py at
|s| <= INV_T) grown with the magnitude of the number it now holds, so
    lse_bound(bias) = TOL * (INV_T + max |finite bias|) / INV_T
bounds val and lse of one launch, unless the launch is already within 4 x the error of torch's own fp32 on the same inputs (the
accuracy-class rule, tests/accuracy_case.bound).  A potential after h half-steps has gone through h such launches, each feeding the next
through an affine map of slope tau <= 1: h * lse_bound.  An index is held to the arbiter's wherever the arbiter's value at that rank is
more than 2 * lse_bound away from both sorted neighbours (two values each off by at most the bound cannot trade places across that);
at most 1 % of the positions may be excused this way (tests/test_match_transport_cpu.py checks that the seeds used here excuse fewer).
The file name sorts before test_gpu_red_zones.py: its red-zone cases have run when that file's audit is collected."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy_case as ac  # noqa: E402
import test_gpu_match_topk as tt  # noqa: E402
import test_gpu_red_zones as rz  # noqa: E402
import transport_case as tc  # noqa: E402
from test_gpu_match import DEV, FP32_EPS, INV_T, SHAPES, TOL, _gather_reference, _module, _planes  # noqa: E402
from test_gpu_match_topk import TIE_PAIRS  # noqa: E402
from test_gpu_parity import GRAD_TOL, rel  # noqa: E402

pytestmark = pytest.mark.gpu
ENTRY = "cocos_corr_topk_bias_f16x3"
WARP_ENTRY = "cocos_sparse_softmax_warp_bias_fwd_f16x3"
B = 3
NEG_INF = float("-inf")
EXCUSED_MAX = 0.01


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def lse_bound(bias):
    fin = bias[torch.isfinite(bias)]
    return TOL * (INV_T + (float(fin.abs().max()) if fin.numel() else 0.0)) / INV_T


_CASES = {}


def _case(Nq, Nk):
    """(q [B,256,Nq], k [B,256,Nk]) unit-norm columns on the device: made once per shape, shared, never written"""
    if (Nq, Nk) not in _CASES:
        _CASES[(Nq, Nk)] = tuple(t.to(DEV) for t in tc.readout_case(B, Nq, Nk))
    return _CASES[(Nq, Nk)]


def _biased(q, k, bias, shared, kk):
    """the entry point on operand planes; `shared`: one key set and one bias row (batch stride 0)"""
    from cocosnet_amd import ops
    kk_, bb = (k[:1].contiguous(), bias[:1].contiguous()) if shared else (k, bias)
    return ops._corr_topk_bias_planes(*_planes(q), *_planes(kk_), bb.to(DEV).contiguous(), INV_T, kk)


def _fp32_arm(q, k, bias):
    with ac.plain_fp32():
        return torch.matmul(q.transpose(1, 2), k) * INV_T + bias.unsqueeze(1)


def _judge(tag, idx, val, lse, q, k, bias, check_idx=True):
    """idx against the arbiter where the arbiter decides, val / lse under the accuracy-class rule or lse_bound -> the figures"""
    kk = idx.shape[-1]
    bias = bias.to(DEV)
    a_idx, a_val, a_lse, z = tc.biased_topk(tc.logits(q, k, INV_T), bias, kk)
    bound = lse_bound(bias)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and tuple(idx.shape) == tuple(a_idx.shape), tag
    assert not bool(torch.isnan(val).any()) and not bool(torch.isnan(lse).any()), f"{tag}: NaN"
    assert int(idx.min()) >= 0 and int(idx.max()) < z.shape[-1], tag
    dec = tc.decided(z, kk, bound)
    excused = 1.0 - dec.double().mean().item()
    if check_idx:
        assert excused <= EXCUSED_MAX, (tag, excused)
        assert torch.equal(idx.long()[dec], a_idx[dec]), f"{tag}: idx differs from the arbiter at {int((idx.long() != a_idx)[dec].sum())} decided positions"
    picked = z.gather(-1, idx.long())
    fin = torch.isfinite(picked)
    assert torch.equal(torch.isfinite(val), fin), f"{tag}: val is not finite exactly where the picked element is"
    e_val = (val.double() - picked)[fin].abs().max().item()
    rows = torch.isfinite(a_lse)
    assert torch.equal(torch.isfinite(lse), rows), f"{tag}: lse is not finite exactly on the rows with a key"
    e_lse = (lse.double() - a_lse)[rows].abs().max().item()
    z32 = _fp32_arm(q, k.expand(q.shape[0], -1, -1), bias.expand(q.shape[0], -1))
    e_val32 = (z32.gather(-1, a_idx).double() - a_val)[torch.isfinite(a_val)].abs().max().item()
    e_lse32 = (torch.logsumexp(z32, -1).double() - a_lse)[rows].abs().max().item()
    print(f"[transport] {tag}: |val - z[idx]| = {e_val:.3e} (fp32 arm {e_val32:.3e})  |lse - logsumexp z| = {e_lse:.3e} (fp32 arm {e_lse32:.3e})  "
          f"bound {bound:.3e}  excused {excused:.4f}")
    assert e_val <= ac.bound(e_val32) or e_val <= bound, (tag, e_val, e_val32, bound)
    assert e_lse <= ac.bound(e_lse32) or e_lse <= bound, (tag, e_lse, e_lse32, bound)
    return e_val, e_lse


GRID = dict(argnames="Nq,Nk,k,shared", argvalues=[(Nq, Nk, k, s) for Nq, Nk in SHAPES for k in (1, 4) for s in (False, True)],
            ids=[f"{Nq}x{Nk}-k{k}-{'shared' if s else 'dense'}" for Nq, Nk in SHAPES for k in (1, 4) for s in (False, True)])


# ---------------------------------------------------------------------------------------------------------------- biased readout
@pytest.mark.parametrize(**GRID)
def test_biased_readout_against_the_arbiter(Nq, Nk, k, shared):
    q, kn = _case(Nq, Nk)
    bias = tc.make_bias(B, Nk, tc.bias_seed(Nq, Nk, shared))
    got = _biased(q, kn, bias, shared, k)
    kn_, bias_ = (kn[:1], bias[:1]) if shared else (kn, bias)
    _judge(f"random bias ({Nq},{Nk}) k={k} {'shared' if shared else 'dense'}", *got, q, kn_, bias_)
    again = _biased(q, kn, bias, shared, k)
    assert all(torch.equal(a, b_) for a, b_ in zip(got, again)), "two calls on the same inputs differ"


@pytest.mark.parametrize(**GRID)
def test_zero_bias_is_the_unbiased_entry_bitwise(Nq, Nk, k, shared):
    """raw += 0 * c is the identity on every accumulator register, so all three outputs are cocos_corr_topk_f16x3's bits"""
    from cocosnet_amd import ops
    q, kn = _case(Nq, Nk)
    want = ops._corr_topk_planes(*_planes(q), *_planes(kn[:1].contiguous() if shared else kn), INV_T, k)
    got = _biased(q, kn, torch.zeros(B, Nk), shared, k)
    for a, b_, what in zip(got, want, ("idx", "val", "lse")):
        assert torch.equal(a, b_), f"{what} differs from cocos_corr_topk_f16x3"


@pytest.mark.parametrize(**GRID)
def test_zero_or_minus_inf_bias_is_the_label_mask(Nq, Nk, k, shared):
    """K47 with one query label: the keys of that label carry bias 0, the others -inf — the labelled entry's indices"""
    from cocosnet_amd import ops
    q, kn = _case(Nq, Nk)
    kl = torch.randint(1, 3, (B, Nk), generator=torch.Generator().manual_seed(Nq + Nk))
    kl[:, :8] = 1
    ql = torch.ones(B, Nq, dtype=torch.int64)
    bias = torch.where(kl == 1, 0.0, NEG_INF)
    i32 = lambda t: t.to(device=DEV, dtype=torch.int32).contiguous()
    want = ops._corr_topk_labels_planes(*_planes(q), *_planes(kn[:1].contiguous() if shared else kn), i32(ql), i32(kl[:1] if shared else kl), INV_T, k)
    got = _biased(q, kn, bias, shared, k)
    assert torch.equal(got[0], want[0]), "idx differs from cocos_corr_topk_labels_f16x3"
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


def test_a_low_logit_with_a_high_bias_wins():
    Nq, Nk = 132, 68
    q, kn = _case(Nq, Nk)
    L = tc.logits(q, kn, INV_T)
    j = L.sum(1).argmin(-1)                                  # per sample the key the queries like least
    bias = torch.zeros(B, Nk)
    bias[torch.arange(B), j.cpu()] = 2.5 * INV_T             # more than the logits' whole range
    idx, val, lse = _biased(q, kn, bias, False, 4)
    _judge("high bias", idx, val, lse, q, kn, bias)
    assert torch.equal(idx[..., 0].long(), j.view(B, 1).expand(-1, Nq))
    assert bool((idx[..., 1:].long() != j.view(B, 1, 1)).all())


@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("shared", [False, True], ids=["dense", "shared"])
def test_duplicated_keys_with_equal_bias_resolve_to_the_lower_index(shared, k):
    """tests/test_gpu_match_topk.py's TIE_PAIRS (one per merge level): keys a < b are both copies of query i and carry the same bias"""
    Nq, Nk = 36, 260
    q, kn = _case(Nq, Nk)
    kn = (kn[:1].expand(B, -1, -1) if shared else kn).clone()
    src = q[:1].expand(B, -1, -1) if shared else q
    bias = tc.make_bias(B, Nk, 77)
    bias[~torch.isfinite(bias)] = -3.0
    for i, (a, b_) in enumerate(TIE_PAIRS):
        kn[:, :, a] = src[:, :, i]
        kn[:, :, b_] = src[:, :, i]
        bias[:, a] = bias[:, b_] = 3.0 + i
    kn = kn.contiguous()
    idx, val, lse = _biased(q, kn, bias, shared, k)
    _judge(f"ties k={k}", idx, val, lse, q, kn[:1] if shared else kn, bias[:1] if shared else bias, check_idx=False)
    for s_ in ([0] if shared else range(B)):
        for i, (a, b_) in enumerate(TIE_PAIRS):
            assert idx[s_, i, :2].tolist() == [a, b_][:k], (s_, i, idx[s_, i].tolist())
            if k > 1:
                assert val[s_, i, 0] == val[s_, i, 1]


@pytest.mark.parametrize("Nq,Nk", [(36, 260), (132, 68)])
@pytest.mark.parametrize("shared", [False, True], ids=["dense", "shared"])
def test_a_bias_run_that_straddles_the_last_tile_of_four_keys(Nq, Nk, shared):
    """everything excluded but the last six keys: two in the run before the 4-key tail, four in the tail (whose bias is the last 16
    bytes of the row — the run after it lies past the descriptor and must read as 'masked already', not as a bias)"""
    q, kn = _case(Nq, Nk)
    bias = torch.full((B, Nk), NEG_INF)
    bias[:, Nk - 6:] = torch.tensor([1.0, -2.0, 4.0, 0.5, -7.0, 3.0])
    for k in (1, 4, 8):
        idx, val, lse = _biased(q, kn, bias, shared, k)
        _judge(f"tail run ({Nq},{Nk}) k={k}", idx, val, lse, q, kn[:1] if shared else kn, bias[:1] if shared else bias, check_idx=k <= 6)
        assert int(idx[..., :min(k, 6)].min()) >= Nk - 6 and bool(torch.isfinite(lse).all())
        if k == 8:
            assert bool((val[..., 6:] == NEG_INF).all()) and bool(torch.isfinite(val[..., :6]).all())


def test_a_row_with_every_key_excluded():
    Nq, Nk = 132, 68
    q, kn = _case(Nq, Nk)
    bias = tc.make_bias(B, Nk, 5)
    bias[1] = NEG_INF
    for k in (1, 4):
        idx, val, lse = _biased(q, kn, bias, False, k)
        assert not bool(torch.isnan(val).any()) and not bool(torch.isnan(lse).any())
        assert int(idx.min()) >= 0 and int(idx.max()) < Nk
        assert bool((lse[1] == NEG_INF).all()) and bool((val[1] == NEG_INF).all())
        assert bool(torch.isfinite(lse[[0, 2]]).all()) and bool(torch.isfinite(val[[0, 2]]).all())


def test_public_op_refuses_and_detaches():
    from cocosnet_amd import ops
    q, kn = _case(132, 68)
    bias = tc.make_bias(B, 68, 9).to(DEV)
    got = ops.corr_topk_biased(q.clone().requires_grad_(True), kn, bias, INV_T, 3)
    want = _biased(q, kn, bias, False, 3)
    assert all(torch.equal(a, b_) for a, b_ in zip(got, want)) and not any(t.requires_grad for t in got)
    with pytest.raises(ops._lib.CocosHipError, match="no CPU fallback"):
        ops.corr_topk_biased(q, kn, bias.cpu(), INV_T, 3)
    with pytest.raises(ValueError, match="not differentiable"):
        ops.corr_topk_biased(q, kn, bias.clone().requires_grad_(True), INV_T, 3)


# ---------------------------------------------------------------------------------------------------------------- Sinkhorn
SINK_SHAPES = [(64, 64), (132, 68), (36, 260)]
_SINK = {}


def _sink_ref(Nq, Nk, iters, tau):
    key = (Nq, Nk, iters, tau)
    if key not in _SINK:
        q, kn = _case(Nq, Nk)
        _SINK[key] = tc.sinkhorn(tc.logits(q, kn, INV_T), iters, tau)
    return _SINK[key]


@pytest.mark.parametrize("tau", [1.0, 0.7])
@pytest.mark.parametrize("iters", [1, 3, 8])
@pytest.mark.parametrize("Nq,Nk", SINK_SHAPES)
def test_sinkhorn_potentials_against_the_restatement(Nq, Nk, iters, tau):
    from cocosnet_amd import ops
    q, kn = _case(Nq, Nk)
    f, g, row_lse = ops.corr_sinkhorn(q, kn, INV_T, iters, tau)
    rf, rg, rl = _sink_ref(Nq, Nk, iters, tau)
    per = lse_bound(torch.cat((rf.reshape(-1), rg.reshape(-1))))
    bound = 2 * iters * per
    e_f, e_g, e_l = ((a.double() - b_).abs().max().item() for a, b_ in ((f, rf), (g, rg), (row_lse, rl)))
    print(f"[transport] sinkhorn ({Nq},{Nk}) iters={iters} tau={tau}: |f - ref| = {e_f:.3e}  |g - ref| = {e_g:.3e}  |row_lse - ref| = {e_l:.3e}  "
          f"per-lse bound {per:.3e} x {2 * iters} half-steps = {bound:.3e}")
    assert f.shape == (B, Nq) and g.shape == (B, Nk) and row_lse.shape == (B, Nq) and not any(t.requires_grad for t in (f, g, row_lse))
    assert e_f <= bound and e_g <= bound and e_l <= bound + per, (e_f, e_g, e_l, bound)
    if tau == 1.0:      # balanced: the column marginals are exact after every full iteration
        col_lse = ops.corr_topk_biased(kn, q, f, INV_T, 1)[2]
        key_mass = torch.exp(g + col_lse + math.log(Nk))
        e_m = (key_mass.double() - 1).abs().max().item()
        print(f"[transport] sinkhorn ({Nq},{Nk}) iters={iters}: |key_mass - 1| = {e_m:.3e}")
        assert e_m <= bound, (e_m, bound)
    again = ops.corr_sinkhorn(q, kn, INV_T, iters, tau)
    assert all(torch.equal(a, b_) for a, b_ in zip((f, g, row_lse), again))


def test_planted_collapse_is_undone_by_five_balanced_iterations():
    """every row's plain argmax is the hub (key 0); the balanced plan's rows point at the planted permutation — both facts hold on the
    fp64 restatement (asserted here and in tests/test_match_transport_cpu.py) and the kernels must reproduce them"""
    from cocosnet_amd import ops
    q, kn, pi = (t.to(DEV) for t in tc.planted())
    L = tc.logits(q, kn, INV_T)
    assert bool((L.argmax(-1) == 0).all())
    rf, rg, _ = tc.sinkhorn(L, 5, 1.0)
    assert torch.equal(tc.biased_topk(L, rg, 1)[0][..., 0], pi)
    plain = ops.corr_topk(q, kn, INV_T, 1)[0][..., 0]
    assert bool((plain == 0).all()), "the unbiased readout does not collapse onto the hub"
    f, g, row_lse = ops.corr_sinkhorn(q, kn, INV_T, 5, 1.0)
    idx, z, lse = ops.corr_topk_biased(q, kn, g, INV_T, 1)
    assert torch.equal(idx[..., 0].long(), pi), f"{int((idx[..., 0].long() != pi).sum())} rows miss the planted permutation"
    assert torch.equal(lse, row_lse)
    mass = torch.exp(f + row_lse + math.log(q.shape[2]))
    print(f"[transport] planted: max |g - ref| = {(g.double() - rg).abs().max().item():.3e}  match_mass in [{mass.min().item():.4f}, {mass.max().item():.4f}]")


# ---------------------------------------------------------------------------------------------------------------- warp
def test_biased_warp_weights_are_the_softmax_of_pair_logit_plus_bias():
    from cocosnet_amd import ops
    Nq, Nk, Cv, k = 132, 68, 5, 4
    q, kn = _case(Nq, Nk)
    gen = torch.Generator().manual_seed(3)
    v = torch.randn(B, Cv, Nk, generator=gen).to(DEV)
    g = tc.make_bias(B, Nk, 11).to(DEV)
    idx = torch.randint(0, Nk, (B, Nq, k), generator=gen).to(DEV)
    g[0, idx[0, 0]] = NEG_INF                                  # query 0 of sample 0: every candidate excluded -> uniform weights
    out, w = ops.sparse_softmax_warp(q, kn, v, idx, INV_T, return_weights=True, k_bias=g)
    # the arbiter's rows, the all-excluded row aside (its softmax is 0 / 0 by definition; the kernel's answer is the documented 1 / k)
    g_ref = g.clone()
    s_pair = tc.logits(q, kn, INV_T).gather(2, idx) + g_ref.double().unsqueeze(1).expand(-1, Nq, -1).gather(2, idx)
    dead = ~torch.isfinite(s_pair).any(-1)
    assert bool(dead[0, 0]) and int(dead.sum()) >= 1
    s_pair[dead] = 0.0
    w_ref = torch.softmax(s_pair, -1)
    out_ref = torch.einsum("bir,bcir->bci", w_ref, v.double().gather(2, idx.reshape(B, 1, -1).expand(-1, Cv, -1)).reshape(B, Cv, Nq, k))
    bound = math.expm1(2 * lse_bound(g)) + 4 * FP32_EPS
    e_w, e_o = (w.double() - w_ref).abs().max().item(), (out.double() - out_ref).abs().max().item() / out_ref.abs().max().item()
    print(f"[transport] biased warp: |w - softmax| = {e_w:.3e}  rel |out - ref| = {e_o:.3e}  (bound {bound:.3e})")
    assert not bool(torch.isnan(w).any()) and not bool(torch.isnan(out).any())
    assert bool((w[0, 0] == 1.0 / k).all())
    assert e_w <= bound and e_o <= bound
    plain = ops.sparse_softmax_warp(q, kn, v, idx, INV_T, return_weights=True)
    zero = ops.sparse_softmax_warp(q, kn, v, idx, INV_T, return_weights=True, k_bias=torch.zeros(B, Nk, device=DEV))
    assert torch.equal(plain[0], zero[0]) and torch.equal(plain[1], zero[1])
    with pytest.raises(ValueError, match="not differentiable"):
        ops.sparse_softmax_warp(q, kn, v, idx, INV_T, k_bias=g.clone().requires_grad_(True))


def _hot_case(fh, fw, seed):
    gen = torch.Generator().manual_seed(seed)
    theta, phi = torch.randn(2, 256, fh, fw, generator=gen).to(DEV), torch.randn(2, 256, fh, fw, generator=gen).to(DEV)
    ref_img = (torch.rand(2, 3, 4 * fh, 4 * fw, generator=gen) * 2 - 1).to(DEV)
    onehot = lambda: torch.zeros(2, 5, 4 * fh, 4 * fw).scatter_(1, torch.randint(0, 5, (2, 1, 4 * fh, 4 * fw), generator=gen), 1.0).to(DEV)
    return theta, phi, ref_img, onehot(), onehot()


TRANSPORT = dict(iters=3, tau=1.0)


@pytest.mark.parametrize("fh,fw", [(16, 16), (12, 20)])
def test_correspondence_sparse_transport_gradients_against_fp64(fh, fw):
    """theta, phi and the values get the gradients of the blend with the potentials held constant: fp64 autograd of the restatement,
    on the candidates the kernel selected (asserted to be the restatement's wherever it decides).  The pooled exemplar is the value
    leaf of the op-level chain, which is bitwise the route's warp."""
    import torch.nn.functional as F
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, _flat, correspondence_sparse
    from oracle.torch_ref import _unit_columns
    k, N = 4, fh * fw
    theta0, phi0, ref_img, seg, ref_seg = _hot_case(fh, fw, 60 + fh)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    theta, phi = theta0.clone().requires_grad_(True), phi0.clone().requires_grad_(True)
    out = correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, 0.01, k, transport=TRANSPORT)
    assert set(out) == {"warp_out", "match_index", "match_weight", "potential_k", "match_mass"}
    assert not out["potential_k"].requires_grad and not out["match_mass"].requires_grad
    idx = out["match_index"].permute(0, 2, 3, 1).reshape(2, N, k)
    g_out = torch.randn(2, 3, 4 * fh, 4 * fw, generator=torch.Generator().manual_seed(9)).to(DEV)
    (out["warp_out"] * g_out).sum().backward()
    # fp64: the restatement's own potentials (detached), the kernel's candidates
    th64, ph64 = theta0.double().requires_grad_(True), phi0.double().requires_grad_(True)
    qn, kn = _unit_columns(th64.reshape(2, 256, -1), True), _unit_columns(ph64.reshape(2, 256, -1), True)
    L = tc.logits(qn.detach(), kn.detach(), 100.0)
    _, g_ref, _ = tc.sinkhorn(L, TRANSPORT["iters"], TRANSPORT["tau"])
    per = lse_bound(g_ref)
    dec = tc.decided(L + g_ref.unsqueeze(1), k, 2 * TRANSPORT["iters"] * per)
    a_idx = tc.biased_topk(L, g_ref, k)[0]
    assert dec.double().mean().item() >= 1 - EXCUSED_MAX and torch.equal(idx[dec], a_idx[dec])
    e_g = (out["potential_k"].reshape(2, N).double() - g_ref).abs().max().item()
    assert e_g <= 2 * TRANSPORT["iters"] * per, (e_g, per)
    v64 = F.avg_pool2d(ref_img.double(), 4).reshape(2, 3, -1).requires_grad_(True)
    o64, w64, _ = tc.sparse_warp(qn, kn, v64, g_ref, 100.0, k, idx=idx)
    (F.interpolate(o64.reshape(2, 3, fh, fw), scale_factor=4, mode="nearest") * g_out.double()).sum().backward()
    errs = {"warp": rel(out["warp_out"], F.interpolate(o64.reshape(2, 3, fh, fw), scale_factor=4, mode="nearest").detach().cpu().numpy()),
            "d theta": rel(theta.grad, th64.grad.cpu().numpy()), "d phi": rel(phi.grad, ph64.grad.cpu().numpy())}
    # the value gradient: the same blend from the ops with the pooled exemplar as a leaf
    planes = ops.OperandPlanes()
    th2, ph2 = theta0.clone().requires_grad_(True), phi0.clone().requires_grad_(True)
    q2, k2 = ops.center_l2norm_planes(_flat(th2), 1, planes), ops.center_l2norm_planes(_flat(ph2), 1, planes)
    with torch.no_grad():
        vq = _flat(ops.warp_values(ref_img, None, 4)).clone()
    vq.requires_grad_(True)
    o2 = ops.sparse_softmax_warp(q2, k2, vq, idx, 100.0, planes, k_bias=out["potential_k"].reshape(2, N))
    warp2 = ops.upsample_nearest(o2.reshape(2, 3, fh, fw), 4)
    assert torch.equal(warp2, out["warp_out"]), "warp_out is not ops.sparse_softmax_warp(k_bias=g) on the selected candidates"
    (warp2 * g_out).sum().backward()
    assert torch.equal(th2.grad, theta.grad) and torch.equal(ph2.grad, phi.grad)
    errs["d v"] = rel(vq.grad, v64.grad.cpu().numpy())
    print(f"[transport] correspondence_sparse transport {fh}x{fw}: " + "  ".join(f"{n} {e:.3e}" for n, e in errs.items()) + f"  (GRAD_TOL {GRAD_TOL:.1e})")
    assert all(e < GRAD_TOL for e in errs.values()), errs
    assert float(theta.grad.abs().max()) > 0 and float(phi.grad.abs().max()) > 0


def test_transport_none_is_todays_route_bitwise(monkeypatch):
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse
    theta, phi, ref_img, seg, ref_seg = _hot_case(8, 8, 77)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    spy = tt._Spy(monkeypatch)
    a = correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, 0.01, 4)
    names_a = list(spy.names)
    spy.take()
    b_ = correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, 0.01, 4, transport=None)
    assert names_a == list(spy.names), "transport=None changes the launch sequence"
    assert sorted(a) == sorted(b_) and all(torch.equal(a[n], b_[n]) for n in a)
    assert not {ENTRY, WARP_ENTRY} & spy.take()
    correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, 0.01, 4, transport=TRANSPORT)
    assert {ENTRY, WARP_ENTRY} <= spy.take()


# ---------------------------------------------------------------------------------------------------------------- module
_MOD = {}
ITERS_MOD = 5


def _mod():
    """(net, ref_img, real, seg, ref_seg, corr): the module tests' smallest case (crop 64, 7 classes, a 16 x 16 grid) and the matrix
    forward(return_corr=True) returns for it — made once, never written"""
    if not _MOD:
        net, ref_img, real, seg, ref_seg = _module("ade20k_options", 1)
        with torch.no_grad():
            corr = net(ref_img, real, seg, ref_seg, return_corr=True)
        _MOD["case"] = (net, ref_img, real, seg, ref_seg, corr)
    return _MOD["case"]


@pytest.mark.parametrize("k", [1, 4])
def test_module_transport_match_against_return_corr(k, monkeypatch):
    net, ref_img, real, seg, ref_seg, corr = _mod()
    Bm, N, Nk = corr.shape
    spy = tt._Spy(monkeypatch)
    with torch.no_grad():
        out = net.transport_match(ref_img, seg, ref_seg, iters=ITERS_MOD, topk=k, hard_warp=True)
    took = spy.take()
    assert ENTRY in took and not took & {"cocos_corr_topk_f16x3", "cocos_corr_match_f16x3", "cocos_row_topk_lse", "cocos_row_argmax_lse"}, sorted(took)
    want_keys = {"match_index", "match_xy", "match_prob", "match_lse", "potential_q", "potential_k", "match_mass", "key_mass", "warp_hard"}
    assert set(out) == want_keys | ({"warp_topk"} if k > 1 else set())
    assert not any(v.requires_grad for v in out.values())
    L = corr.double()
    f, g, row_lse = tc.sinkhorn(L, ITERS_MOD, 1.0)
    per = lse_bound(torch.cat((f.reshape(-1), g.reshape(-1))))
    bound = (2 * ITERS_MOD + 2) * max(per, TOL)         # the half-steps, the readout on top, and the matrix' own element error
    a_idx, a_val, a_lse, z = tc.biased_topk(L, g, k)
    flat = (lambda t: t.reshape(Bm, k, -1).transpose(1, 2)) if k > 1 else (lambda t: t.reshape(Bm, -1, 1))
    idx, prob = flat(out["match_index"]), flat(out["match_prob"]).double()
    dec = tc.decided(z, k, bound)
    assert out["match_index"].dtype == torch.int64 and dec.double().mean().item() >= 1 - EXCUSED_MAX
    assert torch.equal(idx[dec], a_idx[dec])
    errs = {"potential_q": (out["potential_q"].reshape(Bm, N).double() - f).abs().max().item(),
            "potential_k": (out["potential_k"].reshape(Bm, Nk).double() - g).abs().max().item(),
            "match_lse": (out["match_lse"].reshape(Bm, N).double() - a_lse).abs().max().item(),
            "key_mass": (out["key_mass"].double() - 1).abs().max().item()}
    m_ref, _ = tc.masses(L, f, g)
    errs["match_mass"] = ((out["match_mass"].reshape(Bm, N).double() - m_ref).abs() / m_ref).max().item()
    want_p = torch.exp(z.gather(2, idx) - a_lse.unsqueeze(2))
    errs["match_prob"] = ((prob - want_p).abs() / want_p).max().item()
    print(f"[transport] module transport_match k={k}: " + "  ".join(f"{n} {e:.3e}" for n, e in errs.items()) + f"  (bound {bound:.3e})")
    assert all(errs[n] <= bound for n in ("potential_q", "potential_k", "match_lse", "key_mass")), errs
    assert errs["match_mass"] <= math.expm1(2 * bound) and errs["match_prob"] <= math.expm1(2 * bound), errs
    first = out["match_index"][:, 0] if k > 1 else out["match_index"]
    assert torch.equal(out["warp_hard"], _gather_reference(ref_img, first.reshape(Bm, -1), 16, 16, 4))
    # the point of the feature: no exemplar cell serves more queries under the balanced plan than under the softmax
    with torch.no_grad():
        plain = net.match(ref_img, seg, ref_seg)["match_index"].reshape(Bm, -1)
    share = lambda ix: max(int(torch.bincount(ix[b_], minlength=Nk).max()) for b_ in range(Bm))
    print(f"[transport] module: most-used exemplar cell serves {share(plain)} queries under the softmax, {share(first.reshape(Bm, -1))} under transport")


def test_module_sparse_warp_transport():
    net, ref_img, real, seg, ref_seg, _ = _mod()
    out = net.sparse_warp(ref_img, real, seg, ref_seg, topk=4, transport=dict(iters=ITERS_MOD, tau=1.0))
    assert {"warp_out", "match_index", "match_weight", "potential_k", "match_mass"} <= set(out)
    with torch.no_grad():
        m = net.transport_match(ref_img, seg, ref_seg, iters=ITERS_MOD, topk=4)
    # (sparse_warp's planes come from K1 with autograd, transport_match's from the K23 pair: the same candidates, potentials that
    # agree to the planes' rounding — ten half-steps of lse_bound)
    assert torch.equal(out["match_index"], m["match_index"])
    assert (out["potential_k"] - m["potential_k"]).abs().max().item() <= 2 * ITERS_MOD * lse_bound(m["potential_k"])
    out["warp_out"].square().sum().backward()
    for p in (net.theta.weight, net.phi.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    net.zero_grad(set_to_none=True)
    a = net.sparse_warp(ref_img, real, seg, ref_seg, topk=4)
    b_ = net.sparse_warp(ref_img, real, seg, ref_seg, topk=4, transport=None)
    assert sorted(a) == sorted(b_) and all(torch.equal(a[n], b_[n]) for n in a)


OUT_OF_SCOPE = [dict(match_kernel=3), dict(PONO_C=False), dict(warp_patch=True), dict(warp_bilinear=True), dict(warp_cycle_w=1.0),
                dict(two_cycle=True), dict(warp_mask_losstype="cycle")]


@pytest.mark.parametrize("flags", OUT_OF_SCOPE, ids=[next(iter(f)) for f in OUT_OF_SCOPE])
def test_every_out_of_scope_flag_set_raises(flags, monkeypatch):
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse, correspondence_transport
    net, ref_img, real, seg, ref_seg, _ = _mod()
    theta, phi, img, s1, s2 = _hot_case(8, 8, 77)
    cfg = HotPathConfig(**dict(dict(match_kernel=1, PONO_C=True, down=4), **flags))
    with pytest.raises(ValueError, match="transport"):
        correspondence_transport(theta, phi, cfg)
    with pytest.raises(ValueError, match="transport"):
        correspondence_sparse(theta, phi, img, s1, s2, cfg, 0.01, 4, transport=TRANSPORT)
    for name, value in flags.items():
        monkeypatch.setattr(net.opt, name, value)
    with pytest.raises(ValueError, match="transport"):
        net.transport_match(ref_img, seg, ref_seg)
    with pytest.raises(ValueError, match="transport"):
        net.sparse_warp(ref_img, real, seg, ref_seg, transport=TRANSPORT)
    monkeypatch.undo()
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="transport"):
        net.transport_match(ref_img, seg, ref_seg)


# ---------------------------------------------------------------------------------------------------------------- memory
def test_transport_route_allocates_nothing_hw_by_hw():
    """B = 1, a 128 x 128 grid, three iterations: the peak above the live memory stays below 64 MiB — one sixteenth of the 1 GiB that
    ONE [Nq,Nk] fp32 matrix of this grid takes (64 MiB is the matrix of a 64 x 64 grid)"""
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_transport
    N = 128 * 128
    gen = torch.Generator().manual_seed(21)
    theta, phi = torch.randn(1, 256, 128, 128, generator=gen).to(DEV), torch.randn(1, 256, 128, 128, generator=gen).to(DEV)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = correspondence_transport(theta, phi, cfg, iters=3)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"[transport] peak memory above live: {peak / 2 ** 20:.1f} MiB (the matrix: {N * N * 4 / 2 ** 20:.0f} MiB)")
    assert peak < 64 * 2 ** 20
    assert bool(torch.isfinite(out["potential_k"]).all()) and (out["key_mass"].double() - 1).abs().max().item() < 1e-2


# ---------------------------------------------------------------------------------------------------------------- guards
def test_transport_hands_over_live_buffers_only(monkeypatch):
    import test_gpu_live_buffers as lb
    net, ref_img, real, seg, ref_seg, _ = _mod()
    guard = lb._Guard(monkeypatch)
    with torch.no_grad():
        net.transport_match(ref_img, seg, ref_seg, iters=2, topk=4, hard_warp=True)
    out = net.sparse_warp(ref_img, real, seg, ref_seg, topk=4, transport=dict(iters=2, tau=0.7))
    out["warp_out"].sum().backward()
    net.zero_grad(set_to_none=True)
    guard.check(20, 75)


# ---- red zones: the cases join tests/test_gpu_red_zones.py's table at import time, so its coverage report and its "every entry point
# ---- was reached" audit count the two K50 entry points.  Partial query / key tiles, k = 3 and k = 8, a bias with -inf entries: a read
# ---- past k_bias [B,Nk] meets a guard's NaN bits (which would surface in val / lse), a write past idx / val / w lands in a guard
def _rz_corr_topk_biased(c):
    from cocosnet_amd import ops
    q, k = c.data(rz.unit(2, 256, 132, 31)), c.data(rz.unit(2, 256, 68, 32))
    bias = tc.make_bias(2, 68, 45)
    bias[:, -1] = 2.0
    bias = c.data(bias)
    outs = []
    for kk in (3, 8):
        idx, val, lse = ops.corr_topk_biased(q, k, bias, 100.0, kk)
        assert int(idx.min()) >= 0 and int(idx.max()) < 68
        outs += [idx, val, lse]
    f, g, row_lse = ops.corr_sinkhorn(q, k, 100.0, 2, 0.7)
    return outs + [f, g, row_lse]


def _rz_sparse_warp_biased(c):
    from cocosnet_amd import ops
    q, k = c.data(rz.unit(2, 256, 132, 33)), c.data(rz.unit(2, 256, 68, 34))
    gen = torch.Generator().manual_seed(46)
    v = c.data(torch.randn(2, 5, 68, generator=gen))
    idx = c.data(torch.randint(0, 68, (2, 132, 3), generator=gen).to(torch.int32))
    bias = c.data(torch.randn(2, 68, generator=gen) * 5)
    out, w = ops.sparse_softmax_warp(q, k, v, idx, 100.0, return_weights=True, k_bias=bias)
    return [out, w]


RZ_CASES = {"corr_topk_biased-2x132x68-k3+k8+sinkhorn": (_rz_corr_topk_biased, ENTRY),
            "sparse_softmax_warp_biased-2x132x68-k3": (_rz_sparse_warp_biased, WARP_ENTRY)}
for _name, (_body, _) in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_op_inside_red_zones(name, monkeypatch):
    rz.test_red_zones(name, monkeypatch)
    assert RZ_CASES[name][1] in set(rz.COVERAGE[name][0])
