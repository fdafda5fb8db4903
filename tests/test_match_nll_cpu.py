"""K49 (trainable match readout), the parts that need no GPU: the restatement (tests/match_nll_case.py) on a hand-made case, the three
entry points in header, binding table and library, their argument checks (which return before any HIP call), the refusals of
ops.corr_lse / ops.corr_pair_nll, hot_path.correspondence_nll and NoVGGCorrespondence.match_loss in their order, the target and weight
validation, the loss reduction with no supervised position, and in numpy what a lost lo plane measures against the peaked regime's rule."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy_case as ac  # noqa: E402
import match_nll_case as nc  # noqa: E402

SWEEP, PAIR, PAIR_BWD = "cocos_corr_lse_bwd_f16x3", "cocos_pair_logits_f16x3", "cocos_pair_logits_bwd_query_f16x3"
_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


def test_restatement_on_a_hand_made_case():
    """One channel pair, a 2 x 3 content grid (6 queries) against a 3 x 2 exemplar grid (6 keys), inv_t = 1: query i is e_0 for i < 3 and
    e_1 otherwise, key j is e_0 for even j and e_1 for odd j, so L[i,j] is 1 where the two agree and 0 elsewhere: every row and every
    column holds three ones and three zeros, lse = log(3 e + 3).  Target t_i = i, query 4 unsupervised: the pair logits are worked out
    below."""
    q = torch.zeros(1, 2, 6)
    q[0, 0, :3], q[0, 1, 3:] = 1.0, 1.0
    k = torch.zeros(1, 2, 6)
    k[0, 0, 0::2], k[0, 1, 1::2] = 1.0, 1.0
    lse = math.log(3 * math.e + 3)
    row, col = nc.lse_pair(q, k, 1.0)
    assert torch.allclose(row, torch.full((1, 6), lse, dtype=torch.float64)) and torch.allclose(col, torch.full((1, 6), lse, dtype=torch.float64))
    t = torch.tensor([[0, 1, 2, 3, -1, 5]])
    # L[i, t_i]: query 0 (e_0) key 0 (e_0): 1; 1 / 1: e_0 . e_1 = 0; 2 / 2: 1; 3 (e_1) / 3 (e_1): 1; 5 / 5: 1
    s = [1.0, 0.0, 1.0, 1.0, None, 1.0]
    r, c = nc.pair_nll(q, k, t, 1.0)
    for i, si in enumerate(s):
        want = 0.0 if si is None else lse - si
        assert abs(float(r[0, i]) - want) < 1e-12 and abs(float(c[0, i]) - want) < 1e-12, i
    # d row_lse_0 / d q_0 = sum_j p_0j k_j = (3 e e_0 + 3 e_1) / (3 e + 3)
    g = nc.restate(q, k, 1.0, (torch.tensor([[1.0, 0, 0, 0, 0, 0]]), None))
    p1 = math.e / (math.e + 1)
    assert torch.allclose(g["dq"][0, :, 0], torch.tensor([p1, 1 - p1], dtype=torch.float64)) and not g["dq"][0, :, 1:].any()
    # and the key side of the same term: d / d k_j = p_0j q_0
    assert torch.allclose(g["dk"][0, 0], torch.tensor([p1 / 3, (1 - p1) / 3] * 3, dtype=torch.float64)) and not g["dk"][0, 1].any()


def test_header_table_library_and_exports(hip_lib):
    from cocosnet_amd import _lib, build, correspondence, hot_path, ops
    for name in (SWEEP, PAIR, PAIR_BWD):
        assert _lib.PROTOTYPES.get(name, ("",))[0] == "int", f"{name} is not declared in cocos_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    assert "corr_lse_bwd_f16x3.hip" in build.HIP_SOURCES and os.path.exists(os.path.join(build.CSRC_DIR, "corr_lse_bwd_f16x3.hip"))
    assert list(_lib._SIGNATURES[SWEEP][1]) == [_P] * 9 + [_I] * 4 + [_F] * 2 + [_P]
    assert list(_lib._SIGNATURES[PAIR][1]) == [_P] * 6 + [_I] * 4 + [_F] * 2 + [_P]
    assert list(_lib._SIGNATURES[PAIR_BWD][1]) == [_P] * 5 + [_I] * 4 + [_F] * 2 + [_I, _P]
    assert callable(ops.corr_lse) and callable(ops.corr_pair_nll) and callable(hot_path.correspondence_nll)
    assert callable(hot_path.nll_reduce) and callable(correspondence.NoVGGCorrespondence.match_loss)


def test_argument_validation_needs_no_gpu(hip_lib):
    """null and misaligned pointers and zero dims (-1); K = 128, Nq = 66, Nk = 66 (-2): all before any HIP call"""
    one, f = ctypes.c_void_p(16), ctypes.c_float
    err = hip_lib.cocos_last_error_string
    names = ["qh", "ql", "kh", "kl", "row_lse", "col_lse", "g_row", "g_col", "out_t"]

    def call(B=1, K=256, Nq=64, Nk=64, **ptr):
        return hip_lib.cocos_corr_lse_bwd_f16x3(*[ptr.get(n, one) for n in names], B, K, Nq, Nk, f(100.0), f(16.0), None)

    for n in ("qh", "ql", "kh", "kl", "out_t"):
        assert call(**{n: None}) == -1 and b"null" in err(), n
        assert call(**{n: ctypes.c_void_p(24)}) == -1 and b"aligned" in err(), n
    assert call(g_row=None, g_col=None) == -1 and b"both null" in err()
    assert call(g_col=None, col_lse=None, K=128) == -2                   # one null g (with its lse) is legal: the next refusal answers
    assert call(g_row=None, row_lse=None, K=128) == -2
    assert call(row_lse=None) == -1 and b"without its lse" in err() and call(col_lse=None) == -1 and b"without its lse" in err()
    for n in ("row_lse", "col_lse", "g_row", "g_col"):
        assert call(**{n: ctypes.c_void_p(18)}) == -1 and b"aligned" in err(), n
    assert call(K=128) == -2 and b"K == 256" in err()
    assert call(Nq=66) == -2 and b"Nq=66" in err() and call(Nk=66) == -2 and b"Nk=66" in err()
    for zero in (dict(B=0), dict(Nq=0), dict(Nk=0)):
        assert call(**zero) == -1 and b"bad dims" in err(), zero

    def pair(B=1, K=256, Nq=6, Nk=6, **ptr):
        return hip_lib.cocos_pair_logits_f16x3(*[ptr.get(n, one) for n in ("qh", "ql", "kh", "kl", "target", "s")], B, K, Nq, Nk, f(100.0),
                                               f(16.0), None)

    def pair_bwd(B=1, K=256, Nq=6, Nk=6, **ptr):
        return hip_lib.cocos_pair_logits_bwd_query_f16x3(*[ptr.get(n, one) for n in ("kh", "kl", "target", "g", "dq_t")], B, K, Nq, Nk,
                                                         f(100.0), f(16.0), 0, None)

    for n in ("qh", "ql", "kh", "kl", "target", "s"):
        assert pair(**{n: None}) == -1 and b"null" in err(), n
    for n in ("kh", "kl", "target", "g", "dq_t"):
        assert pair_bwd(**{n: None}) == -1 and b"null" in err(), n
    for fn in (pair, pair_bwd):
        assert fn(K=128) == -2 and b"K == 256" in err()
        assert fn(B=0) == -1 and b"bad dims" in err()
        assert fn(kh=ctypes.c_void_p(24)) == -1 and b"aligned" in err()


def test_ops_refuse_in_the_family_order(hip_lib, monkeypatch):
    """TypeError / ValueError first (operands, then the table and its range), then the CPU tensors ("no CPU fallback"), then
    COCOS_PRECISION and the shapes outside corr_match_mutual_ok (which only GPU tensors reach)"""
    from cocosnet_amd import _lib, ops
    q, k = torch.randn(2, 256, 36), torch.randn(2, 256, 8)
    t = torch.zeros(2, 36, dtype=torch.int64)
    for fn, extra in ((ops.corr_lse, ()), (ops.corr_pair_nll, (t,))):
        name = fn.__name__
        with pytest.raises(TypeError, match=name):
            fn(None, k, *extra, 100.0)
        for bad_q, bad_k in ((q[0], k), (q, k[:1]), (q[:, :128], k), (q[:, :128], k[:, :128])):
            with pytest.raises(ValueError, match=name):
                fn(bad_q, bad_k, *extra, 100.0)
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            fn(q, k, *extra, 100.0)
        monkeypatch.setattr(ops, "PRECISION", "fp32")
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):      # the device before the flavour
            fn(q, k, *extra, 100.0)
        monkeypatch.setattr(ops, "PRECISION", "f16x3")
    with pytest.raises(TypeError, match="target"):
        ops.corr_pair_nll(q, k, t.float(), 100.0)
    with pytest.raises(TypeError, match="target"):
        ops.corr_pair_nll(q, k, None, 100.0)
    with pytest.raises(ValueError, match="target is"):
        ops.corr_pair_nll(q, k, t[:, :35], 100.0)
    bad = t.clone()
    bad[1, 7] = 8
    with pytest.raises(ValueError, match="below Nk=8"):
        ops.corr_pair_nll(q, k, bad, 100.0)
    bad[1, 7] = -5                                                            # negative: unsupervised, legal — the next refusal answers
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.corr_pair_nll(q, k, bad, 100.0)


def _cfg(**over):
    from cocosnet_amd.hot_path import HotPathConfig
    return HotPathConfig(**dict(dict(match_kernel=1, PONO_C=True, down=4), **over))


def test_hot_path_scope_targets_and_weights(hip_lib, monkeypatch):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import correspondence_nll
    theta, phi = torch.randn(2, 256, 2, 3), torch.randn(2, 256, 3, 2)
    t = torch.zeros(2, 2, 3, dtype=torch.int64)
    for over in (dict(match_kernel=3), dict(PONO_C=False), dict(warp_patch=True), dict(warp_bilinear=True), dict(warp_cycle_w=1.0),
                 dict(two_cycle=True), dict(warp_mask_losstype="cycle")):
        with pytest.raises(ValueError, match="match_loss"):
            correspondence_nll(theta, phi, t, _cfg(**over))
    with pytest.raises(ValueError, match="match_loss: symmetric"):
        correspondence_nll(theta, phi, t, _cfg(), symmetric=1)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="COCOS_PRECISION"):
        correspondence_nll(theta, phi, t, _cfg())
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    with pytest.raises(ValueError, match="prepared exemplar"):
        correspondence_nll(theta, phi, t, _cfg(), exemplar=object())
    with pytest.raises(ValueError, match="256 channels"):
        correspondence_nll(theta[:, :128], phi[:, :128], t, _cfg())
    with pytest.raises(TypeError, match="match_loss: target"):
        correspondence_nll(theta, phi, t.float(), _cfg())
    with pytest.raises(ValueError, match="match_loss: target is"):
        correspondence_nll(theta, phi, t[:, :1], _cfg())
    bad = t.clone()
    bad[0, 1, 2] = 6
    with pytest.raises(ValueError, match="below 6"):
        correspondence_nll(theta, phi, bad, _cfg())
    w = torch.ones(2, 2, 3)
    with pytest.raises(TypeError, match="match_loss: weight"):
        correspondence_nll(theta, phi, t, _cfg(), weight=w.double())
    with pytest.raises(ValueError, match="match_loss: weight is"):
        correspondence_nll(theta, phi, t, _cfg(), weight=w[:, :1])
    neg = w.clone()
    neg[1, 0, 0] = -0.5
    with pytest.raises(ValueError, match=">= 0"):
        correspondence_nll(theta, phi, t, _cfg(), weight=neg)
    nan = w.clone()
    nan[1, 0, 0] = float("nan")
    with pytest.raises(ValueError, match=">= 0"):
        correspondence_nll(theta, phi, t, _cfg(), weight=nan)
    nan[1, 0, 0] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        correspondence_nll(theta, phi, t, _cfg(), weight=nan)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):        # everything valid: the device is the next refusal
        correspondence_nll(theta, phi, t, _cfg(), weight=w)


def test_module_refuses_before_the_network_runs(hip_lib, monkeypatch):
    from cocosnet_amd import correspondence as cc
    x, seg = torch.zeros(1, 3, 32, 32), torch.zeros(1, 7, 32, 32)
    t = torch.zeros(1, 8, 8, dtype=torch.int64)
    for over in (dict(match_kernel=3), dict(PONO_C=False), dict(warp_bilinear=True), dict(warp_cycle_w=1.0)):
        net = cc.NoVGGCorrespondence(cc.ade20k_options(crop_size=32, semantic_nc=7, **dict(dict(match_kernel=1), **over)))
        monkeypatch.setattr(net, "project", lambda *a, **kw: pytest.fail("the network ran"))
        with pytest.raises(ValueError, match="match_loss"):
            net.match_loss(x, x, seg, seg, t)
    net = cc.NoVGGCorrespondence(cc.ade20k_options(crop_size=32, semantic_nc=7, match_kernel=1))
    monkeypatch.setattr(net, "project", lambda *a, **kw: pytest.fail("the network ran"))
    with pytest.raises(ValueError, match="match_loss: ref_img"):
        net.match_loss(None, x, seg, None, t)
    with pytest.raises(TypeError, match="match_loss: target"):
        net.match_loss(x, x, seg, seg, t.float())


def test_loss_reduction():
    from cocosnet_amd.hot_path import nll_reduce
    r = torch.tensor([[1.0, 2.0, 4.0]], requires_grad=True)
    c = torch.tensor([[0.5, 0.25, 8.0]], requires_grad=True)
    t = torch.tensor([[3, -1, 0]])
    w = torch.tensor([[2.0, 5.0, 1.0]])
    assert float(nll_reduce(r, c, t, None, True)) == (1.5 + 12.0) / 2
    assert float(nll_reduce(r, c, t, None, False)) == (1.0 + 4.0) / 2
    assert float(nll_reduce(r, c, t, w, True)) == (2 * 1.5 + 12.0) / 3          # the unsupervised position's weight counts nowhere
    loss = nll_reduce(r, c, torch.full_like(t, -1), w, True)                    # no supervised position: 0 with zero gradients
    assert float(loss) == 0.0
    loss.backward()
    assert not r.grad.any() and not c.grad.any()


def _named(t, Nk):
    return torch.zeros(t.shape[0], Nk, dtype=torch.bool).scatter_(1, t, True)


def test_reference_keeps_the_slice_cap_for_every_committed_case():
    """rel_slice may leave out at most 5 % of the positions, asserted on the fp64 reference alone, for every case tests/test_gpu_match_nll.py
    judges per slice: the twelve gradient cases (dk of corr_pair_nll at (36, 260): its named columns, match_nll_case.EXCLUDED_SPLIT) and
    the peaked cases at both temperatures"""
    todo = [(Nq, Nk, regime, nc.INV_T) for Nq, Nk, regime in nc.cases()]
    todo += [(Nq, Nk, "peaked", inv_t) for Nq, Nk in ((64, 64), (132, 68)) for inv_t in (100.0, 1000.0)]
    for Nq, Nk, regime, inv_t in todo:
        q, k = nc.make_qk(Nq, Nk, regime)
        ups_lse, ups_nll = nc.upstream(Nq, Nk)
        t = nc.targets(Nq, Nk, unsupervised=0.0)
        for kernel, ref in (("corr_lse", nc.restate(q, k, inv_t, ups_lse)), ("corr_pair_nll", nc.restate(q, k, inv_t, ups_nll, t))):
            for tensor in ("dq", "dk"):
                x = ref[tensor]
                if nc.EXCLUDED_SPLIT.get((kernel, Nq, Nk)) == tensor:
                    x = nc._columns(x, _named(t, Nk))
                share = ac.excluded_share(x)
                assert share <= ac.EXCLUDED_MAX, (kernel, Nq, Nk, regime, inv_t, tensor, share)


def _lost(q, k, a, b, inv_t, which):
    """{"dq", "dk"} of sum a row_lse + sum b col_lse with one lo plane lost: dk is dq of the exchanged problem (as the kernel runs it)"""
    n = lambda x: x.numpy()
    return {"dq": torch.from_numpy(nc.lost_plane_dq(n(q), n(k), n(a), n(b), inv_t, which)),
            "dk": torch.from_numpy(nc.lost_plane_dq(n(k), n(q), n(b), n(a), inv_t, which))}


@pytest.mark.parametrize("inv_t", [100.0, 1000.0])
@pytest.mark.parametrize("Nq,Nk", [(64, 64), (132, 68)])
def test_lost_lo_planes_against_the_peaked_rule(Nq, Nk, inv_t):
    """The peaked cases are judged after match_nll_case.lse_allowance.  fp64 arithmetic with ONE lo plane dropped — the keys' in the
    recomputed S, the keys' in W . Kn, or W's — goes through the same rule, for BOTH tensors under BOTH metrics, against torch's fp32 arm:
    at inv_t = 100 every loss misses the bound at least twofold everywhere.  At inv_t = 1000 a lost plane in S does (its logits move by
    1000 x 2^-12 |q||k|); the two planes of the second product do not and cannot: delta(1000) = 3.9e-4 — what an fp32 lse of magnitude
    1000 is good for, ulp 6.1e-5, through the forward's log2-domain sums — is ABOVE the 2^-12 .. 2^-11 a lost lo plane of W or Kn
    moves a weight by, so at that temperature no bound the fp32 interface can meet separates them; the figures are printed."""
    q, k = nc.make_qk(Nq, Nk, "peaked")
    (a, b), _ = nc.upstream(Nq, Nk)
    ref = nc.restate(q, k, inv_t, (a, b))
    arm = nc.restate(q, k, inv_t, (a, b), dtype=torch.float32)
    allow = nc.lse_allowance(q, k, a, b, inv_t)
    whole = nc.judge("numpy", (nc.B, Nq, Nk), f"peaked-{inv_t:g}-nothing-lost", _lost(q, k, a, b, inv_t, None), arm, ref, allow=allow)
    assert max(r[2] for r in whole.rows) < 1e-12                              # the emulation itself is the reference
    for which in ("k_lo_qk", "k_lo_wk", "w_lo"):
        j = nc.judge("numpy", (nc.B, Nq, Nk), f"peaked-{inv_t:g}-lost-{which}", _lost(q, k, a, b, inv_t, which), arm, ref, allow=allow)
        for tensor, metric, ek, ea, f in j.rows:
            over = ek / ac.bound(ea, f)
            print(f"[match_nll] lost {which} ({Nq},{Nk}) inv_t {inv_t:g} {tensor} {metric}: {over:.1f} x the bound")
            if inv_t == 100.0 or which == "k_lo_qk":
                assert over >= ac.TEETH, (which, Nq, Nk, inv_t, tensor, metric, over)
