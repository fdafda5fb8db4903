"""K50 (the biased readout, the Sinkhorn iteration and the transport match), the parts that need no GPU: the two entry points in header,
binding table and library, their argument checks (which return before any HIP call), the refusals of ops.corr_topk_biased /
corr_sinkhorn / sparse_softmax_warp(k_bias=...), hot_path.correspondence_transport / correspondence_sparse(transport=...) and
NoVGGCorrespondence.transport_match / sparse_warp(transport=...) in the family's order, the launch sequence transport=None leaves alone,
and the restatement (tests/transport_case.py): by hand on a 2 x 3 grid, on the planted collapse, and the share of positions its own
gaps excuse for the seeds the GPU tests use."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transport_case as tc  # noqa: E402

ENTRY = "cocos_corr_topk_bias_f16x3"
WARP_ENTRY = "cocos_sparse_softmax_warp_bias_fwd_f16x3"
_P, _I, _F, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
#: tests/test_gpu_match.py's constants, restated (that module needs a GPU to import): the CPU test below checks they still agree
INV_T, TOL = 100.0, 4 * 9.70e-6
SHAPES = [(64, 64), (256, 128), (132, 68), (36, 260)]


def test_constants_are_the_gpu_tests():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_match.py")).read()
    assert "E_FWD = 9.70e-6" in src and "TOL = 4 * E_FWD" in src and "INV_T = 100.0" in src
    assert "SHAPES = [(64, 64), (256, 128), (132, 68), (36, 260)]" in src


def test_header_table_and_library_carry_the_entry_points(hip_lib):
    from cocosnet_amd import _lib, build
    for name in (ENTRY, WARP_ENTRY):
        assert _lib.PROTOTYPES.get(name, ("",))[0] == "int", f"{name} is not declared in cocos_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    assert "corr_topk_bias_f16x3.hip" in build.HIP_SOURCES and os.path.exists(os.path.join(build.CSRC_DIR, "corr_topk_bias_f16x3.hip"))
    plain = list(_lib._SIGNATURES["cocos_corr_topk_f16x3"][1])
    assert list(_lib._SIGNATURES[ENTRY][1]) == plain[:4] + [_P] + plain[4:]                       # the bias after the planes
    warp = list(_lib._SIGNATURES["cocos_sparse_softmax_warp_fwd_f16x3"][1])
    assert list(_lib._SIGNATURES[WARP_ENTRY][1]) == warp[:6] + [_P] + warp[6:-1] + [_LL, _P]      # the bias after idx, its stride before the stream


def test_argument_validation_needs_no_gpu(hip_lib):
    """null bias, k = 0 / 9, misaligned planes or bias (-1); K != 256, Nk % 4 != 0 (-2): all before any HIP call"""
    one, f = ctypes.c_void_p(16), ctypes.c_float
    err = hip_lib.cocos_last_error_string

    def call(K=256, Nk=64, k=4, stride=0, qh=one, bias=one, out=one):
        return hip_lib.cocos_corr_topk_bias_f16x3(qh, one, one, one, bias, out, one, one, 1, K, 64, Nk, k, f(100.0), f(16.0), stride, None)

    assert call(bias=None) == -1 and b"null bias" in err()
    assert call(out=None) == -1 and b"null" in err()
    assert call(K=128) == -2 and b"K == 256" in err()
    assert call(k=0) == -1 and b"k=0" in err()
    assert call(k=9) == -1 and b"k=9" in err()
    assert call(Nk=4, k=8) == -1 and b"Nk=4" in err()
    assert call(Nk=66) == -2 and b"multiple of 4" in err()
    assert call(stride=64) == -1 and b"k_batch_stride" in err()
    assert call(qh=ctypes.c_void_p(24)) == -1 and b"aligned" in err()
    assert call(bias=ctypes.c_void_p(18)) == -1 and b"aligned" in err()

    def warp(K=256, Nk=64, k=4, stride=64, qh=one, bias=one, w=one):
        return hip_lib.cocos_sparse_softmax_warp_bias_fwd_f16x3(qh, one, one, one, one, one, bias, one, w, 1, K, 64, Nk, 3, k, f(100.0), f(16.0), stride, None)

    assert warp(bias=None) == -1 and b"null" in err()
    assert warp(w=None) == -1 and b"null" in err()
    assert warp(K=128) == -2 and b"K == 256" in err()
    assert warp(k=0) == -1 and warp(k=9) == -1 and b"k=9" in err()
    assert warp(stride=32) == -1 and b"bias_batch_stride" in err()
    assert warp(qh=ctypes.c_void_p(24)) == -1 and b"aligned" in err()
    assert warp(bias=ctypes.c_void_p(18)) == -1 and b"aligned" in err()


def test_ops_refuse_in_the_family_order(hip_lib, monkeypatch):
    """TypeError / ValueError first, then the CPU tensors, then the flavour (which only a GPU tensor reaches)"""
    from cocosnet_amd import _lib, ops
    q, k = torch.randn(2, 256, 36), torch.randn(2, 256, 8)
    bias = torch.zeros(2, 8)
    for bad in (bias.double(), bias.long(), None, [0.0] * 8):
        with pytest.raises(TypeError, match="k_bias"):
            ops.corr_topk_biased(q, k, bad, 100.0, 2)
    for bad in (bias[:1], bias[:, :7], bias.reshape(2, 2, 4)):
        with pytest.raises(ValueError, match="k_bias"):
            ops.corr_topk_biased(q, k, bad, 100.0, 2)
    with pytest.raises(ValueError, match="not differentiable"):
        ops.corr_topk_biased(q, k, bias.clone().requires_grad_(True), 100.0, 2)
    for bad in (0, 9, -1, 2.5, True):
        with pytest.raises(ValueError, match="k="):
            ops.corr_topk_biased(q, k, bias, 100.0, bad)
    with pytest.raises(ValueError):
        ops.corr_topk_biased(q[0], k, bias, 100.0, 2)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.corr_topk_biased(q, k, bias, 100.0, 2)
    # corr_sinkhorn
    for bad in (0, 65, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="iters"):
            ops.corr_sinkhorn(q, k, 100.0, bad)
    for bad in (0, 0.0, -0.5, 1.5, True, None, "1"):
        with pytest.raises(ValueError, match="tau"):
            ops.corr_sinkhorn(q, k, 100.0, 3, bad)
    with pytest.raises(ValueError, match="multiples of 4"):
        ops.corr_sinkhorn(q[:, :, :35], k, 100.0, 3)
    with pytest.raises(ValueError, match="multiples of 4"):
        ops.corr_sinkhorn(q, k[:, :, :6], 100.0, 3)
    with pytest.raises(ValueError):
        ops.corr_sinkhorn(q, k[:1], 100.0, 3)                               # no shared key set
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.corr_sinkhorn(q, k, 100.0, 3, 0.7)
    # sparse_softmax_warp(k_bias=...)
    v, idx = torch.randn(2, 3, 8), torch.zeros(2, 36, 2, dtype=torch.int64)
    with pytest.raises(TypeError, match="k_bias"):
        ops.sparse_softmax_warp(q, k, v, idx, 100.0, k_bias=bias.double())
    with pytest.raises(ValueError, match="k_bias"):
        ops.sparse_softmax_warp(q, k, v, idx, 100.0, k_bias=bias[:1])
    with pytest.raises(ValueError, match="not differentiable"):
        ops.sparse_softmax_warp(q, k, v, idx, 100.0, k_bias=bias.clone().requires_grad_(True))
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.sparse_softmax_warp(q, k, v, idx, 100.0, k_bias=bias)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(TypeError, match="k_bias"):                          # still the first refusal
        ops.corr_topk_biased(q, k, bias.double(), 100.0, 2)
    with pytest.raises(ValueError, match="iters"):
        ops.corr_sinkhorn(q, k, 100.0, 0)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):        # and the device before the flavour
        ops.corr_topk_biased(q, k, bias, 100.0, 2)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.corr_sinkhorn(q, k, 100.0, 3)


def _theta_phi():
    g = torch.Generator().manual_seed(5)
    return torch.randn(1, 256, 2, 2, generator=g), torch.randn(1, 256, 2, 2, generator=g)


OFF_ROUTE = [dict(match_kernel=3), dict(PONO_C=False), dict(warp_patch=True), dict(warp_bilinear=True), dict(warp_cycle_w=1.0),
             dict(two_cycle=True), dict(warp_mask_losstype="cycle")]
BAD_TRANSPORT = ["sinkhorn", 5, True, (5, 1.0), {}, dict(iters=5), dict(iters=5, tau=1.0, eps=1), dict(iters=0, tau=1.0), dict(iters=65, tau=1.0),
                 dict(iters=2.0, tau=1.0), dict(iters=5, tau=0), dict(iters=5, tau=1.5), dict(iters=5, tau=None)]
GOOD = dict(iters=5, tau=1.0)


def test_hot_path_checks_transport(hip_lib, monkeypatch):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse, correspondence_transport
    theta, phi = _theta_phi()
    img, seg = torch.zeros(1, 3, 8, 8), torch.zeros(1, 5, 8, 8)
    base = dict(match_kernel=1, PONO_C=True, down=4)
    cfg = HotPathConfig(**base)
    sparse = lambda c=cfg, th=theta, ph=phi, **kw: correspondence_sparse(th, ph, img, seg, seg, c, 0.01, 2, **kw)
    for bad in BAD_TRANSPORT:
        with pytest.raises(ValueError, match="transport"):
            sparse(transport=bad)
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="transport.*iters"):
            correspondence_transport(theta, phi, cfg, iters=bad)
    for bad in (0, 1.5, None):
        with pytest.raises(ValueError, match="transport.*tau"):
            correspondence_transport(theta, phi, cfg, tau=bad)
    for bad in (0, 9, True):
        with pytest.raises(ValueError, match="topk"):
            correspondence_transport(theta, phi, cfg, topk=bad)
    for flags in OFF_ROUTE:
        off = HotPathConfig(**dict(base, **flags))
        with pytest.raises(ValueError, match="transport"):
            correspondence_transport(theta, phi, off)
        with pytest.raises(ValueError, match="transport"):
            sparse(off, transport=GOOD)
    with pytest.raises(ValueError, match="transport.*prepared exemplar"):
        sparse(exemplar=object(), transport=GOOD)
    with pytest.raises(ValueError, match="transport.*search"):
        sparse(search="patchmatch", transport=GOOD)
    with pytest.raises(ValueError, match="transport.*restrict"):
        sparse(restrict="label", transport=GOOD)
    with pytest.raises(ValueError, match="transport"):
        sparse(th=theta[:, :128], ph=phi[:, :128], transport=GOOD)
    with pytest.raises(ValueError, match="transport"):
        correspondence_transport(theta[:, :128], phi[:, :128], cfg)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="COCOS_PRECISION=fp32.*transport"):
        correspondence_transport(theta, phi, cfg)
    with pytest.raises(ValueError, match="COCOS_PRECISION=fp32.*transport"):
        sparse(transport=GOOD)
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    # in scope: the tensors themselves are refused
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        correspondence_transport(theta, phi, cfg, iters=2, tau=0.5, topk=2)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        sparse(transport=GOOD)


def test_module_refuses_before_the_network_runs(hip_lib, monkeypatch):
    from cocosnet_amd import _lib
    from cocosnet_amd import correspondence as cc
    g = torch.Generator().manual_seed(3)
    img = torch.rand(1, 3, 64, 64, generator=g)
    seg = torch.zeros(1, 7, 64, 64).scatter_(1, torch.randint(0, 7, (1, 1, 64, 64), generator=g), 1.0)
    for flags, block in [(dict(), False)] + [(f, True) for f in OFF_ROUTE[:2]]:
        opt = cc.ade20k_options(**dict(dict(crop_size=64, semantic_nc=7, match_kernel=1), **flags))
        torch.manual_seed(0)
        net = cc.NoVGGCorrespondence(opt).eval()
        if block:
            monkeypatch.setattr(net, "project", lambda *a, **k: pytest.fail("project() ran for a refused transport"))
            with pytest.raises(ValueError, match="transport"):
                net.transport_match(img, seg, seg)
            with pytest.raises(ValueError, match="transport"):
                net.sparse_warp(img, img, seg, seg, transport=GOOD)
            continue
        ran = []
        monkeypatch.setattr(net, "project", lambda *a, **k: ran.append(1) or pytest.fail("project() ran for a refused argument"))
        for kw in (dict(iters=0), dict(iters=65), dict(tau=0), dict(tau=2), dict(topk=0), dict(topk=9)):
            with pytest.raises(ValueError):
                net.transport_match(img, seg, seg, **kw)
        with pytest.raises(ValueError, match="required"):
            net.transport_match(None, seg, seg)
        for bad in BAD_TRANSPORT:
            with pytest.raises(ValueError, match="transport"):
                net.sparse_warp(img, img, seg, seg, transport=bad)
        with pytest.raises(ValueError, match="transport.*search"):
            net.sparse_warp(img, img, seg, seg, transport=GOOD, search="patchmatch")
        with pytest.raises(ValueError, match="transport.*restrict"):
            net.sparse_warp(img, img, seg, seg, transport=GOOD, restrict="label")
        assert not ran
        monkeypatch.undo()
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):      # in scope: the network runs (on the CPU) and the tensors are refused
            net.transport_match(img, seg, seg)


def test_transport_none_leaves_the_launch_sequence_of_sparse_warp_alone(hip_lib, monkeypatch):
    """the calls correspondence_sparse makes into ops, in order, with and without the keyword: the same list, none of them K50's (the
    ops are stubbed with CPU stand-ins, so this runs without a GPU)"""
    from cocosnet_amd import hot_path, ops
    calls = []
    theta, phi = _theta_phi()
    img, seg = torch.zeros(1, 3, 8, 8), torch.zeros(1, 5, 8, 8)

    def stub(name, ret):
        def f(*a, **kw):
            calls.append((name, sorted(kw)))
            return ret(*a, **kw)
        monkeypatch.setattr(ops, name, f)

    monkeypatch.setattr(hot_path, "_hip_fp32", lambda t: True)
    stub("center_l2norm_planes", lambda x, *a, **kw: x)
    stub("corr_topk", lambda qn, kn, inv_t, k, planes: (torch.zeros(1, 4, k, dtype=torch.int32), None, None))
    stub("corr_topk_biased", lambda *a, **kw: pytest.fail("the biased readout ran without transport"))
    stub("corr_sinkhorn", lambda *a, **kw: pytest.fail("the iteration ran without transport"))
    stub("warp_values", lambda img_, seg_, down: torch.zeros(1, 3, 2, 2))
    stub("sparse_softmax_warp", lambda qn, kn, v, idx, inv_t, planes, **kw: (torch.zeros(1, 3, 4), torch.zeros(1, 4, idx.shape[2])))
    stub("upsample_nearest", lambda y, down: y.repeat_interleave(down, 2).repeat_interleave(down, 3))
    cfg = hot_path.HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    a = hot_path.correspondence_sparse(theta, phi, img, seg, seg, cfg, 0.01, 2)
    first, calls[:] = list(calls), []
    b = hot_path.correspondence_sparse(theta, phi, img, seg, seg, cfg, 0.01, 2, transport=None)
    assert first == calls and [n for n, _ in calls] == ["center_l2norm_planes", "center_l2norm_planes", "corr_topk", "warp_values",
                                                         "sparse_softmax_warp", "upsample_nearest"]
    assert dict(calls)["sparse_softmax_warp"] == ["return_weights"], "k_bias is passed on the route without transport"
    assert sorted(a) == sorted(b) == ["match_index", "match_weight", "warp_out"]


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_by_hand_on_a_2x3_grid():
    """exp L = [[1, 2, 4], [2, 1, 1]], mu = 1/2, nu = 1/3.
    Biased top-k with bias = [0, ln 2, -inf]: exp z = [[1, 4, 0], [2, 2, 0]] -> row 0: keys (1, 0), lse ln 5; row 1: a tie, keys (0, 1), lse ln 4.
    One balanced iteration from g = 0: row sums 7 and 4 -> e^f = (1/14, 1/8); column sums of e^f e^L: 1/14 + 2/8 = 9/28,
    2/14 + 1/8 = 15/56, 4/14 + 1/8 = 23/56 -> e^g = (1/3) / those = (28/27, 56/45, 56/69).  Row sums against the final g:
    r0 = 28/27 + 2 * 56/45 + 4 * 56/69, r1 = 2 * 28/27 + 56/45 + 56/69; match_mass = e^f r / mu = (r0 / 7, r1 / 4); key_mass = 1."""
    L = torch.tensor([[[1.0, 2.0, 4.0], [2.0, 1.0, 1.0]]], dtype=torch.float64).log()
    idx, val, lse, z = tc.biased_topk(L, torch.tensor([[0.0, math.log(2.0), tc.NEG_INF]], dtype=torch.float64), 2)
    assert idx.tolist() == [[[1, 0], [0, 1]]]
    assert torch.allclose(val.exp(), torch.tensor([[[4.0, 1.0], [2.0, 2.0]]], dtype=torch.float64), rtol=1e-14)
    assert torch.allclose(lse.exp(), torch.tensor([[5.0, 4.0]], dtype=torch.float64), rtol=1e-14)
    idx3, val3, _, _ = tc.biased_topk(L, torch.tensor([[0.0, math.log(2.0), tc.NEG_INF]], dtype=torch.float64), 3)
    assert idx3[0, :, 2].tolist() == [2, 2] and bool(torch.isinf(val3[0, :, 2]).all())
    lse_all, = tc.biased_topk(L, torch.full((1, 3), tc.NEG_INF), 1)[2:3]
    assert bool((lse_all == tc.NEG_INF).all())                                                   # every key excluded: -inf, no NaN
    f, g, row_lse = tc.sinkhorn(L, 1, 1.0)
    assert torch.allclose(f.exp(), torch.tensor([[1 / 14, 1 / 8]], dtype=torch.float64), rtol=1e-14)
    assert torch.allclose(g.exp(), torch.tensor([[28 / 27, 56 / 45, 56 / 69]], dtype=torch.float64), rtol=1e-14)
    r0, r1 = 28 / 27 + 2 * 56 / 45 + 4 * 56 / 69, 2 * 28 / 27 + 56 / 45 + 56 / 69
    assert torch.allclose(row_lse.exp(), torch.tensor([[r0, r1]], dtype=torch.float64), rtol=1e-14)
    mm, km = tc.masses(L, f, g)
    assert torch.allclose(mm, torch.tensor([[r0 / 7, r1 / 4]], dtype=torch.float64), rtol=1e-14)
    assert torch.allclose(km, torch.ones(1, 3, dtype=torch.float64), rtol=1e-14)
    # tau = 1/2: every potential is half its balanced update -> e^f = (1/sqrt 14, 1/sqrt 8), e^g_j = sqrt((1/3) / sum_i e^f_i e^L_ij)
    f2, g2, _ = tc.sinkhorn(L, 1, 0.5)
    ef = [14 ** -0.5, 8 ** -0.5]
    cols = [ef[0] * a + ef[1] * b for a, b in ((1, 2), (2, 1), (4, 1))]
    assert torch.allclose(f2.exp(), torch.tensor([ef], dtype=torch.float64), rtol=1e-14)
    assert torch.allclose(g2.exp(), torch.tensor([[(1 / 3 / c) ** 0.5 for c in cols]], dtype=torch.float64), rtol=1e-14)
    # the warp: query 0's two best keys under g are given by hand — weights softmax(L + g) on them, potentials without gradient
    qn = torch.eye(3, dtype=torch.float64)[:, :2].unsqueeze(0).clone().requires_grad_(True)       # [1,3,2]
    kn = torch.eye(3, dtype=torch.float64).unsqueeze(0).clone().requires_grad_(True)              # L = inv_t * I (rows 0, 1)
    v = torch.tensor([[[1.0, 10.0, 100.0]]], dtype=torch.float64).requires_grad_(True)
    gg = torch.tensor([[0.0, math.log(3.0), 0.0]], dtype=torch.float64, requires_grad=True)
    out, w, ix = tc.sparse_warp(qn, kn, v, gg, math.log(2.0), 2)
    # z = [[ln 2, ln 3, 0], [0, ln 2 + ln 3, 0]] -> row 0: keys (1, 0), weights (3, 2) / 5; row 1: keys (1, 0), weights (6, 1) / 7
    assert ix.tolist() == [[[1, 0], [1, 0]]]
    assert torch.allclose(w, torch.tensor([[[0.6, 0.4], [6 / 7, 1 / 7]]], dtype=torch.float64), rtol=1e-14)
    assert torch.allclose(out, torch.tensor([[[6.4, 61 / 7]]], dtype=torch.float64), rtol=1e-14)
    out.sum().backward()
    assert gg.grad is None and qn.grad is not None and kn.grad is not None and v.grad is not None


def test_planted_collapse_on_the_restatement_alone():
    q, k, pi = tc.planted()
    assert q.shape == (3, 256, 64) and k.shape == (3, 256, 64) and q.shape[2] % 4 == 0
    L = tc.logits(q, k, INV_T)
    assert bool((L.argmax(-1) == 0).all()), "the plain argmax does not collapse onto the hub"
    gap0 = (L.sort(-1, descending=True).values[..., 0] - L.sort(-1, descending=True).values[..., 1]).min().item()
    f, g, _ = tc.sinkhorn(L, 5, 1.0)
    idx, val, _, _ = tc.biased_topk(L, g, 2)
    assert torch.equal(idx[..., 0], pi), "five balanced iterations do not recover the permutation"
    gap5 = (val[..., 0] - val[..., 1]).min().item()
    print(f"[transport] planted: plain margin {gap0:.2f}, margin after 5 iterations {gap5:.2f} (kernel bound ~1e-3)")
    assert gap0 > 1.0 and gap5 > 1.0       # both facts hold by margins a thousand times the kernels' error
    assert sorted(pi[0, :-1].tolist()) == list(range(1, 64)) and int(pi[0, -1]) == 0


@pytest.mark.parametrize("Nq,Nk", SHAPES)
def test_seeds_of_the_gpu_tests_excuse_less_than_one_percent(Nq, Nk):
    for shared in (False, True):
        q, k = tc.readout_case(3, Nq, Nk)
        bias = tc.make_bias(3, Nk, tc.bias_seed(Nq, Nk, shared))
        if shared:
            k, bias = k[:1], bias[:1]
        fin = torch.isfinite(bias)
        assert 0.03 <= 1 - fin.double().mean().item() <= 0.20
        bound = TOL * (INV_T + bias[fin].abs().max().item()) / INV_T
        z = tc.biased_topk(tc.logits(q, k, INV_T), bias, 1)[3]
        for kk in (1, 4):
            assert 1 - tc.decided(z, kk, bound).double().mean().item() <= 0.01
