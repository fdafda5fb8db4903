"""K47 (the label-restricted match readout), the parts that need no GPU: the entry point in header, binding table and library, its
argument checks (which return before any HIP call), the Python-side refusals of ops.corr_topk_labelled,
hot_path.correspondence_match(restrict=...) / correspondence_sparse(restrict=...) and NoVGGCorrespondence.match / sparse_warp in their
order, hot_path.cell_labels and hot_path.restrict_fallback against the restatement (tests/match_labels_case.py), and the restatement
itself on cases computed by hand."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_labels_case as lc  # noqa: E402

ENTRY = "cocos_corr_topk_labels_f16x3"
_P, _I, _F, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong


def test_header_table_and_library_carry_the_entry_point(hip_lib):
    from cocosnet_amd import _lib, build
    assert _lib.PROTOTYPES.get(ENTRY, ("",))[0] == "int", f"{ENTRY} is not declared in cocos_hip.h"
    assert ENTRY in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, ENTRY)
    assert "corr_topk_f16x3.hip" in build.HIP_SOURCES
    # the unlabelled entry's arguments with the two label pointers after the planes
    assert list(_lib._SIGNATURES[ENTRY][1]) == [_P] * 9 + [_I] * 5 + [_F] * 2 + [_LL, _P]
    plain = list(_lib._SIGNATURES["cocos_corr_topk_f16x3"][1])
    assert list(_lib._SIGNATURES[ENTRY][1]) == plain[:4] + [_P, _P] + plain[4:]


def test_argument_validation_needs_no_gpu(hip_lib):
    """null labels, k = 0 / 9, a misaligned plane (-1); K != 256, Nk % 4 != 0 (-2): all before any HIP call"""
    one, f = ctypes.c_void_p(16), ctypes.c_float
    err = hip_lib.cocos_last_error_string

    def call(K=256, Nk=64, k=4, stride=0, qh=one, ql_=one, kl_=one, out=one):
        return hip_lib.cocos_corr_topk_labels_f16x3(qh, one, one, one, ql_, kl_, out, one, one, 1, K, 64, Nk, k, f(100.0), f(16.0), stride, None)

    assert call(ql_=None) == -1 and b"null" in err()
    assert call(kl_=None) == -1 and b"null" in err()
    assert call(out=None) == -1 and b"null" in err()
    assert call(K=128) == -2 and b"K == 256" in err()
    assert call(k=0) == -1 and b"k=0" in err()
    assert call(k=9) == -1 and b"k=9" in err()
    assert call(Nk=4, k=8) == -1 and b"Nk=4" in err()
    assert call(Nk=66) == -2 and b"multiple of 4" in err()
    assert call(stride=64) == -1 and b"k_batch_stride" in err()
    assert call(qh=ctypes.c_void_p(24)) == -1 and b"aligned" in err()
    assert call(ql_=ctypes.c_void_p(18)) == -1 and b"aligned" in err()


def test_op_refuses_in_the_family_order(hip_lib, monkeypatch):
    """TypeError / ValueError first, then the CPU tensors, then COCOS_PRECISION=fp32 (which only a GPU tensor reaches: the CPU refusal
    comes before it)"""
    from cocosnet_amd import _lib, ops
    q, k = torch.randn(2, 256, 36), torch.randn(2, 256, 8)
    ql_, kl_ = torch.zeros(2, 36, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.int32)
    for bad in (ql_.float(), ql_.to(torch.int16), ql_.bool(), None, [0] * 36):
        with pytest.raises(TypeError, match="q_label"):
            ops.corr_topk_labelled(q, k, bad, kl_, 100.0, 2)
    with pytest.raises(TypeError, match="k_label"):
        ops.corr_topk_labelled(q, k, ql_, kl_.double(), 100.0, 2)
    for bad in (ql_[:1], ql_[:, :35], ql_.reshape(2, 6, 6)):
        with pytest.raises(ValueError, match="q_label"):
            ops.corr_topk_labelled(q, k, bad, kl_, 100.0, 2)
    with pytest.raises(ValueError, match="k_label"):
        ops.corr_topk_labelled(q, k, ql_, kl_[:1], 100.0, 2)
    for bad in (0, 9, -1, 2.5, True):
        with pytest.raises(ValueError, match="k="):
            ops.corr_topk_labelled(q, k, ql_, kl_, 100.0, bad)
    with pytest.raises(ValueError):
        ops.corr_topk_labelled(q[0], k, ql_, kl_, 100.0, 2)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.corr_topk_labelled(q, k, ql_, kl_, 100.0, 2)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(TypeError, match="q_label"):                      # still the first refusal
        ops.corr_topk_labelled(q, k, ql_.float(), kl_, 100.0, 2)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):     # and the device before the flavour
        ops.corr_topk_labelled(q, k, ql_, kl_, 100.0, 2)


def _theta_phi():
    g = torch.Generator().manual_seed(5)
    return torch.randn(1, 256, 2, 2, generator=g), torch.randn(1, 256, 2, 2, generator=g)


def _onehot(g, n, nc, size):
    return torch.zeros(n, nc, size, size).scatter_(1, torch.randint(0, nc, (n, 1, size, size), generator=g), 1.0)


#: what makes a flag set leave the fused match_kernel-1 route
OFF_ROUTE = [dict(match_kernel=3), dict(PONO_C=False)]
PAIR = (torch.zeros(1, 2, 2, dtype=torch.int64), torch.zeros(1, 2, 2, dtype=torch.int32))


def test_correspondence_match_checks_restrict(hip_lib, monkeypatch):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match
    theta, phi = _theta_phi()
    base = dict(match_kernel=1, PONO_C=True, down=4)
    cfg = HotPathConfig(**base)
    g = torch.Generator().manual_seed(1)
    seg, ref_seg = _onehot(g, 1, 5, 8), _onehot(g, 1, 5, 8)
    for bad in ("labels", "", 1, True, (PAIR[0],), PAIR + PAIR[:1], (PAIR[0], None), [1, 2]):
        with pytest.raises(ValueError, match="restrict"):
            correspondence_match(theta, phi, cfg, restrict=bad, seg_map=seg, ref_seg_map=ref_seg)
    with pytest.raises(TypeError, match="restrict"):
        correspondence_match(theta, phi, cfg, restrict=(PAIR[0].float(), PAIR[1]))
    for restrict in ("label", PAIR):
        kw = dict(restrict=restrict, seg_map=seg, ref_seg_map=ref_seg)
        for flags in OFF_ROUTE:
            with pytest.raises(ValueError, match="restrict"):
                correspondence_match(theta, phi, HotPathConfig(**dict(base, **flags)), **kw)
        with pytest.raises(ValueError, match="restrict.*prepared exemplar"):
            correspondence_match(theta, None, cfg, exemplar=object(), **kw)
        with pytest.raises(ValueError, match="restrict.*refine"):
            correspondence_match(theta, phi, cfg, refine=1, **kw)
        with pytest.raises(ValueError, match="restrict"):
            correspondence_match(theta[:, :128], phi[:, :128], cfg, **kw)
        monkeypatch.setattr(ops, "MATCH_FUSED", False)
        with pytest.raises(ValueError, match="MATCH_FUSED.*restrict"):
            correspondence_match(theta, phi, cfg, **kw)
        monkeypatch.setattr(ops, "MATCH_FUSED", True)
        monkeypatch.setattr(ops, "PRECISION", "fp32")
        with pytest.raises(ValueError, match="COCOS_PRECISION=fp32.*restrict"):
            correspondence_match(theta, phi, cfg, **kw)
        monkeypatch.setattr(ops, "PRECISION", "f16x3")
        # in scope: the tensors themselves are refused
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            correspondence_match(theta, phi, cfg, **kw)
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            correspondence_match(theta, phi, cfg, direction="cols", topk=2, **kw)
    # label maps / label tensors that do not fit the grids: ValueError before the device is looked at
    with pytest.raises(ValueError, match="restrict.*seg_map"):
        correspondence_match(theta, phi, cfg, restrict="label")
    with pytest.raises(ValueError, match="restrict.*ref_seg_map"):
        correspondence_match(theta, phi, cfg, restrict="label", seg_map=seg, ref_seg_map=ref_seg[:, :, :4])
    with pytest.raises(ValueError, match="restrict.*classes"):
        correspondence_match(theta, phi, cfg, restrict="label", seg_map=seg, ref_seg_map=ref_seg[:, :4])
    with pytest.raises(ValueError, match="restrict.*do not fit"):
        correspondence_match(theta, phi, cfg, restrict=(PAIR[0].reshape(1, 4), PAIR[1]))
    # restrict = None: today's refusals, unchanged, on every route
    for flags in [dict()] + OFF_ROUTE:
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            correspondence_match(theta, phi, HotPathConfig(**dict(base, **flags)), restrict=None)
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            correspondence_match(theta, phi, HotPathConfig(**dict(base, **flags)))


def test_correspondence_sparse_checks_restrict(hip_lib, monkeypatch):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse
    theta, phi = _theta_phi()
    base = dict(match_kernel=1, PONO_C=True, down=4)
    cfg = HotPathConfig(**base)
    g = torch.Generator().manual_seed(2)
    ref_img, seg, ref_seg = torch.rand(1, 3, 8, 8, generator=g), _onehot(g, 1, 5, 8), _onehot(g, 1, 5, 8)
    run = lambda c=cfg, th=theta, ph=phi, **kw: correspondence_sparse(th, ph, ref_img, seg, ref_seg, c, 0.01, 2, **kw)
    with pytest.raises(ValueError, match="restrict"):
        run(restrict="segments")
    with pytest.raises(TypeError, match="restrict"):
        run(restrict=(PAIR[0], PAIR[1].float()))
    for restrict in ("label", PAIR):
        for flags in OFF_ROUTE:
            with pytest.raises(ValueError, match="restrict"):
                run(HotPathConfig(**dict(base, **flags)), restrict=restrict)
        with pytest.raises(ValueError, match="restrict.*search='patchmatch'"):
            run(restrict=restrict, search="patchmatch")
        with pytest.raises(ValueError, match="restrict.*prepared exemplar"):
            run(restrict=restrict, exemplar=object())
        monkeypatch.setattr(ops, "PRECISION", "fp32")
        with pytest.raises(ValueError, match="COCOS_PRECISION=fp32.*restrict"):
            run(restrict=restrict)
        monkeypatch.setattr(ops, "PRECISION", "f16x3")
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            run(restrict=restrict)
    with pytest.raises(ValueError, match="restrict.*do not fit"):
        run(restrict=(PAIR[0], PAIR[1].reshape(1, 4)))
    # restrict = None: the pinned refusals in their own words, and the CPU refusal
    with pytest.raises(ValueError, match="match_kernel 3 is out of scope \\(the sparse warp"):
        run(HotPathConfig(**dict(base, match_kernel=3)))
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        run()
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        run(restrict=None)


def test_module_refuses_before_the_network_runs(hip_lib, monkeypatch):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd import correspondence as cc
    g = torch.Generator().manual_seed(3)
    ref_img, seg, ref_seg = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1, _onehot(g, 1, 7, 64), _onehot(g, 1, 7, 64)
    pair = (torch.zeros(1, 16, 16, dtype=torch.int64), torch.zeros(1, 16, 16, dtype=torch.int64))

    def net_for(block=True, **flags):
        opt = cc.ade20k_options(**dict(dict(crop_size=64, semantic_nc=7, match_kernel=1), **flags))
        torch.manual_seed(0)
        net = cc.NoVGGCorrespondence(opt).eval()
        if block:
            monkeypatch.setattr(net, "project", lambda *a, **k: pytest.fail("project() ran for a refused restriction"))
            monkeypatch.setattr(net, "_check_exemplar", lambda *a, **k: pytest.fail("the exemplar was looked at for a refused restriction"))
        return net

    calls = [lambda n, **kw: n.match(ref_img, seg, ref_seg, **kw), lambda n, **kw: n.sparse_warp(ref_img, ref_img, seg, ref_seg, topk=2, **kw)]
    for call in calls:
        for restrict in ("label", pair):
            for flags in (dict(match_kernel=3), dict(PONO_C=False)):
                with pytest.raises(ValueError, match="restrict"):
                    call(net_for(**flags), restrict=restrict)
            net = net_for()
            monkeypatch.setattr(ops, "MATCH_FUSED", False)
            with pytest.raises(ValueError, match="MATCH_FUSED.*restrict"):
                call(net, restrict=restrict)
            monkeypatch.setattr(ops, "MATCH_FUSED", True)
            monkeypatch.setattr(ops, "PRECISION", "fp32")
            with pytest.raises(ValueError, match="COCOS_PRECISION=fp32.*restrict"):
                call(net, restrict=restrict)
            monkeypatch.setattr(ops, "PRECISION", "f16x3")
            monkeypatch.setattr(net, "inter_channels", 128)
            with pytest.raises(ValueError, match="restrict"):
                call(net, restrict=restrict)
        with pytest.raises(ValueError, match="restrict"):
            call(net_for(), restrict="class")
        with pytest.raises(TypeError, match="restrict"):
            call(net_for(), restrict=(pair[0].float(), pair[1]))
    net = net_for()
    with pytest.raises(ValueError, match="restrict.*refine"):
        net.match(ref_img, seg, ref_seg, restrict="label", refine=1)
    with pytest.raises(ValueError, match="restrict.*prepared exemplar"):
        net.match(None, seg, None, restrict="label", exemplar=object())
    with pytest.raises(ValueError, match="restrict.*search='patchmatch'"):
        net.sparse_warp(ref_img, ref_img, seg, ref_seg, restrict="label", search="patchmatch")
    # in scope, and restrict = None: the network runs (on the CPU) and the readout refuses the tensors, as before
    net = net_for(block=False)
    for kw in (dict(), dict(restrict=None), dict(restrict="label"), dict(restrict=pair)):
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            net.match(ref_img, seg, ref_seg, **kw)
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            net.sparse_warp(ref_img, ref_img, seg, ref_seg, topk=2, **kw)


def test_readouts_carry_restricted():
    from cocosnet_amd.hot_path import MatchReadout, TopkMatchReadout
    z = torch.zeros(1, 2, 3)
    assert MatchReadout(index=z.long(), prob=z, max_logit=z, lse=z).restricted is None
    assert TopkMatchReadout(index=z.long().unsqueeze(1), prob=z.unsqueeze(1), logit=z.unsqueeze(1), lse=z).restricted is None


# ---------------------------------------------------------------------------------------------------------------- cell labels
def test_cell_labels_majority_and_tie_rule():
    from cocosnet_amd.hot_path import cell_labels
    lab = torch.tensor([[[3, 3, 1, 2],       # cell (0,0): 3 x3, 1 x 0 ... see below
                         [3, 0, 2, 1],
                         [4, 4, 0, 0],
                         [2, 2, 0, 0]]])
    seg = torch.zeros(1, 5, 4, 4).scatter_(1, lab.unsqueeze(1), 1.0)
    # cells: {3,3,3,0} -> 3;  {1,2,2,1} -> a tie of 1 and 2 -> 1;  {4,4,2,2} -> a tie of 2 and 4 -> 2;  {0,0,0,0} -> 0
    want = torch.tensor([[[3, 1], [2, 0]]])
    assert torch.equal(cell_labels(seg, 2), want) and torch.equal(lc.cell_labels(seg, 2), want)
    assert cell_labels(seg, 2).dtype == torch.int64
    assert torch.equal(cell_labels(seg, 1), lab) and torch.equal(cell_labels(seg, 4), torch.tensor([[[0]]]))      # 0 x 5 beats 2 x 4, 3 x 3
    g = torch.Generator().manual_seed(7)
    for nc, size, down in ((5, 24, 4), (7, 32, 8), (3, 12, 3), (2, 16, 2)):
        seg = _onehot(g, 2, nc, size)
        assert torch.equal(cell_labels(seg, down), lc.cell_labels(seg, down)), (nc, size, down)
    for bad in (0, 3, 2.0, True):
        with pytest.raises(ValueError, match="down"):
            cell_labels(torch.zeros(1, 5, 4, 4), bad)
    with pytest.raises(ValueError):
        cell_labels(torch.zeros(5, 4, 4), 2)


# ---------------------------------------------------------------------------------------------------------------- the fallback rule
def _same_partition(eff, restricted, q_lab, want_eff, want_restricted):
    """restrict_fallback returns dense ids: restricted rows must carry one id per original label, the others -1"""
    assert torch.equal(restricted, want_restricted)
    assert bool((eff[~restricted] == -1).all()) and bool((eff[restricted] >= 0).all())
    assert torch.equal(want_eff[~want_restricted], torch.full_like(want_eff[~want_restricted], -1))
    pairs = set(zip(eff[restricted].tolist(), q_lab[restricted].tolist()))
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_fallback_rule_against_the_restatement(k):
    from cocosnet_amd.hot_path import restrict_fallback
    g = torch.Generator().manual_seed(10 + k)
    q_lab = torch.randint(-2, 9, (3, 40), generator=g)
    k_lab = torch.randint(-2, 7, (3, 24), generator=g)
    k_lab[0, :k] = 8                # exactly k keys of label 8 in sample 0,
    k_lab[1, :max(k - 1, 0)] = 8    # k - 1 in sample 1, none in sample 2
    q_lab[:, :4] = 8
    for ql_, kl_ in ((q_lab, k_lab), (q_lab.to(torch.int32), k_lab), (q_lab * 2 ** 33, k_lab * 2 ** 33)):
        q_eff, k_eff, restricted = restrict_fallback(ql_, kl_, k)
        want_eff, want_restricted = lc.fallback(ql_, kl_, k)
        assert q_eff.dtype == k_eff.dtype == torch.int32 and restricted.dtype == torch.bool
        _same_partition(q_eff, restricted, ql_, want_eff, want_restricted)
        assert bool(restricted[0, :4].all()) and not bool(restricted[1, :4].any()) and not bool(restricted[2, :4].any())
        # the effective labels allow exactly what the restatement's allow
        assert torch.equal(lc.allowed(q_eff, k_eff), lc.allowed(want_eff, kl_))
        # and every restricted row has at least k allowed keys: no short rows
        assert int(lc.allowed(q_eff, k_eff).sum(2).min()) >= min(k, 24)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_by_hand():
    L = torch.tensor([[[1.0, 3.0, 3.0, float("-inf")], [float("-inf")] * 4]], dtype=torch.float64)
    idx, val = lc.topk_by_value_then_index(L, 3)
    assert idx.tolist() == [[[1, 2, 0], [0, 1, 2]]] and val[0, 0].tolist() == [3.0, 3.0, 1.0] and bool(torch.isinf(val[0, 1]).all())
    lse = lc.logsumexp(L)
    assert abs(lse[0, 0].item() - torch.logsumexp(L[0, 0, :3], 0).item()) < 1e-15 and lse[0, 1].item() == float("-inf")
    a = lc.allowed(torch.tensor([[0, -1, 2, -3]]), torch.tensor([[0, 2, -1]]))
    assert a.tolist() == [[[True, False, False], [True, True, True], [False, True, False], [True, True, True]]]
    eff, r = lc.fallback(torch.tensor([[0, 0, 1, -1, 5]]), torch.tensor([[0, 0, 1, -1, -1]]), 2)
    assert eff.tolist() == [[0, 0, -1, -1, -1]] and r.tolist() == [[True, True, False, False, False]]
