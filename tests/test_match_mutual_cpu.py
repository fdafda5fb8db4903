"""K48 (mutual match), the parts that need no GPU: the three entry points in header, binding table and library, their argument checks
(which return before any HIP call), the workspace arithmetic, the Python-side refusals of ops.corr_match_mutual / ops.match_round_trip,
hot_path.correspondence_mutual and NoVGGCorrespondence.mutual_match in the family's order, the route predicate with the library call
monkeypatched, and the restatement (tests/match_mutual_case.py) on cases worked out by hand."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_mutual_case as mc  # noqa: E402

SWEEP, WS, TRIP = "cocos_corr_match_mutual_f16x3", "cocos_corr_match_mutual_workspace_bytes", "cocos_match_round_trip"
_P, _I, _F, _Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t


def test_header_table_and_library_carry_the_entry_points(hip_lib):
    from cocosnet_amd import _lib, build
    for name, ret in ((SWEEP, "int"), (WS, "size_t"), (TRIP, "int")):
        assert _lib.PROTOTYPES.get(name, ("",))[0] == ret, f"{name} is not declared in cocos_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    assert "corr_match_mutual_f16x3.hip" in build.HIP_SOURCES and "corr_topk_f16x3.hip" in build.HIP_SOURCES
    assert os.path.exists(os.path.join(build.CSRC_DIR, "corr_match_mutual_f16x3.hip"))
    assert list(_lib._SIGNATURES[SWEEP][1]) == [_P] * 11 + [_Z] + [_I] * 4 + [_F] * 2 + [_P]
    assert list(_lib._SIGNATURES[WS][1]) == [_I] * 3 and _lib._SIGNATURES[WS][0] is _Z
    assert list(_lib._SIGNATURES[TRIP][1]) == [_P] * 6 + [_I] * 5 + [_P]


def test_workspace_is_host_arithmetic(hip_lib):
    ws = hip_lib.cocos_corr_match_mutual_workspace_bytes
    assert ws(1, 4, 4) == 12 * 4                       # one query block: (m, l, index) per key
    assert ws(3, 128, 68) == 12 * 3 * 1 * 68
    assert ws(3, 132, 68) == 12 * 3 * 2 * 68           # a second block for the last 4 queries
    assert ws(8, 4096, 4096) == 12 * 8 * 32 * 4096     # O(B ceil(Nq / 128) Nk): 12.6 MB where the matrix would be 537 MB
    for bad in ((0, 64, 64), (1, 0, 64), (1, 64, 0), (-1, 64, 64), (1, -4, 64), (1, 64, -4)):
        assert ws(*bad) == 0, bad


def test_argument_validation_needs_no_gpu(hip_lib):
    """null and misaligned pointers, zero dims, a short workspace (-1); K = 128, Nq = 66, Nk = 66 (-2): all before any HIP call (no GPU
    is present where this runs)"""
    one, f = ctypes.c_void_p(16), ctypes.c_float
    err = hip_lib.cocos_last_error_string
    names = ["qh", "ql", "kh", "kl", "row_idx", "row_max", "row_lse", "col_idx", "col_max", "col_lse", "ws"]

    def call(B=1, K=256, Nq=64, Nk=64, nbytes=None, **ptr):
        p = [ptr.get(n, one) for n in names]
        nbytes = hip_lib.cocos_corr_match_mutual_workspace_bytes(1, 64, 64) if nbytes is None else nbytes
        return hip_lib.cocos_corr_match_mutual_f16x3(*p, nbytes, B, K, Nq, Nk, f(100.0), f(16.0), None)

    for n in names:
        assert call(**{n: None}) == -1 and b"null" in err(), n
    for n in names[:4]:
        assert call(**{n: ctypes.c_void_p(24)}) == -1 and b"aligned" in err(), n
    for n in names[4:]:
        assert call(**{n: ctypes.c_void_p(18)}) == -1 and b"aligned" in err(), n
    assert call(K=128) == -2 and b"K == 256" in err()
    assert call(Nq=66) == -2 and b"Nq=66" in err()
    assert call(Nk=66) == -2 and b"Nk=66" in err()
    for zero in (dict(B=0), dict(Nq=0), dict(Nk=0)):
        assert call(**zero) == -1 and b"bad dims" in err(), zero
    assert call(nbytes=0) == -1 and b"workspace" in err()
    assert call(nbytes=12 * 64 - 1) == -1 and b"workspace" in err()

    def trip(B=2, grids=(2, 3, 3, 2), **ptr):
        p = [ptr.get(n, one) for n in ("row_idx", "col_idx", "q_back", "q_dist", "k_back", "k_dist")]
        return hip_lib.cocos_match_round_trip(*p, B, *grids, None)

    for n in ("row_idx", "col_idx", "q_back", "q_dist", "k_back", "k_dist"):
        assert trip(**{n: None}) == -1 and b"null" in err(), n
        assert trip(**{n: ctypes.c_void_p(18)}) == -1 and b"aligned" in err(), n
    for bad in (dict(B=0), dict(grids=(0, 3, 3, 2)), dict(grids=(2, 3, 3, 0)), dict(grids=(2, -3, 3, 2))):
        assert trip(**bad) == -1 and b"bad dims" in err(), bad


def test_ops_refuse_in_the_family_order(hip_lib, monkeypatch):
    """TypeError / ValueError first, then the CPU tensors ("no CPU fallback"), then COCOS_PRECISION (which only a GPU tensor reaches)"""
    from cocosnet_amd import _lib, ops
    q, k = torch.randn(2, 256, 36), torch.randn(2, 256, 8)
    with pytest.raises(TypeError):
        ops.corr_match_mutual(None, k, 100.0)
    for bad_q, bad_k in ((q[0], k), (q, k[:1]), (q[:, :128], k)):
        with pytest.raises(ValueError, match="corr_match_mutual"):
            ops.corr_match_mutual(bad_q, bad_k, 100.0)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.corr_match_mutual(q, k, 100.0)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="corr_match_mutual"):            # still the first refusal
        ops.corr_match_mutual(q[0], k, 100.0)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):      # and the device before the flavour
        ops.corr_match_mutual(q, k, 100.0)
    monkeypatch.setattr(ops, "PRECISION", "f16x3")

    r, c = torch.zeros(2, 6, dtype=torch.int64), torch.zeros(2, 6, dtype=torch.int32)
    for bad in (r.float(), r.bool(), None, [0] * 6):
        with pytest.raises(TypeError, match="row_idx"):
            ops.match_round_trip(bad, c, (2, 3), (3, 2))
    with pytest.raises(TypeError, match="col_idx"):
        ops.match_round_trip(r, c.double(), (2, 3), (3, 2))
    for bad in ((2, 3, 1), 6, (0, 6), (2.0, 3), (True, 6), None):
        with pytest.raises(ValueError, match="qgrid"):
            ops.match_round_trip(r, c, bad, (3, 2))
    with pytest.raises(ValueError, match="kgrid"):
        ops.match_round_trip(r, c, (2, 3), (3, -2))
    for bad_r, bad_c in ((r[:1], c), (r[:, :5], c), (r, c.reshape(2, 3, 2)), (r, c[:, :4])):
        with pytest.raises(ValueError, match="do not fit"):
            ops.match_round_trip(bad_r, bad_c, (2, 3), (3, 2))
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.match_round_trip(r, c, (2, 3), (3, 2))
    assert ops.MATCH_MUTUAL_FUSED in (True, False)


def test_fused_shape_predicate(hip_lib):
    from cocosnet_amd import ops
    assert ops.corr_match_mutual_ok(3, 64, 64) and ops.corr_match_mutual_ok(1, 4, 260) and ops.corr_match_mutual_ok(8, 4096, 4096)
    for bad in ((3, 66, 64), (3, 64, 66), (0, 64, 64), (3, 0, 64), (3, 64, 0), (3, 2, 64)):
        assert not ops.corr_match_mutual_ok(*bad), bad


BAD_MAX_DIST = (-1, 1.0, True, None, "1", [0])


def _theta_phi():
    g = torch.Generator().manual_seed(5)
    return torch.randn(1, 256, 2, 2, generator=g), torch.randn(1, 256, 2, 2, generator=g)


def test_correspondence_mutual_refusals(hip_lib, monkeypatch):
    """a bad max_dist before anything else (theta may be anything), then correspondence_match's own refusals, CPU tensors last"""
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_mutual
    theta, phi = _theta_phi()
    base = dict(match_kernel=1, PONO_C=True, down=4)
    cfg = HotPathConfig(**base)
    for bad in BAD_MAX_DIST:
        with pytest.raises(ValueError, match="max_dist"):
            correspondence_mutual(None, None, cfg, max_dist=bad)
    with pytest.raises(ValueError, match="phi_raw or a prepared exemplar"):
        correspondence_mutual(theta, None, cfg)
    with pytest.raises(ValueError, match="phi_raw or a prepared exemplar"):
        correspondence_mutual(theta, phi, cfg, exemplar=object())
    for flags in (dict(), dict(match_kernel=3), dict(PONO_C=False)):
        for fused in (True, False):
            monkeypatch.setattr(ops, "MATCH_MUTUAL_FUSED", fused)
            with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
                correspondence_mutual(theta, phi, HotPathConfig(**dict(base, **flags)), max_dist=1)


def test_route_predicate(hip_lib, monkeypatch):
    """mutual_fused_route with the library's shape answer monkeypatched: every condition of the issue switches the route off alone"""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, mutual_fused_route
    base = dict(match_kernel=1, PONO_C=True, down=4)
    cfg = HotPathConfig(**base)
    asked = []
    monkeypatch.setattr(ops, "corr_match_mutual_ok", lambda B, Nq, Nk: asked.append((B, Nq, Nk)) or True)
    assert mutual_fused_route(cfg, 2, 256, 64, 36, False) and asked == [(2, 64, 36)]
    assert not mutual_fused_route(cfg, 2, 256, 64, 36, True)                                  # a prepared exemplar
    assert not mutual_fused_route(HotPathConfig(**dict(base, match_kernel=3)), 2, 256, 64, 36, False)
    assert not mutual_fused_route(HotPathConfig(**dict(base, PONO_C=False)), 2, 256, 64, 36, False)
    assert not mutual_fused_route(cfg, 2, 128, 64, 36, False)                                 # 128 channels
    assert not mutual_fused_route(cfg, 2, 256, 66, 36, False)                                 # ops.corr_split_ok
    for name, off in (("MATCH_FUSED", False), ("MATCH_MUTUAL_FUSED", False), ("PRECISION", "fp32")):
        monkeypatch.setattr(ops, name, off)
        assert not mutual_fused_route(cfg, 2, 256, 64, 36, False), name
        monkeypatch.undo()
        monkeypatch.setattr(ops, "corr_match_mutual_ok", lambda B, Nq, Nk: True)
    monkeypatch.setattr(ops, "corr_match_mutual_ok", lambda B, Nq, Nk: False)
    assert not mutual_fused_route(cfg, 2, 256, 64, 36, False)


def test_module_refuses_before_the_network_runs(hip_lib, monkeypatch):
    from cocosnet_amd import _lib
    from cocosnet_amd import correspondence as cc
    g = torch.Generator().manual_seed(3)
    onehot = lambda: torch.zeros(1, 7, 32, 32).scatter_(1, torch.randint(0, 7, (1, 1, 32, 32), generator=g), 1.0)
    ref_img, seg, ref_seg = torch.rand(1, 3, 32, 32, generator=g) * 2 - 1, onehot(), onehot()
    torch.manual_seed(0)
    net = cc.NoVGGCorrespondence(cc.ade20k_options(crop_size=32, semantic_nc=7, match_kernel=1)).eval()
    with monkeypatch.context() as m:
        m.setattr(net, "project", lambda *a, **k: pytest.fail("project() ran for a refused max_dist"))
        m.setattr(net, "_check_exemplar", lambda *a, **k: pytest.fail("the exemplar was looked at for a refused max_dist"))
        for bad in BAD_MAX_DIST:
            with pytest.raises(ValueError, match="max_dist"):
                net.mutual_match(ref_img, seg, ref_seg, max_dist=bad)
            with pytest.raises(ValueError, match="max_dist"):
                net.mutual_match(None, seg, None, exemplar=object(), max_dist=bad)
    with pytest.raises(ValueError, match="ref_img and ref_seg_map are required"):
        net.mutual_match(None, seg, ref_seg)
    with pytest.raises(ValueError, match="exemplar"):
        net.mutual_match(None, seg, None, exemplar=object())
    # in scope: the network runs (on the CPU) and the readout refuses the tensors
    for kw in (dict(), dict(max_dist=2, hard_warp=True)):
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            net.mutual_match(ref_img, seg, ref_seg, **kw)


# ---------------------------------------------------------------------------------------------------------------- the restatement
#: a 2 x 3 content grid (rows of L) against a 3 x 2 exemplar grid (columns of L)
L_HAND = torch.tensor([[[5., 1, 0, 0, 0, 0],      # 0 -> 0
                        [4., 1, 3, 0, 0, 0],      # 1 -> 0
                        [0., 2, 2, 0, 0, 1],      # 2 -> 1 (1 and 2 tie: the lower)
                        [0., 0, 0, 0, 0, 6],      # 3 -> 5
                        [0., 0, 0, 3, 3, 0],      # 4 -> 3 (3 and 4 tie)
                        [0., 0, 1, 0, 3, 0]]],    # 5 -> 4
                      dtype=torch.float64)          # columns: 0 <- 0, 1 <- 2, 2 <- 1, 3 <- 4, 4 <- 4 (4 and 5 tie), 5 <- 3


def test_restatement_by_hand():
    (ri, rm, rl), (ci, cm, cl) = mc.readout(L_HAND)
    assert ri.tolist() == [[0, 0, 1, 5, 3, 4]] and rm.tolist() == [[5, 4, 2, 6, 3, 3]]
    assert ci.tolist() == [[0, 2, 1, 4, 4, 3]] and cm.tolist() == [[5, 2, 3, 3, 3, 6]]
    import math
    assert abs(rl[0, 0].item() - math.log(math.exp(5) + math.exp(1) + 4)) < 1e-14
    assert abs(cl[0, 5].item() - math.log(math.exp(6) + math.exp(1) + 4)) < 1e-14
    q_back, q_dist, k_back, k_dist = mc.round_trip(ri, ci, (2, 3), (3, 2))
    assert q_back.tolist() == [[0, 0, 2, 3, 4, 4]]
    assert q_dist.tolist() == [[0, 1, 0, 0, 0, 1]]      # 1 = (1,0) comes back to (0,0); 5 = (2,1) comes back to 4 = (1,1)
    assert k_back.tolist() == [[0, 1, 0, 3, 3, 5]]
    assert k_dist.tolist() == [[0, 0, 1, 0, 1, 0]]      # 2 = (0,1) comes back to 0 = (0,0); 4 = (0,2) to 3 = (1,1): one cell diagonally
    # the same flat positions are two cells apart on either grid: 0 = (0,0), 5 = (2,1) at width 3 and (1,2) at width 2
    z, five = torch.tensor([[0]]), torch.tensor([[5]])
    assert mc.chebyshev(z, five, 3).item() == 2 and mc.chebyshev(z, five, 2).item() == 2 and mc.chebyshev(five, z, 6).item() == 5
    # out-of-range indices are clamped: 7 -> 5, -3 -> 0
    qb, qd, kb, kd = mc.round_trip(torch.tensor([[7, -3, 1, 5, 3, 4]]), torch.tensor([[0, 2, 1, 4, 4, 99]]), (2, 3), (3, 2))
    assert qb.tolist() == [[5, 0, 2, 5, 4, 4]] and qd.tolist() == [[2, 1, 0, 2, 0, 1]]
    assert kb.tolist() == [[5, 1, 0, 3, 3, 4]] and kd.tolist() == [[2, 0, 1, 0, 1, 1]]
    # lowest index among equal maxima, along either dimension
    m, i = mc.argmax_lowest(torch.tensor([[3., 7, 7, 7], [1, 1, 1, 1]]), 1)
    assert i.tolist() == [1, 0] and m.tolist() == [7, 1]
    m, i = mc.argmax_lowest(torch.tensor([[3., 7], [3, 7], [2, 7]]), 0)
    assert i.tolist() == [0, 0]
    q = torch.eye(3).unsqueeze(0)
    assert torch.equal(mc.logits(q, q, 100.0), 100.0 * torch.eye(3, dtype=torch.float64).unsqueeze(0))
