"""K43 (the PatchMatch candidate search), the parts that need no GPU: the entry point in header, binding table and library, its argument
checks (which return before any HIP call), the Python-side refusals of ops.patchmatch_step / patchmatch_topk,
hot_path.correspondence_sparse(search=...) and NoVGGCorrespondence.sparse_warp(search=...), and the numpy restatement the GPU tests
judge the kernel by (tests/patchmatch_case.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patchmatch_case as pc  # noqa: E402
from test_sparse_warp_cpu import OUT_OF_SCOPE, _hot_inputs  # noqa: E402

NAME = "cocos_patchmatch_step_f16x3"


def test_header_table_and_library_carry_the_entry_point(hip_lib):
    from cocosnet_amd import _lib, build, ops
    assert _lib.PROTOTYPES.get(NAME, ("",))[0] == "int", f"{NAME} is not declared in cocos_hip.h"
    assert NAME in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, NAME)
    assert "patchmatch_f16x3.hip" in build.HIP_SOURCES
    assert ops.PATCHMATCH_MAX_RADII == _lib.CONSTANTS["COCOS_PATCHMATCH_MAX_RADII"] >= 1
    _, argtypes = _lib._SIGNATURES[NAME]
    assert [t for t in argtypes] == [ctypes.c_void_p] * 7 + [ctypes.c_int] * 12 + [ctypes.c_float] * 2 + [ctypes.c_void_p]


def test_argument_validation_needs_no_gpu(hip_lib):
    """null planes / outputs, one buffer for both tables, misaligned planes (-1); K != 256, k outside 1..min(8, Nk), empty grids,
    stride < 1, radii outside 0..COCOS_PATCHMATCH_MAX_RADII (-2): all before any HIP call"""
    from cocosnet_amd import _lib
    one, two, f = ctypes.c_void_p(16), ctypes.c_void_p(4096), ctypes.c_float
    err = hip_lib.cocos_last_error_string
    top = _lib.CONSTANTS["COCOS_PATCHMATCH_MAX_RADII"]

    def call(p=None, B=1, K=256, hq=8, wq=8, hk=8, wk=8, k=4, stride=1, radii=3, radius0=4):
        p = (one, one, one, one, one, two, one) if p is None else p
        return hip_lib.cocos_patchmatch_step_f16x3(*p, B, K, hq, wq, hk, wk, k, stride, radii, radius0, 0, 0, f(100.0), f(16.0), None)

    for i in (0, 1, 2, 3, 5, 6):      # (idx_in, the fifth pointer, may be null: the random initialisation)
        assert call(p=(one,) * i + (None,) + (two,) * (6 - i)) == -1 and b"null" in err()
    assert call(p=(one,) * 7) == -1 and b"one buffer" in err()
    assert call(p=(ctypes.c_void_p(24),) + (one,) * 4 + (two, one)) == -1 and b"aligned" in err()
    assert call(K=128) == -2 and b"K == 256" in err()
    for k in (0, 9, -1):
        assert call(k=k) == -2 and b"k=" in err()
    assert call(hk=1, wk=3, k=4) == -2 and b"Nk=3" in err()
    for empty in (dict(B=0), dict(hq=0), dict(wq=0), dict(hk=0), dict(wk=-1)):
        assert call(**empty) == -2 and b"empty" in err()
    assert call(stride=0) == -2 and b"stride=0" in err()
    assert call(radii=top + 1) == -2 and b"radii" in err()
    assert call(radii=-1) == -2 and call(radius0=-1) == -2
    assert call(B=2 ** 20, hq=2 ** 6, wq=2 ** 6) == -2 and b"32-bit" in err()


def test_ops_refuse_on_the_host_and_bad_arguments(hip_lib):
    from cocosnet_amd import _lib, ops
    q, kk = torch.randn(1, 256, 24), torch.randn(1, 256, 12)
    grids = ((4, 6), (3, 4))
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.patchmatch_topk(q, kk, 100.0, 2, grids)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.patchmatch_step(q, kk, None, grids, 100.0, 2, 1, 0, 0, 0, 0)
    for bad_k in (0, 9, 13, 2.0, True):           # 13: more candidates than the 12 keys
        with pytest.raises(ValueError, match="k="):
            ops.patchmatch_topk(q, kk, 100.0, bad_k, grids)
    for bad in (((4, 6),), ((4, 5), (3, 4)), ((4, 6), (3, 5)), ((0, 6), (3, 4)), ((4.0, 6), (3, 4)), None):
        with pytest.raises(ValueError, match="grid"):
            ops.patchmatch_topk(q, kk, 100.0, 2, bad)
    for bad in ((0,), (1, -2), (1.5,), (), 3):
        with pytest.raises(ValueError, match="stride"):
            ops.patchmatch_topk(q, kk, 100.0, 2, grids, strides=bad)
    for bad in (-1, ops.PATCHMATCH_MAX_RADII + 1, (1, -1), 1.5):
        with pytest.raises(ValueError, match="radi"):
            ops.patchmatch_topk(q, kk, 100.0, 2, grids, radii=bad)
    with pytest.raises(ValueError, match="init"):
        ops.patchmatch_topk(q, kk, 100.0, 2, grids, init="coarse")
    with pytest.raises(ValueError, match="stride"):
        ops.patchmatch_step(q, kk, None, grids, 100.0, 2, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="256 channels"):
        ops.patchmatch_topk(q[:, :128], kk[:, :128], 100.0, 2, grids)


def test_search_argument_is_checked(hip_lib):
    from cocosnet_amd import _lib
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse
    theta, phi, ref_img, seg, ref_seg = _hot_inputs()
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    with pytest.raises(ValueError, match="search='bogus'"):
        correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, search="bogus")
    with pytest.raises(ValueError, match="search_opts"):
        correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, search="patchmatch", search_opts=dict(iterations=3))
    with pytest.raises(ValueError, match="search_opts"):
        correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, search="dense", search_opts=dict(seed=1))
    for search in ("dense", "patchmatch"):         # in scope: the tensors themselves are refused
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, topk=2, search=search)


@pytest.mark.parametrize("flags,word", OUT_OF_SCOPE, ids=[w + "-" + "-".join(f) for f, w in OUT_OF_SCOPE])
def test_patchmatch_keeps_the_sparse_route_refusals(hip_lib, flags, word):
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse
    theta, phi, ref_img, seg, ref_seg = _hot_inputs()
    cfg = HotPathConfig(**dict(dict(match_kernel=1, PONO_C=True, down=4), **flags))
    with pytest.raises(ValueError, match=word):
        correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, search="patchmatch")
    with pytest.raises(ValueError, match=word):      # the scope is judged before the selector's name
        correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, search="bogus")


def test_patchmatch_other_refusals(hip_lib, monkeypatch):
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse
    theta, phi, ref_img, seg, ref_seg = _hot_inputs()
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    pm = dict(search="patchmatch")
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="topk"):
            correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, topk=bad, **pm)
    with pytest.raises(ValueError, match="prepared exemplar"):
        correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, exemplar=object(), **pm)
    with pytest.raises(ValueError, match="256 channels"):
        correspondence_sparse(theta[:, :128], phi[:, :128], ref_img, seg, ref_seg, cfg, **pm)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="COCOS_PRECISION=fp32"):
        correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, **pm)


def test_module_refuses_before_the_network_runs(hip_lib, monkeypatch):
    from cocosnet_amd import correspondence as cc
    g = torch.Generator().manual_seed(3)
    onehot = lambda: torch.zeros(1, 7, 64, 64).scatter_(1, torch.randint(0, 7, (1, 1, 64, 64), generator=g), 1.0)
    ref_img, seg, ref_seg = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1, onehot(), onehot()
    for flags, word in OUT_OF_SCOPE:
        opt = cc.ade20k_options(**dict(dict(crop_size=64, semantic_nc=7, match_kernel=1), **flags))
        torch.manual_seed(0)
        net = cc.NoVGGCorrespondence(opt).eval()
        monkeypatch.setattr(net, "project", lambda *a, **k: pytest.fail("project() ran for an out-of-scope flag set"))
        with pytest.raises(ValueError, match=word):
            net.sparse_warp(ref_img, None, seg, ref_seg, search="patchmatch")
    opt = cc.ade20k_options(crop_size=64, semantic_nc=7, match_kernel=1)
    net = cc.NoVGGCorrespondence(opt).eval()
    monkeypatch.setattr(net, "project", lambda *a, **k: pytest.fail("project() ran for a selector that does not exist"))
    with pytest.raises(ValueError, match="search='bogus'"):
        net.sparse_warp(ref_img, None, seg, ref_seg, search="bogus")
    with pytest.raises(ValueError, match="search_opts"):
        net.sparse_warp(ref_img, None, seg, ref_seg, search="patchmatch", search_opts=dict(bogus=1))


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _fmix_int(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def _hash_int(seed, iteration, row, word):
    h = _fmix_int((seed & 0xFFFFFFFF) ^ 0x9E3779B9)
    for x in (iteration, row, word):
        h = _fmix_int(h ^ (x & 0xFFFFFFFF))
    return h


def test_vectorised_hash_is_the_written_one():
    """the numpy hash against the same mix on Python integers, and the finaliser against murmur3's published fixed points"""
    assert _fmix_int(0) == 0 and int(pc.fmix32(0)) == 0
    assert _fmix_int(1) == 0x514E28B7 == int(pc.fmix32(1))
    for seed, it, row, word in [(0, 0, 0, 0), (7, 3, 191, (2 << 8) | (1 << 1) | 1), (-5, 1, 2 ** 31 - 2, (7 << 8) | 0xFF), (2 ** 31 - 1, 9, 12345, 6)]:
        assert int(pc.pm_hash(seed, it, row, word)) == _hash_int(seed, it, row, word)
    rows = np.arange(50)
    assert [int(v) for v in pc.pm_hash(3, 2, rows, 5)] == [_hash_int(3, 2, int(r), 5) for r in rows]


@pytest.mark.parametrize("grids", [((8, 12), (8, 12)), ((8, 12), (6, 8)), ((5, 7), (3, 6)), ((3, 3), (1, 9))])
@pytest.mark.parametrize("seed", [0, 1, -7, 2 ** 31 - 1])
def test_restated_candidates_stay_inside_the_key_grid(grids, seed):
    (hq, wq), (hk, wk) = grids
    Nq, Nk, B = hq * wq, hk * wk, 2
    g = np.random.default_rng(abs(seed) + Nk)
    for k, stride, S, R in [(1, 1, 0, 0), (3, 2, 3, 4), (8, 1, 8, 1 << 20), (4, 40, 2, 1)]:
        tables = [None, g.integers(-3, Nk + 3, (B, Nq, k))]
        for it, table in enumerate(tables):
            cand = pc.pool(table, B, grids, k, stride, S, R, seed, it)
            assert cand.shape == (B, Nq, k * (5 + S)) and cand.min() >= -1 and cand.max() < Nk
            assert (cand[:, :, :k] >= 0).all() and (cand[:, :, 5 * k:] >= 0).all()      # own and search candidates always exist
            if table is None:                                                            # the initialisation is pairwise distinct
                own = np.sort(cand[:, :, :k], axis=2)
                assert (np.diff(own, axis=2) > 0).all()
                assert np.array_equal(cand[:, :, :k], pc.init_table(seed, it, B, Nq, Nk, k))
            else:
                assert np.array_equal(cand[:, :, :k], np.clip(table, 0, Nk - 1))


def test_restated_propagation_by_hand():
    """a 3 x 4 query grid on a 5 x 5 key grid, k = 1, stride 1: query (1, 1) with neighbours naming keys by hand"""
    grids = ((3, 4), (5, 5))
    table = np.zeros((1, 12, 1), dtype=np.int64)
    at = lambda y, x: y * 4 + x
    key = lambda y, x: y * 5 + x
    table[0, at(1, 1), 0] = key(2, 2)
    table[0, at(0, 1), 0] = key(0, 3)      # above: (0, 3) - (-1, 0) = (1, 3)
    table[0, at(2, 1), 0] = key(0, 0)      # below: (0, 0) - (1, 0) leaves the grid
    table[0, at(1, 0), 0] = key(4, 4)      # left:  (4, 4) - (0, -1) leaves the grid
    table[0, at(1, 2), 0] = key(3, 1)      # right: (3, 1) - (0, 1) = (3, 0)
    cand = pc.pool(table, 1, grids, 1, 1, 0, 0, 0, 0)
    assert cand[0, at(1, 1)].tolist() == [key(2, 2), key(1, 3), -1, -1, key(3, 0)]
    corner = cand[0, at(0, 0)]             # no neighbour above or to the left; below is (1, 0) -> (4, 4) - (1, 0) = (3, 4)
    assert corner[0] == 0 and corner[1] == -1 and corner[3] == -1 and corner[2] == key(3, 4)
