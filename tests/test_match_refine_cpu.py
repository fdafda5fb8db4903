"""K44 (the sub-cell match refinement), the parts that need no GPU: the two entry points in header, binding table and library, their
argument checks (which return before any HIP call), the Python-side refusals of ops.match_refine / ops.gather_patches_subcell,
hot_path.correspondence_match(refine=...) and NoVGGCorrespondence.match(refine=...), and the numpy restatement the GPU tests judge the
kernels by (tests/match_refine_case.py) on cases computed by hand."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_refine_case as mc  # noqa: E402

REFINE, GATHER = "cocos_match_refine_f16x3", "cocos_gather_patches_subcell"
_P, _I, _F, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong


def test_header_table_and_library_carry_the_entry_points(hip_lib):
    from cocosnet_amd import _lib, build, ops
    for name in (REFINE, GATHER):
        assert _lib.PROTOTYPES.get(name, ("",))[0] == "int", f"{name} is not declared in cocos_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    assert "plane_pair.hip" in build.HIP_SOURCES
    assert ops.MATCH_REFINE_MAX_RADIUS == _lib.CONSTANTS["COCOS_MATCH_REFINE_MAX_RADIUS"] == 3
    assert list(_lib._SIGNATURES[REFINE][1]) == [_P] * 7 + [_I] * 7 + [_F] * 2 + [_P]
    assert list(_lib._SIGNATURES[GATHER][1]) == [_P] * 4 + [_I] * 7 + [_LL, _P]


def test_refine_argument_validation_needs_no_gpu(hip_lib):
    """null pointers, non-positive sizes, hk wk != Nk, a radius outside 1..3 (-1, each message names the argument); K != 256 (-2): all
    before any HIP call"""
    one, f = ctypes.c_void_p(16), ctypes.c_float
    err = hip_lib.cocos_last_error_string

    def call(p=(one,) * 7, B=1, K=256, Nq=35, Nk=18, hk=3, wk=6, radius=1, inv_t=100.0):
        return hip_lib.cocos_match_refine_f16x3(*p, B, K, Nq, Nk, hk, wk, radius, f(inv_t), f(16.0), None)

    for i in range(7):
        assert call(p=(one,) * i + (None,) + (one,) * (6 - i)) == -1 and b"null" in err()
    for bad, word in ((dict(B=0), b"B=0"), (dict(Nq=0), b"Nq=0"), (dict(Nk=-1), b"Nk=-1"), (dict(hk=0), b"hk=0"), (dict(wk=0), b"wk=0")):
        assert call(**bad) == -1 and word in err(), bad
    assert call(hk=3, wk=5) == -1 and b"hk=3" in err() and b"Nk=18" in err()
    assert call(hk=2 ** 16, wk=2 ** 16 + 1, Nk=2 ** 16) == -1 and b"Nk=" in err()      # hk wk wraps to Nk in 32 bits only
    for r in (0, 4, -1):
        assert call(radius=r) == -1 and b"radius=" in err()
    assert call(inv_t=0.0) == -1 and b"inv_temperature" in err()
    assert call(p=(ctypes.c_void_p(24),) + (one,) * 6) == -1 and b"aligned" in err()
    assert call(K=128) == -2 and b"K == 256" in err()
    assert call(B=2 ** 20, Nq=2 ** 12) == -2 and b"32-bit" in err()


def test_gather_argument_validation_needs_no_gpu(hip_lib):
    one = ctypes.c_void_p(16)
    err = hip_lib.cocos_last_error_string

    def call(p=(one,) * 4, B=1, C=3, fh=5, fw=7, hk=3, wk=6, down=2, stride=None):
        return hip_lib.cocos_gather_patches_subcell(*p, B, C, fh, fw, hk, wk, down, C * hk * down * wk * down if stride is None else stride, None)

    for i in range(4):
        assert call(p=(one,) * i + (None,) + (one,) * (3 - i)) == -1 and b"null" in err()
    for bad, word in ((dict(B=0), b"B=0"), (dict(C=0), b"C=0"), (dict(fh=0), b"fh=0"), (dict(fw=-2), b"fw=-2"), (dict(hk=0), b"hk=0"),
                      (dict(wk=0), b"wk=0"), (dict(down=0), b"down=0")):
        assert call(**bad) == -1 and word in err(), bad
    assert call(stride=7) == -1 and b"img_batch_stride" in err()
    assert call(hk=2 ** 22, down=4, stride=0) == -2 and b"2^24" in err()
    assert call(B=2 ** 15, C=2 ** 10, fh=2 ** 10, fw=2 ** 10, stride=0) == -2 and b"elements" in err()


def test_ops_refuse_on_the_host_and_bad_arguments(hip_lib):
    from cocosnet_amd import _lib, ops
    q, k = torch.randn(1, 256, 35), torch.randn(1, 256, 18)
    idx = torch.zeros(1, 35, dtype=torch.int64)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.match_refine(q, k, idx, (3, 6), 100.0, 1)
    for bad in (0, 4, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="radius"):
            ops.match_refine(q, k, idx, (3, 6), 100.0, bad)
    for bad in ((3, 5), (3,), (0, 18), (3.0, 6), None):
        with pytest.raises(ValueError, match="kgrid|key grid"):
            ops.match_refine(q, k, idx, bad, 100.0, 1)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="inv_t"):
            ops.match_refine(q, k, idx, (3, 6), bad, 1)
    with pytest.raises(ValueError, match="256 channels"):
        ops.match_refine(q[:, :128], k[:, :128], idx, (3, 6), 100.0, 1)
    with pytest.raises(ValueError):
        ops.match_refine(torch.randn(2, 256, 35), k, idx, (3, 6), 100.0, 1)

    img, off = torch.rand(1, 3, 6, 12), torch.zeros(1, 35, 2)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.gather_patches_subcell(img, idx, off, (5, 7), (3, 6), 2)
    with pytest.raises(TypeError, match="off"):
        ops.gather_patches_subcell(img, idx, off.double(), (5, 7), (3, 6), 2)
    for args in ((img, idx, off, (5, 7), (3, 6), 4), (img, idx, off, (5, 6), (3, 6), 2), (img, idx, off[:, :, :1], (5, 7), (3, 6), 2),
                 (img[0], idx, off, (5, 7), (3, 6), 2), (img.expand(3, -1, -1, -1), idx, off, (5, 7), (3, 6), 2),
                 (img, idx, off, (5, 7), (3, 6), 0), (img, idx, off, (5, 7), (0, 6), 2), (img, idx, off, 5, (3, 6), 2)):
        with pytest.raises(ValueError):
            ops.gather_patches_subcell(*args)


def _theta_phi():
    g = torch.Generator().manual_seed(5)
    return torch.randn(1, 256, 2, 2, generator=g), torch.randn(1, 256, 2, 2, generator=g)


#: what makes a flag set leave the fused match_kernel-1 route, and the word of the refusal that names it
OFF_ROUTE = [(dict(match_kernel=3), "match_kernel 3"), (dict(PONO_C=False), "PONO_C")]


def test_correspondence_match_checks_refine(hip_lib, monkeypatch):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match
    theta, phi = _theta_phi()
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    for bad in (-1, 4, 1.0, True, None, "1"):
        with pytest.raises(ValueError, match="refine"):
            correspondence_match(theta, phi, cfg, refine=bad)
    for bad in (0.0, -0.01, "0.01", True):
        for r in (0, 1):
            with pytest.raises(ValueError, match="refine_temperature"):
                correspondence_match(theta, phi, cfg, refine=r, refine_temperature=bad)
    with pytest.raises(ValueError, match="topk=2"):
        correspondence_match(theta, phi, cfg, refine=1, topk=2)
    with pytest.raises(ValueError, match="prepared exemplar"):
        correspondence_match(theta, None, cfg, refine=1, exemplar=object())
    for flags, word in OFF_ROUTE:
        other = HotPathConfig(**dict(dict(match_kernel=1, PONO_C=True, down=4), **flags))
        with pytest.raises(ValueError, match=word):
            correspondence_match(theta, phi, other, refine=1)
    with pytest.raises(ValueError, match="256 channels"):
        correspondence_match(theta[:, :128], phi[:, :128], cfg, refine=2)
    # in scope, and refine = 0 on every route: the tensors themselves are refused
    for r in (0, 1, 3):
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            correspondence_match(theta, phi, cfg, refine=r, refine_temperature=None if r != 3 else 0.02)
    for flags, _ in OFF_ROUTE:
        other = HotPathConfig(**dict(dict(match_kernel=1, PONO_C=True, down=4), **flags))
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            correspondence_match(theta, phi, other, refine=0)
    monkeypatch.setattr(ops, "MATCH_FUSED", False)
    with pytest.raises(ValueError, match="MATCH_FUSED"):
        correspondence_match(theta, phi, cfg, refine=1)
    monkeypatch.setattr(ops, "MATCH_FUSED", True)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="COCOS_PRECISION=fp32"):
        correspondence_match(theta, phi, cfg, refine=1)


def test_readout_without_refinement_has_no_sub_cell_position():
    from cocosnet_amd.hot_path import MatchReadout
    z = torch.zeros(1, 2, 3)
    m = MatchReadout(index=torch.tensor([[[0, 4, 5], [1, 2, 3]]]), prob=z, max_logit=z, lse=z, grid=(2, 3))
    assert m.offset is None and m.window_prob is None
    with pytest.raises(ValueError, match="offset"):
        m.xy_sub()
    m.offset = torch.full((1, 2, 2, 3), 0.25)
    assert m.xy_sub().dtype == torch.float32 and torch.equal(m.xy_sub(), m.xy().float() + 0.25)


def test_module_refuses_before_the_network_runs(hip_lib, monkeypatch):
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd import ops
    g = torch.Generator().manual_seed(3)
    onehot = lambda: torch.zeros(1, 7, 64, 64).scatter_(1, torch.randint(0, 7, (1, 1, 64, 64), generator=g), 1.0)
    ref_img, seg, ref_seg = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1, onehot(), onehot()

    def net_for(**flags):
        opt = cc.ade20k_options(**dict(dict(crop_size=64, semantic_nc=7, match_kernel=1), **flags))
        torch.manual_seed(0)
        net = cc.NoVGGCorrespondence(opt).eval()
        monkeypatch.setattr(net, "project", lambda *a, **k: pytest.fail("project() ran for a refused refinement"))
        monkeypatch.setattr(net, "_check_exemplar", lambda *a, **k: pytest.fail("the exemplar was looked at for a refused refinement"))
        return net

    for flags, word in OFF_ROUTE:
        with pytest.raises(ValueError, match=word):
            net_for(**flags).match(ref_img, seg, ref_seg, refine=1)
    net = net_for()
    for bad in (-1, 4, 2.0, True):
        with pytest.raises(ValueError, match="refine"):
            net.match(ref_img, seg, ref_seg, refine=bad)
    with pytest.raises(ValueError, match="refine_temperature"):
        net.match(ref_img, seg, ref_seg, refine=1, refine_temperature=0.0)
    with pytest.raises(ValueError, match="topk=4"):
        net.match(ref_img, seg, ref_seg, refine=1, topk=4)
    with pytest.raises(ValueError, match="prepared exemplar"):
        net.match(None, seg, None, refine=1, exemplar=object())
    monkeypatch.setattr(ops, "MATCH_FUSED", False)
    with pytest.raises(ValueError, match="MATCH_FUSED"):
        net.match(ref_img, seg, ref_seg, refine=1)
    monkeypatch.setattr(ops, "MATCH_FUSED", True)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="COCOS_PRECISION=fp32"):
        net.match(ref_img, seg, ref_seg, refine=1)
    monkeypatch.setattr(net, "inter_channels", 128)
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    with pytest.raises(ValueError, match="256 channels"):
        net.match(ref_img, seg, ref_seg, refine=1)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_window_membership_by_hand():
    assert mc.window(0, (1, 1), 3) == [(0, 0, 0)]
    assert mc.window(0, (3, 6), 1) == [(0, 0, 0), (1, 1, 0), (6, 0, 1), (7, 1, 1)]                     # a corner centre at r = 1: 4 keys
    assert mc.window(17, (3, 6), 1) == [(10, -1, -1), (11, 0, -1), (16, -1, 0), (17, 0, 0)]
    assert mc.window(99, (3, 6), 1) == mc.window(17, (3, 6), 1) and mc.window(-5, (3, 6), 1) == mc.window(0, (3, 6), 1)      # clamped
    assert [k for k, _, _ in mc.window(3, (3, 6), 1)] == [2, 3, 4, 8, 9, 10]                           # an edge: 6 keys
    assert len(mc.window(8, (3, 6), 1)) == 9 and len(mc.window(8, (3, 6), 2)) == 15 and len(mc.window(8, (3, 6), 3)) == 18
    full = mc.window(27, (8, 8), 3)
    assert len(full) == 49 and full[0] == (0, -3, -3) and full[1] == (1, -2, -3) and full[7] == (8, -3, -2) and full[24] == (27, 0, 0)
    assert all(0 <= k < 18 for j in range(-2, 21) for r in (1, 2, 3) for k, _, _ in mc.window(j, (3, 6), r))


def test_softargmax_by_hand():
    ox, oy, lse = mc.softargmax([3.5], [0], [0])
    assert (ox, oy, lse) == (0.0, 0.0, 3.5)                                                            # one key: offset 0, lse_win = s
    keys, dx, dy = zip(*mc.window(0, (3, 6), 1))
    ox, oy, lse = mc.softargmax([0.0, math.log(3.0), 0.0, math.log(3.0)], dx, dy)                       # weights 1/8, 3/8, 1/8, 3/8
    assert abs(ox - 0.75) < 1e-15 and abs(oy - 0.5) < 1e-15 and abs(lse - math.log(8.0)) < 1e-15
    ox, oy, lse = mc.softargmax([1e4, 1e4 - 800.0], [0, 1], [0, 0])                                     # no overflow, a dead neighbour
    assert (ox, oy, lse) == (0.0, 0.0, 1e4)


def test_refine_restatement_on_a_one_by_one_key_grid():
    g = np.random.default_rng(0)
    qv, kv = g.standard_normal((2, 5, 256)) / 16, g.standard_normal((2, 1, 256)) / 16
    off, lse = mc.refine(qv, kv, np.array([[0, 1, -1, 7, 0]] * 2), (1, 1), 2, 100.0)
    assert not off.any()
    s = 100.0 * np.einsum("bic,bc->bi", qv, kv[:, 0])                       # lse_win = m + log(exp(0)) = s, up to fp64's dot-product order
    assert np.abs(lse - s).max() < 1e-13


def test_gather_restatement_by_hand():
    img = np.arange(2 * 4 * 6, dtype=np.float64).reshape(1, 2, 4, 6)                                    # a 2 x 3 key grid, down = 2
    idx = np.array([[4, 0]])                                                                            # a 1 x 2 content grid
    zero = mc.gather_subcell(img, idx, np.zeros((1, 2, 2)), (1, 2), (2, 3), 2)
    assert np.array_equal(zero[0, :, :, :2], img[0, :, 2:4, 2:4]) and np.array_equal(zero[0, :, :, 2:], img[0, :, 0:2, 0:2])
    # cell 0 moved by (+0.25, -0.5) cells = (+0.5, -1) pixels; cell 1 by (-1, +5): clamped to column 0 / the last row
    out = mc.gather_subcell(img, idx, np.array([[[0.25, -0.5], [-1.0, 5.0]]]), (1, 2), (2, 3), 2)
    assert np.array_equal(out[0, :, :, :2], (img[0, :, 1:3, 2:4] + img[0, :, 1:3, 3:5]) / 2)
    assert np.array_equal(out[0, :, :, 2:], np.broadcast_to(img[0, :, 3:4, 0:1], (2, 2, 2)))
    shared = mc.gather_subcell(img, np.array([[4, 0], [1, 1]]), np.zeros((2, 2, 2)), (1, 2), (2, 3), 2)  # one exemplar for two samples
    assert np.array_equal(shared[0], zero[0]) and np.array_equal(shared[1, :, :, :2], img[0, :, 0:2, 2:4])
