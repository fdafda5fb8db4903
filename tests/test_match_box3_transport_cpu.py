"""K54 (transport on the fused match_kernel-3 route), the parts that need no GPU: the entry point in header, binding table and library,
the argument checks of the C entry point (all of which answer before any HIP call), the refusal order of the ops, that
`transport_match(match_kernel=3)` still refuses as before, the case helper by hand on a tiny grid, and — on the arbiter alone — that
the inputs the GPU tests use leave fewer than 1 % of the ranks undecided."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transport_box3_case as bc  # noqa: E402
import transport_case as tc  # noqa: E402

ENTRY = "cocos_box3_topk_bias_f16x3"


def test_header_table_and_library_carry_the_entry_point(hip_lib):
    from cocosnet_amd import _lib, build
    assert _lib.PROTOTYPES.get(ENTRY, ("",))[0] == "int", f"{ENTRY} is not declared in cocos_hip.h"
    assert ENTRY in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, ENTRY)
    # derived from the header: cocos_box3_topk_f16x3's list with the bias behind the five operands
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib._SIGNATURES[ENTRY] == (I, [P] * 9 + [I] * 5 + [F, F] + [I, I] + [P])
    assert "box3_fused_f16x3.hip" in build.HIP_SOURCES      # the BIAS instantiations live in K37 / K41's template


def test_argument_validation_needs_no_gpu(hip_lib):
    """null pointers (the bias among them), a misaligned bias, k outside 1..8 or above Nk, unknown flag bits and unsupported grids are
    rejected before any HIP call, with check_box3_readout's codes and this entry point's name"""
    one, odd, f = ctypes.c_void_p(16), ctypes.c_void_p(20), ctypes.c_float
    m = getattr(hip_lib, ENTRY)
    ok = lambda **kw: dict(dict(t=one, mu=one, a=one, nu=one, b=one, bias=one, idx=one, val=one, lse=one, B=1, Nq=256, Nk=256, h=4, w=64,
                                scale=100.0, k=4, flags=0), **kw)
    call = lambda d: m(d["t"], d["mu"], d["a"], d["nu"], d["b"], d["bias"], d["idx"], d["val"], d["lse"], d["B"], d["Nq"], d["Nk"], d["h"],
                       d["w"], f(2304.0), f(d["scale"]), d["k"], d["flags"], None)
    err = hip_lib.cocos_last_error_string
    for name in ("t", "mu", "a", "nu", "b", "bias", "idx", "val", "lse"):
        assert call(ok(**{name: None})) == -1 and b"null" in err(), name
    assert call(ok(bias=odd)) == -1 and b"k_bias must be 16-byte aligned" in err()
    assert call(ok(bias=ctypes.c_void_p(24))) == -1 and b"aligned" in err()      # 8-byte aligned is not enough
    for name in ("t", "nu", "b"):
        assert call(ok(**{name: odd})) == -1 and b"aligned" in err(), name
    assert call(ok(k=0)) == -1 and b"k=0" in err()
    assert call(ok(k=9)) == -1 and b"k=9" in err()
    assert call(ok(k=-3)) == -1 and b"k=-3" in err()
    assert call(ok(k=0, h=16, w=16)) == -1 and b"k=0" in err()              # a bad k is refused whatever the shape
    assert call(ok(flags=2)) == -1 and b"flags" in err()                    # COCOS_BOX3_G_ACCUMULATE belongs to the backward
    assert call(ok(flags=4)) == -1 and b"flags" in err()
    assert call(ok(B=0)) == -1
    assert call(ok(scale=0.0)) == -1
    assert call(ok(h=16, w=16)) == -2 and b"64- or 128-wide" in err()       # a 16-wide grid
    assert call(ok(Nk=512)) == -2                                           # Nq != Nk
    assert call(ok(h=2, Nq=128, Nk=128)) == -2                              # not a multiple of 256 positions
    assert call(ok(h=3, w=64, Nq=256, Nk=256)) == -2                        # Nq != h * w
    assert call(ok(h=16, w=16, bias=odd)) == -2                             # the shape is refused before the bias's alignment is asked
    call(ok(k=9))
    assert err().startswith(b"box3_topk_bias_f16x3:")
    # the biased entry serves every k the unbiased one does: all eight BIAS instantiations have no scratch
    assert hip_lib.cocos_box3_topk_max_k() == 8


def test_ops_refuse_in_order(hip_lib):
    """argument errors first (bias dtype, bias shape, a bias that requires a gradient, k; iters, tau), then the device, then shapes"""
    from cocosnet_amd import _lib, ops
    N = 256
    t, s, bias = torch.zeros(N * N), torch.ones(1, N), torch.zeros(1, N)
    args = lambda kb, k=4, **kw: ((t, s, s, s, s, kb, 4, 64, 2304.0, 100.0, k), kw)
    run = lambda a: ops.box3_topk_biased(*a[0], **a[1])
    with pytest.raises(TypeError, match="k_bias must be a float32 tensor"):
        run(args(bias.double()))
    with pytest.raises(TypeError, match="k_bias must be a float32 tensor"):
        run(args(None))
    with pytest.raises(ValueError, match="k_bias is"):
        run(args(torch.zeros(1, N + 4)))
    with pytest.raises(ValueError, match="not differentiable"):
        run(args(bias.clone().requires_grad_(True)))
    for k in (0, 9, 2.0):
        with pytest.raises(ValueError, match="k="):
            run(args(bias, k))
    with pytest.raises(ValueError, match="k_bias is"):          # an argument error wins over the device
        run(args(torch.zeros(2, N), 9))
    for transposed in (False, True):
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            run(args(bias, transposed=transposed))
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):      # the device wins over a shape mismatch
        ops.box3_topk_biased(torch.zeros(7), s, s, s, s, bias, 4, 64, 2304.0, 100.0, 4)

    sink = lambda iters, tau=1.0: ops.box3_sinkhorn(t, s, s, s, s, 4, 64, 2304.0, 100.0, iters, tau)
    for iters in (0, -1, 1.5, True, ops.SINKHORN_MAX_ITERS + 1):
        with pytest.raises(ValueError, match="iters="):
            sink(iters)
    for tau in (0, 0.0, -0.5, 1.5, "1", True, float("nan")):
        with pytest.raises(ValueError, match="tau="):
            sink(3, tau)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        sink(3, 0.5)


def test_boxed_corr_methods_refuse_cpu_tensors(hip_lib):
    from cocosnet_amd import _lib
    from cocosnet_amd.hot_path import _BoxedCorr
    th = torch.zeros(1, 256, 4, 64)
    corr = _BoxedCorr(th, th, 100.0)
    with pytest.raises(ValueError, match="iters="):      # before the statistics or T are made
        corr.sinkhorn(0)
    with pytest.raises(ValueError, match="tau="):
        corr.sinkhorn(2, 2.0)
    assert corr._cache == {}
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        corr.sinkhorn(2)


def test_transport_on_the_match_kernel_1_route_still_refuses_match_kernel_3():
    """K54 adds to the box route's ops; hot_path.correspondence_transport and its message are as they were"""
    from cocosnet_amd.hot_path import _ROUTE, HotPathConfig, correspondence_transport
    th = torch.zeros(1, 256, 4, 64)
    with pytest.raises(ValueError, match="match_kernel 1 route"):
        correspondence_transport(th, th, HotPathConfig(match_kernel=3, PONO_C=True, down=4))
    assert "match_kernel 1 route" in _ROUTE["transport"]


# ---------------------------------------------------------------------------------------------------------------- the case helper
def test_case_helper_by_hand():
    """lse_bound, directed and excused_share on numbers worked out by hand"""
    bias = torch.tensor([[0.0, -7.5, bc.NEG_INF, 2.0]])
    assert bc.lse_bound(bias) == pytest.approx(bc.TOL * 107.5 / 100.0, rel=1e-12)
    assert bc.lse_bound(torch.full((1, 4), bc.NEG_INF)) == bc.TOL
    assert bc.lse_bound(bias, tol=1.0, inv_t=10.0) == pytest.approx(1.75)
    # one query, four keys: z = L + bias = [1, -6.5, -inf, 3] -> sorted 3, 1, -6.5, -inf; every gap is far above 2 * bound
    L = torch.tensor([[[1.0, 1.0, 5.0, 1.0]]], dtype=torch.float64)
    idx, val, lse, z = tc.biased_topk(L, bias, 2)
    assert idx.tolist() == [[[3, 0]]] and val.tolist() == [[[3.0, 1.0]]]
    assert lse.item() == pytest.approx(math.log(math.exp(3) + math.exp(1) + math.exp(-6.5)), rel=1e-14)
    assert bc.excused_share(L, bias, 2) == 0.0
    # two keys 1e-6 apart: both of the two ranks are excused, the third is not asked for
    L2 = torch.tensor([[[2.0, 2.0 + 1e-6, -4.0, -9.0]]], dtype=torch.float64)
    assert bc.excused_share(L2, torch.zeros(1, 4), 2) == 1.0
    assert bc.excused_share(L2, torch.zeros(1, 4), 1) == 1.0
    M = torch.arange(6.0).reshape(1, 2, 3)
    assert torch.equal(bc.directed(M, True), M.transpose(1, 2)) and bc.directed(M, False) is M


def test_inputs_are_the_box_readout_tests_inputs():
    """the helper's CPU inputs are tests/test_gpu_match_box3.py's `_case` formula: same seeds, same generator, same arithmetic"""
    h, w, B = 4, 64, 2
    theta, phi = bc.inputs(h, w, B)
    g = lambda seed: torch.randn(B, 256, h, w, generator=torch.Generator().manual_seed(seed))
    assert torch.equal(theta, g(464) + 0.1)
    assert torch.equal(phi, 0.3 * theta.roll((1, 7), (2, 3)) + g(465) - 0.05)
    L = bc._arbiter(theta, phi)
    assert L.dtype == torch.float64 and L.shape == (B, 256, 256) and float(L.abs().max()) <= bc.INV_T * (1 + 1e-12)
    for transposed in (False, True):
        bias = bc.bias_for(h, w, B, transposed)
        assert bias.shape == (B, 256) and 0.03 <= 1 - torch.isfinite(bias).double().mean().item() <= 0.20
    assert not torch.equal(bc.bias_for(h, w, B, False), bc.bias_for(h, w, B, True))


_L = {}


def _arbiter_of(h, w, B):
    if (h, w) not in _L:
        _L[(h, w)] = bc._arbiter(*bc.inputs(h, w, B))
    return _L[(h, w)]


@pytest.mark.parametrize("h,w,B", bc.GRIDS, ids=bc.GRID_IDS)
def test_inputs_of_the_gpu_tests_excuse_less_than_one_percent(h, w, B):
    """on the arbiter alone: with the GPU tests' inputs and bias, fewer than 1 % of the ranks are closer than 2 * lse_bound to a
    neighbour — the index comparison judges nearly every rank"""
    L = _arbiter_of(h, w, B)
    for transposed in (False, True):
        bias = bc.bias_for(h, w, B, transposed)
        for k in (1, 4):
            share = bc.excused_share(bc.directed(L, transposed), bias, k)
            print(f"[transport-box3] ({h},{w}) {'transposed' if transposed else 'rows'} k={k}: excused {share:.5f} at bound {bc.lse_bound(bias):.3e}")
            assert share <= bc.EXCUSED_MAX, (h, w, transposed, k, share)


def test_sinkhorn_on_the_arbiter_meets_the_column_marginal():
    """the iteration the GPU test compares against, on the box logits: after every balanced iteration the key masses are 1"""
    L = _arbiter_of(4, 64, 2)
    f, g, row_lse = tc.sinkhorn(L, 3, 1.0)
    match_mass, key_mass = tc.masses(L, f, g)
    assert float((key_mass - 1).abs().max()) < 1e-12
    assert torch.allclose(match_mass, torch.exp(f + row_lse + math.log(L.shape[1])), rtol=1e-12)


def test_planted_collapse_on_the_arbiter_alone():
    """the hub serves every interior row under the plain argmax; five balanced iterations leave no key with more than a handful"""
    theta, phi, hub = bc.planted()
    L = bc._arbiter(theta, phi)
    N = L.shape[2]
    share = bc.hub_share(L, hub)
    assert float(share.min()) >= bc.PLANT_MIN_SHARE, share
    f, g, _ = tc.sinkhorn(L, 5, 1.0)
    after = bc.loads(tc.biased_topk(L, g, 1)[0][..., 0], N)
    print(f"[transport-box3] planted: hub share {float(share.min()):.3f}, max load after 5 iterations {int(after.max())}")
    assert int(after.max()) <= bc.PLANT_MAX_LOAD and int(after[:, hub].max()) <= bc.PLANT_MAX_LOAD


# ---------------------------------------------------------------------------------------------------------------- hot path, module
def _cfg(**kw):
    from cocosnet_amd.hot_path import HotPathConfig
    return HotPathConfig(**dict(dict(match_kernel=3, PONO_C=True, down=4), **kw))


OFF_ROUTE = [dict(match_kernel=1), dict(match_kernel=2), dict(PONO_C=False), dict(warp_patch=True), dict(warp_bilinear=True),
             dict(warp_cycle_w=1.0), dict(two_cycle=True), dict(warp_mask_losstype="cycle")]


@pytest.mark.parametrize("flags", OFF_ROUTE, ids=[next(iter(f)) + "=" + str(next(iter(f.values()))) for f in OFF_ROUTE])
def test_every_off_route_flag_set_raises_naming_box_transport(flags):
    from cocosnet_amd.hot_path import _ROUTE, correspondence_transport_box3
    th = torch.zeros(1, 256, 4, 64)
    with pytest.raises(ValueError) as e:
        correspondence_transport_box3(th, th, _cfg(**flags))
    assert str(e.value).endswith(_ROUTE["transport_box3"]) and "match_kernel 3 route" in _ROUTE["transport_box3"]


def test_hot_path_refusal_order(monkeypatch):
    """arguments (topk, iters, tau), then the flag set, precision and the switch, channels — all before a tensor is looked at; then the
    device; then the shapes"""
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import correspondence_sparse_box3, correspondence_transport_box3
    th, bad = torch.zeros(1, 256, 4, 64), _cfg(match_kernel=1)
    with pytest.raises(ValueError, match="topk=9"):
        correspondence_transport_box3(th, th, bad, topk=9, iters=0)
    with pytest.raises(ValueError, match="iters=0"):
        correspondence_transport_box3(th, th, bad, iters=0, tau=2.0)
    with pytest.raises(ValueError, match="tau=2.0"):
        correspondence_transport_box3(th, th, bad, tau=2.0)
    with pytest.raises(ValueError, match="match_kernel 1 is out of scope"):
        correspondence_transport_box3(th, th, bad)               
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="COCOS_PRECISION=fp32"):
        correspondence_transport_box3(th, th, _cfg())
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    monkeypatch.setattr(ops, "MATCH_FUSED", False)
    with pytest.raises(ValueError, match="MATCH_FUSED"):
        correspondence_transport_box3(th, th, _cfg())
    monkeypatch.setattr(ops, "MATCH_FUSED", True)
    with pytest.raises(ValueError, match="needs 256 channels"):
        correspondence_transport_box3(torch.zeros(1, 64, 4, 64), torch.zeros(1, 64, 4, 64), _cfg())
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):      # the device before the shapes: a 16-wide grid on the CPU
        correspondence_transport_box3(torch.zeros(1, 256, 16, 16), torch.zeros(1, 256, 16, 16), _cfg())
    # the sparse warp: its own scope first, then the transport dict, all before a tensor is looked at
    img, seg = torch.zeros(1, 3, 16, 256), torch.zeros(1, 5, 16, 256)
    for transport, what in (({"iters": 3}, "transport="), ("yes", "transport=str"), ({"iters": 0, "tau": 1.0}, "iters=0"),
                            ({"iters": 3, "tau": 0.0}, "tau=0.0"), ({"iters": 3, "tau": 1.0, "x": 1}, "transport=")):
        with pytest.raises(ValueError, match=what):
            correspondence_sparse_box3(th, th, img, seg, seg, _cfg(), transport=transport)
    with pytest.raises(ValueError, match="topk=0"):
        correspondence_sparse_box3(th, th, img, seg, seg, _cfg(), topk=0, transport={"iters": 0, "tau": 1.0})
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        correspondence_sparse_box3(th, th, img, seg, seg, _cfg(), transport={"iters": 2, "tau": 1.0})


def test_module_refuses_before_the_network_runs(monkeypatch):
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd.hot_path import _ROUTE
    for options, over in (("ade20k_options", dict(match_kernel=1)), ("ade20k_options", dict(match_kernel=3, PONO_C=False))):
        net = cc.NoVGGCorrespondence(getattr(cc, options)(crop_size=64, semantic_nc=7, **over))
        monkeypatch.setattr(net, "project", lambda *a, **k: pytest.fail("the network ran"))
        with pytest.raises(ValueError) as e:
            net.transport_match_box3(None, None, None)
        assert str(e.value).endswith(_ROUTE["transport_box3"])
    net = cc.NoVGGCorrespondence(cc.ade20k_options(crop_size=64, semantic_nc=7, match_kernel=3))
    monkeypatch.setattr(net, "project", lambda *a, **k: pytest.fail("the network ran"))
    with pytest.raises(ValueError, match="iters="):
        net.transport_match_box3(None, None, None, iters=65)
    with pytest.raises(ValueError, match="topk="):
        net.transport_match_box3(None, None, None, topk=0)
    with pytest.raises(ValueError, match="ref_img and ref_seg_map are required"):
        net.transport_match_box3(None, None, None)
    with pytest.raises(ValueError, match="transport="):
        net.sparse_warp_box3(None, None, None, None, transport={"tau": 1.0})
    with pytest.raises(ValueError, match="tau="):
        net.sparse_warp_box3(None, None, None, None, transport={"iters": 2, "tau": 3})


def test_pair_entry_and_op_refusals(hip_lib):
    """the biased pair forward: declared, exported, a null bias refused before any HIP call; the op's bias checks"""
    from cocosnet_amd import _lib, ops
    name = "cocos_box3_sparse_softmax_warp_bias_fwd"
    assert _lib.PROTOTYPES.get(name, ("",))[0] == "int" and name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    one, f = ctypes.c_void_p(16), ctypes.c_float
    m = getattr(hip_lib, name)
    ptrs = [one] * 12
    for i in range(12):
        assert m(*[None if j == i else one for j in range(12)], 1, 256, 2, 2, 2, 2, 3, 2, f(100.0), None) == -1, i
        assert b"null" in hip_lib.cocos_last_error_string()
    assert m(*ptrs, 1, 256, 2, 2, 2, 2, 3, 9, f(100.0), None) == -1 and b"k=9" in hip_lib.cocos_last_error_string()
    assert m(*ptrs, 1, 128, 2, 2, 2, 2, 3, 2, f(100.0), None) == -2
    th, v, s, idx = torch.zeros(1, 256, 2, 2), torch.zeros(1, 3, 4), torch.ones(1, 4), torch.zeros(1, 4, 2, dtype=torch.int64)
    call = lambda kb: ops.box3_sparse_softmax_warp(th, th, s, s, s, s, v, idx, 100.0, k_bias=kb)
    with pytest.raises(TypeError, match="k_bias must be a float32 tensor"):
        call(torch.zeros(1, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="k_bias is"):
        call(torch.zeros(1, 5))
    with pytest.raises(ValueError, match="not differentiable"):
        call(torch.zeros(1, 4, requires_grad=True))
