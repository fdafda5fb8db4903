"""K55 (label restriction on the fused match_kernel-3 route), the parts that need no GPU: the entry point in header, binding table and
library, the argument checks of the C entry point (all of which answer before any HIP call), the refusal order of the op, the hot
path and the module, and that `match(restrict=...)` under match_kernel 3 still refuses as before."""
import ctypes

import pytest
import torch

ENTRY = "cocos_box3_topk_labels_f16x3"


def test_header_table_and_library_carry_the_entry_point(hip_lib):
    from cocosnet_amd import _lib, build
    assert _lib.PROTOTYPES.get(ENTRY, ("",))[0] == "int", f"{ENTRY} is not declared in cocos_hip.h"
    assert ENTRY in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, ENTRY)
    # derived from the header: cocos_box3_topk_f16x3's list with the two label arrays behind the five operands
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib._SIGNATURES[ENTRY] == (I, [P] * 10 + [I] * 5 + [F, F] + [I, I] + [P])
    assert "box3_fused_f16x3.hip" in build.HIP_SOURCES      # the LABELS instantiations live in K37 / K41's template


def test_argument_validation_needs_no_gpu(hip_lib):
    """null pointers (the labels among them), misaligned labels, k outside 1..8 or above Nk, unknown flag bits and unsupported grids
    are rejected before any HIP call, with check_box3_readout's codes and this entry point's name"""
    one, odd, f = ctypes.c_void_p(16), ctypes.c_void_p(20), ctypes.c_float
    m = getattr(hip_lib, ENTRY)
    ok = lambda **kw: dict(dict(t=one, mu=one, a=one, nu=one, b=one, ql=one, kl=one, idx=one, val=one, lse=one, B=1, Nq=256, Nk=256, h=4,
                                w=64, scale=100.0, k=4, flags=0), **kw)
    call = lambda d: m(d["t"], d["mu"], d["a"], d["nu"], d["b"], d["ql"], d["kl"], d["idx"], d["val"], d["lse"], d["B"], d["Nq"], d["Nk"],
                       d["h"], d["w"], f(2304.0), f(d["scale"]), d["k"], d["flags"], None)
    err = hip_lib.cocos_last_error_string
    for name in ("t", "mu", "a", "nu", "b", "ql", "kl", "idx", "val", "lse"):
        assert call(ok(**{name: None})) == -1 and b"null" in err(), name
    for name in ("ql", "kl"):
        for addr in (17, 18, 22):
            assert call(ok(**{name: ctypes.c_void_p(addr)})) == -1 and b"must be 4-byte aligned" in err(), (name, addr)
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
    assert call(ok(h=16, w=16, ql=odd, kl=odd)) == -2                       # 4-byte aligned labels pass their check; the shape is refused
    call(ok(k=9))
    assert err().startswith(b"box3_topk_labels_f16x3:")
    # the labelled entry serves every k the unlabelled one does: all eight LABELS instantiations have no scratch
    assert hip_lib.cocos_box3_topk_max_k() == 8


def test_op_refuses_in_order(hip_lib, monkeypatch):
    """a non-tensor or another label dtype (TypeError), a label shape, a bad k (ValueError), then the device, then the shapes"""
    from cocosnet_amd import _lib, ops
    N = 256
    t, s, lab = torch.zeros(N * N), torch.ones(1, N), torch.zeros(1, N, dtype=torch.int64)
    run = lambda ql=lab, kl=lab, k=4, t=t, **kw: ops.box3_topk_labelled(t, s, s, s, s, ql, kl, 4, 64, 2304.0, 100.0, k, **kw)
    with pytest.raises(TypeError, match="t: expected a tensor"):
        run(t=None)
    for bad in (lab.float(), lab.to(torch.int16), lab.bool(), None, [0] * N):
        with pytest.raises(TypeError, match="q_label must be an int32 or int64 tensor"):
            run(ql=bad)
        with pytest.raises(TypeError, match="k_label must be an int32 or int64 tensor"):
            run(kl=bad)
    with pytest.raises(TypeError, match="q_label must be"):          # the dtype wins over the shape and over k
        run(ql=torch.zeros(2, N), k=9)
    with pytest.raises(ValueError, match="q_label is"):
        run(ql=torch.zeros(1, N + 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="k_label is"):
        run(kl=torch.zeros(2, N, dtype=torch.int64))
    with pytest.raises(ValueError, match="k_label is"):              # a label shape wins over k
        run(kl=torch.zeros(N, dtype=torch.int64), k=9)
    for k in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="k="):
            run(k=k)
    monkeypatch.setattr(ops, "box3_topk_ok", lambda k: k != 8)      # a k whose instantiation does not ship is refused, not materialised
    with pytest.raises(ValueError, match="no instantiation serves it"):
        run(k=8)
    monkeypatch.undo()
    for transposed in (False, True):
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            run(transposed=transposed)
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            run(ql=lab.to(torch.int32), kl=lab.to(torch.int32), transposed=transposed)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):      # the device wins over a shape mismatch
        run(t=torch.zeros(7))
    monkeypatch.setattr(ops, "PRECISION", "fp32")                          # ... and over the precision
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        run()


def test_boxed_corr_method_refuses_cpu_tensors(hip_lib):
    from cocosnet_amd import _lib
    from cocosnet_amd.hot_path import _BoxedCorr
    th = torch.zeros(1, 256, 4, 64)
    lab = torch.zeros(1, 256, dtype=torch.int32)
    for rows in (True, False):
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            _BoxedCorr(th, th, 100.0).match_labelled(rows, lab, lab, 2)


def test_restrict_on_the_match_kernel_1_route_still_refuses_match_kernel_3(monkeypatch):
    """K55 adds `_box3` entry points; match(restrict=) and correspondence_match(restrict=) keep their message under match_kernel 3"""
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd.hot_path import _ROUTE, HotPathConfig, correspondence_match, correspondence_sparse
    th = torch.zeros(1, 256, 4, 64)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    with pytest.raises(ValueError, match="restrict runs on the fused match_kernel 1 route only"):
        correspondence_match(th, th, cfg, restrict="label")
    with pytest.raises(ValueError, match="restrict runs on the fused match_kernel 1 route only"):
        correspondence_sparse(th, th, None, None, None, cfg, restrict="label")
    assert _ROUTE["restrict"] == ": restrict runs on the fused match_kernel 1 route only"
    net = cc.NoVGGCorrespondence(cc.ade20k_options(crop_size=64, semantic_nc=7, match_kernel=3))
    monkeypatch.setattr(net, "project", lambda *a, **k: pytest.fail("the network ran"))
    with pytest.raises(ValueError, match="match: match_kernel 3 is out of scope: restrict runs on the fused match_kernel 1 route only"):
        net.match(None, None, None, restrict="label")


# ---------------------------------------------------------------------------------------------------------------- hot path, module
def _cfg(**kw):
    from cocosnet_amd.hot_path import HotPathConfig
    return HotPathConfig(**dict(dict(match_kernel=3, PONO_C=True, down=4), **kw))


OFF_ROUTE = [dict(match_kernel=1), dict(match_kernel=2), dict(PONO_C=False)]
OFF_PLAIN = [dict(warp_patch=True), dict(warp_bilinear=True), dict(warp_cycle_w=1.0), dict(two_cycle=True), dict(warp_mask_losstype="cycle")]
_ids = lambda sets: [next(iter(f)) + "=" + str(next(iter(f.values()))) for f in sets]


@pytest.mark.parametrize("flags", OFF_ROUTE, ids=_ids(OFF_ROUTE))
def test_every_off_route_flag_set_raises_naming_restrict(flags):
    from cocosnet_amd.hot_path import _ROUTE, correspondence_match_box3, correspondence_sparse_box3
    th = torch.zeros(1, 256, 4, 64)
    assert "match_kernel 3 route" in _ROUTE["restrict_box3"] and "restrict" in _ROUTE["restrict_box3"]
    for call in (lambda: correspondence_match_box3(th, th, _cfg(**flags), restrict="label"),
                 lambda: correspondence_sparse_box3(th, th, None, None, None, _cfg(**flags), restrict="label")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value).endswith(_ROUTE["restrict_box3"]) and "restrict" in str(e.value).split(_ROUTE["restrict_box3"])[0]


@pytest.mark.parametrize("flags", OFF_PLAIN, ids=_ids(OFF_PLAIN))
def test_the_sparse_warp_needs_the_plain_flag_set(flags):
    """the restricted sparse warp refuses what the sparse warp refuses, naming restrict; the readout has no warp and takes these flags
    as match() does (it then ends at the device)"""
    from cocosnet_amd import _lib
    from cocosnet_amd.hot_path import _ROUTE, correspondence_match_box3, correspondence_sparse_box3
    th = torch.zeros(1, 256, 4, 64)
    lab = torch.zeros(1, 4, 64, dtype=torch.int64)
    with pytest.raises(ValueError, match="restrict") as e:
        correspondence_sparse_box3(th, th, None, None, None, _cfg(**flags), restrict="label")
    assert str(e.value).endswith(_ROUTE["restrict_box3"])
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        correspondence_match_box3(th, th, _cfg(**flags), restrict=(lab, lab))


def test_hot_path_refusal_order(monkeypatch):
    """arguments (direction, topk, restrict's form and dtype), then the flag set, precision and the switch, channels — all before a
    tensor is looked at; then the labels' fit, the device, the shapes"""
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import correspondence_match_box3, correspondence_sparse_box3
    th, bad = torch.zeros(1, 256, 4, 64), _cfg(match_kernel=1)
    lab = torch.zeros(1, 4, 64, dtype=torch.int64)
    with pytest.raises(ValueError, match="direction 'diag'"):
        correspondence_match_box3(th, th, bad, direction="diag", topk=9, restrict="label")
    with pytest.raises(ValueError, match="topk=9"):
        correspondence_match_box3(th, th, bad, topk=9, restrict="labels")
    for restrict in ("labels", 3, (lab,), (lab, lab, lab), (lab, None)):
        with pytest.raises(ValueError, match="restrict="):
            correspondence_match_box3(th, th, bad, restrict=restrict)
    with pytest.raises(TypeError, match="restrict: the labels must be int32 or int64"):
        correspondence_match_box3(th, th, bad, restrict=(lab, lab.float()))
    with pytest.raises(ValueError, match="restrict: match_kernel 1 is out of scope"):
        correspondence_match_box3(th, th, bad, restrict="label")
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="restrict: COCOS_PRECISION=fp32"):
        correspondence_match_box3(th, th, _cfg(), restrict="label")
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    monkeypatch.setattr(ops, "MATCH_FUSED", False)
    with pytest.raises(ValueError, match="restrict: ops.MATCH_FUSED"):
        correspondence_match_box3(th, th, _cfg(), restrict="label")
    monkeypatch.setattr(ops, "MATCH_FUSED", True)
    with pytest.raises(ValueError, match="restrict: needs 256 channels"):
        correspondence_match_box3(torch.zeros(1, 64, 4, 64), torch.zeros(1, 64, 4, 64), _cfg(), restrict="label")
    # a tensor is looked at from here on: the label maps / the pair must fit the grids ...
    seg = torch.zeros(1, 5, 16, 256)
    with pytest.raises(ValueError, match="restrict='label' needs seg_map"):
        correspondence_match_box3(th, th, _cfg(), restrict="label")
    with pytest.raises(ValueError, match="restrict='label' needs ref_seg_map"):
        correspondence_match_box3(th, th, _cfg(), restrict="label", seg_map=seg, ref_seg_map=seg[:, :, :8])
    with pytest.raises(ValueError, match="restrict: labels"):
        correspondence_match_box3(th, th, _cfg(), restrict=(lab, lab[:, :2]))
    # ... then the device, before the shapes: a 16-wide grid on the CPU
    for direction in ("rows", "cols"):
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            correspondence_match_box3(th, th, _cfg(), restrict="label", seg_map=seg, ref_seg_map=seg, direction=direction, topk=4)
    t16, l16 = torch.zeros(1, 256, 16, 16), torch.zeros(1, 16, 16, dtype=torch.int32)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        correspondence_match_box3(t16, t16, _cfg(), restrict=(l16, l16))
    # restrict = None is correspondence_match on the same arguments: it ends where that ends
    with pytest.raises(_lib.CocosHipError, match="correspondence_match: .*no CPU fallback"):
        correspondence_match_box3(th, th, _cfg())
    with pytest.raises(ValueError, match="correspondence_match: direction"):
        correspondence_match_box3(th, th, _cfg(), direction="diag")

    # the sparse warp: restrict with transport, then the scope, all before a tensor is looked at
    img = torch.zeros(1, 3, 16, 256)
    with pytest.raises(ValueError, match="restrict with transport is out of scope"):
        correspondence_sparse_box3(th, th, img, seg, seg, _cfg(), restrict="label", transport={"iters": 2, "tau": 1.0})
    with pytest.raises(ValueError, match="restrict with transport is out of scope"):      # (also with a malformed transport)
        correspondence_sparse_box3(th, th, img, seg, seg, bad, restrict=(lab, lab), transport={"iters": 0})
    with pytest.raises(ValueError, match="topk=0"):
        correspondence_sparse_box3(th, th, img, seg, seg, bad, topk=0, restrict="label")
    with pytest.raises(ValueError, match="restrict="):
        correspondence_sparse_box3(th, th, img, seg, seg, bad, restrict="yes")
    with pytest.raises(ValueError, match="restrict: match_kernel 1 is out of scope"):
        correspondence_sparse_box3(th, th, img, seg, seg, bad, restrict="label")
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        correspondence_sparse_box3(th, th, img, seg, seg, _cfg(), restrict="label")
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):      # restrict = None: the route as it was
        correspondence_sparse_box3(th, th, img, seg, seg, _cfg())


def test_module_refuses_before_the_network_runs(monkeypatch):
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd.hot_path import _ROUTE
    lab = torch.zeros(1, 16, 16, dtype=torch.int64)
    for over in (dict(match_kernel=1), dict(match_kernel=3, PONO_C=False)):
        net = cc.NoVGGCorrespondence(cc.ade20k_options(crop_size=64, semantic_nc=7, **over))
        monkeypatch.setattr(net, "project", lambda *a, **k: pytest.fail("the network ran"))
        for call in (lambda: net.match_box3(None, None, None), lambda: net.match_box3(None, None, None, restrict=(lab, lab)),
                     lambda: net.sparse_warp_box3(None, None, None, None, restrict="label")):
            with pytest.raises(ValueError, match="restrict") as e:
                call()
            assert str(e.value).endswith(_ROUTE["restrict_box3"])
    net = cc.NoVGGCorrespondence(cc.ade20k_options(crop_size=64, semantic_nc=7, match_kernel=3))
    monkeypatch.setattr(net, "project", lambda *a, **k: pytest.fail("the network ran"))
    with pytest.raises(ValueError, match="direction"):
        net.match_box3(None, None, None, direction="diag")
    with pytest.raises(ValueError, match="topk="):
        net.match_box3(None, None, None, topk=0)
    with pytest.raises(ValueError, match="blend"):
        net.match_box3(None, None, None, blend="soft")
    with pytest.raises(ValueError, match="hard_warp"):
        net.match_box3(None, None, None, direction="cols", hard_warp=True)
    with pytest.raises(ValueError, match="restrict="):
        net.match_box3(None, None, None, restrict="region")
    with pytest.raises(TypeError, match="restrict: the labels must be int32 or int64"):
        net.match_box3(None, None, None, restrict=(lab.float(), lab))
    with pytest.raises(ValueError, match="restrict: ref_img and ref_seg_map are required"):
        net.match_box3(None, None, None)
    with pytest.raises(ValueError, match="restrict with transport is out of scope"):
        net.sparse_warp_box3(None, None, None, None, restrict="label", transport={"iters": 2, "tau": 1.0})
    with pytest.raises(ValueError, match="restrict="):
        net.sparse_warp_box3(None, None, None, None, restrict=7)
    with pytest.raises(ValueError, match="ref_img and ref_seg_map are required"):
        net.sparse_warp_box3(None, None, None, None, restrict="label")
