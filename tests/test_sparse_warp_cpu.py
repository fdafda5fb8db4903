"""K42 (the differentiable k-sparse warp), the parts that need no GPU: the entry points in header, binding table and library, their
argument checks (which return before any HIP call), and the Python-side refusals of ops.sparse_softmax_warp,
hot_path.correspondence_sparse and NoVGGCorrespondence.sparse_warp."""
import ctypes

import pytest
import torch

NEW_SYMBOLS = ("cocos_sparse_softmax_warp_fwd_f16x3", "cocos_sparse_softmax_warp_bwd_query_f16x3", "cocos_sparse_softmax_warp_bwd_key_f16x3",
               "cocos_transpose_f32")


def test_header_table_and_library_carry_the_entry_points(hip_lib):
    from cocosnet_amd import _lib, build
    for name in NEW_SYMBOLS:
        assert _lib.PROTOTYPES.get(name, ("",))[0] == "int", f"{name} is not declared in cocos_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(hip_lib, name)
    assert "plane_pair.hip" in build.HIP_SOURCES


def test_argument_validation_needs_no_gpu(hip_lib):
    """null pointers (-1), k outside 1..min(8, Nk) (-1), K != 256 (-2), misaligned planes (-1): all before any HIP call"""
    one, f = ctypes.c_void_p(16), ctypes.c_float
    err = hip_lib.cocos_last_error_string
    tail = lambda K, Nk, k, B=1, Nq=64, Cv=3: (B, K, Nq, Nk, Cv, k, f(100.0), f(16.0), None)
    fwd = lambda K=256, Nk=64, k=4, p=(one,) * 8, **kw: hip_lib.cocos_sparse_softmax_warp_fwd_f16x3(*p, *tail(K, Nk, k, **kw))
    bq = lambda K=256, Nk=64, k=4, p=(one,) * 8, **kw: hip_lib.cocos_sparse_softmax_warp_bwd_query_f16x3(*p, *tail(K, Nk, k, **kw))
    bk = lambda K=256, Nk=64, k=4, p=(one,) * 9, **kw: hip_lib.cocos_sparse_softmax_warp_bwd_key_f16x3(*p, *tail(K, Nk, k, **kw))
    for call, n in ((fwd, 8), (bq, 8), (bk, 9)):
        assert call(K=128) == -2 and b"K == 256" in err()
        assert call(k=0) == -1 and b"k=0" in err()
        assert call(k=9) == -1 and b"k=9" in err()
        assert call(Nk=4, k=8) == -1 and b"Nk=4" in err()
        assert call(B=0) == -1 and call(Cv=0) == -1 and call(Nq=0) == -1
        assert call(p=(ctypes.c_void_p(24),) + (one,) * (n - 1)) == -1 and b"aligned" in err()
    for i in range(8):
        assert fwd(p=(one,) * i + (None,) + (one,) * (7 - i)) == -1 and b"null" in err()
    for i in range(7):      # (dq_t, the eighth pointer, may be null)
        assert bq(p=(one,) * i + (None,) + (one,) * (7 - i)) == -1 and b"null" in err()
    for i in (2, 4, 5, 6):      # dout_t, w, entries, offsets
        assert bk(p=(one,) * i + (None,) + (one,) * (8 - i)) == -1 and b"null" in err()
    assert bk(p=(one,) * 7 + (None, None)) == -1 and b"null" in err()                  # neither dk_t nor dv_t
    assert bk(p=(None,) + (one,) * 8) == -1 and b"dk_t needs" in err()                 # dk_t without the query planes
    t = hip_lib.cocos_transpose_f32
    assert t(None, one, 1, 4, 4, None) == -1 and b"null" in err()
    assert t(one, one, 1, 0, 4, None) == -1
    assert t(one, one, 70000, 4, 4, None) == -2 and b"launch grid" in err()


def test_op_refuses_on_the_host(hip_lib):
    from cocosnet_amd import _lib, ops
    q, k, v = torch.randn(1, 256, 8), torch.randn(1, 256, 12), torch.randn(1, 3, 12)
    idx = torch.zeros(1, 8, 2, dtype=torch.int64)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.sparse_softmax_warp(q, k, v, idx, 100.0)
    for bad in (idx.float(), idx.to(torch.int16), idx.bool()):
        with pytest.raises(TypeError, match="idx"):
            ops.sparse_softmax_warp(q, k, v, bad, 100.0)
    for args in ((q, k, v, idx[:, :7]), (q, k, v[:, :, :11], idx), (q, k[:, :128], v, idx), (q, k, v, idx[0]),
                 (q[:, :128], k[:, :128], v, idx), (torch.randn(2, 256, 8), k, v, idx)):
        with pytest.raises(ValueError):
            ops.sparse_softmax_warp(*args, 100.0)
    with pytest.raises(ValueError, match="k=9"):
        ops.sparse_softmax_warp(q, k, v, torch.zeros(1, 8, 9, dtype=torch.int64), 100.0)
    with pytest.raises(ValueError, match="k=5"):                                       # more candidates than keys
        ops.sparse_softmax_warp(q, k[:, :, :4], v[:, :, :4], torch.zeros(1, 8, 5, dtype=torch.int64), 100.0)


OUT_OF_SCOPE = [(dict(match_kernel=3), "match_kernel 3"), (dict(PONO_C=False), "PONO_C"), (dict(warp_patch=True), "warp_patch"),
                (dict(warp_bilinear=True), "warp_bilinear"), (dict(warp_cycle_w=1.0), "cycle"), (dict(two_cycle=True), "cycle"),
                (dict(warp_mask_losstype="cycle"), "cycle")]


def _hot_inputs():
    g = torch.Generator().manual_seed(5)
    onehot = lambda: torch.zeros(1, 5, 8, 8).scatter_(1, torch.randint(0, 5, (1, 1, 8, 8), generator=g), 1.0)
    return torch.randn(1, 256, 2, 2, generator=g), torch.randn(1, 256, 2, 2, generator=g), torch.rand(1, 3, 8, 8, generator=g), onehot(), onehot()


@pytest.mark.parametrize("flags,word", OUT_OF_SCOPE, ids=[w + "-" + "-".join(f) for f, w in OUT_OF_SCOPE])
def test_correspondence_sparse_names_what_is_out_of_scope(hip_lib, flags, word):
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse
    theta, phi, ref_img, seg, ref_seg = _hot_inputs()
    cfg = HotPathConfig(**dict(dict(match_kernel=1, PONO_C=True, down=4), **flags))
    with pytest.raises(ValueError, match=word):
        correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg)


def test_correspondence_sparse_other_refusals(hip_lib, monkeypatch):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse
    theta, phi, ref_img, seg, ref_seg = _hot_inputs()
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="topk"):
            correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, topk=bad)
    with pytest.raises(ValueError, match="topk=5"):                                    # four exemplar positions
        correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, topk=5)
    with pytest.raises(ValueError, match="prepared exemplar"):
        correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, exemplar=object())
    with pytest.raises(ValueError, match="256 channels"):
        correspondence_sparse(theta[:, :128], phi[:, :128], ref_img, seg, ref_seg, cfg)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):                   # in scope: the tensors themselves are refused
        correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, topk=2)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="COCOS_PRECISION=fp32"):
        correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg)


def test_module_sparse_warp_refuses_before_the_network_runs(hip_lib, monkeypatch):
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
            net.sparse_warp(ref_img, None, seg, ref_seg)
    opt = cc.ade20k_options(crop_size=64, semantic_nc=7, match_kernel=1)
    net = cc.NoVGGCorrespondence(opt).eval()
    with pytest.raises(ValueError, match="topk"):
        net.sparse_warp(ref_img, None, seg, ref_seg, topk=9)
    with pytest.raises(ValueError, match="ref_img"):
        net.sparse_warp(None, None, seg, ref_seg)
