"""K39 top-k match readout, the parts that need no GPU: the three entry points in header, binding table and library, their argument
checks (which return before any launch), the Python-side refusals and TopkMatchReadout's index arithmetic."""
import ctypes

import pytest
import torch

NEW_SYMBOLS = ("cocos_corr_topk_f16x3", "cocos_row_topk_lse", "cocos_gather_blend_patches")
NEW_UNITS = ("corr_topk_f16x3.hip", "row_topk_lse.hip", "gather_warp.hip")


def test_header_table_and_library_carry_the_three_entry_points(hip_lib):
    from cocosnet_amd import _lib, build
    for name in NEW_SYMBOLS:
        assert _lib.PROTOTYPES.get(name, ("",))[0] == "int", f"{name} is not declared in cocos_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(hip_lib, name)
    for unit in NEW_UNITS:
        assert unit in build.HIP_SOURCES


def test_topk_max_is_a_header_constant(hip_lib):
    from cocosnet_amd import _lib, ops
    assert _lib.CONSTANTS["COCOS_MATCH_TOPK_MAX"] == 8 == ops.MATCH_TOPK_MAX
    # the fused kernel ships at least K = 2 and K = 4 and never more than the header's maximum
    assert 4 <= hip_lib.cocos_corr_topk_max_k() <= 8
    assert ops.corr_topk_ok(2) and ops.corr_topk_ok(4) and not ops.corr_topk_ok(0) and not ops.corr_topk_ok(9)
    assert all(ops.corr_topk_ok(k) == (k <= hip_lib.cocos_corr_topk_max_k()) for k in range(1, 9))


def test_argument_validation_needs_no_gpu(hip_lib):
    """null pointers, k outside 1..min(8, Nk), unsupported shapes and bad strides are rejected before any HIP call"""
    one, f = ctypes.c_void_p(16), ctypes.c_float
    err = hip_lib.cocos_last_error_string
    t = lambda K=256, Nk=64, k=4, stride=0, B=1, kl=one, lse=one: hip_lib.cocos_corr_topk_f16x3(
        one, one, one, kl, one, one, lse, B, K, 64, Nk, k, f(100.0), f(16.0), stride, None)
    assert t(kl=None) == -1 and b"null" in err()
    assert t(lse=None) == -1
    assert t(k=0) == -1 and b"k=0" in err()
    assert t(k=9) == -1 and b"k=9" in err()
    assert t(Nk=4, k=8) == -1 and b"Nk=4" in err()
    assert t(K=128) == -2 and b"K == 256" in err()
    assert t(Nk=66) == -2 and b"cocos_row_topk_lse" in err()
    assert t(B=2, stride=64) == -1 and b"k_batch_stride" in err()
    assert t(B=0) == -1
    assert hip_lib.cocos_corr_topk_f16x3(ctypes.c_void_p(24), one, one, one, one, one, one, 1, 256, 64, 64, 2, f(100.0), f(16.0), 0,
                                         None) == -1 and b"aligned" in err()
    r = hip_lib.cocos_row_topk_lse
    assert r(None, one, one, one, 1, 4, 8, 2, None) == -1 and b"null" in err()
    assert r(one, one, one, one, 1, 0, 8, 2, None) == -1
    assert r(one, one, one, one, 1, 4, 8, 0, None) == -1 and b"k=0" in err()
    assert r(one, one, one, one, 1, 4, 8, 9, None) == -1
    assert r(one, one, one, one, 1, 4, 3, 4, None) == -1 and b"Nk=3" in err()
    g = hip_lib.cocos_gather_blend_patches
    assert g(one, None, one, one, 1, 3, 8, 8, 4, 2, 0, None) == -1 and b"null" in err()
    assert g(one, one, None, one, 1, 3, 8, 8, 4, 2, 0, None) == -1
    assert g(one, one, one, one, 1, 3, 8, 8, 4, 0, 0, None) == -1 and b"k=0" in err()
    assert g(one, one, one, one, 1, 3, 8, 8, 4, 9, 0, None) == -1
    assert g(one, one, one, one, 1, 3, 10, 8, 4, 2, 0, None) == -2 and b"multiples of down" in err()
    assert g(one, one, one, one, 2, 3, 8, 8, 4, 2, 5, None) == -1 and b"img_batch_stride" in err()


def test_ops_fail_loudly_on_cpu_tensors(hip_lib):
    from cocosnet_amd import _lib, ops
    x = torch.randn(1, 256, 8)
    idx, w = torch.zeros(1, 2, 2, 2, dtype=torch.int64), torch.ones(1, 2, 2, 2)
    for call in (lambda: ops.corr_topk(x, x, 100.0, 2), lambda: ops.row_topk_lse(torch.randn(1, 4, 8), 2),
                 lambda: ops.gather_blend_patches(torch.randn(1, 3, 8, 8), idx, w, 2, 2, 4)):
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            call()


def _cpu_net(seed=0):
    from cocosnet_amd import correspondence as cc
    opt = cc.ade20k_options(crop_size=64, semantic_nc=7, match_kernel=1)
    torch.manual_seed(seed)
    net = cc.NoVGGCorrespondence(opt)
    net.init_weights(opt.init_type, opt.init_variance)
    return net.eval()


def _cpu_inputs():
    g = torch.Generator().manual_seed(3)
    onehot = lambda: torch.zeros(1, 7, 64, 64).scatter_(1, torch.randint(0, 7, (1, 1, 64, 64), generator=g), 1.0)
    return torch.rand(1, 3, 64, 64, generator=g) * 2 - 1, onehot(), onehot()


def test_match_refuses_bad_topk_and_blend(hip_lib):
    from cocosnet_amd import _lib
    net = _cpu_net()
    ref_img, seg, ref_seg = _cpu_inputs()
    for bad in (9, 0, -1, 2.0, True):
        with pytest.raises(ValueError, match="topk"):
            net.match(ref_img, seg, ref_seg, topk=bad)
    with pytest.raises(ValueError, match="blend"):
        net.match(ref_img, seg, ref_seg, topk=2, blend="x")
    with pytest.raises(ValueError, match="hard_warp"):                       # stays refused
        net.match(ref_img, seg, ref_seg, direction="cols", hard_warp=True, topk=2)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):         # valid arguments: the readout itself refuses CPU tensors
        net.match(ref_img, seg, ref_seg, topk=2, blend="full")


def test_correspondence_match_topk_on_cpu_tensors(hip_lib):
    from cocosnet_amd import _lib
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    theta, phi = torch.randn(1, 256, 2, 2), torch.randn(1, 256, 2, 2)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        correspondence_match(theta, phi, cfg, topk=2)
    with pytest.raises(ValueError, match="topk=5"):                          # four positions: k <= Nk is checked first
        correspondence_match(theta, phi, cfg, topk=5)
    with pytest.raises(ValueError, match="topk=9"):
        correspondence_match(theta, phi, cfg, topk=9)


def test_topk_readout_xy_on_a_hand_made_index():
    from cocosnet_amd.hot_path import TopkMatchReadout
    idx = torch.tensor([[[[0, 7]], [[12, 31]]]])                 # B = 1, k = 2, a 1 x 2 grid asking about a 4 x 8 one
    z = torch.zeros(idx.shape)
    r = TopkMatchReadout(index=idx, prob=z, logit=z, lse=z[:, 0], grid=(4, 8))
    xy = r.xy()
    assert xy.shape == (1, 2, 2, 1, 2) and xy.dtype == torch.int64
    assert xy[0, 0, 0].tolist() == [[0, 7]] and xy[0, 0, 1].tolist() == [[0, 0]]      # rank 0: x, y
    assert xy[0, 1, 0].tolist() == [[4, 7]] and xy[0, 1, 1].tolist() == [[1, 3]]      # rank 1
    assert torch.equal(xy[:, :, 1] * 8 + xy[:, :, 0], idx)
    own = TopkMatchReadout(index=torch.arange(12).reshape(1, 2, 2, 3), prob=z, logit=z, lse=z, grid=None).xy()   # its own 2 x 3 grid
    assert torch.equal(own[:, :, 1] * 3 + own[:, :, 0], torch.arange(12).reshape(1, 2, 2, 3))
