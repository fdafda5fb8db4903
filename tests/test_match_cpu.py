"""K36 match readout, the parts that need no GPU: MatchReadout's index arithmetic, the argument checks of `NoVGGCorrespondence.match`
(which raise before any kernel is reached), and the three entry points in header, binding table and library."""
import ctypes

import pytest
import torch

NEW_SYMBOLS = ("cocos_corr_match_f16x3", "cocos_row_argmax_lse", "cocos_gather_patches")


def _readout(index, grid=None):
    from cocosnet_amd.hot_path import MatchReadout
    z = torch.zeros(index.shape)
    return MatchReadout(index=index, prob=z, max_logit=z, lse=z, grid=grid)


def test_xy_round_trip_on_a_square_grid():
    idx = torch.tensor([[[0, 3], [12, 15]]])                # positions on a 4 x 4 grid asked from a 2 x 2 one
    xy = _readout(idx, grid=(4, 4)).xy()
    assert xy.shape == (1, 2, 2, 2) and xy.dtype == torch.int64
    assert xy[0, 0].tolist() == [[0, 3], [0, 3]]            # x
    assert xy[0, 1].tolist() == [[0, 0], [3, 3]]            # y
    assert torch.equal(xy[:, 1] * 4 + xy[:, 0], idx)


def test_xy_round_trip_on_a_non_square_grid():
    h, w = 4, 8
    idx = torch.arange(h * w).flip(0).reshape(1, h, w)      # every cell of the 4 x 8 grid once, as its own grid (grid=None)
    r = _readout(idx)
    xy = r.xy()
    assert xy.shape == (1, 2, h, w)
    assert int(xy[0, 0].max()) == w - 1 and int(xy[0, 1].max()) == h - 1
    assert torch.equal(xy[:, 1] * w + xy[:, 0], idx)
    assert xy[0, :, 0, 0].tolist() == [w - 1, h - 1] and xy[0, :, h - 1, w - 1].tolist() == [0, 0]
    other = _readout(idx, grid=(8, 4)).xy()                 # the same flat indices on an 8 x 4 grid: another width
    assert torch.equal(other[:, 1] * 4 + other[:, 0], idx) and int(other[0, 0].max()) == 3


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


def test_match_argument_validation(hip_lib):
    from cocosnet_amd import _lib, inference
    net, other = _cpu_net(0), _cpu_net(1)
    ref_img, seg, ref_seg = _cpu_inputs()
    with pytest.raises(ValueError, match="hard_warp"):
        net.match(ref_img, seg, ref_seg, direction="cols", hard_warp=True)
    with pytest.raises(ValueError, match="direction"):
        net.match(ref_img, seg, ref_seg, direction="diagonal")
    with pytest.raises(ValueError, match="required"):
        net.match(None, seg, ref_seg)
    rec = inference.prepare_exemplar(other, ref_img, ref_seg)
    with pytest.raises(ValueError, match="THIS network"):
        net.match(None, seg, None, exemplar=rec)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        net.match(ref_img, seg, ref_seg)
    own = inference.prepare_exemplar(net, ref_img, ref_seg)      # a record of THIS network, on the CPU: the same refusal
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        net.match(None, seg, None, exemplar=own)


def test_ops_fail_loudly_on_cpu_tensors(hip_lib):
    from cocosnet_amd import _lib, ops
    x = torch.randn(1, 256, 8)
    for call in (lambda: ops.corr_match(x, x, 100.0), lambda: ops.row_argmax_lse(torch.randn(1, 4, 8)),
                 lambda: ops.gather_patches(torch.randn(1, 3, 8, 8), torch.zeros(1, 4, dtype=torch.int64), 2, 2, 4)):
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            call()
    assert ops.MATCH_FUSED is True


def test_header_table_and_library_carry_the_three_entry_points(hip_lib):
    from cocosnet_amd import _lib, build
    for name in NEW_SYMBOLS:
        assert _lib.PROTOTYPES.get(name, ("",))[0] == "int", f"{name} is not declared in cocos_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(hip_lib, name)
    for unit in ("corr_topk_f16x3.hip", "row_topk_lse.hip", "gather_warp.hip"):      # K36a / K36b are the K = 1 instantiations
        assert unit in build.HIP_SOURCES


def test_argument_validation_needs_no_gpu(hip_lib):
    """null pointers, unsupported shapes and bad strides are rejected before any HIP call"""
    one, f = ctypes.c_void_p(16), ctypes.c_float
    m = hip_lib.cocos_corr_match_f16x3
    assert m(None, one, one, one, one, one, one, 1, 256, 64, 64, f(100.0), f(16.0), 0, None) == -1
    assert b"null" in hip_lib.cocos_last_error_string()
    assert m(one, one, one, one, one, one, None, 1, 256, 64, 64, f(100.0), f(16.0), 0, None) == -1
    assert m(one, one, one, one, one, one, one, 1, 128, 64, 64, f(100.0), f(16.0), 0, None) == -2
    assert m(one, one, one, one, one, one, one, 1, 256, 64, 66, f(100.0), f(16.0), 0, None) == -2
    assert m(one, one, one, one, one, one, one, 2, 256, 64, 64, f(100.0), f(16.0), 64, None) == -1
    assert m(one, one, one, one, one, one, one, 0, 256, 64, 64, f(100.0), f(16.0), 0, None) == -1
    r = hip_lib.cocos_row_argmax_lse
    assert r(None, one, one, one, 1, 4, 8, None) == -1 and b"null" in hip_lib.cocos_last_error_string()
    assert r(one, one, one, one, 1, 0, 8, None) == -1
    g = hip_lib.cocos_gather_patches
    assert g(one, None, one, 1, 3, 8, 8, 4, 0, None) == -1 and b"null" in hip_lib.cocos_last_error_string()
    assert g(one, one, one, 1, 3, 10, 8, 4, 0, None) == -2 and b"multiples of down" in hip_lib.cocos_last_error_string()
    assert g(one, one, one, 2, 3, 8, 8, 4, 5, None) == -1 and b"img_batch_stride" in hip_lib.cocos_last_error_string()
