"""K26 (fused parameter-free norm + SPADE modulation) without a GPU: the entry points validate their arguments before any HIP
call, the workspace query follows the segment layout, and the SPADE router picks the fused route only for the exact norm classes."""
import ctypes

import pytest
import torch
import torch.nn as nn

f = ctypes.c_float
one = ctypes.c_void_p(16)


def _err(hip_lib):
    return hip_lib.cocos_last_error_string()


def test_workspace_query(hip_lib):
    ws = hip_lib.cocos_norm_spade_workspace_floats
    assert ws(16, 128, 256 * 256) == 4 * 16 * 128 * 64          # 64 segments of 1024 per plane
    assert ws(16, 1024, 64) == 4 * 16 * 1024
    assert ws(1, 5, 63) == 4 * 5
    assert ws(2, 3, 1025) == 4 * 2 * 3 * 2
    assert ws(0, 3, 4) == 0 and ws(1, 0, 4) == 0 and ws(1, 3, 0) == 0


def test_entry_points_reject_null_pointers(hip_lib):
    assert hip_lib.cocos_norm_spade_stats(None, one, one, 2, 3, 16, 0, f(1e-5), None) == -1
    assert b"null" in _err(hip_lib)
    assert hip_lib.cocos_norm_spade_stats(one, one, None, 2, 3, 16, 0, f(1e-5), None) == -1
    assert hip_lib.cocos_norm_spade_apply(one, one, None, one, one, one, None, None, 2, 3, 16, 0, f(0.2), None) == -1
    assert hip_lib.cocos_norm_spade_apply(one, one, one, one, one, one, one, None, 2, 3, 16, 0, f(0.2), None) == -1
    assert b"workspace" in _err(hip_lib)
    assert hip_lib.cocos_norm_spade_bwd_stats(one, one, one, None, one, one, one, one, 2, 3, 16, 1, f(0.2), None) == -1
    assert hip_lib.cocos_norm_spade_bwd_apply(one, one, one, one, None, one, None, f(1.0), one, None, None, None, None, 2, 3, 16, 0,
                                              f(0.2), None) == -1
    assert b"null" in _err(hip_lib)


def test_entry_points_reject_bad_shapes(hip_lib):
    assert hip_lib.cocos_norm_spade_stats(one, one, one, 0, 3, 16, 0, f(1e-5), None) == -1
    assert b"bad dims" in _err(hip_lib)
    assert hip_lib.cocos_norm_spade_stats(one, one, one, 2, 3, 16, 2, f(1e-5), None) == -1      # per_sample must be 0 | 1
    assert hip_lib.cocos_norm_spade_apply(one, one, one, one, one, one, None, None, 2, -1, 16, 0, f(0.2), None) == -1
    assert hip_lib.cocos_norm_spade_bwd_stats(one, one, one, one, one, one, one, one, 2, 3, 0, 1, f(0.2), None) == -1
    assert hip_lib.cocos_norm_spade_bwd_apply(one, one, one, one, one, one, None, f(1.0), one, None, None, None, None, 2, 3, 1 << 29, 0,
                                              f(0.2), None) == -1
    assert b"bad dims" in _err(hip_lib)
    # a workspace that is not 16-byte aligned cannot hold the fp64 partials
    assert hip_lib.cocos_norm_spade_stats(one, one, ctypes.c_void_p(20), 2, 3, 16, 0, f(1e-5), None) == -1
    assert b"aligned" in _err(hip_lib)


def test_router_picks_the_exact_parameter_free_classes():
    from cocosnet_amd import spade
    from cocosnet_amd.dist import SyncBatchNorm2d
    kind = spade._norm_spade_kind
    assert kind(nn.BatchNorm2d(8, affine=False)) == "batch"
    assert kind(nn.BatchNorm2d(8, affine=False, track_running_stats=False)) == "batch"
    assert kind(nn.InstanceNorm2d(8, affine=False)) == "instance"
    assert kind(SyncBatchNorm2d(8, affine=False)) == "syncbatch"
    assert kind(nn.BatchNorm2d(8, affine=True)) is None
    assert kind(nn.InstanceNorm2d(8, affine=True)) is None
    assert kind(nn.InstanceNorm2d(8, track_running_stats=True)) is None
    assert kind(SyncBatchNorm2d(8, affine=True)) is None

    class MyBN(nn.BatchNorm2d):
        pass
    assert kind(MyBN(8, affine=False)) is None
    assert kind(None) is None
    assert spade.NORM_FUSED is True


def test_cpu_tensors_keep_the_module_route():
    """On the CPU the router leaves the norm to its module (and the modulation to torch): same numbers as the plain chain."""
    from cocosnet_amd import spade
    torch.manual_seed(0)
    x, g, b = (torch.randn(2, 4, 5, 6) for _ in range(3))
    for m in (nn.BatchNorm2d(4, affine=False), nn.InstanceNorm2d(4, affine=False)):
        ref = torch.nn.functional.leaky_relu(m(x) * (1 + g) + b, 0.2)
        assert torch.allclose(spade.modulate(x, g, b, False, m, 0.2), ref)


def test_operator_rejects_unknown_kinds_and_single_values():
    from cocosnet_amd import ops
    x = torch.zeros(1, 3, 1, 1)
    with pytest.raises(ValueError, match="kind"):
        ops.norm_spade(x, x, x, "layer")
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.norm_spade(x, x, x, "batch")
    with pytest.raises(ValueError, match="Expected more than 1 spatial element when training"):
        ops.norm_spade(torch.zeros(4, 3, 1, 1), torch.zeros(4, 3, 1, 1), torch.zeros(4, 3, 1, 1), "instance")
