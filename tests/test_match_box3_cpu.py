"""K37 (match readout on the fused match_kernel-3 route), the parts that need no GPU: the entry point in header, binding table and
library, the op's refusal of CPU tensors, and the argument checks of the C entry point and of the new branch of
`correspondence_match` (all of which answer before any kernel is reached)."""
import ctypes

import pytest
import torch

SYMBOL = "cocos_box3_match_f16x3"


def test_header_table_and_library_carry_the_entry_point(hip_lib):
    from cocosnet_amd import _lib, build
    assert _lib.PROTOTYPES.get(SYMBOL, ("",))[0] == "int", f"{SYMBOL} is not declared in cocos_hip.h"
    assert SYMBOL in _lib.EXPORTED_SYMBOLS
    assert hasattr(hip_lib, SYMBOL)
    assert _lib.CONSTANTS["COCOS_BOX3_T_TRANSPOSED"] == 1
    assert "box3_fused_f16x3.hip" in build.HIP_SOURCES      # the unit that holds the kernel (next to K19, whose helpers it uses)


def test_op_fails_loudly_on_cpu_tensors(hip_lib):
    from cocosnet_amd import _lib, ops
    N = 256
    t, s = torch.zeros(N * N), torch.ones(1, N)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.box3_match(t, s, s, s, s, 4, 64, 2304.0, 100.0)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.box3_match(t, s, s, s, s, 4, 64, 2304.0, 100.0, transposed=True)


def test_argument_validation_needs_no_gpu(hip_lib):
    """null pointers, unknown flag bits, unsupported shapes and misaligned pointers are rejected before any HIP call"""
    one, odd, f = ctypes.c_void_p(16), ctypes.c_void_p(20), ctypes.c_float
    m = hip_lib.cocos_box3_match_f16x3
    ok = lambda **kw: dict(dict(t=one, mu=one, a=one, nu=one, b=one, idx=one, mx=one, lse=one, B=1, Nq=256, Nk=256, h=4, w=64,
                                scale=100.0, flags=0), **kw)
    call = lambda d: m(d["t"], d["mu"], d["a"], d["nu"], d["b"], d["idx"], d["mx"], d["lse"], d["B"], d["Nq"], d["Nk"], d["h"], d["w"],
                       f(2304.0), f(d["scale"]), d["flags"], None)
    err = hip_lib.cocos_last_error_string
    for name in ("t", "mu", "a", "nu", "b", "idx", "mx", "lse"):
        assert call(ok(**{name: None})) == -1 and b"null" in err(), name
    assert call(ok(flags=2)) == -1 and b"flags" in err()          # COCOS_BOX3_G_ACCUMULATE belongs to the backward
    assert call(ok(flags=4)) == -1 and b"flags" in err()
    assert call(ok(B=0)) == -1
    assert call(ok(scale=0.0)) == -1
    assert call(ok(h=16, w=16)) == -2 and b"64- or 128-wide" in err()      # a 16-wide grid
    assert call(ok(Nk=512)) == -2                                          # Nq != Nk
    assert call(ok(h=2, Nq=128, Nk=128)) == -2                             # not a multiple of 256 positions
    assert call(ok(h=3, w=64, Nq=256, Nk=256)) == -2                       # Nq != h * w
    for name in ("t", "nu", "b"):
        assert call(ok(**{name: odd})) == -1 and b"aligned" in err(), name
    # the supported set is cocos_box3_fused_supported(Nq, Nk, 1, h, w), no more and no less
    sup = hip_lib.cocos_box3_fused_supported
    shapes = ((256, 256, 4, 64), (256, 256, 2, 128), (5120, 5120, 40, 128), (256, 256, 16, 16), (256, 512, 4, 64), (192, 192, 3, 64))
    assert [sup(Nq, Nk, 1, h, w) for Nq, Nk, h, w in shapes] == [1, 1, 1, 0, 0, 0]
    for Nq, Nk, h, w in shapes[3:]:
        assert call(ok(Nq=Nq, Nk=Nk, h=h, w=w)) == -2, (Nq, Nk, h, w)


def test_new_branch_argument_validation_needs_no_gpu(hip_lib):
    """correspondence_match on the match_kernel-3 flags: the checks that run before the route is chosen, and the refusal of CPU tensors"""
    from cocosnet_amd import _lib
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    th = torch.zeros(1, 256, 4, 64)
    with pytest.raises(ValueError, match="direction"):
        correspondence_match(th, th, cfg, direction="diagonal")
    with pytest.raises(ValueError, match="phi_raw or a prepared exemplar"):
        correspondence_match(th, None, cfg)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        correspondence_match(th, th, cfg)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        correspondence_match(th, th, cfg, direction="cols")
