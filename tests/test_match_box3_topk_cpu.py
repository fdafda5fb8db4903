"""K41 (top-k match readout on the fused match_kernel-3 route), the parts that need no GPU: the two entry points in header, binding
table and library, what cocos_box3_topk_max_k() says and that `ops.box3_topk_ok` reads it, the argument checks of the C entry point
(all of which answer before any kernel is reached) and the op's refusal of CPU tensors."""
import ctypes

import pytest
import torch

NEW_SYMBOLS = ("cocos_box3_topk_f16x3", "cocos_box3_topk_max_k")


def test_header_table_and_library_carry_the_entry_points(hip_lib):
    from cocosnet_amd import _lib, build
    for name in NEW_SYMBOLS:
        assert _lib.PROTOTYPES.get(name, ("",))[0] == "int", f"{name} is not declared in cocos_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(hip_lib, name)
    # the binding is derived from the header: 8 pointers, 5 ints, 2 floats, k, flags, the stream
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib._SIGNATURES["cocos_box3_topk_f16x3"] == (I, [P] * 8 + [I] * 5 + [F, F] + [I, I] + [P])
    assert _lib._SIGNATURES["cocos_box3_topk_max_k"] == (I, [])
    assert "box3_fused_f16x3.hip" in build.HIP_SOURCES      # the unit that holds the kernel (one template with K37)


def test_max_k_and_the_python_gate_agree(hip_lib):
    from cocosnet_amd import _lib, ops
    max_k = hip_lib.cocos_box3_topk_max_k()
    # K = 2 and K = 4 ship at least, and never more than the header's maximum
    assert 4 <= max_k <= 8 == _lib.CONSTANTS["COCOS_MATCH_TOPK_MAX"]
    assert [ops.box3_topk_ok(k) for k in range(0, 10)] == [1 <= k <= max_k for k in range(0, 10)]


def test_argument_validation_needs_no_gpu(hip_lib):
    """null pointers, k outside 1..8 or above Nk, unknown flag bits, unsupported shapes and misaligned pointers are rejected before any
    HIP call"""
    one, odd, f = ctypes.c_void_p(16), ctypes.c_void_p(20), ctypes.c_float
    m = hip_lib.cocos_box3_topk_f16x3
    ok = lambda **kw: dict(dict(t=one, mu=one, a=one, nu=one, b=one, idx=one, val=one, lse=one, B=1, Nq=256, Nk=256, h=4, w=64,
                                scale=100.0, k=4, flags=0), **kw)
    call = lambda d: m(d["t"], d["mu"], d["a"], d["nu"], d["b"], d["idx"], d["val"], d["lse"], d["B"], d["Nq"], d["Nk"], d["h"], d["w"],
                       f(2304.0), f(d["scale"]), d["k"], d["flags"], None)
    err = hip_lib.cocos_last_error_string
    for name in ("t", "mu", "a", "nu", "b", "idx", "val", "lse"):
        assert call(ok(**{name: None})) == -1 and b"null" in err(), name
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
    for name in ("t", "nu", "b"):
        assert call(ok(**{name: odd})) == -1 and b"aligned" in err(), name
    for k in range(hip_lib.cocos_box3_topk_max_k() + 1, 9):                 # an instantiation that does not ship
        assert call(ok(k=k)) == -2 and b"cocos_row_topk_lse" in err(), k
    # the messages carry this entry point's name, and K37's entry keeps its own
    call(ok(k=9))
    assert err().startswith(b"box3_topk_f16x3:")
    hip_lib.cocos_box3_match_f16x3(None, one, one, one, one, one, one, one, 1, 256, 256, 4, 64, f(2304.0), f(100.0), 0, None)
    assert err().startswith(b"box3_match_f16x3:")


def test_op_fails_loudly_on_cpu_tensors(hip_lib):
    from cocosnet_amd import _lib, ops
    N = 256
    t, s = torch.zeros(N * N), torch.ones(1, N)
    for transposed in (False, True):
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            ops.box3_topk(t, s, s, s, s, 4, 64, 2304.0, 100.0, 4, transposed=transposed)


def test_new_branch_refuses_cpu_tensors_and_bad_k(hip_lib):
    from cocosnet_amd import _lib
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    th = torch.zeros(1, 256, 4, 64)
    for direction in ("rows", "cols"):
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            correspondence_match(th, th, cfg, direction=direction, topk=4)
    with pytest.raises(ValueError, match="topk=9"):
        correspondence_match(th, th, cfg, topk=9)
