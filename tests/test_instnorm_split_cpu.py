"""K34 without a GPU: the translation unit is part of the build, header / library / binding agree on its three symbols, the workspace
size is host arithmetic that covers what the two calls carve out of it, and the entry points reject bad arguments before any HIP call."""
import ctypes

NEW_SYMBOLS = ("cocos_instnorm_prelu_split_workspace_floats", "cocos_instnorm_prelu_split_fwd", "cocos_instnorm_prelu_split_bwd")
SLICE = 16384


def test_translation_unit_is_built_and_symbols_agree(hip_lib):
    from cocosnet_amd import _lib, build
    assert "instnorm_split.hip" in build.HIP_SOURCES
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES and name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name


def _needed_floats(planes, N):
    """What the calls keep per (plane, slice): forward (mean, M2), backward (sum dz, sum dz xn), one fp64 da partial (two floats), one
    maximum."""
    S = -(-N // SLICE)
    return planes * S * (2 + 2 + 2 + 1)


def test_workspace_size_is_host_arithmetic(hip_lib):
    ws = hip_lib.cocos_instnorm_prelu_split_workspace_floats
    for planes, N in ((1, 1), (6, 16388), (2, 262144)):
        assert ws(planes, N) > 0
        assert ws(planes, N) >= _needed_floats(planes, N), (planes, N)
    # monotone in the planes and in the number of slices; constant inside one slice count
    assert ws(1, 1) <= ws(2, 1) <= ws(3, 1) < ws(64, 1)
    sizes = [ws(4, n) for n in (1, SLICE, SLICE + 1, 2 * SLICE, 2 * SLICE + 1, 16 * SLICE, 16 * SLICE + 1)]
    assert sizes == sorted(sizes) and sizes[0] == sizes[1] < sizes[2] == sizes[3] < sizes[4] < sizes[5] < sizes[6]
    assert ws(0, 16) == 0 and ws(3, 0) == 0 and ws(-1, -1) == 0
    assert ws(2048, 1 << 20) >= _needed_floats(2048, 1 << 20)           # no 32-bit overflow: 9.2e5 floats ... 64 slices x 2048 planes


def test_bad_arguments_are_rejected_before_any_hip_call(hip_lib):
    one, f = ctypes.c_void_p(16), ctypes.c_float
    fwd, bwd = hip_lib.cocos_instnorm_prelu_split_fwd, hip_lib.cocos_instnorm_prelu_split_bwd
    assert fwd(None, None, one, one, one, one, None, 1, 16, f(1e-5), None) == -1 and b"null" in hip_lib.cocos_last_error_string()
    assert fwd(one, None, one, one, None, one, None, 1, 16, f(1e-5), None) == -1            # stats is an output, not optional
    assert fwd(one, None, one, one, one, None, None, 1, 16, f(1e-5), None) == -1            # nor is the workspace
    assert fwd(one, None, one, one, one, one, None, 0, 16, f(1e-5), None) == -1 and b"bad dims" in hip_lib.cocos_last_error_string()
    assert fwd(one, None, one, one, one, one, None, 1, 0, f(1e-5), None) == -1
    assert bwd(one, None, one, None, one, one, None, None, one, None, 1, 16, f(1e-5), None) == -1      # dy
    assert bwd(one, None, one, one, None, one, None, None, one, None, 1, 16, f(1e-5), None) == -1      # stats
    assert bwd(one, None, one, one, one, one, None, None, one, None, 1, -4, f(1e-5), None) == -1
    assert bwd(one, None, one, one, one, None, None, one, one, one, 1, 16, f(1e-5), None) == -1 and b"without dx" in hip_lib.cocos_last_error_string()
    assert bwd(one, None, one, one, one, one, None, one, ctypes.c_void_p(20), None, 1, 16, f(1e-5), None) == -1 \
        and b"8-byte" in hip_lib.cocos_last_error_string()


def test_switch_is_a_plain_module_attribute():
    from cocosnet_amd import ops
    assert isinstance(ops.INSTNORM_SPLIT, bool) and callable(ops.instnorm_prelu_split)
