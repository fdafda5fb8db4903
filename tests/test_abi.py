"""CPU checks of the drop-in boundary: the C-ABI library builds for gfx950 without a GPU, loads,
and exports exactly what include/cocos_hip.h declares; the Python binding is derived from the header, type by type; the
product path refuses to run without a GPU instead of falling back to anything."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "cocos_hip.h")


def _declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(cocos_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_expected_entry_points():
    syms = _declared_symbols()
    for must in ("cocos_center_l2norm_fwd", "cocos_center_l2norm_bwd", "cocos_corr_softmax_warp_fwd",
                 "cocos_corr_softmax_warp_bwd", "cocos_corr_materialize", "cocos_row_softmax_fwd",
                 "cocos_row_softmax_bwd", "cocos_version", "cocos_last_error_string"):
        assert must in syms


def test_library_exports_every_declared_symbol(hip_lib):
    for name in _declared_symbols():
        assert hasattr(hip_lib, name), f"{name} declared in cocos_hip.h but not exported"


def test_binding_signature_table_matches_header(hip_lib):
    from cocosnet_amd import _lib
    assert sorted(_lib.EXPORTED_SYMBOLS) == _declared_symbols()


_P, _I, _F, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
#: prototypes of include/cocos_hip.h written out by hand as ctypes (not computed from the header): between them every type the
#: binding maps and every awkward shape — (void), const char*, size_t / long long / float returns, int64_t, double, long long and
#: const unsigned* / int* / struct* / float* const* parameters, comments holding , and ) inside a parameter list, /* nullable */
#: marks, many lines, the x2 groups of the pair launches
EXPECTED_SIGNATURES = {
    "cocos_version": (_I, []),
    "cocos_last_error_string": (ctypes.c_char_p, []),
    "cocos_corr_softmax_warp_saved_logits_bytes": (ctypes.c_size_t, [_I] * 3),
    "cocos_corr_softmax_warp_fwd_f16x3": (_I, [_P] * 11 + [_I] * 5 + [_F, _F] + [_P, _P, _P]),
    "cocos_ema_multi_update": (_I, [_P, _I, ctypes.c_double, _P, _P]),
    "cocos_gather_patches": (_I, [_P] * 3 + [_I] * 5 + [_LL, _P]),
    "cocos_wta_scale_mask_bytes": (_LL, [_LL, _I]),
    "cocos_warp_head_bilinear_tap": (_F, [_I] * 4),
    "cocos_row_softmax_fwd": (_I, [_P, _P, ctypes.c_int64, _I, _P]),
    "cocos_loss_partials": (_I, [_I, _P]),
    "cocos_proj_center_l2norm_planes_f16x3": (_I, [_I] + [_P] * 10 * 2 + [_I] * 4 + [_F, _F] + [_P]),
    "cocos_weight_absmax_multi_workspace_floats": (_LL, [_P, _I]),
}


@pytest.mark.parametrize("name", sorted(EXPECTED_SIGNATURES))
def test_derived_signature_equals_the_hand_written_one(name):
    from cocosnet_amd import _lib
    res, argtypes = _lib._SIGNATURES[name]
    want_res, want_args = EXPECTED_SIGNATURES[name]
    assert res is want_res, (name, res)
    assert len(argtypes) == len(want_args), (name, len(argtypes))
    for i, (got, want) in enumerate(zip(argtypes, want_args)):
        assert got is want, (name, i, got, want)


def test_parser_on_a_synthetic_header():
    from cocosnet_amd import _lib
    text = """
    #ifndef COCOS_GUARD_H
    #define COCOS_GUARD_H
    #define COCOS_A 3            /* a comment, (with) both */
    #define COCOS_B (-2)
    #define COCOS_C (1 << 4)     // 16
    typedef void* cocos_stream_t;
    typedef struct cocos_entry { float* p; long long n; } cocos_entry;
    int cocos_f(const float* x /* nullable: f(a, b), or (c) */, int n,   // trailing ) and , too
                const cocos_entry* entries /* host, nullable */,
                double mu, cocos_stream_t stream);
    const char* cocos_g(void);
    #endif
    """
    prototypes, signatures, constants = _lib.parse_header(text)
    assert constants == {"COCOS_A": 3, "COCOS_B": -2, "COCOS_C": 16}
    assert list(signatures) == ["cocos_f", "cocos_g"]
    assert prototypes["cocos_f"] == ("int", ["const float* x", "int n", "const cocos_entry* entries", "double mu", "cocos_stream_t stream"])
    assert signatures["cocos_f"] == (_I, [_P, _I, _P, ctypes.c_double, _P])
    assert signatures["cocos_g"] == (ctypes.c_char_p, []) and prototypes["cocos_g"] == ("const char*", [])
    for bad in ("int cocos_h(unsigned n);", "int cocos_h(short n, cocos_stream_t stream);", "short cocos_h(void);",
                "void* cocos_h(int n);", "int cocos_h(int);", "int cocos_h(int (*callback)(int));",
                "#define COCOS_D (COCOS_A + 1)", "#define COCOS_D 1.5", "#define COCOS_D 0x10u"):
        with pytest.raises(_lib.CocosHipError, match="cocos_h|COCOS_D"):
            _lib.parse_header(text + bad + "\n")


def test_every_integer_define_of_the_header_is_a_constant():
    from cocosnet_amd import _lib
    names = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(COCOS_\w+)[ \t]+\S", open(HEADER).read(), flags=re.M)
    assert len(names) == len(set(names)) >= 40 and "COCOS_HIP_H" not in names
    assert list(_lib.CONSTANTS) == names
    assert all(type(v) is int for v in _lib.CONSTANTS.values())
    literal = dict(COCOS_OK=0, COCOS_ERR_INVALID=-1, COCOS_ERR_UNSUPPORTED=-2, COCOS_ERR_HIP=-3, COCOS_ERR_WORKSPACE=-4,
                   COCOS_WARP_HEAD_NEAREST=0, COCOS_WARP_HEAD_BILINEAR=1, COCOS_WARP_HEAD_PATCH=2,
                   COCOS_GAN_HINGE_D_REAL=0, COCOS_GAN_HINGE_D_FAKE=1, COCOS_GAN_NEG_MEAN=2, COCOS_GAN_MEAN=3, COCOS_GAN_LS=4,
                   COCOS_GAN_BCE=5,
                   COCOS_WPREP_CONV_FWD=0, COCOS_WPREP_CONV_DGRAD=1, COCOS_WPREP_CONV_FWD_BF16=2, COCOS_WPREP_CONV_DGRAD_BF16=3,
                   COCOS_WPREP_ROWS=4, COCOS_WPREP_FRAG=5,
                   COCOS_OPTIM_ENTRY_ELEMS=1 << 24)
    for name, value in literal.items():
        assert _lib.CONSTANTS[name] == value, name
    err = _lib.CocosHipError("x")
    assert err.code == 0 and not err.unsupported
    err.code = -2
    assert err.unsupported


def test_python_names_of_header_constants_keep_their_values():
    from cocosnet_amd import ops
    assert ops._HEAD_MODES == {"nearest": 0, "bilinear": 1, "patch": 2}
    assert ops.GAN_MODES == {"hinge_d_real": 0, "hinge_d_fake": 1, "neg_mean": 2, "mean": 3, "ls": 4, "bce": 5}
    assert ops.WPREP_LAYOUTS == {"conv_fwd": 0, "conv_dgrad": 1, "conv_fwd_bf16": 2, "conv_dgrad_bf16": 3, "rows": 4, "frag": 5}
    assert (ops.PAIR_LOSS_MAX_SEGMENTS, ops.GAN_LOSS_MAX_TENSORS) == (16, 8)
    assert (ops.CENTER_POSITIONS, ops.CENTER_CHANNELS, ops.CENTER_NONE) == (0, 1, 2)


@pytest.mark.parametrize("family, entry", [("OPTIM", "cocos_optim_constant"), ("WPREP", "cocos_weight_prepare_constant")])
def test_header_constants_are_what_the_library_was_built_with(family, entry, hip_lib):
    """COCOS_<family>_CONST_<X> = k selects COCOS_<family>_<X>: the header's value against the built library's, for every k"""
    from cocosnet_amd import _lib
    prefix = f"COCOS_{family}_CONST_"
    selectors = {v: n[len(prefix):] for n, v in _lib.CONSTANTS.items() if n.startswith(prefix)}
    assert sorted(selectors) == list(range(len(selectors))) and len(selectors) >= 2
    fn = getattr(hip_lib, entry)
    for k, what in selectors.items():
        assert fn(k) == _lib.CONSTANTS[f"COCOS_{family}_{what}"] > 0, (k, what)
    assert fn(len(selectors)) == 0 and fn(-1) == 0


def test_version_and_error_string(hip_lib):
    assert hip_lib.cocos_version() >= 100
    assert isinstance(hip_lib.cocos_last_error_string(), bytes)


def test_argument_validation_needs_no_gpu(hip_lib):
    """Null pointers / unsupported shapes are rejected before any HIP call is made."""
    rc = hip_lib.cocos_corr_softmax_warp_fwd(None, None, None, None, None, None, 1, 256, 4, 4, 3,
                                             ctypes.c_float(100.0), None)
    assert rc == -1 and b"null" in hip_lib.cocos_last_error_string()
    one = ctypes.c_void_p(16)
    rc = hip_lib.cocos_corr_softmax_warp_fwd(one, one, one, one, one, None, 1, 2304, 4, 4, 3,
                                             ctypes.c_float(100.0), None)
    assert rc == -2 and b"K == 256" in hip_lib.cocos_last_error_string()
    rc = hip_lib.cocos_corr_softmax_warp_fwd(one, one, one, one, one, None, 1, 256, 4, 4, 161,
                                             ctypes.c_float(100.0), None)
    assert rc == -2
    assert hip_lib.cocos_corr_softmax_warp_bwd_workspace_bytes(8, 256, 4096, 4096, 154) == 8 * 4096 * 4
    rc = hip_lib.cocos_row_softmax_fwd(one, one, 0, 16, None)
    assert rc == -1


def test_k0_streaming_planners_and_validation_need_no_gpu(hip_lib):
    """Host-side planning of the K0 streaming kernels: padded k extent of the register-resident weight planes,
    number of partial tiles of the weight-gradient reduction (0 = shape goes to the general split GEMM), and the
    argument checks that run before any HIP call."""
    kpad = hip_lib.cocos_proj1x1_stream_kpad
    assert [kpad(k) for k in (1, 64, 256, 257, 407, 416, 417, 0, -3)] == [256, 256, 256, 416, 416, 416, 0, 0, 0]
    parts = hip_lib.cocos_proj1x1_dw_partials_f16x3
    assert parts(8, 407, 256, 4096) == 128            # the benchmark shape: 16 chunks of 256 positions per image
    assert parts(8, 256, 256, 4096) == 128
    assert parts(1, 3, 2, 64) == 1                    # tiny grids: one chunk
    assert parts(5, 416, 130, 192) == 15              # >= 4 k-steps (64 positions) per chunk
    assert parts(2, 300, 407, 128) == 0               # more than 256 output channels
    assert parts(2, 449, 256, 128) == 0               # more than 448 input channels
    assert parts(1, 5, 3, 21) == 0                    # HW not a multiple of 4
    one = ctypes.c_void_p(16)
    f = ctypes.c_float
    rc = hip_lib.cocos_proj1x1_stream_f16x3(one, one, one, None, None, one, 2, 417, 256, 64, None, None)
    assert rc == -2 and b"K <= 416" in hip_lib.cocos_last_error_string()
    rc = hip_lib.cocos_proj1x1_stream_f16x3(one, one, one, None, None, one, 2, 256, 256, 100, None, None)
    assert rc == -2
    rc = hip_lib.cocos_proj1x1_stream_f16x3(None, one, one, None, None, one, 2, 256, 256, 64, None, None)
    assert rc == -1
    rc = hip_lib.cocos_proj1x1_dw_f16x3(one, one, one, None, one, one, 2, 256, 256, 64, None, None, None)
    assert rc == -1 and b"go together" in hip_lib.cocos_last_error_string()
    rc = hip_lib.cocos_proj1x1_dw_f16x3(one, one, one, None, one, None, 2, 256, 300, 64, None, None, None)
    assert rc == -2
    rc = hip_lib.cocos_warp_values(one, one, one, 1, 3, 5, 10, 10, 4, None)
    assert rc == -2 and b"multiple of down" in hip_lib.cocos_last_error_string()
    rc = hip_lib.cocos_warp_values(None, one, one, 1, 3, 5, 8, 8, 4, None)
    assert rc == -1
    rc = hip_lib.cocos_split_f16_rows(one, one, one, 4, 8, 7, f(1.0), None, None, None)
    assert rc == -1
    rc = hip_lib.cocos_absmax_accumulate(one, 0, one, None)
    assert rc == -1
    rc = hip_lib.cocos_center_l2norm_bwd_amax(one, one, one, one, None, None, 1, 16, 8, 1, f(1e-16), None, None)
    assert rc == -1 and b"amax" in hip_lib.cocos_last_error_string()
    assert hip_lib.cocos_box3_logits_bwd_workspace_bytes(8, 64, 64) > 2 * 8 * (256 * 4096 + 4096 * 4) * 4


def test_product_path_fails_loudly_on_cpu_tensors(hip_lib):
    from cocosnet_amd import _lib, ops
    x = torch.randn(1, 256, 8)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.center_l2norm(x, True)
    with pytest.raises(_lib.CocosHipError):
        ops.corr_softmax_warp(x, x, torch.randn(1, 3, 8), 100.0)


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under cocosnet_amd/ may import it."""
    pkg = os.path.join(REPO, "cocosnet_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "corr_oracle" not in src, f
