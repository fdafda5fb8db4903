"""K30 without a GPU: the new entry points are declared, bound and validate their arguments before any launch; the bilinear backward's
tap tables are the adjoint of F.interpolate's formula; the hot path on CPU tensors does not depend on ops.WARP_HEAD_MODES."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

_P, _I = ctypes.c_void_p, ctypes.c_int
#: the K30 entry points as include/cocos_hip.h declares them, written out by hand: the anchor that the derived binding is held to
NEW = {"cocos_warp_head_fwd_ex": (_I, [_P] * 3 + [_I] * 7 + [_P]),
       "cocos_warp_head_bwd_ex": (_I, [_P] * 7 + [_I] * 7 + [_P]),
       "cocos_warp_values_patch_amax": (_I, [_P] * 3 + [_I] * 6 + [_P, _P]),
       "cocos_warp_head_bilinear_tap": (ctypes.c_float, [_I] * 4)}


def test_header_declares_the_new_entry_points_and_the_binding_matches(hip_lib):
    from cocosnet_amd import _lib
    for name, literal in NEW.items():
        assert name in _lib.PROTOTYPES, name + " is not declared in cocos_hip.h"
        ret, args = _lib.PROTOTYPES[name]
        res, argtypes = _lib._SIGNATURES[name]
        assert (res, argtypes) == literal, name
        assert len(argtypes) == len(args), name
        assert res is (ctypes.c_float if ret == "float" else ctypes.c_int), name
        for a, ty in zip(args, argtypes):
            if "*" in a or a.startswith("cocos_stream_t"):
                assert ty is ctypes.c_void_p, (name, a)
            else:
                assert a.startswith("int ") and ty is ctypes.c_int, (name, a)
        assert hasattr(hip_lib, name)
    for mode, value in (("NEAREST", 0), ("BILINEAR", 1), ("PATCH", 2)):
        assert _lib.CONSTANTS["COCOS_WARP_HEAD_" + mode] == value


def test_argument_validation_of_the_new_entry_points_needs_no_gpu(hip_lib):
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    err = hip_lib.cocos_last_error_string
    fwd, bwd, val = hip_lib.cocos_warp_head_fwd_ex, hip_lib.cocos_warp_head_bwd_ex, hip_lib.cocos_warp_values_patch_amax
    # forward: null, mode, dims, y_bi only with nearest, patch consistency, width / alignment
    assert fwd(None, one, None, 1, 3, 3, 4, 4, 4, 1, None) == -1 and b"null" in err()
    assert fwd(one, one, None, 1, 3, 3, 4, 4, 4, 3, None) == -1 and b"mode" in err()
    assert fwd(one, one, None, 1, 4, 3, 4, 4, 4, 1, None) == -1 and b"bad dims" in err()
    assert fwd(one, one, one, 1, 3, 3, 4, 4, 4, 1, None) == -1 and b"y_bi" in err()
    assert fwd(one, one, None, 1, 40, 48, 4, 4, 4, 2, None) == -1 and b"down^2" in err()
    assert fwd(one, one, None, 1, 3, 3, 4, 3, 2, 1, None) == -2 and b"multiple of 4" in err()
    assert fwd(one, odd, None, 1, 3, 3, 4, 4, 4, 1, None) == -2
    # backward: null, mode, dims (Cs = 0 is fine, Ci + Cs = 0 is not), patch consistency, grid width, alignment
    assert bwd(one, None, None, None, one, one, one, 1, 3, 0, 4, 4, 4, 1, None) == -1 and b"null" in err()
    assert bwd(one, None, None, one, one, one, None, 1, 3, 0, 4, 4, 4, 1, None) == -1 and b"null" in err()
    assert bwd(one, None, None, one, one, one, one, 1, 3, 0, 4, 4, 4, 7, None) == -1 and b"mode" in err()
    assert bwd(one, None, None, one, one, one, one, 1, 0, 0, 4, 4, 4, 1, None) == -1 and b"bad dims" in err()
    assert bwd(one, None, None, one, one, one, one, 1, 40, 0, 4, 4, 4, 2, None) == -1 and b"down^2" in err()
    assert bwd(one, None, None, one, one, one, one, 1, 3, 0, 4, 6, 4, 1, None) == -2 and b"multiple of 4" in err()
    assert bwd(one, None, odd, one, one, one, one, 1, 3, 0, 4, 4, 4, 1, None) == -1 and b"aligned" in err()
    # the nearest mode with mask channels (round 6's shape): missing gradients are zeros, a missing o is refused
    assert bwd(None, None, None, None, one, one, one, 1, 3, 2, 4, 4, 4, 0, None) == -1 and b"null" in err()
    # patch values: null, dims, divisibility
    assert val(None, None, one, 1, 3, 0, 8, 8, 4, None, None) == -1 and b"null" in err()
    assert val(one, None, None, 1, 3, 0, 8, 8, 4, None, None) == -1
    assert val(one, None, one, 1, 3, 0, 8, 8, 0, None, None) == -1 and b"bad dims" in err()
    assert val(one, one, one, 1, 3, 5, 10, 10, 4, None, None) == -2 and b"multiple of down" in err()
    assert hip_lib.cocos_warp_head_bilinear_tap(3, 0, 0, 0) == -1.0
    assert hip_lib.cocos_warp_head_bilinear_tap(4, 8, 0, 0) == -1.0


@pytest.mark.parametrize("d", [2, 4])
@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_tap_tables_are_the_adjoint_of_the_interpolation_formula(d, n, hip_lib):
    """A[x, X] built in fp64 from s = max((X + .5)/d - .5, 0), i0 = floor(s), i1 = min(i0 + 1, n - 1), lambda = s - i0; the kernel's table
    must give exactly A[x, d*x - d/2 + idx] inside the window, and A must be zero outside it.  A is also checked against
    F.interpolate itself (fp64)."""
    A = torch.zeros(n, n * d, dtype=torch.float64)
    for X in range(n * d):
        s = max((X + 0.5) / d - 0.5, 0.0)
        i0 = int(s)
        i1 = min(i0 + 1, n - 1)
        lam = s - i0
        A[i0, X] += 1.0 - lam
        A[i1, X] += lam
    eye = torch.eye(n, dtype=torch.float64).reshape(n, 1, 1, n)
    up = F.interpolate(eye.expand(n, 1, 2, n), scale_factor=d, mode="bilinear", align_corners=False)[:, 0, 0]      # [n, n*d]
    assert float((up - A).abs().max()) < 1e-15
    seen = torch.zeros_like(A, dtype=torch.bool)
    for x in range(n):
        for idx in range(2 * d):
            X = d * x - d // 2 + idx
            if 0 <= X < n * d:
                tap = hip_lib.cocos_warp_head_bilinear_tap(d, idx, int(x == 0), int(x == n - 1))
                assert tap == float(A[x, X]), (x, idx, tap, float(A[x, X]))
                seen[x, X] = True
    assert float(A[~seen].abs().max() if bool((~seen).any()) else 0.0) == 0.0
    lams = sorted({round(float(v), 6) for v in A.flatten().tolist()} - {0.0, 1.0})
    assert set(lams) <= ({0.125, 0.375, 0.625, 0.875} if d == 4 else {0.25, 0.75})


FLAG_SETS = [dict(warp_bilinear=True, warp_cycle_w=0.1, warp_mask_losstype="direct"),
             dict(warp_bilinear=True, warp_cycle_w=1.0, two_cycle=True, warp_mask_losstype="none"),
             dict(warp_patch=True, warp_cycle_w=1.0, warp_mask_losstype="none"),
             dict(warp_patch=True, warp_bilinear=True, warp_mask_losstype="direct"),
             dict(show_corr=True, warp_mask_losstype="direct", isTrain=False)]


@pytest.mark.parametrize("flags", FLAG_SETS)
def test_hot_path_on_cpu_tensors_does_not_depend_on_the_switch(flags, monkeypatch):
    """CPU tensors keep the framework route whatever ops.WARP_HEAD_MODES says: the attention kernels are replaced by torch stand-ins
    (they have no CPU form), the K30 ops raise if reached, and both settings give bit-identical outputs and gradients."""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_hot_path

    def center_l2norm(x, mode, *a, **k):
        x = x - x.mean(dim=1, keepdim=True)
        return x / (x.norm(dim=1, keepdim=True) + 1e-12)

    def corr_softmax_warp(q, k, v, inv_t, planes=None):
        p = torch.softmax(torch.einsum("bcq,bck->bqk", q, k) * inv_t, dim=2)
        return torch.einsum("bqk,bck->bcq", p, v)

    def reached(*a, **k):
        raise AssertionError("a K30 op was reached with CPU tensors")

    monkeypatch.setattr(ops, "center_l2norm", center_l2norm)
    monkeypatch.setattr(ops, "corr_softmax_warp", corr_softmax_warp)
    monkeypatch.setattr(ops, "warp_head", reached)
    monkeypatch.setattr(ops, "warp_values", reached)
    f = dict(isTrain=True)
    f.update(flags)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4, **f)
    B, fh, fw, nc = 1, 4, 8, 5
    g = torch.Generator().manual_seed(3)
    runs = []
    for modes in (False, True):
        monkeypatch.setattr(ops, "WARP_HEAD_MODES", modes)
        g.manual_seed(3)
        th = torch.randn(B, 256, fh, fw, generator=g).requires_grad_(True)
        ph = torch.randn(B, 256, fh, fw, generator=g).requires_grad_(True)
        img = torch.rand(B, 3, fh * 4, fw * 4, generator=g)
        real = torch.rand(B, 3, fh * 4, fw * 4, generator=g)
        seg = torch.rand(B, nc, fh * 4, fw * 4, generator=g)
        out = correspondence_hot_path(th, ph, img, real, seg, seg, cfg, temperature=0.1)
        keys = sorted(out)
        sum((out[k] * torch.randn(out[k].shape, generator=g)).sum() for k in keys).backward()
        runs.append(([out[k].detach() for k in keys], th.grad, ph.grad, keys))
    a, b = runs
    assert a[3] == b[3]
    for u, v in zip(a[0], b[0]):
        assert torch.equal(u, v)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_switch_and_mode_checks_need_no_gpu():
    from cocosnet_amd import ops
    assert ops.WARP_HEAD_MODES is True or os.environ.get("COCOS_WARP_HEAD_MODES") == "0"
    o = torch.randn(1, 3, 16)
    assert not ops.warp_head_ok(o, 3, 4, 4, 4, "bilinear")            # CPU tensor
    with pytest.raises(ValueError):
        ops.warp_head(o, 3, 4, 4, 4, mode="cubic")
