"""K46 (gradients of the sub-cell refinement), the parts that need no GPU: the three entry points in header, binding table and library,
their argument checks (which return before any HIP call), the Python-side refusals of ops.soft_match_offset / ops.subcell_warp,
hot_path.correspondence_flow and NoVGGCorrespondence.flow_warp, and the restatement the GPU tests judge the kernels by
(tests/match_flow_case.py): its analytic gradients against torch.autograd on a torch-fp64 implementation of the same functions."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_flow_case as fc  # noqa: E402
import match_refine_case as mc  # noqa: E402

QUERY, KEY, GATHER = "cocos_match_refine_bwd_query_f16x3", "cocos_match_refine_bwd_key_f16x3", "cocos_gather_patches_subcell_bwd_off"
_P, _I, _F, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong


def test_header_table_and_library_carry_the_entry_points(hip_lib):
    from cocosnet_amd import _lib, build
    for name in (QUERY, KEY, GATHER):
        assert _lib.PROTOTYPES.get(name, ("",))[0] == "int", f"{name} is not declared in cocos_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    assert "plane_pair.hip" in build.HIP_SOURCES
    assert list(_lib._SIGNATURES[QUERY][1]) == [_P] * 8 + [_I] * 7 + [_F] * 2 + [_P]
    assert list(_lib._SIGNATURES[KEY][1]) == [_P] * 6 + [_I] * 7 + [_F] * 2 + [_P]
    assert list(_lib._SIGNATURES[GATHER][1]) == [_P] * 5 + [_I] * 7 + [_LL, _P]


def test_match_kernels_validate_their_arguments_without_a_gpu(hip_lib):
    """per entry point: a null pointer (-1; dq_t alone may be null), K = 128 (-2), radius 0 and 4 (-1), hk wk != Nk (-1) — and the
    rest of the contract once: sizes, scales, alignment, the 32-bit tables.  All before any HIP call."""
    one, f = ctypes.c_void_p(16), ctypes.c_float
    err = hip_lib.cocos_last_error_string

    def query(p=(one,) * 8, B=1, K=256, Nq=35, Nk=18, hk=3, wk=6, radius=1, inv_t=100.0, scale=16.0):
        return hip_lib.cocos_match_refine_bwd_query_f16x3(*p, B, K, Nq, Nk, hk, wk, radius, f(inv_t), f(scale), None)

    def key(p=(one,) * 6, B=1, K=256, Nq=35, Nk=18, hk=3, wk=6, radius=1, inv_t=100.0, scale=16.0):
        return hip_lib.cocos_match_refine_bwd_key_f16x3(*p, B, K, Nq, Nk, hk, wk, radius, f(inv_t), f(scale), None)

    for call, n, nullable in ((query, 8, (7,)), (key, 6, ())):
        for i in range(n):
            if i not in nullable:
                assert call(p=(one,) * i + (None,) + (one,) * (n - 1 - i)) == -1 and b"null" in err(), (call.__name__, i)
        assert call(K=128) == -2 and b"K == 256" in err()
        for r in (0, 4):
            assert call(radius=r) == -1 and b"radius=" in err()
        assert call(hk=3, wk=5) == -1 and b"hk=3" in err() and b"Nk=18" in err()
        for bad, word in ((dict(B=0), b"B=0"), (dict(Nq=0), b"Nq=0"), (dict(Nk=-1), b"Nk=-1"), (dict(hk=0), b"hk=0")):
            assert call(**bad) == -1 and word in err(), bad
        assert call(inv_t=0.0) == -1 and call(scale=-1.0) == -1 and b"inv_temperature" in err()
        assert call(p=(ctypes.c_void_p(24),) + (one,) * (n - 1)) == -1 and b"aligned" in err()
        assert call(B=2 ** 16, Nq=2 ** 12, radius=1) == -2 and b"32-bit" in err()            # B Nq W = 9 * 2^28 >= 2^31
        assert call(B=2 ** 16, Nq=2 ** 12, radius=1, K=128) == -2
    assert query(p=(one,) * 7 + (ctypes.c_void_p(8),)) == -1 and b"aligned" in err()          # dq_t, when given, is written as float4


def test_gather_backward_validates_its_arguments_without_a_gpu(hip_lib):
    one = ctypes.c_void_p(16)
    err = hip_lib.cocos_last_error_string

    def call(p=(one,) * 5, B=1, C=3, fh=5, fw=7, hk=3, wk=6, down=2, stride=None):
        return hip_lib.cocos_gather_patches_subcell_bwd_off(*p, B, C, fh, fw, hk, wk, down,
                                                            C * hk * down * wk * down if stride is None else stride, None)

    for i in range(5):
        assert call(p=(one,) * i + (None,) + (one,) * (4 - i)) == -1 and b"null" in err()
    for bad, word in ((dict(B=0), b"B=0"), (dict(C=0), b"C=0"), (dict(fh=0), b"fh=0"), (dict(wk=0), b"wk=0"), (dict(down=0), b"down=0")):
        assert call(**bad) == -1 and word in err(), bad
    assert call(stride=7) == -1 and b"img_batch_stride" in err()
    assert call(hk=2 ** 22, down=4, stride=0) == -2 and b"2^24" in err()


def test_ops_refuse_on_the_host_and_bad_arguments(hip_lib):
    from cocosnet_amd import _lib, ops
    q, k = torch.randn(1, 256, 35), torch.randn(1, 256, 18)
    idx = torch.zeros(1, 35, dtype=torch.int64)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.soft_match_offset(q, k, idx, (3, 6), 100.0, 1)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.soft_match_offset(q.clone().requires_grad_(True), k, idx, (3, 6), 100.0, 3)
    for bad in (0, 4, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="soft_match_offset: radius"):
            ops.soft_match_offset(q, k, idx, (3, 6), 100.0, bad)
    for bad in ((3, 5), (3,), (0, 18), (3.0, 6), None):
        with pytest.raises(ValueError, match="kgrid|key grid"):
            ops.soft_match_offset(q, k, idx, bad, 100.0, 1)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="inv_t"):
            ops.soft_match_offset(q, k, idx, (3, 6), bad, 1)
    with pytest.raises(ValueError, match="256 channels"):
        ops.soft_match_offset(q[:, :128], k[:, :128], idx, (3, 6), 100.0, 1)
    with pytest.raises(ValueError):
        ops.soft_match_offset(torch.randn(2, 256, 35), k, idx, (3, 6), 100.0, 1)

    img, off = torch.rand(1, 3, 6, 12), torch.zeros(1, 35, 2)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.subcell_warp(img, idx, off, (5, 7), (3, 6), 2)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.subcell_warp(img, idx, off.clone().requires_grad_(True), (5, 7), (3, 6), 2)
    with pytest.raises(ValueError, match="gradient to the exemplar image is not built"):
        ops.subcell_warp(img.clone().requires_grad_(True), idx, off, (5, 7), (3, 6), 2)
    with pytest.raises(TypeError, match="off"):
        ops.subcell_warp(img, idx, off.double(), (5, 7), (3, 6), 2)
    for args in ((img, idx, off, (5, 7), (3, 6), 4), (img, idx, off, (5, 6), (3, 6), 2), (img, idx, off[:, :, :1], (5, 7), (3, 6), 2),
                 (img[0], idx, off, (5, 7), (3, 6), 2), (img.expand(3, -1, -1, -1), idx, off, (5, 7), (3, 6), 2),
                 (img, idx, off, (5, 7), (3, 6), 0), (img, idx, off, (5, 7), (0, 6), 2), (img, idx, off, 5, (3, 6), 2)):
        with pytest.raises(ValueError):
            ops.subcell_warp(*args)


#: flag sets outside correspondence_sparse's scope, and the words of ITS refusal (correspondence_flow raises the same)
OFF_ROUTE = [(dict(match_kernel=3), "correspondence_sparse: match_kernel 3 is out of scope"), (dict(PONO_C=False), "correspondence_sparse: needs PONO_C"),
             (dict(warp_patch=True), "correspondence_sparse: warp_patch is out of scope"),
             (dict(warp_bilinear=True), "correspondence_sparse: warp_bilinear is out of scope"),
             (dict(warp_cycle_w=1.0), "correspondence_sparse: the cycle terms"), (dict(two_cycle=True), "correspondence_sparse: the cycle terms")]


def test_correspondence_flow_refusals(hip_lib, monkeypatch):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_flow, correspondence_sparse
    g = torch.Generator().manual_seed(5)
    theta, phi = torch.randn(1, 256, 2, 2, generator=g), torch.randn(1, 256, 2, 2, generator=g)
    img, seg = torch.rand(1, 3, 8, 8, generator=g), torch.zeros(1, 2, 8, 8)
    base = dict(match_kernel=1, PONO_C=True, down=4)
    cfg = HotPathConfig(**base)
    for flags, words in OFF_ROUTE:
        other = HotPathConfig(**dict(base, **flags))
        with pytest.raises(ValueError, match=words):
            correspondence_flow(theta, phi, img, other)
        with pytest.raises(ValueError, match=words):      # ... which are correspondence_sparse's own
            correspondence_sparse(theta, phi, img, seg, seg, other)
    for bad in (0, 4, -1, 1.0, True, None, "1"):
        with pytest.raises(ValueError, match="correspondence_flow: radius"):
            correspondence_flow(theta, phi, img, cfg, radius=bad)
    for bad in (0.0, -0.01, "0.01", True):
        with pytest.raises(ValueError, match="refine_temperature"):
            correspondence_flow(theta, phi, img, cfg, refine_temperature=bad)
    with pytest.raises(ValueError, match="prepared exemplar"):
        correspondence_flow(theta, None, img, cfg, exemplar=object())
    with pytest.raises(ValueError, match="256 channels"):
        correspondence_flow(theta[:, :128], phi[:, :128], img, cfg)
    with pytest.raises(ValueError, match="ref_img"):
        correspondence_flow(theta, phi, img[:, :, :4], cfg)
    with pytest.raises(ValueError, match="gradient to the exemplar image is not built"):
        correspondence_flow(theta, phi, img.clone().requires_grad_(True), cfg)
    for r in (1, 3):      # in scope: the tensors themselves are refused
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            correspondence_flow(theta, phi, img, cfg, radius=r, refine_temperature=None if r == 1 else 0.02)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="COCOS_PRECISION=fp32"):
        correspondence_flow(theta, phi, img, cfg)


def test_module_refuses_before_the_network_runs(hip_lib, monkeypatch):
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd import ops
    g = torch.Generator().manual_seed(3)
    onehot = lambda: torch.zeros(1, 7, 64, 64).scatter_(1, torch.randint(0, 7, (1, 1, 64, 64), generator=g), 1.0)
    ref_img, seg, ref_seg = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1, onehot(), onehot()

    def net_for(**flags):
        opt = cc.ade20k_options(**dict(dict(crop_size=64, semantic_nc=7, match_kernel=1), **flags))
        torch.manual_seed(0)
        net = cc.NoVGGCorrespondence(opt).eval()
        monkeypatch.setattr(net, "project", lambda *a, **k: pytest.fail("project() ran for a refused flow_warp"))
        return net

    for flags, words in OFF_ROUTE:
        with pytest.raises(ValueError, match=words):
            net_for(**flags).flow_warp(ref_img, ref_img, seg, ref_seg)
    net = net_for()
    for bad in (0, 4, 2.0, True):
        with pytest.raises(ValueError, match="radius"):
            net.flow_warp(ref_img, ref_img, seg, ref_seg, radius=bad)
    with pytest.raises(ValueError, match="refine_temperature"):
        net.flow_warp(ref_img, ref_img, seg, ref_seg, refine_temperature=0.0)
    with pytest.raises(ValueError, match="ref_img and ref_seg_map are required"):
        net.flow_warp(None, ref_img, seg, None)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="COCOS_PRECISION=fp32"):
        net.flow_warp(ref_img, ref_img, seg, ref_seg)


# ---------------------------------------------------------------------------------------------------------------- the restatement
KGRID = (3, 6)
CENTRES = [0, 5, 12, 17, 3, 6, 8, 9, -4, 40]      # corners, edges, the interior, out of range on both sides


def _window_case(seed):
    g = np.random.default_rng(seed)
    unit = lambda n: (lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True))(g.standard_normal((2, n, 256)))
    qv, kv = unit(len(CENTRES)), unit(18)
    idx = np.array([CENTRES, CENTRES[::-1]])
    return qv, kv, idx, g.standard_normal((2, len(CENTRES), 2))


@pytest.mark.parametrize("inv_t", [10.0, 100.0])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_window_backward_restatement_against_autograd(r, inv_t):
    """ds, dq, dk of tests/match_flow_case.refine_bwd against torch.autograd (fp64) of the soft-argmax, on a 3 x 6 key grid with
    centres at the corners, on the edges and in the interior; the slots outside the grid are exactly 0, and the forward the
    function differentiates is tests/match_refine_case.refine's"""
    qv, kv, idx, doff = _window_case(10 * r)
    ds, dq, dk = fc.refine_bwd(qv, kv, idx, KGRID, r, inv_t, doff)
    q, k = (torch.tensor(t, requires_grad=True) for t in (qv, kv))
    off = fc.t_refine_off(q, k, torch.tensor(idx), KGRID, r, inv_t)
    assert np.abs(off.detach().numpy() - mc.refine(qv, kv, idx, KGRID, r, inv_t)[0]).max() < 1e-12
    (off * torch.tensor(doff)).sum().backward()
    for name, got, want in (("dq", dq, q.grad.numpy()), ("dk", dk, k.grad.numpy())):
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name
    assert np.abs(dq).max() > 0 and np.abs(dk).max() > 0
    # ds is the gradient at the logits: scaling q by (1 + eps) scales every logit, so <ds, s> is the directional derivative along q
    for b in range(2):
        for i, c in enumerate(idx[b]):
            inside = {fc.slot(dx, dy, r) for _, dx, dy in mc.window(c, KGRID, r)}
            assert all(ds[b, i, e] == 0.0 for e in range((2 * r + 1) ** 2) if e not in inside)
            assert abs(ds[b, i].sum()) < 1e-12          # a softmax's logit gradients sum to 0
            keys = [key for key, _, _ in mc.window(c, KGRID, r)]
            slots = [fc.slot(dx, dy, r) for _, dx, dy in mc.window(c, KGRID, r)]
            assert np.abs(inv_t * ds[b, i, slots] @ kv[b, keys] - dq[b, i]).max() < 1e-12
    # the torch restatement of the same formulas (the GPU tests' fp32 arm), in fp64
    t = fc.t_refine_bwd(torch.tensor(qv), torch.tensor(kv), torch.tensor(idx), KGRID, r, inv_t, torch.tensor(doff))
    for got, want in zip(t, (ds, dq, dk)):
        assert np.abs(got.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("down", [2, 4])
def test_gather_backward_restatement_against_autograd(down):
    """doff of tests/match_flow_case.gather_bwd_off against torch.autograd (fp64) of the bilinear gather, offsets in (-3, 3) kept away
    from the sampling kinks; cells clamped at a border get exactly 0 on that axis"""
    g = torch.Generator().manual_seed(down)
    grid, B = (2, 5), 2
    img = torch.rand(B, 3, KGRID[0] * down, KGRID[1] * down, generator=g, dtype=torch.float64)
    idx = torch.tensor([CENTRES, CENTRES[::-1]])
    off = fc.away_from_kinks((torch.rand(B, 10, 2, generator=g) * 2 - 1) * 2.99, down).double()
    off[0, 0], off[0, 1], off[0, 3] = torch.tensor([-1.3, -1.3]), torch.tensor([2.2, -1.6]), torch.tensor([1.3, 2.4])   # corners: out
    dout = torch.randn(B, 3, grid[0] * down, grid[1] * down, generator=g, dtype=torch.float64)
    leaf = off.clone().requires_grad_(True)
    out = fc.t_gather_subcell(img, idx, leaf, grid, KGRID, down)
    assert np.abs(out.detach().numpy() - mc.gather_subcell(img.numpy(), idx.numpy(), off.numpy(), grid, KGRID, down)).max() < 1e-12
    (out * dout).sum().backward()
    want = leaf.grad.numpy()
    got = fc.gather_bwd_off(img.numpy(), idx.numpy(), off.numpy(), dout.numpy(), grid, KGRID, down)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max() and np.abs(want).max() > 0
    assert (got[0, 0] == 0).all() and (got[0, 1] == 0).all() and (got[0, 3] == 0).all()       # every pixel of these cells is clamped on both axes
    t = fc.t_gather_bwd_off(img, idx, off, dout, grid, KGRID, down)
    assert np.abs(t.numpy() - want).max() <= 1e-12 * np.abs(want).max()


def test_offsets_are_moved_off_the_kinks():
    off = torch.tensor([[0.5, 0.25003], [-1.0, 0.3]])
    moved = fc.away_from_kinks(off, 4)
    t = moved.double() * 4
    assert float((t - t.round()).abs().min()) >= 1e-3 and torch.equal(moved[1, 1], off[1, 1])
