"""K53 (the match loss on the match_kernel-3 route), the parts that need no GPU: the arbiter (tests/match_box3_nll_case.py) against the
box decomposition the kernels compute, stated on the host in fp64 with hot_path._unfold3_stats' CPU branch at a 5 x 7 grid
(hot_path._box3_logits itself launches K6 and has no CPU route; the GPU file compares with it); the new entry points in header,
binding table and library; their refusals, which return before any HIP call; the refusal order of ops, hot path and module on CPU
tensors with every out-of-scope flag set; target and weight validation; the reduction with no supervised cell."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_box3_nll_case as mc  # noqa: E402

LSE_BWD, PAIR_FWD, PAIR_BWD = "cocos_box3_lse_bwd_f16x3", "cocos_box3_pair_logit_fwd", "cocos_box3_pair_logit_bwd_pair"
_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


def _box_logits_host(theta, phi, inv_t):
    """z = inv_t a_p b_q (S[p,q] - kc mu_p nu_q), S[p,q] = sum over the 3x3 offsets d of C[p+d, q+d] (zero outside the grid)"""
    from cocosnet_amd.hot_path import _unfold3_stats
    B, C, h, w = theta.shape
    kc = 9.0 * C
    (mu, a), (nu, b) = _unfold3_stats(theta, kc), _unfold3_stats(phi, kc)
    c = torch.einsum("bci,bcj->bij", theta.reshape(B, C, -1), phi.reshape(B, C, -1)).reshape(B, h, w, h, w)
    s = torch.zeros_like(c)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            s[:, y0:y1, x0:x1, y0:y1, x0:x1] += c[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    s = s.reshape(B, h * w, h * w)
    return inv_t * a.unsqueeze(2) * b.unsqueeze(1) * (s - kc * mu.unsqueeze(2) * nu.unsqueeze(1))


def test_arbiter_agrees_with_the_box_decomposition():
    theta, phi = (t.double() for t in mc.diffuse(2, (5, 7), 3, C=16))
    z, zb = mc.logits(theta, phi), _box_logits_host(theta, phi, mc.INV_T)
    assert float((z - zb).abs().max()) < 1e-9 * float(z.abs().max())
    t = mc.targets(2, (5, 7), 1)
    out = mc.arbiter(theta, phi, t)
    flat = t.reshape(2, -1)
    assert not out["match_nll"][flat < 0].any() and not out["back_nll"][flat < 0].any()
    assert bool((out["match_nll"][flat >= 0] > 0).all())
    b, i = 1, 7
    j = int(flat[b, i])
    assert j >= 0
    assert abs(float(out["match_nll"][b, i]) - float(torch.logsumexp(zb[b, i], 0) - zb[b, i, j])) < 1e-9
    assert abs(float(out["back_nll"][b, i]) - float(torch.logsumexp(zb[b, :, j], 0) - zb[b, i, j])) < 1e-9


def test_fp32_arm_of_the_arbiter_stays_inside_the_plain_bound():
    """the arbiter's own fp32 arm against its fp64 self on the diffuse case: outputs within 2e-4, gradients within 1e-3 (max error
    over max reference) — the plain bounds leave room for an fp32 computation"""
    theta, phi = mc.diffuse(2, (5, 7), 11)
    t, w = mc.targets(2, (5, 7), 2), mc.weights(2, (5, 7), 3)
    res = {}
    for dt in (torch.float64, torch.float32):
        th, ph = theta.to(dt).requires_grad_(True), phi.to(dt).requires_grad_(True)
        out = mc.arbiter(th, ph, t, weight=w)
        out["loss_match"].backward()
        res[dt] = (out["match_nll"].detach().double(), out["back_nll"].detach().double(), th.grad.double(), ph.grad.double())
    rel = lambda x, r: float((x - r).abs().max() / r.abs().max())
    errs = [rel(x, r) for x, r in zip(res[torch.float32], res[torch.float64])]
    print("[match_box3_nll] fp32 arm:", errs)
    assert max(errs[:2]) < 2e-4 and max(errs[2:]) < 1e-3


def test_header_table_library_and_exports(hip_lib):
    from cocosnet_amd import _lib, build, correspondence, hot_path, ops
    for name in (LSE_BWD, PAIR_FWD, PAIR_BWD):
        assert _lib.PROTOTYPES.get(name, ("",))[0] == "int", f"{name} is not declared in cocos_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    assert hasattr(hip_lib, "cocos_box3_lse_bwd_colpart_bytes")
    assert "box3_lse_bwd_f16x3.hip" in build.HIP_SOURCES and os.path.exists(os.path.join(build.CSRC_DIR, "box3_lse_bwd_f16x3.hip"))
    assert list(_lib._SIGNATURES[LSE_BWD][1]) == [_P] * 14 + [_I] * 5 + [_F] * 2 + [_I, _P]
    assert list(_lib._SIGNATURES[PAIR_FWD][1]) == [_P] * 9 + [_I] * 6 + [_F, _P]
    assert list(_lib._SIGNATURES[PAIR_BWD][1]) == [_P] * 10 + [_I] * 6 + [_F, _P]
    # the column partials of the existing backward plus one maximum per wave
    assert hip_lib.cocos_box3_lse_bwd_colpart_bytes(2, 256, 256) == (2 * 2 * 2 * 256 + 2 * 2 * 4) * 4
    assert hip_lib.cocos_box3_lse_bwd_colpart_bytes(0, 256, 256) == 0
    for fn in (ops.box3_lse, ops.box3_pair_logits, ops.box3_gather_keys, hot_path.correspondence_nll_box3):
        assert callable(fn)
    assert callable(correspondence.NoVGGCorrespondence.match_loss_box3)


def test_abi_refusals_need_no_gpu(hip_lib):
    one, f = ctypes.c_void_p(16), ctypes.c_float
    err = hip_lib.cocos_last_error_string
    names = ["t", "mu", "a", "nu", "b", "lse", "g_lse", "G", "dmu", "da", "dnu", "db", "colpart", "gmax"]

    def call(B=1, Nq=256, Nk=256, h=4, w=64, scale=100.0, flags=0, **ptr):
        return hip_lib.cocos_box3_lse_bwd_f16x3(*[ptr.get(n, one) for n in names], B, Nq, Nk, h, w, f(2304.0), f(scale), flags, None)

    for flags in (4, 8, 7, -1):
        assert call(flags=flags) == -1 and b"flags" in err(), flags
    for n in names:
        if n != "g_lse":
            assert call(**{n: None}) == -1 and b"null" in err(), n
    assert call(g_lse=None, Nq=100) == -2                                   # a null g_lse is legal: the next refusal answers
    assert call(B=0) == -1 and call(scale=0.0) == -1
    for shape in (dict(Nq=100, Nk=100, h=10, w=10), dict(Nq=128, Nk=128, h=2, w=64), dict(Nq=256, Nk=512), dict(h=8, w=32),
                  dict(Nq=35, Nk=35, h=5, w=7)):
        kw = dict(dict(Nq=256, Nk=256, h=4, w=64), **shape)
        assert not hip_lib.cocos_box3_fused_supported(kw["Nq"], kw["Nk"], 1, kw["h"], kw["w"])
        assert call(**kw) == -2 and b"64- or 128-wide" in err(), shape
    for n in ("t", "G", "nu", "b", "colpart"):
        assert call(**{n: ctypes.c_void_p(24)}) == -1 and b"aligned" in err(), n
    # the smallest 64- and 128-wide grids of the GPU tests are supported shapes
    assert hip_lib.cocos_box3_fused_supported(256, 256, 1, 4, 64) and hip_lib.cocos_box3_fused_supported(256, 256, 1, 2, 128)
    assert hip_lib.cocos_box3_fused_supported(5120, 5120, 1, 40, 128)

    def pair(B=1, K=256, **ptr):
        return hip_lib.cocos_box3_pair_logit_fwd(*[ptr.get(n, one) for n in ("th", "ph", "mu", "a", "nu", "b", "idx", "z", "c")], B, K, 2, 3,
                                                 3, 2, f(100.0), None)

    def pair_bwd(B=1, K=256, **ptr):
        return hip_lib.cocos_box3_pair_logit_bwd_pair(*[ptr.get(n, one) for n in ("idx", "c", "a", "nu", "b", "dz", "g", "hb", "dmu", "da")],
                                                      B, K, 2, 3, 3, 2, f(100.0), None)

    for n in ("th", "ph", "mu", "a", "nu", "b", "idx", "z", "c"):
        assert pair(**{n: None}) == -1 and b"null" in err(), n
    for n in ("idx", "c", "a", "nu", "b", "dz", "g"):
        assert pair_bwd(**{n: None}) == -1 and b"null" in err(), n
    for fn in (pair, pair_bwd):
        assert fn(K=128) == -2 and b"K == 256" in err()
        assert fn(B=0) == -1
    assert pair(th=ctypes.c_void_p(24)) == -1 and b"aligned" in err()


def test_ops_refuse_in_the_family_order(hip_lib, monkeypatch):
    """TypeError / ValueError of the arguments, then the CPU tensors ("no CPU fallback"), before the flavour and the shapes"""
    from cocosnet_amd import _lib, ops
    B, h, w = 1, 4, 64
    N = h * w
    t, s = torch.zeros(B * N * N), torch.ones(B, N)
    with pytest.raises(TypeError, match="box3_lse"):
        ops.box3_lse(None, s, s, s, s, h, w, 2304.0, 100.0)
    with pytest.raises(TypeError, match="box3_lse"):
        ops.box3_lse(t.double(), s, s, s, s, h, w, 2304.0, 100.0)
    for bad in (dict(h=5), dict(t=t[:-1]), dict(a=s[:, :-1]), dict(scale=0.0)):
        kw = dict(dict(t=t, a=s, h=h, scale=100.0), **bad)
        with pytest.raises(ValueError, match="box3_lse"):
            ops.box3_lse(kw["t"], s, kw["a"], s, s, kw["h"], w, 2304.0, kw["scale"])
    for prec in ("f16x3", "fp32"):                                            # the device before the flavour
        monkeypatch.setattr(ops, "PRECISION", prec)
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            ops.box3_lse(t, s, s, s, s, h, w, 2304.0, 100.0)
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    s35 = torch.ones(1, 35)                                                   # a 5 x 7 grid is a valid argument: the device answers first
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.box3_lse(torch.zeros(35 * 35), s35, s35, s35, s35, 5, 7, 2304.0, 100.0)

    theta, phi = torch.randn(2, 256, 2, 3), torch.randn(2, 256, 3, 2)
    st = torch.ones(2, 6)
    idx = torch.zeros(2, 6, dtype=torch.int64)
    name = "box3_pair_logits"
    with pytest.raises(TypeError, match=name):
        ops.box3_pair_logits(theta, phi, st, st, st, st, idx.float(), 100.0)
    with pytest.raises(TypeError, match=name):
        ops.box3_pair_logits(theta, phi, st, st, st, st, None, 100.0)
    for args in ((theta[0], phi, st, st, st, st, idx), (theta, phi[:1], st, st, st, st, idx), (theta[:, :128], phi[:, :128], st, st, st, st, idx),
                 (theta, phi, st[:, :5], st, st, st, idx), (theta, phi, st, st, st, st, idx[:, :5])):
        with pytest.raises(ValueError, match=name):
            ops.box3_pair_logits(*args, 100.0)
    with pytest.raises(ValueError, match="inv_temperature"):
        ops.box3_pair_logits(theta, phi, st, st, st, st, idx, 0.0)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.box3_pair_logits(theta, phi, st, st, st, st, idx - 3, 100.0)      # negative entries are legal
    with pytest.raises(TypeError, match="box3_gather_keys"):
        ops.box3_gather_keys(st, idx.float())
    with pytest.raises(ValueError, match="box3_gather_keys"):
        ops.box3_gather_keys(st[0], idx)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.box3_gather_keys(st, idx)


def _cfg(**over):
    from cocosnet_amd.hot_path import HotPathConfig
    return HotPathConfig(**dict(dict(match_kernel=3, PONO_C=True, down=4), **over))


def test_hot_path_scope_targets_and_weights(hip_lib, monkeypatch):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import correspondence_nll_box3 as nll
    theta, phi = torch.randn(2, 256, 2, 3), torch.randn(2, 256, 2, 3)
    t = torch.zeros(2, 2, 3, dtype=torch.int64)
    for over in (dict(match_kernel=1), dict(PONO_C=False), dict(warp_patch=True), dict(warp_bilinear=True), dict(warp_cycle_w=1.0),
                 dict(two_cycle=True), dict(warp_mask_losstype="cycle")):
        with pytest.raises(ValueError, match="match_loss_box3"):
            nll(None, None, t, _cfg(**over))                                  # before any tensor is looked at
    with pytest.raises(ValueError, match="match_loss_box3: symmetric"):
        nll(theta, phi, t, _cfg(), symmetric=1)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="match_loss_box3: COCOS_PRECISION"):
        nll(None, None, t, _cfg())
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    with pytest.raises(ValueError, match="match_loss_box3: a prepared exemplar"):
        nll(theta, phi, t, _cfg(), exemplar=object())
    with pytest.raises(ValueError, match="match_loss_box3: needs 256 channels"):
        nll(theta[:, :128], phi[:, :128], t, _cfg())
    with pytest.raises(TypeError, match="match_loss_box3: target"):
        nll(theta, phi, t.float(), _cfg())
    with pytest.raises(ValueError, match="match_loss_box3: target is"):
        nll(theta, phi, t[:, :1], _cfg())
    bad = t.clone()
    bad[0, 1, 2] = 6
    with pytest.raises(ValueError, match="below 6"):
        nll(theta, phi, bad, _cfg())
    w = torch.ones(2, 2, 3)
    with pytest.raises(TypeError, match="match_loss_box3: weight"):
        nll(theta, phi, t, _cfg(), weight=w.double())
    with pytest.raises(ValueError, match="match_loss_box3: weight is"):
        nll(theta, phi, t, _cfg(), weight=w[:, :1])
    for v in (-0.5, float("nan"), float("inf")):
        badw = w.clone()
        badw[1, 0, 0] = v
        with pytest.raises(ValueError, match="match_loss_box3: weight must be finite and >= 0"):
            nll(theta, phi, t, _cfg(), weight=badw)
    with pytest.raises(ValueError, match="requires a gradient"):
        nll(theta, phi, t, _cfg(), weight=w.clone().requires_grad_(True))
    with pytest.raises(_lib.CocosHipError, match="match_loss_box3.*no CPU fallback"):      # everything valid (a 2 x 3 grid is a shape
        nll(theta, phi, t - 1, _cfg(), weight=w)                                           # refusal): the device is the next refusal


def test_match_loss_messages_are_unchanged():
    """_nll_targets is shared: match_loss keeps its own name in every message"""
    from cocosnet_amd.hot_path import _nll_targets
    with pytest.raises(TypeError, match="^match_loss: target must be"):
        _nll_targets(torch.zeros(1, 2, 3), None, 1, 2, 3, 6)
    with pytest.raises(ValueError, match="^match_loss: weight is"):
        _nll_targets(torch.zeros(1, 2, 3, dtype=torch.int64), torch.ones(1, 2, 2), 1, 2, 3, 6)


def test_module_refuses_before_the_network_runs(hip_lib, monkeypatch):
    from cocosnet_amd import correspondence as cc
    assert hasattr(cc.NoVGGCorrespondence, "match_loss_box3")
    x, seg = torch.zeros(1, 3, 32, 32), torch.zeros(1, 7, 32, 32)
    t = torch.zeros(1, 8, 8, dtype=torch.int64)
    for over in (dict(match_kernel=1), dict(PONO_C=False), dict(warp_patch=True), dict(warp_bilinear=True), dict(warp_cycle_w=1.0)):
        net = cc.NoVGGCorrespondence(cc.ade20k_options(crop_size=32, semantic_nc=7, **dict(dict(match_kernel=3), **over)))
        monkeypatch.setattr(net, "project", lambda *a, **kw: pytest.fail("the network ran"))
        with pytest.raises(ValueError, match="match_loss_box3"):
            net.match_loss_box3(x, x, seg, seg, t)
    net = cc.NoVGGCorrespondence(cc.ade20k_options(crop_size=32, semantic_nc=7, match_kernel=3))
    monkeypatch.setattr(net, "project", lambda *a, **kw: pytest.fail("the network ran"))
    with pytest.raises(ValueError, match="match_loss_box3: symmetric"):
        net.match_loss_box3(x, x, seg, seg, t, symmetric=None)
    with pytest.raises(ValueError, match="match_loss_box3: ref_img"):
        net.match_loss_box3(None, x, seg, None, t)
    with pytest.raises(TypeError, match="match_loss_box3: target"):
        net.match_loss_box3(x, x, seg, seg, t.float())
    with pytest.raises(ValueError, match="match_loss: match_kernel 3"):      # match_loss itself still refuses this route
        net.match_loss(x, x, seg, seg, t)


def test_loss_reduction_with_no_supervised_cell():
    from cocosnet_amd.hot_path import nll_reduce
    r = torch.tensor([[1.0, 2.0, 4.0]], requires_grad=True)
    c = torch.tensor([[0.5, 0.25, 8.0]], requires_grad=True)
    loss = nll_reduce(r, c, torch.full((1, 3), -1), None, True)
    assert float(loss) == 0.0
    loss.backward()
    assert not r.grad.any() and not c.grad.any()
    out = mc.arbiter(*(x.double() for x in mc.diffuse(1, (3, 4), 5, C=8)), mc.targets(1, (3, 4), 0, "all_negative"))
    assert float(out["loss_match"]) == 0.0 and not out["match_nll"].any() and not out["back_nll"].any()
