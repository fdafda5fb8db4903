"""K52 (the trainable sub-cell flow warp on the match_kernel-3 route), the parts that need no GPU: the entry points in header, binding
table and library, their argument checks (which return before any HIP call), the Python-side refusals of ops.box3_soft_match_offset,
hot_path.correspondence_flow_box3 and NoVGGCorrespondence.flow_warp_box3 in their order, the refusals flow_warp and match(refine=1)
keep for match_kernel 3, and the arbiter of the GPU tests (tests/match_box3_flow_case.py) checked by hand and against autograd."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box3_sparse_case as bc  # noqa: E402
import match_box3_flow_case as xc  # noqa: E402
import match_refine_case as mc  # noqa: E402

NEW_SYMBOLS = ("cocos_box3_match_refine_fwd", "cocos_box3_match_refine_bwd_pair", "cocos_box3_match_refine_bwd_theta",
               "cocos_box3_match_refine_bwd_key")


def test_header_table_and_library_carry_the_entry_points(hip_lib):
    from cocosnet_amd import _lib, build
    for name in NEW_SYMBOLS:
        assert _lib.PROTOTYPES.get(name, ("",))[0] == "int", f"{name} is not declared in cocos_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(hip_lib, name)
    assert "box3_pair.hip" in build.HIP_SOURCES
    assert os.path.exists(os.path.join(build.CSRC_DIR, "box3_pair.hip"))


def test_argument_validation_needs_no_gpu(hip_lib):
    """null pointers (-1), an empty grid or batch (-1), radius outside 1..3 (-1), a non-positive inv_temperature (-1), K != 256 (-2),
    B Nq W past the 32-bit tables (-2), misaligned rows (-1): all before any HIP call"""
    one, f = ctypes.c_void_p(16), ctypes.c_float
    err = hip_lib.cocos_last_error_string
    dims = lambda K=256, g=(4, 4, 4, 4), r=2, B=1: (B, K) + tuple(g) + (r,)
    fwd = lambda p=(one,) * 10, inv_t=100.0, **kw: hip_lib.cocos_box3_match_refine_fwd(*p, *dims(**kw), f(inv_t), None)
    pair = lambda p=(one,) * 10, inv_t=100.0, **kw: hip_lib.cocos_box3_match_refine_bwd_pair(*p, *dims(**kw), f(inv_t), None)
    theta = lambda p=(one,) * 4, **kw: hip_lib.cocos_box3_match_refine_bwd_theta(*p, *dims(**kw), None)
    key = lambda p=(one,) * 9, **kw: hip_lib.cocos_box3_match_refine_bwd_key(*p, *dims(**kw), None)
    for call in (fwd, pair, theta, key):
        assert call(K=128) == -2 and b"K == 256" in err()
        for bad in (0, 4, -1):
            assert call(r=bad) == -1 and f"radius={bad}".encode() in err()
        assert call(B=0) == -1 and b"non-positive size" in err()
        for i in range(4):                                     # an empty content or exemplar grid
            assert call(g=tuple(0 if n == i else 4 for n in range(4))) == -1 and b"non-positive size" in err()
        assert call(g=(8192, 8192, 4, 4), r=3) == -2 and b"32-bit tables" in err()          # 2^26 queries x 49 slots
        assert call(B=2, g=(4, 4, 32768, 32768), r=1) == -2 and b"32-bit tables" in err()     # 2^31 keys
    for call in (fwd, pair):
        for bad in (0.0, -1.0):
            assert call(inv_t=bad) == -1 and b"inv_temperature" in err()
    for i in range(10):
        assert fwd(p=(one,) * i + (None,) + (one,) * (9 - i)) == -1 and b"null" in err()
    for i in range(7):          # (hb, dmu, da — the last three pointers — may be null)
        assert pair(p=(one,) * i + (None,) + (one,) * (9 - i)) == -1 and b"null" in err()
    for i in range(4):
        assert theta(p=(one,) * i + (None,) + (one,) * (3 - i)) == -1 and b"null" in err()
    for i in (4, 5):            # entries, offsets
        assert key(p=(one,) * i + (None,) + (one,) * (8 - i)) == -1 and b"null" in err()
    assert key(p=(one,) * 6 + (None,) * 3) == -1 and b"null" in err()                                   # no output at all
    assert key(p=(None,) + (one,) * 8) == -1 and b"dph_t needs" in err()                                # dph_t without the theta rows
    assert key(p=(one, None) + (one,) * 7) == -1 and b"dph_t needs" in err()                            # dph_t without g
    assert key(p=(one, None, one, one, one, one, None, one, one)) == -1 and b"dnu needs" in err()       # dnu without g
    assert key(p=(one,) * 3 + (None,) + (one,) * 5) == -1 and b"dnu needs" in err()                     # dnu without mu
    assert key(p=(one,) * 2 + (None,) + (one,) * 6) == -1 and b"db needs" in err()                      # db without hb
    odd = ctypes.c_void_p(24)
    assert fwd(p=(odd,) + (one,) * 9) == -1 and b"aligned" in err()
    assert fwd(p=(one, odd) + (one,) * 8) == -1 and b"aligned" in err()
    assert theta(p=(odd,) + (one,) * 3) == -1 and b"aligned" in err()
    assert theta(p=(one,) * 3 + (odd,)) == -1 and b"aligned" in err()
    assert key(p=(odd,) + (one,) * 8) == -1 and b"aligned" in err()
    assert key(p=(one,) * 6 + (odd,) + (one,) * 2) == -1 and b"aligned" in err()


def _op_inputs(B=1, grid=(2, 4), kgrid=(3, 4)):
    theta, phi = bc.features(B, grid, kgrid, 11)
    (mu, a), (nu, b) = bc.stats(theta), bc.stats(phi)
    return [theta, phi, mu, a, nu, b, torch.zeros(B, grid[0] * grid[1], dtype=torch.int64), grid, kgrid]


def test_op_refuses_on_the_host_in_order(hip_lib):
    """grid, kgrid, radius, inv_rt; then the shapes, the channels and the statistics; then TypeError for the idx dtype and ValueError for
    its size; then "no CPU fallback" — every message names the function"""
    from cocosnet_amd import _lib, ops
    args = _op_inputs()
    call = lambda a, inv_rt=100.0, radius=1: ops.box3_soft_match_offset(*a, inv_rt, radius)
    swap = lambda i, t, base=None: (base or args)[:i] + [t] + (base or args)[i + 1:]
    theta, phi, mu, a, nu, b, idx, grid, kgrid = args
    bad_idx = swap(6, idx.float())
    for bad in ((2, 0), (2,), 8, (2.0, 4)):
        with pytest.raises(ValueError, match="box3_soft_match_offset: grid"):
            call(swap(7, bad, bad_idx))                                                # the grid comes before everything else
        with pytest.raises(ValueError, match="box3_soft_match_offset: kgrid"):
            call(swap(8, bad, bad_idx))
    for bad in (0, 4, 1.0, True, None):
        with pytest.raises(ValueError, match="box3_soft_match_offset: radius"):
            call(bad_idx, radius=bad)
    for bad in (0.0, -5.0):
        with pytest.raises(ValueError, match="box3_soft_match_offset: inv_rt"):
            call(bad_idx, inv_rt=bad)
    for bad in (swap(0, theta[0], bad_idx), swap(0, theta[:, :, :1], bad_idx), swap(1, phi[:, :, :2], bad_idx),
                swap(0, torch.randn(2, 256, 2, 4), bad_idx), swap(7, (4, 2), bad_idx), swap(8, (4, 3), bad_idx)):
        with pytest.raises(ValueError, match="box3_soft_match_offset: (expected|shape mismatch)"):
            call(bad)
    with pytest.raises(ValueError, match="box3_soft_match_offset: needs 256 channels"):
        call([theta[:, :128], phi[:, :128]] + bad_idx[2:])
    for i, what in ((2, "mu"), (3, "a"), (4, "nu"), (5, "b")):                         # statistics of the wrong size, before idx
        with pytest.raises(ValueError, match=rf"box3_soft_match_offset: {what} is"):
            call(swap(i, args[i][:, :5], bad_idx))
    for bad in (idx.float(), idx.to(torch.int16), idx.bool()):
        with pytest.raises(TypeError, match="box3_soft_match_offset: idx"):
            call(swap(6, bad))
    with pytest.raises(ValueError, match="box3_soft_match_offset: idx is"):
        call(swap(6, idx[:, :7]))
    with pytest.raises(_lib.CocosHipError, match="box3_soft_match_offset.*no CPU fallback"):
        call(args)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):                   # flat positions and a [B,fh,fw] table are taken
        call([theta.reshape(1, 256, 8), phi.reshape(1, 256, 12)] + args[2:6] + [idx.reshape(1, 2, 4).to(torch.int32), grid, kgrid])


OUT_OF_SCOPE = [(dict(match_kernel=1), "match_kernel 1"), (dict(PONO_C=False), "PONO_C"), (dict(warp_patch=True), "warp_patch"),
                (dict(warp_bilinear=True), "warp_bilinear"), (dict(warp_cycle_w=1.0), "cycle"), (dict(two_cycle=True), "cycle"),
                (dict(warp_mask_losstype="cycle"), "cycle")]


class _NoTensor:
    """stands where theta / phi would: the scope is checked before any tensor is looked at (only the width is read)"""
    shape = (1, 256, 2, 2)

    def __getattr__(self, name):
        pytest.fail(f"a tensor was looked at ({name}) before the scope was checked")


def _hot_inputs():
    g = torch.Generator().manual_seed(5)
    return torch.randn(1, 256, 2, 2, generator=g), torch.randn(1, 256, 2, 2, generator=g), torch.rand(1, 3, 8, 8, generator=g)


@pytest.mark.parametrize("flags,word", OUT_OF_SCOPE, ids=[w + "-" + "-".join(f) for f, w in OUT_OF_SCOPE])
def test_correspondence_flow_box3_names_what_is_out_of_scope(hip_lib, flags, word):
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_flow_box3
    cfg = HotPathConfig(**dict(dict(match_kernel=3, PONO_C=True, down=4), **flags))
    with pytest.raises(ValueError, match=word) as e:
        correspondence_flow_box3(_NoTensor(), _NoTensor(), _hot_inputs()[2], cfg, radius=0)      # (the flags come before the radius)
    assert str(e.value).startswith("correspondence_flow_box3:") and "match_kernel 3 route" in str(e.value)


def test_correspondence_flow_box3_other_refusals_in_order(hip_lib, monkeypatch):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_flow_box3
    theta, phi, ref_img = _hot_inputs()
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    no = _NoTensor()
    with pytest.raises(ValueError, match="correspondence_flow_box3: a prepared exemplar"):     # before the width, the radius, the temperature
        correspondence_flow_box3(no, no, ref_img, cfg, radius=0, refine_temperature=-1.0, exemplar=object())
    narrow = type("Narrow", (_NoTensor,), {"shape": (1, 128, 2, 2)})()
    with pytest.raises(ValueError, match="correspondence_flow_box3: needs 256 channels"):
        correspondence_flow_box3(narrow, narrow, ref_img, cfg, radius=0)
    for bad in (0, 4, 1.0, True, None):
        with pytest.raises(ValueError, match="correspondence_flow_box3: radius"):
            correspondence_flow_box3(no, no, ref_img, cfg, radius=bad, refine_temperature=-1.0)
    for bad in (0, -0.1, "cold", True):
        with pytest.raises(ValueError, match="correspondence_flow_box3: refine_temperature"):
            correspondence_flow_box3(no, no, ref_img, cfg, refine_temperature=bad)
    with pytest.raises(ValueError, match="correspondence_flow_box3: ref_img"):
        correspondence_flow_box3(theta, phi, ref_img[:, :, :4], cfg)
    with pytest.raises(ValueError, match="correspondence_flow_box3: ref_img requires a gradient"):
        correspondence_flow_box3(theta, phi, ref_img.clone().requires_grad_(True), cfg)
    with pytest.raises(_lib.CocosHipError, match="correspondence_flow_box3.*no CPU fallback"):     # in scope: the tensors are refused
        correspondence_flow_box3(theta, phi, ref_img, cfg, radius=3, refine_temperature=0.02)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="COCOS_PRECISION=fp32"):
        correspondence_flow_box3(no, no, ref_img, cfg)


def test_module_refuses_before_the_network_runs_and_the_old_refusals_stay(hip_lib, monkeypatch):
    from cocosnet_amd import correspondence as cc
    g = torch.Generator().manual_seed(3)
    onehot = lambda: torch.zeros(1, 7, 64, 64).scatter_(1, torch.randint(0, 7, (1, 1, 64, 64), generator=g), 1.0)
    ref_img, seg, ref_seg = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1, onehot(), onehot()

    def net_for(**flags):
        opt = cc.ade20k_options(**dict(dict(crop_size=64, semantic_nc=7, match_kernel=3), **flags))
        torch.manual_seed(0)
        net = cc.NoVGGCorrespondence(opt).eval()
        monkeypatch.setattr(net, "project", lambda *a, **k: pytest.fail("project() ran for a call that is out of scope"))
        return net

    assert callable(getattr(cc.NoVGGCorrespondence, "flow_warp_box3", None))
    for flags, word in OUT_OF_SCOPE:
        with pytest.raises(ValueError, match=word) as e:
            net_for(**flags).flow_warp_box3(ref_img, None, seg, ref_seg)
        assert str(e.value).startswith("flow_warp_box3:")
    net = net_for()
    for bad in (0, 4, 1.0, True):
        with pytest.raises(ValueError, match="flow_warp_box3: radius"):
            net.flow_warp_box3(ref_img, None, seg, ref_seg, radius=bad)
    with pytest.raises(ValueError, match="flow_warp_box3: refine_temperature"):
        net.flow_warp_box3(ref_img, None, seg, ref_seg, refine_temperature=0.0)
    with pytest.raises(ValueError, match="flow_warp_box3: ref_img and ref_seg_map are required"):
        net.flow_warp_box3(None, None, seg, ref_seg)
    # the members built for match_kernel 1 keep refusing this route: the new method is no new branch of theirs
    with pytest.raises(ValueError, match="match_kernel 3"):
        net.flow_warp(ref_img, None, seg, ref_seg)
    with pytest.raises(ValueError, match="match_kernel 3"):
        net.match(ref_img, seg, ref_seg, refine=1)
    monkeypatch.setattr(net, "inter_channels", 128)
    with pytest.raises(ValueError, match="flow_warp_box3: needs 256 channels"):
        net.flow_warp_box3(ref_img, None, seg, ref_seg)


# ---------------------------------------------------------------------------------------------------------------- the arbiter, by hand
def _z_dense(theta, phi, inv_rt):
    """every logit [B,Nq,Nk] of the unfold formulation"""
    return inv_rt * torch.einsum("bci,bcj->bij", bc.unit_unfolded(theta), bc.unit_unfolded(phi))


def test_arbiter_on_a_one_cell_exemplar_grid():
    """1 x 1 exemplar grid: the window holds the centre alone at every radius — offset 0, lse_win = z"""
    theta, phi = (t.double() for t in bc.features(2, (2, 3), (1, 1), 3, C=8))
    z = _z_dense(theta, phi, 10.0)[:, :, 0]
    for r in (1, 2, 3):
        off, lse, p, inside = xc.arbiter(theta, phi, torch.tensor([[0, 5, -3, 0, 0, 9]] * 2), r, 10.0, parts=True)
        assert int(inside.sum()) == 2 * 6 and bool((off == 0).all())
        assert float((lse - z).abs().max()) < 1e-12


def test_arbiter_corner_centre_has_four_keys():
    """r = 1 around the corner key 0 of a 3 x 4 grid: the keys (0,0), (0,1), (1,0), (1,1) in slots 4, 5, 7, 8; the soft-argmax by hand"""
    theta, phi = (t.double() for t in bc.features(1, (2, 2), (3, 4), 4, C=8))
    off, lse, p, inside = xc.arbiter(theta, phi, torch.zeros(1, 4, dtype=torch.int64), 1, 10.0, parts=True)
    assert inside[0, 0].tolist() == [False] * 4 + [True, True, False, True, True]
    assert [k for k, _, _ in mc.window(0, (3, 4), 1)] == [0, 1, 4, 5]
    z = _z_dense(theta, phi, 10.0)[0, :, [0, 1, 4, 5]]                                 # [Nq,4]
    w = torch.softmax(z, dim=-1)
    assert float((off[0, :, 0] - (w[:, 1] + w[:, 3])).abs().max()) < 1e-12            # dx = 1 for keys 1 and 5
    assert float((off[0, :, 1] - (w[:, 2] + w[:, 3])).abs().max()) < 1e-12            # dy = 1 for keys 4 and 5
    assert float((lse[0] - torch.logsumexp(z, dim=-1)).abs().max()) < 1e-12
    assert float(p[0][~inside[0]].abs().max()) == 0.0


def test_arbiter_last_column_takes_no_tap_from_a_next_row():
    """1 x 3 exemplar grid, centre in the last column: the window is keys 1 and 2 (nothing wraps), and the logits are the tap sums over
    2-D coordinates (bc.tap_R, loops with both in-grid tests)"""
    theta, phi = (t.double() for t in bc.features(1, (1, 3), (1, 3), 6, C=8))
    idx = torch.full((1, 3), 2)
    off, lse, p, inside = xc.arbiter(theta, phi, idx, 1, 10.0, parts=True)
    assert inside[0, 0].tolist() == [False, False, False, True, True, False, False, False, False]
    (mu, a), (nu, b) = bc.stats(theta), bc.stats(phi)
    z_tap = 10.0 * a.unsqueeze(2) * b.unsqueeze(1) * (bc.tap_R(theta, phi) - 72.0 * mu.unsqueeze(2) * nu.unsqueeze(1))
    assert float((lse[0] - torch.logsumexp(z_tap[0][:, 1:], dim=-1)).abs().max()) < 1e-12
    assert float((off[0, :, 0] + torch.softmax(z_tap[0][:, 1:], dim=-1)[:, 0]).abs().max()) < 1e-12      # dx = -1 for key 1
    # on a 2 x 3 grid key 2 = (0, 2) has key 3 = (1, 0) as its flat successor: the tap d = (0, 1) must not reach it
    theta2, phi2 = (t.double() for t in bc.features(1, (1, 3), (2, 3), 7, C=8))
    (mu, a), (nu, b) = bc.stats(theta2), bc.stats(phi2)
    z_tap = 10.0 * a.unsqueeze(2) * b.unsqueeze(1) * (bc.tap_R(theta2, phi2) - 72.0 * mu.unsqueeze(2) * nu.unsqueeze(1))
    off2, lse2, _, inside2 = xc.arbiter(theta2, phi2, idx, 1, 10.0, parts=True)
    assert inside2[0, 0].tolist() == [False, False, False, True, True, False, True, True, False]       # keys 1, 2, 4, 5
    assert float((lse2[0] - torch.logsumexp(z_tap[0][:, [1, 2, 4, 5]], dim=-1)).abs().max()) < 1e-12


def test_arbiter_with_statistics_is_the_arbiter():
    theta, phi = (t.double() for t in bc.features(2, (5, 7), (3, 6), 8, C=8))
    idx = xc.centre_table(2, (5, 7), (3, 6), 9)
    (mu, a), (nu, b) = bc.stats(theta), bc.stats(phi)
    for r in (1, 2, 3):
        want, got = xc.arbiter(theta, phi, idx, r, 10.0), xc.arbiter_stats(theta, phi, mu, a, nu, b, idx, r, 10.0)
        assert all(float((x - y).abs().max()) < 1e-10 for x, y in zip(want, got))
        assert float(want[0].abs().max()) <= r


def test_arbiter_gradients_agree_with_autograd():
    """the backward the kernels implement, written out in fp64 — dz_s = p_s ((dx_s - o_x) doff_x + (dy_s - o_y) doff_y), then
    g = dz inv_rt a b on R, da = sum dz inv_rt b c, dmu = -kc sum g nu, and the key side scattered — against torch.autograd of
    arbiter_stats"""
    import match_flow_case as fc
    import torch.nn.functional as F
    B, grid, kgrid, r, inv_rt, C = 2, (3, 4), (4, 3), 2, 10.0, 8
    theta, phi = (t.double() for t in bc.features(B, grid, kgrid, 12, C=C))
    idx = xc.centre_table(B, grid, kgrid, 13)
    stats = [t.detach().clone().requires_grad_(True) for pair in (bc.stats(theta), bc.stats(phi)) for t in pair]
    mu, a, nu, b = stats
    th, ph = theta.clone().requires_grad_(True), phi.clone().requires_grad_(True)
    off, _ = xc.arbiter_stats(th, ph, mu, a, nu, b, idx, r, inv_rt)
    doff = torch.randn(off.shape, generator=torch.Generator().manual_seed(14)).double()
    grads = torch.autograd.grad(off, [th, ph, mu, a, nu, b], doff)
    # by hand
    keys, inside, dx, dy = fc.t_window(idx, kgrid, r)
    uq, uk = F.unfold(theta, 3, padding=1), F.unfold(phi, 3, padding=1)                # [B,9C,N]
    kc = 9.0 * C
    pick = lambda t: torch.stack([t[n][keys[n]] for n in range(B)])
    c = torch.einsum("bci,biwc->biw", uq, bc.gather(uk, keys)) - kc * mu.detach().unsqueeze(-1) * pick(nu.detach())
    z = (inv_rt * a.detach().unsqueeze(-1) * pick(b.detach()) * c).masked_fill(~inside, float("-inf"))
    p = torch.softmax(z, dim=-1)
    o = torch.stack(((p * dx).sum(-1), (p * dy).sum(-1)), dim=-1)
    dz = p * ((dx - o[..., :1]) * doff[..., :1] + (dy - o[..., 1:]) * doff[..., 1:])
    g = dz * inv_rt * a.detach().unsqueeze(-1) * pick(b.detach())
    hb = dz * inv_rt * a.detach().unsqueeze(-1) * c
    dmu = -kc * (g * pick(nu.detach())).sum(-1)
    da = (dz * inv_rt * pick(b.detach()) * c).sum(-1)
    dnu, db, duk = torch.zeros_like(nu), torch.zeros_like(b), torch.zeros_like(uk)
    for n in range(B):
        dnu[n].index_add_(0, keys[n].reshape(-1), (-kc * g[n] * mu.detach()[n].unsqueeze(-1)).reshape(-1))
        db[n].index_add_(0, keys[n].reshape(-1), hb[n].reshape(-1))
        duk[n].index_add_(1, keys[n].reshape(-1), (g[n].unsqueeze(0) * uq[n].unsqueeze(-1)).reshape(9 * C, -1))
    duq = torch.einsum("biw,biwc->bci", g, bc.gather(uk, keys))
    dth = F.fold(duq, grid, 3, padding=1)
    dph = F.fold(duk, kgrid, 3, padding=1)
    for name, x, y in zip(("dtheta", "dphi", "dmu", "da", "dnu", "db"), grads, (dth, dph, dmu, da, dnu.detach(), db.detach())):
        assert float((x - y).abs().max()) <= 1e-10 * max(1.0, float(x.abs().max())), name
    assert float(grads[0].abs().max()) > 0 and float(grads[4].abs().max()) > 0
