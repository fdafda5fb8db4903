"""K51 (the trainable k-sparse warp on the match_kernel-3 route), the parts that need no GPU: the entry points in header, binding table
and library, their argument checks (which return before any HIP call), the Python-side refusals of ops.box3_sparse_softmax_warp,
hot_path.correspondence_sparse_box3 and NoVGGCorrespondence.sparse_warp_box3, and the two host-side checks of the definition: the fp64
arbiter of the GPU tests at full support against the dense restatement, and the kernels' tap formula against the unfolded product."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box3_sparse_case as bc  # noqa: E402

NEW_SYMBOLS = ("cocos_box3_sparse_softmax_warp_fwd", "cocos_box3_sparse_softmax_warp_bwd_pair", "cocos_box3_sparse_softmax_warp_bwd_theta",
               "cocos_box3_sparse_softmax_warp_bwd_key")


def test_header_table_and_library_carry_the_entry_points(hip_lib):
    from cocosnet_amd import _lib, build
    for name in NEW_SYMBOLS:
        assert _lib.PROTOTYPES.get(name, ("",))[0] == "int", f"{name} is not declared in cocos_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(hip_lib, name)
    assert "box3_pair.hip" in build.HIP_SOURCES
    assert os.path.exists(os.path.join(build.CSRC_DIR, "box3_pair.hip"))


def test_argument_validation_needs_no_gpu(hip_lib):
    """null pointers (-1), an empty grid or batch (-1), k outside 1..min(8, Nk) (-1), K != 256 (-2), misaligned rows (-1): all before
    any HIP call"""
    one, f = ctypes.c_void_p(16), ctypes.c_float
    err = hip_lib.cocos_last_error_string
    dims = lambda K=256, g=(4, 4, 4, 4), k=4, B=1: (B, K) + tuple(g)
    fwd = lambda p=(one,) * 11, Cv=3, k=4, **kw: hip_lib.cocos_box3_sparse_softmax_warp_fwd(*p, *dims(k=k, **kw), Cv, k, f(100.0), None)
    pair = lambda p=(one,) * 12, Cv=3, k=4, **kw: hip_lib.cocos_box3_sparse_softmax_warp_bwd_pair(*p, *dims(k=k, **kw), Cv, k, f(100.0), None)
    theta = lambda p=(one,) * 4, Cv=3, k=4, **kw: hip_lib.cocos_box3_sparse_softmax_warp_bwd_theta(*p, *dims(k=k, **kw), k, None)
    key = lambda p=(one,) * 12, Cv=3, k=4, **kw: hip_lib.cocos_box3_sparse_softmax_warp_bwd_key(*p, *dims(k=k, **kw), Cv, k, None)
    for call in (fwd, pair, theta, key):
        assert call(K=128) == -2 and b"K == 256" in err()
        assert call(k=0) == -1 and b"k=0" in err()
        assert call(k=9) == -1 and b"k=9" in err()
        assert call(g=(4, 4, 1, 4), k=8) == -1 and b"Nk=4" in err()
        assert call(B=0) == -1 and b"bad dims" in err()
        for i in range(4):                                     # an empty content or exemplar grid
            assert call(g=tuple(0 if n == i else 4 for n in range(4))) == -1 and b"bad dims" in err()
    for call in (fwd, pair, key):
        assert call(Cv=0) == -1
    for i in range(11):
        assert fwd(p=(one,) * i + (None,) + (one,) * (10 - i)) == -1 and b"null" in err()
    for i in range(9):          # (hb, dmu, da — the last three pointers — may be null)
        assert pair(p=(one,) * i + (None,) + (one,) * (11 - i)) == -1 and b"null" in err()
    for i in range(4):
        assert theta(p=(one,) * i + (None,) + (one,) * (3 - i)) == -1 and b"null" in err()
    for i in (6, 7):            # entries, offsets
        assert key(p=(one,) * i + (None,) + (one,) * (11 - i)) == -1 and b"null" in err()
    assert key(p=(one,) * 8 + (None,) * 4) == -1 and b"null" in err()                                  # no output at all
    assert key(p=(None,) + (one,) * 11) == -1 and b"dph_t needs" in err()                              # dph_t without the theta rows
    assert key(p=(one, None) + (one,) * 10) == -1 and b"dv_t needs" in err()                           # dv_t without dout_t
    assert key(p=(one,) * 5 + (None,) + (one,) * 6) == -1 and b"dnu needs" in err()                    # dnu without mu
    assert key(p=(one,) * 3 + (None,) + (one,) * 8) == -1 and b"db needs" in err()                     # db without hb
    odd = ctypes.c_void_p(24)
    assert fwd(p=(odd,) + (one,) * 10) == -1 and b"aligned" in err()
    assert fwd(p=(one, odd) + (one,) * 9) == -1 and b"aligned" in err()
    assert theta(p=(odd,) + (one,) * 3) == -1 and b"aligned" in err()
    assert theta(p=(one,) * 3 + (odd,)) == -1 and b"aligned" in err()
    assert key(p=(odd,) + (one,) * 11) == -1 and b"aligned" in err()
    assert key(p=(one,) * 8 + (odd,) + (one,) * 3) == -1 and b"aligned" in err()


def _op_inputs(B=1, grid=(2, 4), kgrid=(3, 4), Cv=3, k=2):
    theta, phi = bc.features(B, grid, kgrid, 11)
    (mu, a), (nu, b) = bc.stats(theta), bc.stats(phi)
    v = torch.randn(B, Cv, kgrid[0] * kgrid[1])
    idx = torch.zeros(B, grid[0] * grid[1], k, dtype=torch.int64)
    return [theta, phi, mu, a, nu, b, v, idx]


def test_op_refuses_on_the_host(hip_lib):
    """the family's order: TypeError for the idx dtype, ValueError for shapes, channels, k and a statistics tensor of the wrong size,
    then "no CPU fallback" """
    from cocosnet_amd import _lib, ops
    args = _op_inputs()
    call = lambda *a, **kw: ops.box3_sparse_softmax_warp(*a, 100.0, **kw)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        call(*args)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        call(*args, return_weights=True)
    swap = lambda i, t: args[:i] + [t] + args[i + 1:]
    theta, phi, mu, a, nu, b, v, idx = args
    for bad in (idx.float(), idx.to(torch.int16), idx.bool()):
        with pytest.raises(TypeError, match="idx"):
            call(*swap(7, bad))
    with pytest.raises(TypeError, match="idx"):                                        # the dtype comes before the shapes
        call(*swap(7, idx[:, :3].float()))
    for bad in (swap(7, idx[:, :7]), swap(7, idx[0]), swap(6, v[:, :, :11]), swap(6, v[0]), swap(1, phi[:, :128]), swap(0, theta[0]),
                swap(0, torch.randn(2, 256, 2, 4)), swap(1, phi[:, :, :0])):
        with pytest.raises(ValueError):
            call(*bad)
    with pytest.raises(ValueError, match="256 channels"):
        call(theta[:, :128], phi[:, :128], *args[2:])
    with pytest.raises(ValueError, match="k=9"):
        call(*swap(7, torch.zeros(1, 8, 9, dtype=torch.int64)))
    few = _op_inputs(kgrid=(2, 2), k=5)                                                # more candidates than keys
    with pytest.raises(ValueError, match="k=5"):
        call(*few)
    for i, what in ((2, "mu"), (3, "a"), (4, "nu"), (5, "b")):                         # statistics of the wrong size (nu for mu, ...)
        with pytest.raises(ValueError, match=rf"{what} is"):
            call(*swap(i, args[i][:, :5]))
    with pytest.raises(ValueError, match="mu is"):                                     # a bad statistic comes before the device
        call(*swap(2, nu))


OUT_OF_SCOPE = [(dict(match_kernel=1), "match_kernel 1"), (dict(PONO_C=False), "PONO_C"), (dict(warp_patch=True), "warp_patch"),
                (dict(warp_bilinear=True), "warp_bilinear"), (dict(warp_cycle_w=1.0), "cycle"), (dict(two_cycle=True), "cycle"),
                (dict(warp_mask_losstype="cycle"), "cycle")]


def _hot_inputs():
    g = torch.Generator().manual_seed(5)
    onehot = lambda: torch.zeros(1, 5, 8, 8).scatter_(1, torch.randint(0, 5, (1, 1, 8, 8), generator=g), 1.0)
    return torch.randn(1, 256, 2, 2, generator=g), torch.randn(1, 256, 2, 2, generator=g), torch.rand(1, 3, 8, 8, generator=g), onehot(), onehot()


class _NoTensor:
    """stands where theta / phi would: the scope is checked before any tensor is looked at (only the width is read)"""
    shape = (1, 256, 2, 2)

    def __getattr__(self, name):
        pytest.fail(f"a tensor was looked at ({name}) before the scope was checked")


@pytest.mark.parametrize("flags,word", OUT_OF_SCOPE, ids=[w + "-" + "-".join(f) for f, w in OUT_OF_SCOPE])
def test_correspondence_sparse_box3_names_what_is_out_of_scope(hip_lib, flags, word):
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse_box3
    _, _, ref_img, seg, ref_seg = _hot_inputs()
    cfg = HotPathConfig(**dict(dict(match_kernel=3, PONO_C=True, down=4), **flags))
    with pytest.raises(ValueError, match=word) as e:
        correspondence_sparse_box3(_NoTensor(), _NoTensor(), ref_img, seg, ref_seg, cfg)
    assert "match_kernel 3 route" in str(e.value)
    if "match_kernel" in flags:
        assert "match_kernel" in str(e.value).split("(")[0]


def test_correspondence_sparse_box3_other_refusals(hip_lib, monkeypatch):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse_box3
    theta, phi, ref_img, seg, ref_seg = _hot_inputs()
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="topk"):
            correspondence_sparse_box3(_NoTensor(), _NoTensor(), ref_img, seg, ref_seg, cfg, topk=bad)
    with pytest.raises(ValueError, match="topk=5"):                                    # four exemplar positions
        correspondence_sparse_box3(theta, phi, ref_img, seg, ref_seg, cfg, topk=5)
    with pytest.raises(ValueError, match="prepared exemplar"):
        correspondence_sparse_box3(_NoTensor(), _NoTensor(), ref_img, seg, ref_seg, cfg, exemplar=object())
    with pytest.raises(ValueError, match="256 channels"):
        correspondence_sparse_box3(theta[:, :128], phi[:, :128], ref_img, seg, ref_seg, cfg)
    with pytest.raises(ValueError, match="ref_img"):
        correspondence_sparse_box3(theta, phi, ref_img[:, :, :4], seg, ref_seg, cfg, topk=2)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):                   # in scope: the tensors themselves are refused
        correspondence_sparse_box3(theta, phi, ref_img, seg, ref_seg, cfg, topk=2)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="COCOS_PRECISION=fp32"):
        correspondence_sparse_box3(_NoTensor(), _NoTensor(), ref_img, seg, ref_seg, cfg)


def test_module_sparse_warp_box3_refuses_before_the_network_runs(hip_lib, monkeypatch):
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

    for flags, word in OUT_OF_SCOPE:
        with pytest.raises(ValueError, match=word):
            net_for(**flags).sparse_warp_box3(ref_img, None, seg, ref_seg)
    net = net_for()
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="topk"):
            net.sparse_warp_box3(ref_img, None, seg, ref_seg, topk=bad)
    with pytest.raises(ValueError, match="prepared exemplar"):
        net.sparse_warp_box3(None, None, seg, ref_seg)
    monkeypatch.setattr(net, "inter_channels", 128)
    with pytest.raises(ValueError, match="256 channels"):
        net.sparse_warp_box3(ref_img, None, seg, ref_seg)
    # sparse_warp keeps refusing this route: the new method is no new branch of it
    with pytest.raises(ValueError, match="match_kernel 3"):
        net.sparse_warp(ref_img, None, seg, ref_seg)


# ---------------------------------------------------------------------------------------------------------------- the definition, on the host
def test_arbiter_at_full_support_is_the_dense_restatement():
    """k = Nk, idx = every key: the arbiter equals unfold + centre + normalise + softmax over all keys + matmul, in fp64"""
    theta, phi = (t.double() for t in bc.features(2, (3, 2), (2, 4), 21))
    v = torch.randn(2, 5, 8, generator=torch.Generator().manual_seed(22)).double()
    idx = torch.arange(8).expand(2, 6, 8)
    out, w = bc.arbiter(theta, phi, v, idx, 100.0, weights=True)
    assert float((out - bc.dense(theta, phi, v, 100.0)).abs().max()) < 1e-12
    assert float(w.sum(-1).sub(1).abs().max()) < 1e-12
    perm = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4]).expand(2, 6, 8)                      # the order of the candidates does not matter
    assert float((bc.arbiter(theta, phi, v, perm, 100.0) - out).abs().max()) < 1e-12
    # out-of-range entries are clamped: -3 names key 0, 99 names key 7
    a = bc.arbiter(theta, phi, v, torch.tensor([-3, 99]).expand(2, 6, 2), 100.0)
    b = bc.arbiter(theta, phi, v, torch.tensor([0, 7]).expand(2, 6, 2), 100.0)
    assert torch.equal(a, b)


@pytest.mark.parametrize("grid,kgrid", [((1, 8), (1, 8)), ((8, 1), (8, 1)), ((1, 8), (8, 1)), ((2, 2), (2, 2)), ((5, 7), (4, 9))],
                         ids=lambda g: f"{g[0]}x{g[1]}")
def test_tap_formula_is_the_unfolded_product(grid, kgrid):
    """R by taps with both in-grid tests on 2-D coordinates == <unfold(theta)[:,p], unfold(phi)[:,q]> (zero padding), and the logit
    inv_t a_p b_q (R - kc mu_p nu_q) == the arbiter's: the border and wrap rule of the kernels, pinned on the host.  A rule that
    tested the flat index instead would, in the last column, pick up the first cell of the next row — the 1-wide and 2-wide grids
    make every cell a border cell."""
    g = torch.Generator().manual_seed(grid[0] * 100 + kgrid[1])
    C = 6
    theta, phi = torch.randn(2, C, *grid, generator=g).double() + 0.2, torch.randn(2, C, *kgrid, generator=g).double() - 0.1
    R = bc.tap_R(theta, phi)
    uq, uk = F.unfold(theta, kernel_size=3, padding=1), F.unfold(phi, kernel_size=3, padding=1)
    assert float((R - torch.einsum("bci,bcj->bij", uq, uk)).abs().max()) < 1e-12
    (mu, a), (nu, b) = bc.stats(theta), bc.stats(phi)
    z = a.unsqueeze(2) * b.unsqueeze(1) * (R - 9 * C * mu.unsqueeze(2) * nu.unsqueeze(1))
    want = torch.einsum("bci,bcj->bij", bc.unit_unfolded(theta), bc.unit_unfolded(phi))
    assert float((z - want).abs().max()) < 1e-12


def test_host_statistics_are_the_hot_paths():
    """bc.stats (the unfolded definition) == hot_path._unfold3_stats' box-sum form on the host, in fp64"""
    from cocosnet_amd.hot_path import _unfold3_stats
    theta, _ = bc.features(2, (5, 7), (4, 9), 31, C=8)
    mu, a = bc.stats(theta.double())
    mu2, a2 = _unfold3_stats(theta.double(), 72.0)
    assert float((mu - mu2).abs().max()) < 1e-12 and float(((a - a2) / a).abs().max()) < 1e-9
