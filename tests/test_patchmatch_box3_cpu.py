"""K57 (the PatchMatch candidate search on the match_kernel-3 route), the parts that need no GPU: the entry point in header, binding
table and library, its argument checks (which return before any HIP call, in the documented order), the Python-side refusals of
ops.patchmatch_step_box3 / patchmatch_topk_box3, the `search` / `search_opts` arguments of hot_path.correspondence_sparse_box3 and
NoVGGCorrespondence.sparse_warp_box3, and the coarse-start rule as a function of shapes."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_box3_sparse_cpu import OUT_OF_SCOPE, _hot_inputs, _NoTensor  # noqa: E402

NAME = "cocos_patchmatch_step_box3"


def test_header_table_and_library_carry_the_entry_point(hip_lib):
    from cocosnet_amd import _lib, build
    assert _lib.PROTOTYPES.get(NAME, ("",))[0] == "int", f"{NAME} is not declared in cocos_hip.h"
    assert NAME in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, NAME)
    assert "patchmatch_box3.hip" in build.HIP_SOURCES
    assert os.path.exists(os.path.join(build.CSRC_DIR, "patchmatch_pool.h"))
    _, argtypes = _lib._SIGNATURES[NAME]
    assert [t for t in argtypes] == [ctypes.c_void_p] * 9 + [ctypes.c_int] * 12 + [ctypes.c_float] + [ctypes.c_void_p]


def test_argument_validation_needs_no_gpu_and_keeps_its_order(hip_lib):
    """null rows / statistics / outputs, one buffer for both tables, a non-positive temperature (-1); K != 256, an empty grid, k, stride,
    radii, radius0, the 32-bit tables (-2); misaligned rows (-1) last — each call breaks one rule and every rule after it, so the
    message shows which check came first.  All before any HIP call: this process has no GPU."""
    from cocosnet_amd import _lib
    one, two, odd, f = ctypes.c_void_p(16), ctypes.c_void_p(4096), ctypes.c_void_p(24), ctypes.c_float
    err = hip_lib.cocos_last_error_string
    top = _lib.CONSTANTS["COCOS_PATCHMATCH_MAX_RADII"]

    def call(p=None, B=1, K=256, fh=8, fw=8, gh=8, gw=8, k=4, stride=1, radii=3, radius0=4, inv_t=100.0):
        p = (one,) * 7 + (two, one) if p is None else p
        return hip_lib.cocos_patchmatch_step_box3(*p, B, K, fh, fw, gh, gw, k, stride, radii, radius0, 0, 0, f(inv_t), None)

    for i in (0, 1, 2, 3, 4, 5, 7, 8):      # (idx_in, the seventh pointer, may be null: the random initialisation)
        assert call(p=(one,) * i + (None,) + (two,) * (8 - i)) == -1 and b"null" in err()
    assert call(p=(one,) * 9) == -1 and b"one buffer" in err()
    assert call(inv_t=0.0) == -1 and b"inv_temperature" in err()
    assert call(inv_t=-1.0) == -1 and b"inv_temperature" in err()
    assert call(K=128) == -2 and b"K == 256" in err()
    for empty in (dict(B=0), dict(fh=0), dict(fw=0), dict(gh=0), dict(gw=-1)):
        assert call(**empty) == -2 and b"empty" in err()
    for k in (0, 9, -1):
        assert call(k=k) == -2 and b"k=" in err()
    assert call(gh=1, gw=3, k=4) == -2 and b"Nk=3" in err()
    assert call(stride=0) == -2 and b"stride=0" in err()
    assert call(radii=top + 1) == -2 and b"radii" in err()
    assert call(radii=-1) == -2 and b"radii" in err()
    assert call(radius0=-1) == -2 and b"radius0" in err()
    assert call(B=2 ** 20, fh=2 ** 6, fw=2 ** 6) == -2 and b"32-bit" in err()
    for i in (0, 1):
        assert call(p=(one,) * i + (odd,) + (one,) * (6 - i) + (two, one)) == -1 and b"aligned" in err()
    # the order: a call that breaks one rule and EVERY later one reports that rule
    rules = [(dict(inv_t=0.0), b"inv_temperature"), (dict(K=128), b"K == 256"), (dict(B=0), b"empty"), (dict(k=0), b"k="),
             (dict(stride=0), b"stride"), (dict(radii=-1), b"radii"), (dict(radius0=-1), b"radius0")]
    misaligned = (odd, odd) + (one,) * 5 + (two, one)
    for n, (_, word) in enumerate(rules):
        later = {key: v for kw, _ in rules[n:] for key, v in kw.items()}
        assert call(p=misaligned, **later) in (-1, -2) and word in err(), (n, err())
    everything = {key: v for kw, _ in rules for key, v in kw.items()}
    assert call(p=(odd, odd) + (one,) * 7, **everything) == -1 and b"one buffer" in err()
    assert call(p=(None, odd) + (one,) * 7, **everything) == -1 and b"null" in err()


def _op_inputs(grid=(4, 6), kgrid=(3, 4), B=1):
    g = torch.Generator().manual_seed(1)
    Nq, Nk = grid[0] * grid[1], kgrid[0] * kgrid[1]
    return (torch.randn(B, 256, *grid, generator=g), torch.randn(B, 256, *kgrid, generator=g), torch.zeros(B, Nq), torch.ones(B, Nq),
            torch.zeros(B, Nk), torch.ones(B, Nk))


def test_ops_refuse_on_the_host_and_bad_arguments(hip_lib):
    from cocosnet_amd import _lib, ops
    args = _op_inputs()
    step = lambda *a, idx=None, inv_t=100.0, k=2, stride=1, radii=0, radius0=0, seed=0, it=0: ops.patchmatch_step_box3(
        *a, idx, inv_t, k, stride, radii, radius0, seed, it)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.patchmatch_topk_box3(*args, 100.0, 2)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        step(*args)
    for bad_k in (0, 9, 13, 2.0, True):           # 13: more candidates than the 12 keys
        with pytest.raises(ValueError, match="k="):
            ops.patchmatch_topk_box3(*args, 100.0, bad_k)
        with pytest.raises(ValueError, match="k="):
            step(*args, k=bad_k)
    for bad in (0.0, -1.0, None, True):
        with pytest.raises(ValueError, match="inv_t"):
            ops.patchmatch_topk_box3(*args, bad, 2)
        with pytest.raises(ValueError, match="inv_t"):
            step(*args, inv_t=bad)
    for bad in ((0,), (1, -2), (1.5,), (), 3):
        with pytest.raises(ValueError, match="stride"):
            ops.patchmatch_topk_box3(*args, 100.0, 2, strides=bad)
    for bad in (-1, ops.PATCHMATCH_MAX_RADII + 1, (1, -1), 1.5):
        with pytest.raises(ValueError, match="radi"):
            ops.patchmatch_topk_box3(*args, 100.0, 2, radii=bad)
    with pytest.raises(ValueError, match="init"):
        ops.patchmatch_topk_box3(*args, 100.0, 2, init="coarse")
    with pytest.raises(ValueError, match="stride"):
        step(*args, stride=0)
    with pytest.raises(ValueError, match="radii"):
        step(*args, radii=ops.PATCHMATCH_MAX_RADII + 1)
    with pytest.raises(ValueError, match="seed"):
        step(*args, seed=2 ** 31)
    with pytest.raises(ValueError, match="256 channels"):
        ops.patchmatch_topk_box3(args[0][:, :128], args[1][:, :128], *args[2:], 100.0, 2)
    with pytest.raises(ValueError, match="expected theta_raw"):
        ops.patchmatch_topk_box3(args[0].reshape(1, 256, 24), *args[1:], 100.0, 2)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.patchmatch_topk_box3(args[0].expand(2, -1, -1, -1), *args[1:], 100.0, 2)
    for i, what in ((2, "mu"), (3, "a"), (4, "nu"), (5, "b")):
        wrong = list(args)
        wrong[i] = args[i][:, :5]
        with pytest.raises(ValueError, match=rf"{what} is"):
            ops.patchmatch_topk_box3(*wrong, 100.0, 2)
    with pytest.raises(TypeError, match="index table"):
        step(*args, idx=torch.zeros(1, 24, 2))
    with pytest.raises(ValueError, match="index table"):
        step(*args, idx=torch.zeros(1, 24, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="index table"):
        ops.patchmatch_topk_box3(*args, 100.0, 2, init=torch.zeros(1, 23, 2, dtype=torch.int32))


def test_search_argument_is_checked(hip_lib):
    from cocosnet_amd import _lib
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse_box3
    theta, phi, ref_img, seg, ref_seg = _hot_inputs()
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    no = _NoTensor()
    with pytest.raises(ValueError, match="search='bogus'") as e:
        correspondence_sparse_box3(no, no, ref_img, seg, ref_seg, cfg, search="bogus")
    assert "correspondence_sparse_box3" in str(e.value)
    with pytest.raises(ValueError, match="search_opts"):
        correspondence_sparse_box3(no, no, ref_img, seg, ref_seg, cfg, search="patchmatch", search_opts=dict(iterations=3))
    with pytest.raises(ValueError, match="search_opts"):
        correspondence_sparse_box3(no, no, ref_img, seg, ref_seg, cfg, search="dense", search_opts=dict(seed=1))
    with pytest.raises(ValueError, match="search") as e:
        correspondence_sparse_box3(no, no, ref_img, seg, ref_seg, cfg, search="patchmatch", restrict="label")
    assert "restrict" in str(e.value)
    labels = (torch.zeros(1, 2, 2, dtype=torch.int64),) * 2
    with pytest.raises(ValueError, match="search"):
        correspondence_sparse_box3(no, no, ref_img, seg, ref_seg, cfg, search="patchmatch", restrict=labels)
    with pytest.raises(ValueError, match="search") as e:
        correspondence_sparse_box3(no, no, ref_img, seg, ref_seg, cfg, search="patchmatch", transport=dict(iters=3, tau=1.0))
    assert "transport" in str(e.value)
    for search in ("dense", "patchmatch"):         # in scope: the tensors themselves are refused
        with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
            correspondence_sparse_box3(theta, phi, ref_img, seg, ref_seg, cfg, topk=2, search=search)


@pytest.mark.parametrize("flags,word", OUT_OF_SCOPE, ids=[w + "-" + "-".join(f) for f, w in OUT_OF_SCOPE])
def test_patchmatch_keeps_the_route_refusals(hip_lib, flags, word):
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse_box3
    _, _, ref_img, seg, ref_seg = _hot_inputs()
    cfg = HotPathConfig(**dict(dict(match_kernel=3, PONO_C=True, down=4), **flags))
    for search in ("patchmatch", "bogus"):      # the scope is judged before the selector's name, and before any tensor is looked at
        with pytest.raises(ValueError, match=word) as e:
            correspondence_sparse_box3(_NoTensor(), _NoTensor(), ref_img, seg, ref_seg, cfg, search=search)
        assert "match_kernel 3 route" in str(e.value)


def test_patchmatch_other_refusals(hip_lib, monkeypatch):
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse_box3
    theta, phi, ref_img, seg, ref_seg = _hot_inputs()
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    pm = dict(search="patchmatch")
    no = _NoTensor()
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="topk"):
            correspondence_sparse_box3(no, no, ref_img, seg, ref_seg, cfg, topk=bad, **pm)
    with pytest.raises(ValueError, match="topk=5"):                                    # four exemplar positions
        correspondence_sparse_box3(theta, phi, ref_img, seg, ref_seg, cfg, topk=5, **pm)
    with pytest.raises(ValueError, match="prepared exemplar"):
        correspondence_sparse_box3(no, no, ref_img, seg, ref_seg, cfg, exemplar=object(), **pm)
    with pytest.raises(ValueError, match="256 channels"):
        correspondence_sparse_box3(theta[:, :128], phi[:, :128], ref_img, seg, ref_seg, cfg, **pm)
    monkeypatch.setattr(ops, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="COCOS_PRECISION=fp32"):
        correspondence_sparse_box3(no, no, ref_img, seg, ref_seg, cfg, **pm)


def test_module_refuses_before_the_network_runs(hip_lib, monkeypatch):
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
            net_for(**flags).sparse_warp_box3(ref_img, None, seg, ref_seg, search="patchmatch")
    net = net_for()
    with pytest.raises(ValueError, match="search='bogus'"):
        net.sparse_warp_box3(ref_img, None, seg, ref_seg, search="bogus")
    with pytest.raises(ValueError, match="search_opts"):
        net.sparse_warp_box3(ref_img, None, seg, ref_seg, search="patchmatch", search_opts=dict(bogus=1))
    with pytest.raises(ValueError, match="search_opts"):
        net.sparse_warp_box3(ref_img, None, seg, ref_seg, search="dense", search_opts=dict(seed=1))
    with pytest.raises(ValueError, match="search") as e:
        net.sparse_warp_box3(ref_img, None, seg, ref_seg, search="patchmatch", restrict="label")
    assert "restrict" in str(e.value)
    with pytest.raises(ValueError, match="search") as e:
        net.sparse_warp_box3(ref_img, None, seg, ref_seg, search="patchmatch", transport=dict(iters=3, tau=1.0))
    assert "transport" in str(e.value)
    with pytest.raises(ValueError, match="topk"):
        net.sparse_warp_box3(ref_img, None, seg, ref_seg, topk=9, search="patchmatch")


def test_coarse_start_rule_is_a_function_of_the_shapes(hip_lib, monkeypatch):
    """fused: equal half grids the fused box family takes (256x256 -> 128x128, 128x128 -> 64x64) at a k its top-k readout serves;
    materialised: the half-grid chain at or below 256 MiB per matrix; random: an odd side, k above the half-grid keys, a half grid too
    large, unequal grids"""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import PATCHMATCH_BOX3_COARSE_CAP, _patchmatch_coarse_route_box3 as route
    assert PATCHMATCH_BOX3_COARSE_CAP == 256 * 2 ** 20
    assert ops.box3_fused_ok(1, 256, 64, 64) and ops.box3_fused_ok(1, 256, 128, 128) and ops.box3_topk_ok(4)
    assert route(1, 256, 256, 256, 256, 256, 4) == "fused"
    assert route(1, 256, 128, 128, 128, 128, 4) == "fused"
    assert route(8, 256, 128, 128, 128, 128, 1) == "fused"
    # small grids the fused family does not take: the chain, while B Nc Nkc 4 bytes <= 256 MiB
    assert route(2, 256, 8, 8, 8, 8, 3) == "materialised"
    assert route(1, 256, 64, 64, 64, 64, 4) == "materialised"            # 32 x 32 half grid: 1024^2 x 4 B = 4 MiB
    assert route(1, 256, 16, 16, 16, 16, 8) == "materialised"
    assert route(1, 256, 512, 64, 512, 64, 4) == "materialised"          # a 256 x 32 half grid: 8192^2 x 4 B = 256 MiB exactly
    assert route(2, 256, 512, 64, 512, 64, 4) == "random"                # twice that
    assert route(2, 256, 128, 256, 128, 256, 4) == "fused"               # a 64 x 128 half grid is one the fused family takes
    assert route(1, 256, 512, 512, 512, 512, 4) == "random"              # a 256 x 256 half grid: T alone is 16 GiB
    assert route(2, 256, 6, 8, 8, 6, 3) == "random"                      # unequal grids: the dense box readout is built for equal ones
    assert route(1, 256, 128, 128, 256, 256, 4) == "random"
    for odd in ((7, 8, 8, 8), (8, 7, 8, 8), (8, 8, 5, 8), (8, 8, 8, 9)):
        assert route(2, 256, *odd, 3) == "random"
    assert route(2, 256, 4, 4, 4, 4, 5) == "random"                      # four half-grid keys < k
    assert route(2, 256, 4, 4, 4, 4, 4) == "materialised"
    monkeypatch.setattr(ops, "MATCH_FUSED", False)                       # without the fused readout the cap decides alone
    assert route(1, 256, 128, 128, 128, 128, 4) == "materialised"        # 4096^2 x 4 B = 64 MiB
    assert route(8, 256, 128, 128, 128, 128, 4) == "random"              # 512 MiB
