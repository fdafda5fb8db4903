"""K30: the row pass's head in bilinear and patch mode, without mask channels and with the cycle term's second gradient
(csrc/warp_head.hip, ops.warp_head(mode=...)), the patch flavour of K14 (ops.warp_values(patch=True)) and their routing in
hot_path.correspondence_hot_path (ops.WARP_HEAD_MODES).

Bounds.  Copies (patch mode, views, un/fold) are compared with torch.equal.  The bilinear kernels are held to torch's fp64
F.interpolate and its autograd; the bound is what the framework's own fp32 op makes of the same inputs against the same fp64
result, times 2, plus one fp32 ulp of the reference tensor's max (the rule the fused Adam tests use), separately for the border
rows / columns (clamped taps) and the interior.  D = sum_c d o * o is held to 1e-6 of max|D| against fp64, the bound the nearest head
is held to in test_gpu_plane_prep.py.  Through the hot path the new route is held to the committed reference fixtures at
test_gpu_parity.py's bounds; differences between the two arms are printed (run with -s), and gradients of the two arms — the same
fp32 arithmetic up to the order of a few sums — must agree to that file's gradient bound.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cocosnet_amd import ops
from oracle import golden_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT_TOL = 2e-4        # tests/test_gpu_parity.py
GRAD_TOL = 1e-3

# (B, Ci, Cs, h, w, d)
SHAPES = [(16, 3, 0, 64, 64, 4), (8, 3, 19, 64, 64, 4), (2, 48, 0, 128, 128, 4), (1, 3, 5, 6, 8, 2), (1, 12, 0, 16, 16, 2),
          (2, 3, 2, 12, 20, 4), (1, 2, 1, 5, 8, 3), (1, 3, 0, 1, 4, 4)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale


def _ulp(x):
    return float(np.spacing(np.float32(x)))


class _Tap(torch.autograd.Function):
    """Stands where the K2 / K19 backward stands (as in test_gpu_plane_prep.py): it receives d o itself."""
    seen = {}

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        cell = ops._recall_amax(g)
        _Tap.seen = {"amax": None if cell is None else float(cell), "d": ops._rowdot_cached(g, x), "left": ops._tls.known_rowdot,
                     "g": g}
        return g


def _patch_channels(Ci, d):
    return Ci if Ci % (d * d) == 0 else Ci * d * d


# ---------------------------------------------------------------------------------------------------------- 1. copies are bitwise
@pytest.mark.parametrize("B,Ci,Cs,h,w,d", SHAPES)
def test_patch_mode_is_fold_and_its_backward_is_unfold_bit_for_bit(B, Ci, Cs, h, w, d, monkeypatch):
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    Ci = _patch_channels(Ci, d)
    N, H, W = h * w, h * d, w * d
    leaf = _rand(B, Ci + Cs, N, seed=h + w).requires_grad_(True)
    o = _Tap.apply(leaf)
    assert ops.warp_head_ok(o, Ci, h, w, d, "patch")
    y, m, yv = ops.warp_head(o, Ci, h, w, d, mode="patch", want_y=True)
    assert torch.equal(y, F.fold(o[:, :Ci], (H, W), d, stride=d))
    assert yv.data_ptr() == o.data_ptr() and yv.shape == (B, Ci, N) and torch.equal(yv, o[:, :Ci])
    if Cs:
        assert m.data_ptr() == o[:, Ci:].data_ptr() and torch.equal(m, o[:, Ci:].reshape(B, Cs, h, w))
    else:
        assert m is None
    g_img = _rand(*y.shape, seed=1)
    outs, grads = [y], [g_img]
    if Cs:
        outs.append(m); grads.append(_rand(B, Cs, h, w, seed=2, scale=2.0))
    torch.autograd.backward(outs, grads)
    o2 = leaf.detach().clone().requires_grad_(True)
    outs2 = [F.fold(o2[:, :Ci], (H, W), d, stride=d)] + ([o2[:, Ci:].reshape(B, Cs, h, w)] if Cs else [])
    torch.autograd.backward(outs2, grads)
    assert torch.equal(leaf.grad, o2.grad)
    seen = _Tap.seen
    assert seen["amax"] == float(leaf.grad.abs().max())
    want = (leaf.grad.double() * leaf.detach().double()).sum(1)
    assert float((seen["d"].double() - want).abs().max()) <= 1e-6 * float(want.abs().max()) + 1e-30
    assert seen["left"] is None


@pytest.mark.parametrize("B,Ci,Cs,H,W,d", [(2, 3, 0, 256, 256, 4), (1, 3, 20, 64, 32, 4), (2, 3, 4, 12, 20, 2), (1, 2, 1, 9, 6, 3)])
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_warp_values_patch_is_unfold_plus_sampled_labels(B, Ci, Cs, H, W, d, precision, monkeypatch):
    monkeypatch.setattr(ops, "PRECISION", precision)
    img = _rand(B, Ci, H, W, seed=3)
    seg = _rand(B, Cs, H, W, seed=4, scale=3.0) if Cs else None
    out = ops.warp_values(img, seg, d, patch=True)
    ref = F.unfold(img, d, stride=d).reshape(B, Ci * d * d, H // d, W // d)
    if Cs:
        ref = torch.cat((ref, F.interpolate(seg, scale_factor=1 / d, mode="nearest")), 1)
    assert torch.equal(out, ref)
    cell = ops._recall_amax(out.reshape(B, out.shape[1], -1))
    if precision == "f16x3":
        assert cell is not None and float(cell) == float(ref.abs().max())
    else:
        assert cell is None


# ------------------------------------------------------------------------------- 2 + 3. bilinear against torch fp64, by-products
def _regions(t, lo_rows, lo_cols):
    """(border, interior) boolean masks over the last two axes of t."""
    Hh, Ww = t.shape[-2], t.shape[-1]
    yy = torch.arange(Hh, device=t.device)
    xx = torch.arange(Ww, device=t.device)
    by = (yy < lo_rows) | (yy >= Hh - lo_rows)
    bx = (xx < lo_cols) | (xx >= Ww - lo_cols)
    border = (by[:, None] | bx[None, :]).expand_as(t)
    return border, ~border


def _held(name, ours, fw, ref, lines):
    """ours / fw fp32 tensors against the fp64 ref, per region; asserts the 2 x framework + 1 ulp rule."""
    top = float(ref.abs().max())
    for region, mask in ours[1].items():
        if not bool(mask.any()):
            continue
        e_ours = float((ours[0].double() - ref)[mask].abs().max())
        e_fw = float((fw.double() - ref)[mask].abs().max())
        bound = 2.0 * e_fw + _ulp(top)
        lines.append(f"K30_HEAD_ERR {name} {region}: ours {e_ours:.3e} framework {e_fw:.3e} bound {bound:.3e} max|ref| {top:.3e}")
        print(lines[-1])
        assert e_ours <= bound, lines[-1]


# every shape with and without d y; with and without d warp_mask where there are mask channels
BILINEAR_CASES = [s + (gm, gy) for s in SHAPES for gm in ((False, True) if s[2] else (False,)) for gy in (False, True)]


@pytest.mark.parametrize("B,Ci,Cs,h,w,d,with_gmask,with_gy", BILINEAR_CASES)
def test_bilinear_head_matches_fp64_interpolate_and_leaves_amax_and_rowdot(B, Ci, Cs, h, w, d, with_gmask, with_gy, monkeypatch):
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    N = h * w
    lines = []
    leaf = _rand(B, Ci + Cs, N, seed=3 * h + w).requires_grad_(True)
    o = _Tap.apply(leaf)
    assert ops.warp_head_ok(o, Ci, h, w, d, "bilinear")
    res = ops.warp_head(o, Ci, h, w, d, mode="bilinear", want_y=with_gy)
    y, m = res[0], res[1]
    assert (m is None) == (Cs == 0)
    if Cs:
        assert m.data_ptr() == o[:, Ci:].data_ptr()
    if with_gy:
        assert res[2].data_ptr() == o.data_ptr() and res[2].shape == (B, Ci, N)

    def torch_route(dtype):
        o_t = leaf.detach().to(dtype).requires_grad_(True)
        y_t = F.interpolate(o_t[:, :Ci].reshape(B, Ci, h, w), scale_factor=d, mode="bilinear", align_corners=False)
        return o_t, y_t

    o64, y64 = torch_route(torch.float64)
    o32, y32 = torch_route(torch.float32)
    tag = f"B{B}_Ci{Ci}_Cs{Cs}_{h}x{w}_d{d}_gm{int(with_gmask)}_gy{int(with_gy)}"
    b_f, i_f = _regions(y64, (d + 1) // 2, (d + 1) // 2)
    _held("fwd " + tag, (y.detach(), {"border": b_f, "interior": i_f}), y32.detach(), y64.detach(), lines)

    g_img = _rand(*y.shape, seed=11)
    g_mask = _rand(B, Cs, h, w, seed=12, scale=2.0) if with_gmask else None
    g_y = _rand(B, Ci, N, seed=13, scale=0.5) if with_gy else None

    def backward(o_t, y_t, dtype):
        outs, grads = [y_t], [g_img.to(dtype)]
        if g_mask is not None:
            outs.append(o_t[:, Ci:].reshape(B, Cs, h, w)); grads.append(g_mask.to(dtype))
        if g_y is not None:
            outs.append(o_t[:, :Ci]); grads.append(g_y.to(dtype))
        torch.autograd.backward(outs, grads)
        return o_t.grad

    outs, grads = [y], [g_img]
    if g_mask is not None:
        outs.append(m); grads.append(g_mask)
    if g_y is not None:
        outs.append(res[2]); grads.append(g_y)
    torch.autograd.backward(outs, grads)
    d64, d32 = backward(o64, y64, torch.float64), backward(o32, y32, torch.float32)
    ours = leaf.grad
    v = lambda t: t[:, :Ci].reshape(B, Ci, h, w)
    b_b, i_b = _regions(v(d64), 1, 1)
    _held("bwd " + tag, (v(ours), {"border": b_b, "interior": i_b}), v(d32), v(d64), lines)
    if Cs:       # the mask rows are a copy (or zero)
        assert torch.equal(ours[:, Ci:], g_mask.reshape(B, Cs, N) if with_gmask else torch.zeros_like(ours[:, Ci:]))
    # by-products: the consumer's max|d o| is the tensor's own, D is the fp64 row dot of the fp64-autograd d o
    seen = _Tap.seen
    assert seen["g"].data_ptr() == ours.data_ptr() or torch.equal(seen["g"], ours)
    assert seen["amax"] == float(ours.abs().max())
    want = (d64 * leaf.detach().double()).sum(1)
    err_d = float((seen["d"].double() - want).abs().max())
    lines.append(f"K30_HEAD_ERR rowdot {tag}: {err_d:.3e} bound {1e-6 * float(want.abs().max()):.3e}")
    print(lines[-1])
    assert err_d <= 1e-6 * float(want.abs().max()) + 1e-30
    assert seen["left"] is None          # consumed


def test_bilinear_backward_is_a_fixed_order_gather():
    """Two runs from the same inputs: bit-identical d o (the framework's backward is an atomic scatter)."""
    B, Ci, Cs, h, w, d = 4, 3, 0, 64, 64, 4
    o = _rand(B, Ci, h * w, seed=1)
    g = _rand(B, Ci, h * d, w * d, seed=2)
    runs = []
    for _ in range(2):
        leaf = o.clone().requires_grad_(True)
        ops.warp_head(leaf * 1.0, Ci, h, w, d, mode="bilinear")[0].backward(g)
        runs.append(leaf.grad.clone())
    assert torch.equal(runs[0], runs[1])


def test_nearest_with_side_output_and_default_arguments():
    """want_bi: nearest warp_out and the bilinear side output from one launch; default arguments are the round-6 function."""
    B, Ci, Cs, h, w, d = 2, 3, 4, 8, 12, 4
    o = _rand(B, Ci + Cs, h * w, seed=5).requires_grad_(True)
    y, m, bi = ops.warp_head(o * 1.0, Ci, h, w, d, want_bi=True)
    img = o.detach()[:, :Ci].reshape(B, Ci, h, w)
    assert torch.equal(y, F.interpolate(img, scale_factor=d, mode="nearest"))
    ref = F.interpolate(img.double(), scale_factor=d, mode="bilinear", align_corners=False)
    fw = F.interpolate(img, scale_factor=d, mode="bilinear", align_corners=False)
    assert float((bi.double() - ref).abs().max()) <= 2 * float((fw.double() - ref).abs().max()) + _ulp(float(ref.abs().max()))
    y0, m0 = ops.warp_head(o.detach(), Ci, h, w, d)
    assert torch.equal(y0, y) and torch.equal(m0, m)
    # a loss on the side output reaches o as well
    g1, g2 = _rand(*y.shape, seed=6), _rand(*bi.shape, seed=7)
    torch.autograd.backward([y, bi], [g1, g2])
    def torch_route(dtype):
        o_t = o.detach().to(dtype).requires_grad_(True)
        i_t = o_t[:, :Ci].reshape(B, Ci, h, w)
        torch.autograd.backward([F.interpolate(i_t, scale_factor=d, mode="nearest"),
                                 F.interpolate(i_t, scale_factor=d, mode="bilinear", align_corners=False)], [g1.to(dtype), g2.to(dtype)])
        return o_t.grad
    d64, d32 = torch_route(torch.float64), torch_route(torch.float32)
    assert float((o.grad.double() - d64).abs().max()) <= 2 * float((d32.double() - d64).abs().max()) + _ulp(float(d64.abs().max()))
    with pytest.raises(ValueError):
        ops.warp_head(o.detach(), Ci, h, w, d, mode="cubic")


# ------------------------------------------------------------------------------------------------------ 4-8. through the hot path
FLAG_SETS = {
    # README training commands: CelebA-HQ mask, CelebA-HQ edge, DeepFashion; plus the edge set with --two_cycle and a patch + cycle set
    "celeba_mask": dict(warp_bilinear=True, warp_cycle_w=0.1, warp_mask_losstype="direct", nc=19),
    "celeba_edge": dict(warp_bilinear=True, warp_cycle_w=1.0, warp_mask_losstype="none", nc=15),
    "celeba_edge_two": dict(warp_bilinear=True, warp_cycle_w=1.0, two_cycle=True, warp_mask_losstype="none", nc=15),
    "fashion": dict(warp_patch=True, warp_bilinear=True, warp_mask_losstype="none", nc=20),
    "patch_cycle": dict(warp_patch=True, warp_cycle_w=1.0, warp_mask_losstype="none", nc=3),
}
COPY_ONLY = ("fashion", "patch_cycle")       # their new kernels are copies: outputs bit for bit


def _hot_inputs(name, mk, B=2, fh=64, fw=64, seed=0):      # (the 64-wide grid: match_kernel 3 then takes its fused family, K19)
    f = dict(FLAG_SETS[name])
    nc = f.pop("nc")
    g = torch.Generator(device=DEV).manual_seed(100 + seed)
    mkp = lambda *s: torch.randn(*s, device=DEV, generator=g)
    th = mkp(B, 256, fh, fw)
    perm = torch.randperm(fh * fw, device=DEV, generator=g)
    ph = 0.2 * th.reshape(B, 256, -1)[:, :, perm].reshape(B, 256, fh, fw) + mkp(B, 256, fh, fw) + 0.1
    H, W = fh * 4, fw * 4
    ref_img = torch.rand(B, 3, H, W, device=DEV, generator=g) * 2 - 1
    real_img = torch.rand(B, 3, H, W, device=DEV, generator=g) * 2 - 1
    lab = torch.randint(0, nc, (B, 1, H, W), device=DEV, generator=g)
    seg = torch.zeros(B, nc, H, W, device=DEV).scatter_(1, lab, 1.0)
    from cocosnet_amd.hot_path import HotPathConfig
    cfg = HotPathConfig(match_kernel=mk, PONO_C=True, down=4, isTrain=True, **f)
    return cfg, th, ph, ref_img, real_img, seg


def _hot_step(name, mk, modes, monkeypatch, **kw):
    from cocosnet_amd.hot_path import correspondence_hot_path
    monkeypatch.setattr(ops, "WARP_HEAD_MODES", modes)
    cfg, th, ph, ref_img, real_img, seg = _hot_inputs(name, mk, **kw)
    th, ph = th.requires_grad_(True), ph.requires_grad_(True)
    out = correspondence_hot_path(th, ph, ref_img, real_img, seg, seg, cfg)
    keys = sorted(out)
    g = torch.Generator(device=DEV).manual_seed(7)
    cot = [torch.randn(out[k].shape, device=DEV, generator=g) for k in keys]
    torch.autograd.backward([out[k] for k in keys], cot)
    return {k: out[k].detach() for k in keys}, th.grad, ph.grad


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("mk", [1, 3])
@pytest.mark.parametrize("name", sorted(FLAG_SETS))
def test_hot_path_new_route_against_the_framework_route(name, mk, precision, monkeypatch):
    monkeypatch.setattr(ops, "PRECISION", precision)
    monkeypatch.setattr(ops, "PROJ_PRECISION", precision)
    counts, res, on_head_dout = {}, {}, []
    real = ops._lib.call
    state = {"head_dout": None}

    def watched(name, *args):
        # a row-dot or max|.| pass over the d o that the most recent head backward wrote would be the pass that head exists to remove
        if name in ("cocos_warp_head_bwd_ex", "cocos_warp_head_bwd"):
            state["head_dout"] = args[4] if name.endswith("_ex") else args[3]
        elif name in ("cocos_rowdot_f64", "cocos_absmax_accumulate") and args[0] == state["head_dout"]:
            on_head_dout.append((name, state["modes"]))
        elif name == "cocos_absmax4" and state["head_dout"] in args[0:12:3]:
            on_head_dout.append((name, state["modes"]))
        return real(name, *args)

    monkeypatch.setattr(ops._lib, "call", watched)
    for modes in (False, True):
        state.update(modes=modes, head_dout=None)
        with ops.KernelTimer(tags=("rowdot", "absmax", "warp_head_bwd")) as t:
            res[modes] = _hot_step(name, mk, modes, monkeypatch)
            torch.cuda.synchronize()
        counts[modes] = {k: len(v) for k, v in t.events.items()}
    (o0, dt0, dp0), (o1, dt1, dp1) = res[False], res[True]
    assert sorted(o0) == sorted(o1)
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))
    for k in o0:
        if name in COPY_ONLY:
            assert torch.equal(o0[k], o1[k]), k
        print(f"K30_HEAD_ERR hot_path {name} mk{mk} {precision} arm-to-arm {k}: {rel(o1[k], o0[k]):.3e}")
    for key, a, b in (("d theta", dt1, dt0), ("d phi", dp1, dp0)):
        print(f"K30_HEAD_ERR hot_path {name} mk{mk} {precision} arm-to-arm {key}: {rel(a, b):.3e}")
        assert rel(a, b) < GRAD_TOL, key
    print(f"K30_HEAD_CALLS {name} mk{mk} {precision} framework route {counts[False]} new route {counts[True]}")
    heads = counts[True].get("warp_head_bwd", 0)
    assert heads >= 1 and counts[False].get("warp_head_bwd", 0) == 0
    # no row-dot and no max|.| pass over a d o that a head produced (backward variants that take D from the host side call
    # cocos_rowdot_f64; the others never did), and none more than the framework route makes in all
    assert not on_head_dout, on_head_dout
    assert counts[True].get("rowdot", 0) <= counts[False].get("rowdot", 0), counts
    assert counts[True].get("absmax", 0) <= counts[False].get("absmax", 0), counts


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", ["celeba_cycle", "celebamask_train_mk1", "celebamask_train_mk3", "patch_256", "fashion_patch_mk3",
                                  "b1_showcorr"])
def test_new_route_matches_reference_fixtures(name, precision, monkeypatch):
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_hot_path
    monkeypatch.setattr(ops, "PRECISION", precision)
    monkeypatch.setattr(ops, "PROJ_PRECISION", precision)
    monkeypatch.setattr(ops, "WARP_HEAD_MODES", True)
    dev = lambda a, grad=False: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).requires_grad_(grad)
    c = gc.CASES[name]
    inp = gc.make_inputs(name)
    golden = gc.load_golden(name)
    cfg = HotPathConfig(**gc.hot_path_flags(name))
    th, ph = dev(inp.theta_raw, True), dev(inp.phi_raw, True)
    seen = []
    real = ops._lib.call
    monkeypatch.setattr(ops._lib, "call", lambda n, *a: (seen.append(n), real(n, *a))[1])
    res = correspondence_hot_path(th, ph, dev(inp.ref_img), dev(inp.real_img), dev(inp.seg_map), dev(inp.ref_seg_map), cfg,
                                  **c.get("fwd", {}))
    assert "cocos_warp_head_fwd_ex" in seen, seen         # the route under test was taken
    errs = gc.compare_with_golden(name, {k: v.detach().cpu().numpy() for k, v in res.items()}, golden)
    print(f"K30_HEAD_ERR golden {name} {precision} outputs {errs}")
    assert errs and max(errs.values()) < OUT_TOL, errs
    if c.get("grads"):
        G = gc.grad_weights(name, {k: tuple(v.shape) for k, v in res.items()})
        sum((res[k] * dev(G[k])).sum() for k in res).backward()
        for g, key in ((th.grad, "theta_raw"), (ph.grad, "phi_raw")):
            err = gc.grad_error(name, key, g.detach().double().cpu().numpy(), golden)
            print(f"K30_HEAD_ERR golden {name} {precision} d {key} {err:.3e}")
            assert err < GRAD_TOL, (key, err)
        assert "cocos_warp_head_bwd_ex" in seen


@pytest.mark.parametrize("name", ["celeba_edge", "fashion"])
def test_no_framework_resampling_kernel_is_left(name, monkeypatch):
    """Forward + backward under the profiler: no bilinear up-sampling, im2col / col2im or average-pooling kernel of the framework."""
    from torch.profiler import ProfilerActivity, profile
    launches = {}
    for modes in (False, True):
        _hot_step(name, 3, modes, monkeypatch)                       # warm-up
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            _hot_step(name, 3, modes, monkeypatch)
            torch.cuda.synchronize()
        kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        launches[modes] = len(kernels)
        if modes:
            for k in kernels:
                low = k.lower()
                assert not any(s in low for s in ("upsample_bilinear2d", "im2col", "col2im", "avg_pool2d")), k
            assert any("cocos::warp_head_bwd_kernel" in k for k in kernels), kernels
    print(f"K30_HEAD_LAUNCHES {name} framework route {launches[False]} new route {launches[True]}")


@pytest.mark.parametrize("mk", [1, 3])
def test_celeba_edge_gradients_are_reproducible(mk, monkeypatch):
    a = _hot_step("celeba_edge", mk, True, monkeypatch)
    b = _hot_step("celeba_edge", mk, True, monkeypatch)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k


@pytest.mark.parametrize("name", sorted(FLAG_SETS))
def test_new_flag_sets_hand_over_live_buffers_only(name, monkeypatch):
    from test_gpu_live_buffers import _Guard
    guard = _Guard(monkeypatch)
    _hot_step(name, 3, True, monkeypatch, B=1)
    guard.check(8, 40)


def test_peak_memory_of_a_celeba_edge_step_is_not_above_the_framework_route(monkeypatch):
    peaks = {}
    for modes in (False, True, False, True):
        _hot_step("celeba_edge", 1, modes, monkeypatch, B=16, fh=64, fw=64)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        _hot_step("celeba_edge", 1, modes, monkeypatch, B=16, fh=64, fw=64)
        torch.cuda.synchronize()
        peaks[modes] = torch.cuda.max_memory_allocated() - base
    print(f"K30_HEAD_PEAK celeba_edge B=16 64x64 framework route {peaks[False] / 2**20:.1f} MiB new route {peaks[True] / 2**20:.1f} MiB")
    assert peaks[True] <= peaks[False], peaks


# ------------------------------------------------------------------------------------------------------ 9. one head op, one arm
@pytest.mark.parametrize("d", [4, 2])      # the unrolled window sums and the generic loop
def test_one_head_op_defaults_and_a_missing_mask_gradient(d, monkeypatch):
    """ops.warp_head with default arguments (round 6's function, now the nearest mode of the one op): F.interpolate(nearest) and the
    mask view bit for bit; a backward in which nothing used the mask equals one with an explicit zero gradient — d o, D and the
    remembered max|d o| bit for bit — through autograd and at the entry point, where the absent gradient is a NULL pointer."""
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    B, Ci, Cs, h, w = 2, 3, 2, 3, 4
    bits = lambda t: t.contiguous().view(torch.int32)
    base = _rand(B, Ci + Cs, h * w, seed=40 + d)
    y, m = ops.warp_head(base, Ci, h, w, d)
    assert torch.equal(bits(y), bits(F.interpolate(base[:, :Ci].reshape(B, Ci, h, w), scale_factor=d, mode="nearest")))
    assert m.data_ptr() == base[:, Ci:].data_ptr() and torch.equal(bits(m), bits(base[:, Ci:].reshape(B, Cs, h, w)))
    g = _rand(*y.shape, seed=41)

    def through_autograd(explicit_zero):
        leaf = base.clone().requires_grad_(True)
        y, m = ops.warp_head(_Tap.apply(leaf), Ci, h, w, d)
        if explicit_zero:
            torch.autograd.backward([y, m], [g, torch.zeros_like(m)])
        else:
            y.backward(g)
        return leaf.grad, _Tap.seen["d"], _Tap.seen["amax"]

    def at_the_entry_point(g_mask):
        dout, drow, cell = torch.empty_like(base), torch.empty(B, h * w, device=DEV), torch.zeros(1, device=DEV)
        ops._call("warp_head_bwd", "cocos_warp_head_bwd_ex", g.data_ptr(), ops._ptr(g_mask), 0, base.data_ptr(), dout.data_ptr(),
                  drow.data_ptr(), cell.data_ptr(), B, Ci, Cs, h, w, d, ops._HEAD_MODES["nearest"], ops._stream())
        return dout, drow, float(cell)

    for absent, zero in ((through_autograd(False), through_autograd(True)),
                         (at_the_entry_point(None), at_the_entry_point(torch.zeros(B, Cs, h, w, device=DEV)))):
        assert torch.equal(bits(absent[0]), bits(zero[0])) and torch.equal(bits(absent[1]), bits(zero[1]))
        assert absent[2] is not None and absent[2] == zero[2] == float(absent[0].abs().max())
        assert not bool(absent[0][:, Ci:].any())


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_modes_off_still_selects_the_nearest_head_bit_for_bit(precision, monkeypatch):
    """The direct-mask flag set (round 6's): with ops.WARP_HEAD_MODES off the restricted condition still selects the head, through the
    one op — every output and the theta / phi gradients equal those with the switch on, bit for bit."""
    monkeypatch.setattr(ops, "PRECISION", precision)
    monkeypatch.setattr(ops, "PROJ_PRECISION", precision)
    monkeypatch.setitem(FLAG_SETS, "ade_direct", dict(warp_mask_losstype="direct", nc=7))
    real, seen = ops._lib.call, {}
    res = {}
    for modes in (False, True):
        seen[modes] = []
        monkeypatch.setattr(ops._lib, "call", lambda n, *a, _m=modes: (seen[_m].append(n), real(n, *a))[1])
        res[modes] = _hot_step("ade_direct", 1, modes, monkeypatch, B=1, fh=8, fw=16)
    for modes in (False, True):
        assert "cocos_warp_head_fwd_ex" in seen[modes] and "cocos_warp_head_bwd_ex" in seen[modes], (modes, seen[modes])
    (o0, dt0, dp0), (o1, dt1, dp1) = res[False], res[True]
    assert sorted(o0) == sorted(o1) and {"warp_out", "warp_mask"} <= set(o0) and "warp_out_bi" not in o0
    bits = lambda t: t.contiguous().view(torch.int32)
    for k in o0:
        assert torch.equal(bits(o0[k]), bits(o1[k])), k
    assert torch.equal(bits(dt0), bits(dt1)) and torch.equal(bits(dp0), bits(dp1))
