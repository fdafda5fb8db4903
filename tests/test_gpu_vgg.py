"""K27 (cocosnet_amd/csrc/vgg_glue.hip, ops.vgg_preprocess / relu / relu_pool2) and the VGG19 drop-in (cocosnet_amd.vgg) on the GPU:
each kernel bitwise against the framework's fp32 ops (ties, NaNs, odd sizes, every optional operand), the max|.| cells exact, no
activation max|.| pass left in front of a convolution, the module against an fp64 copy and against the reference's golden, live
pointers, memory, and determinism."""
import bisect
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import vgg_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL_KEYS = ["r11", "r12", "p1", "r21", "r22", "p2", "r31", "r32", "r33", "r34", "p3",
            "r41", "r42", "r43", "r44", "p4", "r51", "r52", "r53", "r54", "p5"]
STEP_KEYS = ["r12", "r22", "r32", "r42", "r52"]


@pytest.fixture(autouse=True)
def _need_gpu(hip_lib, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from cocosnet_amd import ops, vgg
    monkeypatch.setattr(ops, "CONV_PRECISION", "f16x3")
    monkeypatch.setattr(vgg, "FUSED", True)


def _same(a, b, what=""):
    """bitwise-equal values (torch.equal), NaN where the other has NaN"""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), f"{what}: NaN pattern differs"
    assert torch.equal(a[~na], b[~nb]), f"{what}: {int((a[~na] != b[~nb]).sum())} elements differ"


def _cell_is_absmax(cell, t, what=""):
    ref = t.abs().max().reshape(1) if t.numel() else torch.zeros(1, device=t.device)
    _same(cell.reshape(1), ref, what + " max|.| cell")


def _recalled(t):
    from cocosnet_amd import ops
    c = ops._recall_amax(t, consume=False)
    assert c is not None, "no max|.| cell left for the next convolution"
    return c


def _capture_grad(t):
    """[the max|.| cell left with the gradient autograd hands to `t`], looked up in the hook: the backward runs in autograd's device
    thread, and the producer -> consumer table is per thread (the consumer, a convolution's backward, runs in the same one)"""
    from cocosnet_amd import ops
    seen = []
    t.register_hook(lambda g: seen.append(ops._recall_amax(g, consume=False)))
    return seen


def _tied(shape, seed, nan=0):
    """integer-rounded values: many exact ties inside the 2x2 windows, about half of them <= 0 (all-negative windows too)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    y = torch.round(torch.randn(shape, device=DEV, generator=g) * 1.5 - 0.3)
    if nan:
        idx = torch.randint(0, y.numel(), (nan,), device=DEV, generator=g)
        y.view(-1)[idx] = float("nan")
    return y


def _randn(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, device=DEV, generator=g)


# ---- kernel contract, bitwise -------------------------------------------------------------------------------------------------
PRE_SHAPES = [(2, 3, 17, 23), (3, 3, 32, 64), (1, 3, 40, 40), (1, 3, 5, 3)]


@pytest.mark.parametrize("shape", PRE_SHAPES)
@pytest.mark.parametrize("nc", [False, True])
def test_preprocess_forward_backward_bitwise(shape, nc):
    from cocosnet_amd import ops
    from cocosnet_amd.vgg import vgg_preprocess_torch
    x = torch.rand(shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) * (2 if nc else 1) - (1 if nc else 0)
    dy = _randn(shape, 4)
    xa = x.clone().requires_grad_(True)
    xb = x.clone().requires_grad_(True)
    ya, yb = ops.vgg_preprocess(xa, nc), vgg_preprocess_torch(xb, nc)
    _same(ya, yb, "preprocess")
    _cell_is_absmax(_recalled(ya), yb, "preprocess")
    ya.backward(dy)
    yb.backward(dy)
    _same(xa.grad, xb.grad, "preprocess backward")


RELU_SIZES = [1, 7, 4096, 1000003, 3 * 64 * 33 * 35]


@pytest.mark.parametrize("n", RELU_SIZES)
def test_relu_forward_backward_bitwise(n):
    from cocosnet_amd import ops
    y = _tied((n,), 10 + n % 97, nan=min(3, n // 5))
    dr = _randn((n,), 11)
    if n > 10:
        dr[::7] = float("inf")              # inf next to a zero mask: a select gives 0, a multiply would give NaN
    r = ops.relu(y)
    _same(r, F.relu(y), "relu")
    _cell_is_absmax(_recalled(r), r, "relu")
    yn = y.nan_to_num(0.5)                  # (the backward without NaNs in the saved source)
    ya, yb = yn.clone().requires_grad_(True), yn.clone().requires_grad_(True)
    seen = _capture_grad(ya)
    ops.relu(ya).backward(dr)
    F.relu(yb).backward(dr)
    _same(ya.grad, yb.grad, "relu backward")
    assert seen[0] is not None, "no max|.| cell left with the gradient"
    _cell_is_absmax(seen[0], yb.grad, "relu backward")


POOL_SHAPES = [(2, 5, 7, 9), (2, 8, 6, 10), (2, 16, 33, 64), (1, 4, 32, 32), (2, 3, 2, 2), (1, 2, 3, 5), (3, 6, 16, 12)]


def _framework_pool(r, mode):
    return F.max_pool2d(r, 2, 2) if mode == "max" else F.avg_pool2d(r, 2, 2)


@pytest.mark.parametrize("shape", POOL_SHAPES)
@pytest.mark.parametrize("mode", ["max", "avg"])
@pytest.mark.parametrize("keep_r", [True, False])
def test_relu_pool2_forward_bitwise(shape, mode, keep_r):
    from cocosnet_amd import ops
    for seed, nan in ((20, 0), (21, 4)):
        y = _tied(shape, seed, nan=nan)
        r_ref = F.relu(y)
        p_ref = _framework_pool(r_ref, mode)
        out = ops.relu_pool2(y, mode, keep_r)
        r, p = out if keep_r else (None, out)
        _same(p, p_ref, f"{mode} pool")
        if keep_r:
            _same(r, r_ref, "relu of relu_pool2")
        _cell_is_absmax(_recalled(p), p_ref, f"{mode} pool")


def _framework_pool_grads(y, mode, dr, dp):
    yy = y.clone().requires_grad_(True)
    r = F.relu(yy)
    p = _framework_pool(r, mode)
    outs, grads = [], []
    if dr is not None:
        outs.append(r), grads.append(dr)
    if dp is not None:
        outs.append(p), grads.append(dp)
    torch.autograd.backward(outs, grads)
    return yy.grad


@pytest.mark.parametrize("shape", POOL_SHAPES)
@pytest.mark.parametrize("mode", ["max", "avg"])
def test_relu_pool2_backward_kernel_bitwise(shape, mode):
    """cocos_relu_pool2_bwd directly: dr / dp each absent, src = r and src = y, against autograd of r -> (r, pool(r))"""
    from cocosnet_amd import _lib, ops
    B, C, H, W = shape
    y = _tied(shape, 30)
    r = F.relu(y)
    dr_full = torch.round(_randn(shape, 31) * 4) / 4          # (exact quarters: dr + dp / 4 has ties in the sums too)
    dp_full = torch.round(_randn((B, C, H // 2, W // 2), 32) * 4) / 4
    for has_dr, has_dp in ((True, True), (True, False), (False, True)):
        dr, dp = (dr_full if has_dr else None), (dp_full if has_dp else None)
        want = _framework_pool_grads(y, mode, dr, dp)
        for src in (r, y):
            dy = torch.full_like(y, float("nan"))
            cell = torch.zeros(1, device=DEV)
            _lib.call("cocos_relu_pool2_bwd", src.data_ptr(), ops._ptr(dr), ops._ptr(dp), dy.data_ptr(), cell.data_ptr(), B * C, H, W,
                      0 if mode == "max" else 1, ops._stream())
            tag = f"{mode} dr={has_dr} dp={has_dp} src={'r' if src is r else 'y'}"
            _same(dy, want, tag)
            _cell_is_absmax(cell, want, tag)


@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (2, 16, 33, 64), (3, 6, 16, 12)])
@pytest.mark.parametrize("mode", ["max", "avg"])
@pytest.mark.parametrize("keep_r", [True, False])
def test_relu_pool2_autograd_bitwise(shape, mode, keep_r):
    """ops.relu_pool2 under autograd (src = r with keep_r, y without) against the framework; the gradient leaves its cell"""
    from cocosnet_amd import ops
    B, C, H, W = shape
    y = _tied(shape, 40)
    dr = _randn(shape, 41)
    dp = _randn((B, C, H // 2, W // 2), 42)
    grads = [(dr, dp), (None, dp), (dr, None)] if keep_r else [(None, dp)]
    for g_r, g_p in grads:
        yy = y.clone().requires_grad_(True)
        seen = _capture_grad(yy)
        out = ops.relu_pool2(yy, mode, keep_r)
        r, p = out if keep_r else (None, out)
        outs = [o for o, g in ((r, g_r), (p, g_p)) if g is not None]
        torch.autograd.backward(outs, [g for g in (g_r, g_p) if g is not None])
        want = _framework_pool_grads(y, mode, g_r, g_p)
        _same(yy.grad, want, f"{mode} keep_r={keep_r} dr={g_r is not None} dp={g_p is not None}")
        assert seen[0] is not None, "no max|.| cell left with the gradient"
        _cell_is_absmax(seen[0], want)


def test_no_cells_under_bf16(monkeypatch):
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", "bf16")
    y = _randn((2, 4, 8, 8), 50)
    assert ops._recall_amax(ops.relu(y), consume=False) is None
    assert ops._recall_amax(ops.relu_pool2(y, "max"), consume=False) is None


# ---- the module ---------------------------------------------------------------------------------------------------------------
def _net(pool="max", nc=False, frozen=True):
    from cocosnet_amd.vgg import VGG19_feature_color_torchversion
    net = VGG19_feature_color_torchversion(pool=pool, vgg_normal_correct=nc)
    net.load_state_dict(vgg_case.state_dict(), strict=True)
    net = net.to(DEV).eval()
    if frozen:
        for q in net.parameters():
            q.requires_grad_(False)
    return net


def _image(B, H, W, nc, seed):
    x = torch.rand(B, 3, H, W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    return x * 2 - 1 if nc else x


def _fwd_bwd(net, x, keys, seed=7):
    xx = x.clone().requires_grad_(True)
    outs = net(xx, keys)
    g = torch.Generator(device=DEV).manual_seed(seed)
    torch.autograd.backward(outs, [torch.randn(o.shape, device=DEV, generator=g) for o in outs])
    return [o.detach() for o in outs], xx.grad


@pytest.mark.parametrize("pool", ["max", "avg"])
def test_module_equals_hip_convs_with_framework_glue_bitwise(pool, monkeypatch):
    """K27 changes no number: with the same K16 convolutions (whose split scale is the exact max|.|, from K27's cell or from its own
    pass) the drop-in's outputs and input gradient equal those of the framework glue bit for bit."""
    from cocosnet_amd import vgg
    net, x = _net(pool, True), _image(2, 64, 96, True, 60)
    outs, dx = _fwd_bwd(net, x, ALL_KEYS)
    monkeypatch.setattr(vgg, "FUSED", False)
    outs_f, dx_f = _fwd_bwd(net, x, ALL_KEYS)
    for k, a, b in zip(ALL_KEYS, outs, outs_f):
        _same(a, b, k)
    _same(dx, dx_f, "input gradient")


def test_no_activation_absmax_pass(monkeypatch):
    from cocosnet_amd import _lib
    net, x = _net("max", False), _image(2, 64, 64, False, 61)
    weights = {q.data_ptr() for q in net.parameters()}
    seen, real_call = [], _lib.call

    def spy(name, *args):
        seen.append((name, args))
        return real_call(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    _fwd_bwd(net, x, STEP_KEYS)
    torch.cuda.synchronize()
    names = [n for n, _ in seen]
    assert names.count("cocos_relu_pool2_fwd") == 4 and names.count("cocos_relu_pool2_bwd") == 4
    assert "cocos_vgg_preprocess_fwd" in names and "cocos_vgg_preprocess_bwd" in names
    assert any("conv" in n for n in names)
    for name, args in seen:
        if name == "cocos_absmax_accumulate":
            assert args[0] in weights, "a max|.| pass over an activation or an activation gradient"
        assert name != "cocos_absmax4"


def _fp64_copy(net):
    seq = {}
    for name, cin, cout in vgg_case.LAYERS:
        c = nn.Conv2d(cin, cout, 3, padding=1).to(DEV).double()
        src = getattr(net, name)
        c.weight.data.copy_(src.weight.detach())
        c.bias.data.copy_(src.bias.detach())
        seq[name] = c
    return seq


def _fp64_forward(convs, x, pool, nc, tape=None):
    """the reference's forward in fp64 from plain nn.Conv2d / F.relu / pools.  `tape` = (relu masks, max-pool indices) of the fp32
    drop-in: replayed instead of the fp64 run's own branches."""
    from cocosnet_amd.vgg import vgg_preprocess_torch
    x = vgg_preprocess_torch(x, nc)
    out = {}
    for key in ALL_KEYS:
        if key[0] == "r":
            y = convs[f"conv{key[1]}_{key[2]}"](x)
            x = out[key] = y * tape[0][key] if tape is not None else F.relu(y)
        else:
            if pool == "avg":
                x = out[key] = F.avg_pool2d(x, 2, 2)
            elif tape is not None:
                idx = tape[1][key]
                x = out[key] = x.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
            else:
                x = out[key] = F.max_pool2d(x, 2, 2)
    return [out[k] for k in ALL_KEYS]


def _rel(a, r):
    return ((a.double() - r).abs().max() / r.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("pool", ["max", "avg"])
@pytest.mark.parametrize("nc", [False, True])
def test_module_against_fp64(pool, nc, monkeypatch):
    """Outputs within 1e-4 of max|ref| per key, and the input gradient within 1e-4 on the drop-in's own branch pattern.  On its OWN
    branches the fp64 copy differs wherever an fp32 value sits within rounding of a ReLU kink or of a tie in a max window (the whole
    gradient of a window then goes to another element): that distance is a property of fp32 itself, so it is held against the
    framework's own fp32 module (its convolutions and glue) at 3x, with 1e-3 as the floor."""
    from cocosnet_amd import ops, vgg
    net = _net(pool, nc)
    x = _image(2, 256, 256, nc, 70)
    outs, dx = _fwd_bwd(net, x, ALL_KEYS, seed=71)
    monkeypatch.setattr(ops, "CONV_PRECISION", "torch")
    monkeypatch.setattr(vgg, "FUSED", False)
    _, dx_framework = _fwd_bwd(net, x, ALL_KEYS, seed=71)
    g = torch.Generator(device=DEV).manual_seed(71)
    grads = [torch.randn(o.shape, device=DEV, generator=g).double() for o in outs]
    convs = _fp64_copy(net)
    masks = {k: (o > 0).double() for k, o in zip(ALL_KEYS, outs) if k[0] == "r"}
    idx = {k: F.max_pool2d(outs[ALL_KEYS.index(k) - 1], 2, 2, return_indices=True)[1] for k in ALL_KEYS if k[0] == "p"}
    errs = {}
    for tag, tape in (("own", None), ("replayed", (masks, idx))):
        xd = x.double().requires_grad_(True)
        ref = _fp64_forward(convs, xd, pool, nc, tape)
        torch.autograd.backward(ref, grads)
        if tape is None:
            for k, a, r in zip(ALL_KEYS, outs, ref):
                errs[k] = _rel(a, r.detach())
        errs["dx_" + tag] = _rel(dx, xd.grad)
        if tape is None:
            errs["dx_own_framework_fp32"] = _rel(dx_framework, xd.grad)
    print(f"\n[vgg fp64] pool={pool} nc={nc} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k in ALL_KEYS:
        assert errs[k] <= 1e-4, (k, errs[k])
    assert errs["dx_replayed"] <= 1e-4, errs["dx_replayed"]
    assert errs["dx_own"] <= max(1e-3, 3 * errs["dx_own_framework_fp32"]), errs


@pytest.mark.parametrize("nc", [0, 1])
def test_module_reproduces_the_reference_golden(nc):
    g = np.load(os.path.join(GOLDEN, f"vgg19_nc{nc}.npz"))
    net = _net("max", bool(nc))
    x = torch.from_numpy(g["x"]).to(DEV).requires_grad_(True)
    outs = net(x, list(vgg_case.GOLDEN_KEYS))
    vgg_case.loss(outs).backward()
    errs = {k: _rel(o.detach(), torch.from_numpy(g[k]).to(DEV).double()) for k, o in zip(vgg_case.GOLDEN_KEYS, outs)}
    errs["dx"] = _rel(x.grad, torch.from_numpy(g["dx"]).to(DEV).double())
    print(f"\n[vgg golden] nc={nc} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-4, errs


def test_maps_without_a_window_take_the_framework_route_and_its_error():
    """A map smaller than one 2x2 window: the kernel's COCOS_ERR_UNSUPPORTED sends the pool to the framework, which raises as the
    reference's pool does."""
    from cocosnet_amd import ops
    net = _net("max", False)
    y = _randn((1, 4, 1, 6), 80)
    with pytest.raises(ops._lib.CocosHipError) as e:
        ops.relu_pool2(y, "max")
    assert e.value.code == -2
    with pytest.raises(RuntimeError, match="too small"):
        net._relu_pool(y, net.pool1, False)


# ---- live pointers (the guard idea of test_gpu_live_buffers.py) ---------------------------------------------------------------
def _live_blocks():
    blocks = []
    for seg in torch.cuda.memory_snapshot():
        addr = seg["address"]
        for b in seg["blocks"]:
            blocks.append((addr, b["size"], b["state"] == "active_allocated"))
            addr += b["size"]
    blocks.sort()
    return blocks


def test_every_pointer_argument_is_a_live_allocation(monkeypatch):
    from cocosnet_amd import _lib
    calls, pointers, dead = [0], [0], []
    real_call, sigs = _lib.call, _lib._SIGNATURES

    def checked_call(name, *args):
        blocks = _live_blocks()
        starts = [b[0] for b in blocks]
        for i, (a, ty) in enumerate(zip(args, sigs[name][1])):
            if ty is not ctypes.c_void_p or not isinstance(a, int) or a == 0:
                continue
            j = bisect.bisect_right(starts, a) - 1
            if j < 0 or a >= blocks[j][0] + blocks[j][1]:
                continue
            pointers[0] += 1
            if not blocks[j][2]:
                dead.append((name, i, hex(a), blocks[j][1]))
        calls[0] += 1
        return real_call(name, *args)

    net, x = _net("max", True), _image(2, 48, 64, True, 90)
    monkeypatch.setattr(_lib, "call", checked_call)
    _fwd_bwd(net, x, ["r11", "p1", "r22", "r32", "p3", "r42", "r52"])
    _fwd_bwd(_net("avg", False), x, STEP_KEYS)
    torch.cuda.synchronize()
    assert calls[0] >= 60 and pointers[0] >= 150, (calls[0], pointers[0])
    assert not dead, f"pointers into freed blocks at call time: {dead[:8]}"


# ---- memory and determinism ---------------------------------------------------------------------------------------------------
def _peak_fwd_bwd(net, x):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    _fwd_bwd(net, x, STEP_KEYS)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_peak_memory_below_the_framework_glue(monkeypatch):
    from cocosnet_amd import vgg
    net, x = _net("max", False), _image(4, 256, 256, False, 100)
    _peak_fwd_bwd(net, x)                        # (warm: workspaces, cells)
    fused = _peak_fwd_bwd(net, x)
    monkeypatch.setattr(vgg, "FUSED", False)
    _peak_fwd_bwd(net, x)
    framework = _peak_fwd_bwd(net, x)
    print(f"\n[vgg memory] fwd + input bwd peak: drop-in {fused / 2**20:.0f} MiB, framework glue {framework / 2**20:.0f} MiB")
    assert fused < framework


def test_forward_only_call_saves_nothing():
    net, x = _net("max", False), _image(2, 64, 64, False, 110)
    packed = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: packed.append(t.shape) or t, lambda t: t):
        outs = net(x, STEP_KEYS)
    assert not packed, packed[:4]
    assert all(o.grad_fn is None for o in outs)


@pytest.mark.parametrize("pool", ["max", "avg"])
def test_deterministic(pool):
    net, x = _net(pool, False), _image(2, 128, 128, False, 120)
    a_outs, a_dx = _fwd_bwd(net, x, ALL_KEYS)
    b_outs, b_dx = _fwd_bwd(net, x, ALL_KEYS)
    for k, a, b in zip(ALL_KEYS, a_outs, b_outs):
        assert torch.equal(a, b), k
    assert torch.equal(a_dx, b_dx)
