"""K26 (cocosnet_amd/csrc/norm_spade.hip, ops.norm_spade): parameter-free batch / sync-batch / instance norm + SPADE modulation +
LeakyReLU, forward and backward, against the fp64 framework formulation; running buffers against nn.BatchNorm2d; two ranks emulated
on one GPU; accuracy under a large mean; determinism; the route taken by non-PONO SPADE; and the networks against fp64 copies."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(2, 16, 12, 12), (1, 5, 7, 9), (3, 64, 32, 32), (2, 8, 160, 160), (4, 1024, 8, 8)]


@pytest.fixture(autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _inputs(shape, seed, offset=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(shape, device="cuda", generator=g) * 1.5 + 0.3 + offset
    gamma = torch.randn(shape, device="cuda", generator=g) * 0.5
    beta = torch.randn(shape, device="cuda", generator=g) * 0.5
    dy = torch.randn(shape, device="cuda", generator=g)
    return x, gamma, beta, dy


def _ref_norm(kind, x, rm, rv, use_batch, eps=1e-5):
    if kind == "instance":
        return F.instance_norm(x, eps=eps)
    return F.batch_norm(x, rm, rv, training=use_batch, momentum=0.0, eps=eps)


def _fp64_reference(kind, x, gamma, beta, dy, y32, slope, rm=None, rv=None, use_batch=True):
    """The framework formulation in fp64, on the fp32 arm's branch pattern (no comparison straddles a LeakyReLU kink)."""
    xd, gd, bd = (t.detach().double().requires_grad_(True) for t in (x, gamma, beta))
    z = _ref_norm(kind, xd, None if rm is None else rm.double(), None if rv is None else rv.double(), use_batch) * (1 + gd) + bd
    mult = torch.where(y32.detach() > 0, 1.0, slope).double() if slope != 1.0 else 1.0
    y = z * mult
    y.backward(dy.double())
    return y.detach(), xd.grad, gd.grad, bd.grad


def _close(a, r, tol, what):
    err = ((a.double() - r).abs() / r.abs().clamp_min(1.0)).max().item()
    assert err <= tol, f"{what}: {err:.3e}"


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind,training", [("batch", True), ("batch", False), ("syncbatch", True), ("syncbatch", False),
                                           ("instance", True)])
@pytest.mark.parametrize("slope", [0.2, 1.0])
def test_operator_matches_fp64(shape, kind, training, slope):
    from cocosnet_amd import ops
    x, gamma, beta, dy = _inputs(shape, 3)
    C = shape[1]
    rm = rv = None
    if kind != "instance":
        g = torch.Generator(device="cuda").manual_seed(5)
        rm = torch.randn(C, device="cuda", generator=g) * 0.3
        rv = torch.rand(C, device="cuda", generator=g) * 1.5 + 0.5
    xa, ga, ba = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    rm32 = None if rm is None else rm.clone()
    rv32 = None if rv is None else rv.clone()
    y = ops.norm_spade(xa, ga, ba, kind, rm32, rv32, None, training=training, momentum=0.1, slope=slope)
    y.backward(dy)
    ref = _fp64_reference(kind, x, gamma, beta, dy, y, slope, rm, rv, use_batch=training)
    for a, r, what in zip((y, xa.grad, ga.grad, ba.grad), ref, ("y", "dx", "dgamma", "dbeta")):
        _close(a, r, 1e-5, f"{kind} train={training} slope={slope} {shape} {what}")


@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("kind", ["batch", "syncbatch"])
def test_running_buffers_follow_batchnorm2d(momentum, kind):
    from cocosnet_amd import ops
    from cocosnet_amd.dist import SyncBatchNorm2d
    shape = (3, 24, 10, 14)
    C = shape[1]
    ours = (nn.BatchNorm2d if kind == "batch" else SyncBatchNorm2d)(C, affine=False, momentum=momentum).cuda()
    ref = nn.BatchNorm2d(C, affine=False, momentum=momentum).cuda().double()
    for step in range(3):
        x, gamma, beta, _ = _inputs(shape, 10 + step, offset=step)
        ops.norm_spade(x, gamma, beta, kind, ours.running_mean, ours.running_var, ours.num_batches_tracked, True, momentum)
        ref(x.double())
    assert int(ours.num_batches_tracked) == int(ref.num_batches_tracked) == 3
    for a, r in ((ours.running_mean, ref.running_mean), (ours.running_var, ref.running_var)):
        assert ((a.double() - r).abs() / r.abs().clamp_min(1e-3)).max().item() <= 1e-6
    ref.eval()
    x, gamma, beta, _ = _inputs(shape, 99)
    y = ops.norm_spade(x, gamma, beta, kind, ours.running_mean, ours.running_var, ours.num_batches_tracked, False, momentum, slope=0.2)
    yr = F.leaky_relu(ref(x.double()) * (1 + gamma.double()) + beta.double(), 0.2)
    _close(y, yr, 1e-5, "eval after three steps")


@pytest.mark.parametrize("shape", [(4, 16, 12, 12), (2, 8, 160, 160), (4, 64, 7, 9)])
def test_two_ranks_on_one_gpu_equal_the_full_batch(shape):
    """The low-level steps per half of a batch, statistics combined between them as the Function does with a live group."""
    from cocosnet_amd import ops
    x, gamma, beta, dy = _inputs(shape, 7)
    slope, eps = 0.2, 1e-5
    xa, ga, ba = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    y_full = ops.norm_spade(xa, ga, ba, "syncbatch", slope=slope)
    y_full.backward(dy)
    full = ops.norm_spade_stats(x, False, eps)
    h = shape[0] // 2
    halves = [slice(0, h), slice(h, shape[0])]
    parts = [ops.norm_spade_stats(x[s].contiguous(), False, eps) for s in halves]
    merged = ops.merge_norm_stats(torch.stack(parts), eps)
    for i, what in ((0, "count"), (1, "mean"), (2, "M2"), (3, "invstd")):
        err = ((merged[i].double() - full[i].double()).abs() / full[i].double().abs().clamp_min(1e-6)).max().item()
        assert err <= 1e-6, (what, err)
    mean, invstd = merged[1].contiguous(), merged[3].contiguous()
    ins = [[t[s].contiguous() for t in (x, gamma, beta, dy)] for s in halves]
    sums = sum(ops.norm_spade_bwd_stats(xi, gi, bi, di, mean, invstd, False, slope) for xi, gi, bi, di in ins)
    inv_count = 1.0 / float(merged[0, 0])
    for s, (xi, gi, bi, di) in zip(halves, ins):
        yi = ops.norm_spade_apply(xi, gi, bi, mean, invstd, False, slope)
        dxi, dgi, dbi = ops.norm_spade_bwd_apply(xi, gi, bi, di, mean, invstd, sums.contiguous(), inv_count, False, slope)
        for a, r, what in ((yi, y_full[s], "y"), (dxi, xa.grad[s], "dx"), (dgi, ga.grad[s], "dgamma"), (dbi, ba.grad[s], "dbeta")):
            err = (a - r).abs().max().item()
            assert err <= 1e-6 * max(1.0, r.abs().max().item()), (what, err)


@pytest.mark.parametrize("kind", ["batch", "instance"])
def test_accuracy_under_a_large_mean(kind):
    """x = 100 + N(0, 1): sum x^2 - n mean^2 in fp32 loses the variance; the Welford / Chan statistics do not."""
    from cocosnet_amd import ops
    shape = (4, 32, 64, 64)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = 100.0 + torch.randn(shape, device="cuda", generator=g)
    gamma = torch.randn(shape, device="cuda", generator=g) * 0.5
    beta = torch.randn(shape, device="cuda", generator=g) * 0.5
    y = ops.norm_spade(x, gamma, beta, kind, slope=1.0)
    yr = _ref_norm(kind, x.double(), None, None, True) * (1 + gamma.double()) + beta.double()
    assert (y.double() - yr).abs().max().item() <= 2e-5


def test_forward_and_backward_are_bitwise_reproducible():
    from cocosnet_amd import ops
    shape = (16, 128, 64, 64)
    x, gamma, beta, dy = _inputs(shape, 4)

    def run(kind):
        xa, ga, ba = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
        y = ops.norm_spade(xa, ga, ba, kind, slope=0.2)
        y.backward(dy)
        return [y.detach(), xa.grad, ga.grad, ba.grad]
    for kind in ("batch", "instance"):
        a, b = run(kind), run(kind)
        for u, v in zip(a, b):
            assert torch.equal(u, v), kind


_VIEW_OPS = {"aten::empty", "aten::empty_like", "aten::empty_strided", "aten::contiguous", "aten::view", "aten::reshape",
             "aten::detach", "aten::alias", "aten::as_strided", "aten::clone", "aten::slice", "aten::select", "aten::expand"}


@pytest.mark.parametrize("kind", ["batch", "syncbatch", "instance"])
def test_non_pono_spade_takes_the_fused_route(kind):
    """One non-PONO SPADE norm + modulate, forward and backward, under the profiler: no framework batch / instance norm kernel,
    no K17, no framework op over a full-size tensor (small per-channel ops are allowed); K26's kernels are there."""
    from torch.profiler import ProfilerActivity, profile
    from cocosnet_amd import spade
    from cocosnet_amd.dist import SyncBatchNorm2d
    shape = (2, 64, 32, 32)
    C = shape[1]
    m = {"batch": lambda: nn.BatchNorm2d(C, affine=False), "syncbatch": lambda: SyncBatchNorm2d(C, affine=False),
         "instance": lambda: nn.InstanceNorm2d(C, affine=False)}[kind]().cuda()
    x, gamma, beta, dy = _inputs(shape, 8)
    x.requires_grad_(True); gamma.requires_grad_(True); beta.requires_grad_(True)
    y = spade.modulate(x, gamma, beta, False, m, 0.2)             # warm-up (workspace pools, code objects)
    y.backward(dy)
    torch.cuda.synchronize()
    x.grad = gamma.grad = beta.grad = None      # (a second backward would ADD into the leaves' .grad: the test's own full-size op)
    launches = {}
    for direction in ("forward", "backward"):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], record_shapes=True) as prof:
            if direction == "forward":
                y = spade.modulate(x, gamma, beta, False, m, 0.2)
            else:
                y.backward(dy)
            torch.cuda.synchronize()
        events = prof.events()
        kernels = [e.name for e in events if e.device_type == torch.autograd.DeviceType.CUDA]
        for k in kernels:
            low = k.lower()
            assert "batch_norm" not in low and "instance_norm" not in low and "spade_modulate" not in low, (direction, k)
        assert any("cocos::ns_" in k for k in kernels), (direction, kernels)
        full = [e.name for e in events if e.name.startswith("aten::") and e.name not in _VIEW_OPS
                and any(list(s) == list(shape) for s in (e.input_shapes or []) if isinstance(s, (list, tuple)))]
        assert not full, (direction, full)
        launches[direction] = len(kernels)
    print(f"NORM_SPADE_LAUNCHES {kind} {launches}")


def _train_param_free_norms(net):
    from cocosnet_amd.dist import SyncBatchNorm2d
    n = 0
    for mod in net.modules():
        if type(mod) in (nn.BatchNorm2d, nn.InstanceNorm2d, SyncBatchNorm2d) and not mod.affine:
            mod.train()
            n += 1
    return n


def _corr_vs_fp64(overrides, forced):
    """NoVGGCorrespondence.project() (the adaptors' non-PONO SPADE blocks, the residual blocks, theta / phi) against an fp64 copy of
    itself: the network in eval mode (frozen spectral norms), its parameter-free norms in training mode (batch statistics)."""
    import kink_tape
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd import ops
    opt = cc.ade20k_options(**overrides)
    torch.manual_seed(0)
    net = cc.NoVGGCorrespondence(opt).cuda()
    net.init_weights(opt.init_type, opt.init_variance)
    net.eval()
    assert _train_param_free_norms(net) > 0
    B, size, nc = 2, 64, opt.semantic_nc
    g = torch.Generator(device="cuda").manual_seed(2)
    img = torch.rand(B, 3, size, size, device="cuda", generator=g) * 2 - 1
    real = torch.rand(B, 3, size, size, device="cuda", generator=g) * 2 - 1
    lab = torch.randint(0, nc, (B, 1, size // 8, size // 8), device="cuda", generator=g).repeat_interleave(8, 2).repeat_interleave(8, 3)
    seg = torch.zeros(B, nc, size, size, device="cuda").scatter_(1, lab, 1.0)
    ref_seg = seg.flip(0).contiguous()
    net64 = copy.deepcopy(net).double()
    probes = {"theta.weight": lambda n: n.theta.weight, "phi.bias": lambda n: n.phi.bias,
              "adaptive_model_seg.head_0.norm_0.mlp_gamma.weight": lambda n: n.adaptive_model_seg.head_0.norm_0.mlp_gamma.weight,
              "adaptive_model_img.G_middle_1.norm_1.mlp_beta.weight": lambda n: n.adaptive_model_img.G_middle_1.norm_1.mlp_beta.weight,
              "adaptive_model_seg.G_middle_1.conv_0.weight_orig": lambda n: n.adaptive_model_seg.G_middle_1.conv_0.weight_orig,
              "adaptive_model_img.layer1.0.weight_orig": lambda n: n.adaptive_model_img.layer1[0].weight_orig,
              "layer.0.conv1.weight": lambda n: n.layer[0].conv1.weight}
    tape = kink_tape.KinkTape() if forced else None

    def run(m, dt, G=None):
        m.zero_grad()
        th, ph = m.project(img.to(dt), real.to(dt), seg.to(dt), ref_seg.to(dt))
        if G is None:
            G = [torch.randn(t.shape, device="cuda", generator=g) for t in (th, ph)]
        torch.autograd.backward([th, ph], [G[0].to(dt), G[1].to(dt)])
        out = {"theta_raw": th.detach(), "phi_raw": ph.detach()}
        out.update({"d " + k: f(m).grad.clone() for k, f in probes.items()})
        return out, G
    with kink_tape.install(tape):
        want, G = run(net64, torch.float64)
        if tape is not None:
            tape.rewind("replay")
        with ops.KernelTimer() as kt:
            got, _ = run(net, torch.float32, G)
        assert "norm_spade_fwd" in kt.summary() and "norm_spade_bwd" in kt.summary()
    return {k: float((got[k].double() - want[k]).abs().max() / (want[k].abs().max() + 1e-300)) for k in want}


CORR_FLAGS = {"syncbatch": dict(semantic_nc=6, PONO=False, isTrain=True),
              "instance": dict(semantic_nc=6, PONO=False, isTrain=True, norm_G="spectralspadeinstance3x3")}


@pytest.mark.parametrize("name", sorted(CORR_FLAGS))
def test_netcorr_non_pono_against_an_fp64_copy(name):
    errs = _corr_vs_fp64(CORR_FLAGS[name], forced=False)
    print("NORM_SPADE_E2E", name, errs)
    for k in ("theta_raw", "phi_raw", "d theta.weight", "d phi.bias"):
        assert errs[k] < 1e-3, (k, errs)


@pytest.mark.parametrize("name", sorted(CORR_FLAGS))
def test_netcorr_non_pono_every_gradient_on_the_fp64_branch_pattern(name):
    errs = _corr_vs_fp64(CORR_FLAGS[name], forced=True)
    print("NORM_SPADE_E2E_FORCED", name, errs)
    bad = {k: v for k, v in errs.items() if not v < 1e-3}
    assert not bad, bad


def _generator_vs_fp64(forced):
    import kink_tape
    from cocosnet_amd import ops, translation as tl
    opt = tl.celebahq_edge_train_options(PONO=False)
    torch.manual_seed(0)
    G = tl.SPADEGenerator(opt).cuda()
    G.init_weights(opt.init_type, opt.init_variance)
    G.eval()
    assert _train_param_free_norms(G) > 0
    g = torch.Generator(device="cuda").manual_seed(21)
    B = 2
    seg = torch.rand(B, 15, 256, 256, device="cuda", generator=g)
    cbn = torch.cat((torch.rand(B, 3, 256, 256, device="cuda", generator=g) * 2 - 1, seg), 1)
    gy = torch.randn(B, 3, 256, 256, device="cuda", generator=g)
    probes = {"fc.weight": lambda n: n.fc.weight, "conv_img.weight": lambda n: n.conv_img.weight,
              "up_3.conv_1.weight_orig": lambda n: n.up_3.conv_1.weight_orig, "head_0.conv_0.weight_orig": lambda n: n.head_0.conv_0.weight_orig,
              "up_1.norm_0.mlp_gamma.weight": lambda n: n.up_1.norm_0.mlp_gamma.weight}
    G64 = copy.deepcopy(G).double()

    def run(m, dt):
        m.zero_grad()
        y = m(seg.to(dt), warp_out=cbn.to(dt))
        y.backward(gy.to(dt))
        out = {"fake_image": y.detach()}
        out.update({"d " + k: f(m).grad.clone() for k, f in probes.items()})
        return out
    tape = kink_tape.KinkTape() if forced else None
    with kink_tape.install(tape):
        want = run(G64, torch.float64)
        if tape is not None:
            tape.rewind("replay")
        with ops.KernelTimer() as kt:
            got = run(G, torch.float32)
        assert "norm_spade_fwd" in kt.summary()
    return {k: float((got[k].double() - want[k]).abs().max() / (want[k].abs().max() + 1e-300)) for k in want}


def test_generator_non_pono_against_an_fp64_copy():
    errs = _generator_vs_fp64(forced=False)
    print("NORM_SPADE_GEN", errs)
    assert errs["fake_image"] < 1e-3, errs


def test_generator_non_pono_every_gradient_on_the_fp64_branch_pattern():
    errs = _generator_vs_fp64(forced=True)
    print("NORM_SPADE_GEN_FORCED", errs)
    bad = {k: v for k, v in errs.items() if not v < 1e-3}
    assert not bad, bad
