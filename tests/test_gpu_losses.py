"""K28 on the GPU: each loss kernel against an fp64 restatement on the same fp32 inputs and against the framework's own fp32 ops, the
gradients against the framework's autograd, determinism, no host synchronisation, the whole block against the reference-generated
goldens, the launch and memory budget, and live pointers.

Bounds (from the arithmetic, not from a run): per element at most two fp32 roundings, fp64 sums, one final rounding, so
  pair_loss, gan_loss hinge / ls / w:  |err| <= 2^-22 x (the same loss with every term replaced by its absolute value);
  gan_loss original, mask_nll:         one logf / expf-class call per term in addition: |err| <= 2^-21 x (1 + weighted mean |log|);
  every case:                          |err| <= 2 x the framework's fp32 error on the same input + one fp32 ulp of the result;
  gradients:                           <= 2^-22 relative per element against the framework's autograd, exact zeros where it has them.
For gan_mode 'original' the framework's gradient is `sigmoid(x) - label` formed in fp32: a difference that cancels, so its own
per-element RELATIVE error has no bound and no independent kernel can sit within 2^-22 of it element by element.  There the bound is
2^-22 of the factor g / (n T) that multiplies a number in [-1, 1] (absolute, the rounding of the sigmoid), checked against fp64."""
import bisect
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E22, E21 = 2.0 ** -22, 2.0 ** -21


def _ulp(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def _check_value(got, want64, fw32, denom, bound, what):
    """got / fw32: fp32 results of ours / the framework; want64: fp64 restatement; denom: the bound's scale"""
    err, fw_err = abs(float(got) - float(want64)), abs(float(fw32) - float(want64))
    print(f"{what}: ours {float(got):.9g} fp64 {float(want64):.9g} err {err:.3g} bound {bound * float(denom):.3g} framework err {fw_err:.3g}")
    assert err <= bound * float(denom), (what, err, bound * float(denom))
    assert err <= 2 * fw_err + _ulp(want64), (what, err, fw_err)


def _check_grad(got, want, what, rel=E22):
    assert got.shape == want.shape, what
    g, w = got.double(), want.double()
    err = (g - w).abs()
    worst = float((err / w.abs().clamp_min(1e-300)).max()) if w.numel() else 0.0
    print(f"{what}: worst relative gradient error {worst:.3g}")
    assert bool((err <= rel * w.abs()).all()), (what, worst)
    assert bool((got[want == 0] == 0).all()), what


def _rand(g, *shape, ints=False):
    x = torch.randn(*shape, device=DEV, generator=g)
    return (x * 2).round() if ints else x


# ---- pair_loss --------------------------------------------------------------------------------------------------------------------
def _pair_fw(a, b, w, c1, c2):
    """the framework's op sequence (util.weighted_l1_loss / F.l1_loss / util.mse_loss) in a's dtype"""
    d = a - b if b is not None else a - 0
    l1 = torch.abs(d)
    if w is not None:
        l1 = l1 * w.view(-1, *([1] * (a.dim() - 1))).expand_as(l1)
    return c1 * l1.mean(), c2 * torch.mean(d ** 2)


PAIR_CASES = {
    "aligned_w": dict(shape=(8, 16, 32, 32), w=True, b=True, c=(0.25, 0.0)),
    "both_coefficients": dict(shape=(4, 8, 16, 16), w=True, b=True, c=(0.125, 1.0)),
    "ties": dict(shape=(4, 8, 16, 16), w=False, b=True, c=(1.0, 1.0), ints=True),
    "null_b": dict(shape=(2, 3, 40, 40), w=False, b=False, c=(0.0, 1.0)),
    "null_w_odd_n": dict(shape=(3, 5, 7, 11), w=False, b=True, c=(10.0, 0.0)),
    "inner_not_multiple_of_4": dict(shape=(4, 3, 5, 7), w=True, b=True, c=(1.0, 0.5)),
    "unaligned_slices": dict(shape=(4, 8, 9, 9), w=False, b=True, c=(5.0, 0.0), slices=True),
    "n_1": dict(shape=(1,), w=False, b=True, c=(1.0, 1.0)),
    "n_2pow25": dict(shape=(8, (1 << 22) + 1), w=True, b=True, c=(1.0, 0.0)),
}


def _pair_inputs(cfg, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    shape = cfg["shape"]
    if cfg.get("slices"):          # the two halves of a batch-concatenated tensor, off by one element: 4-byte alignment only
        flat = _rand(g, 2 * int(np.prod(shape)) + 1)
        n = int(np.prod(shape))
        a, b = flat[1:n + 1].view(shape), flat[n + 1:].view(shape)
        assert a.data_ptr() % 16 != 0 and a.is_contiguous()
    else:
        a = _rand(g, *shape, ints=cfg.get("ints", False))
        b = _rand(g, *shape, ints=cfg.get("ints", False)) if cfg["b"] else None
    w = torch.rand(shape[0], device=DEV, generator=g) if cfg["w"] else None
    return a, b, w


@pytest.mark.parametrize("name", sorted(PAIR_CASES))
def test_pair_loss_against_fp64_and_framework(name, hip_lib):
    from cocosnet_amd import ops
    cfg = PAIR_CASES[name]
    a, b, w = _pair_inputs(cfg, 11)
    c1, c2 = cfg["c"]
    if not cfg.get("slices"):
        a_k = leaf = a.clone().requires_grad_(True)
    else:
        base = a._base.detach().clone().requires_grad_(True)
        n = a.numel()
        a_k, b = base[1:n + 1].view(a.shape), base[n + 1:].view(a.shape).detach()
        leaf = base
    out = ops.pair_loss([(a_k, b, w, c1, c2)])
    assert out.shape == (2, 2) and torch.equal(out[0], out[1])
    out2 = ops.pair_loss([(a_k, b, w, c1, c2)])
    assert torch.equal(out, out2)                                   # determinism
    gout = torch.tensor([[0.7, 0.0], [0.0, 1.3]], device=DEV)       # L1 through its own cell, MSE through the sum cell
    grad, = torch.autograd.grad((out * gout).sum(), leaf)
    grad2, = torch.autograd.grad((out2 * gout).sum(), leaf)
    assert torch.equal(grad, grad2)
    # framework fp32 + autograd, fp64 restatement
    a_f = a_k.detach().clone().requires_grad_(True)
    l1_f, l2_f = _pair_fw(a_f, b, w, c1, c2)
    grad_f, = torch.autograd.grad(0.7 * l1_f + 1.3 * l2_f, a_f)
    l1_d, l2_d = _pair_fw(a_k.detach().double(), None if b is None else b.double(), None if w is None else w.double(), c1, c2)
    if c1:
        _check_value(out[0, 0], l1_d, l1_f, l1_d, E22, name + " L1")
    else:
        assert float(out[0, 0]) == 0
    if c2:
        _check_value(out[0, 1], l2_d, l2_f, l2_d, E22, name + " MSE")
    else:
        assert float(out[0, 1]) == 0
    got = grad[1:a.numel() + 1].view(a.shape) if cfg.get("slices") else grad
    _check_grad(got, grad_f, name)
    if cfg.get("slices"):
        assert float(grad[0]) == 0 and bool((grad[a.numel() + 1:] == 0).all())      # b receives none
    if cfg.get("ints"):
        ties = (a_k.detach() == b)
        assert int(ties.sum()) > 100 and bool((got[ties] == 0).all())


def test_pair_loss_sixteen_segments(hip_lib):
    from cocosnet_amd import ops
    g = torch.Generator(device=DEV).manual_seed(16)
    shapes = [(2, 3 + i, 5, 4 + (i % 3)) for i in range(16)]
    A = [_rand(g, *s).requires_grad_(True) for s in shapes]
    Bs = [_rand(g, *s) for s in shapes]
    W = [torch.rand(2, device=DEV, generator=g) if i % 2 else None for i in range(16)]
    cs = [(0.5 + i, float(i % 3 == 0)) for i in range(16)]
    out = ops.pair_loss([(a, b, w, c1, c2) for a, b, w, (c1, c2) in zip(A, Bs, W, cs)])
    assert out.shape == (17, 2)
    grads = torch.autograd.grad(out[16].sum(), A)
    tot1 = tot2 = 0.0
    for i in range(16):
        a_f = A[i].detach().clone().requires_grad_(True)
        l1_f, l2_f = _pair_fw(a_f, Bs[i], W[i], *cs[i])
        l1_d, l2_d = _pair_fw(A[i].detach().double(), Bs[i].double(), None if W[i] is None else W[i].double(), *cs[i])
        _check_value(out[i, 0], l1_d, l1_f, l1_d, E22, f"segment {i} L1")
        if cs[i][1]:
            _check_value(out[i, 1], l2_d, l2_f, l2_d, E22, f"segment {i} MSE")
        _check_grad(grads[i], torch.autograd.grad(l1_f + l2_f, a_f)[0], f"segment {i}")
        tot1, tot2 = tot1 + float(l1_d), tot2 + float(l2_d)
    assert abs(float(out[16, 0]) - tot1) <= E22 * tot1 and abs(float(out[16, 1]) - tot2) <= E22 * tot2
    with pytest.raises(ValueError):
        ops.pair_loss([(A[0], Bs[0], None, 1.0, 0.0)] * 17)


def test_pair_loss_copy_rate_inputs_need_no_gradient(hip_lib):
    """an input that needs no gradient gets none (and no workgroup); a segment list where nothing needs one still runs forward"""
    from cocosnet_amd import ops
    g = torch.Generator(device=DEV).manual_seed(2)
    a0, a1, b = _rand(g, 2, 8, 8), _rand(g, 2, 8, 8).requires_grad_(True), _rand(g, 2, 8, 8)
    out = ops.pair_loss([(a0, b, None, 1.0, 0.0), (a1, b, None, 1.0, 1.0)])
    out[2].sum().backward()
    assert a0.grad is None and a1.grad is not None and b.grad is None
    assert not ops.pair_loss([(a0, b, None, 1.0, 0.0)]).requires_grad


# ---- gan_loss ---------------------------------------------------------------------------------------------------------------------
def _gan_fw(xs, mode, label):
    tot = 0
    for x in xs:
        if mode == "hinge_d_real":
            m = -torch.mean(torch.min(x - 1, torch.zeros(1, device=x.device, dtype=x.dtype).expand_as(x)))
        elif mode == "hinge_d_fake":
            m = -torch.mean(torch.min(-x - 1, torch.zeros(1, device=x.device, dtype=x.dtype).expand_as(x)))
        elif mode == "neg_mean":
            m = -torch.mean(x)
        elif mode == "mean":
            m = torch.mean(x)
        elif mode == "ls":
            m = F.mse_loss(x, torch.full((1,), label, device=x.device, dtype=x.dtype).expand_as(x))
        else:
            m = F.binary_cross_entropy_with_logits(x, torch.full((1,), label, device=x.device, dtype=x.dtype).expand_as(x))
        tot = tot + torch.mean(m.view(1, -1), dim=1)
    return tot / len(xs)


def _gan_abs(xs, mode, label):
    """the same loss with every term replaced by its absolute value (fp64)"""
    tot = 0.0
    for x in xs:
        x = x.double()
        if mode == "hinge_d_real":
            t = torch.min(x - 1, torch.zeros_like(x)).abs()
        elif mode == "hinge_d_fake":
            t = torch.min(-x - 1, torch.zeros_like(x)).abs()
        elif mode in ("neg_mean", "mean"):
            t = x.abs()
        elif mode == "ls":
            t = (x - label) ** 2
        else:
            t = ((1 - label) * x).abs() + F.logsigmoid(x).abs()
        tot += float(t.mean())
    return tot / len(xs)


@pytest.mark.parametrize("mode,label", [("hinge_d_real", 0.0), ("hinge_d_fake", 0.0), ("neg_mean", 0.0), ("mean", 0.0), ("ls", 1.0),
                                        ("ls", 0.0), ("bce", 1.0), ("bce", 0.0), ("bce", 0.9)])
def test_gan_loss_against_fp64_and_framework(mode, label, hip_lib):
    from cocosnet_amd import ops
    g = torch.Generator(device=DEV).manual_seed(7)
    xs = [_rand(g, 8, 1, 35, 35), _rand(g, 8, 1, 19, 19), _rand(g, 3, 1, 1, 1), _rand(g, 1 << 21)[1:]]      # the last: unaligned
    xs[0].view(-1)[:200] = 1.0           # hinge arguments exactly at the kinks
    xs[0].view(-1)[200:400] = -1.0
    xs = [x.requires_grad_(True) for x in xs]
    out = ops.gan_loss(xs, mode, label)
    assert out.shape == (1,) and torch.equal(out, ops.gan_loss(xs, mode, label))
    grads = torch.autograd.grad(out.sum() * 1.7, xs)
    assert all(torch.equal(a, b) for a, b in zip(grads, torch.autograd.grad(ops.gan_loss(xs, mode, label).sum() * 1.7, xs)))
    xf = [x.detach().clone().requires_grad_(True) for x in xs]
    fw = _gan_fw(xf, mode, label)
    want = _gan_fw([x.detach().double() for x in xs], mode, label)
    if mode == "bce":
        _check_value(out, want, fw, 1 + _gan_abs(xs, mode, label), E21, f"{mode} {label}")
    else:
        _check_value(out, want, fw, _gan_abs(xs, mode, label), E22, f"{mode} {label}")
    grads_f = torch.autograd.grad(fw.sum() * 1.7, xf)
    if mode == "bce":        # see the module docstring: absolute, against fp64
        xd = [x.detach().double().requires_grad_(True) for x in xs]
        grads_d = torch.autograd.grad(_gan_fw(xd, mode, label).sum() * 1.7, xd)
        for i, (gk, gd, gf) in enumerate(zip(grads, grads_d, grads_f)):
            scale = 1.7 / (xs[i].numel() * len(xs))
            err, fw_err = float((gk.double() - gd).abs().max()), float((gf.double() - gd).abs().max())
            print(f"bce {label} tensor {i}: gradient error {err:.3g} (framework {fw_err:.3g}), bound {E22 * scale:.3g}")
            assert err <= E22 * scale and err <= 2 * fw_err + _ulp(scale)
    else:
        for i, (gk, gf) in enumerate(zip(grads, grads_f)):
            _check_grad(gk, gf, f"{mode} {label} tensor {i}")


def test_ganloss_module_on_the_gpu_matches_its_framework_route(hip_lib, monkeypatch):
    from cocosnet_amd import losses
    g = torch.Generator(device=DEV).manual_seed(8)
    nested = [[_rand(g, 4, 8, 9, 9), _rand(g, 4, 1, 6, 6)], [_rand(g, 4, 8, 5, 5), _rand(g, 4, 1, 3, 3)]]
    for gan_mode in ("hinge", "ls", "original", "w"):
        crit = losses.GANLoss(gan_mode, tensor=torch.cuda.FloatTensor)
        for real, for_d in ((True, True), (False, True), (True, False)):
            monkeypatch.setattr(losses, "FUSED", True)
            got, got_t = crit(nested, real, for_d), crit(nested[0][1], real, for_d)
            monkeypatch.setattr(losses, "FUSED", False)
            want, want_t = crit(nested, real, for_d), crit(nested[0][1], real, for_d)
            assert got.shape == want.shape == (1,) and got_t.shape == want_t.shape == ()
            assert abs(float(got) - float(want)) <= 1e-6 * (1 + abs(float(want))) and abs(float(got_t) - float(want_t)) <= 1e-6 * (1 + abs(float(want_t)))


# ---- mask_nll ---------------------------------------------------------------------------------------------------------------------
def _mask_inputs(nc, B, H, W, Hr, Wr, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.softmax(torch.randn(B, nc, H // 4, W // 4, device=DEV, generator=g) * 3, dim=1)
    gt = torch.randint(0, nc, (B, 1, H, W), device=DEV, generator=g)
    ref = torch.randint(0, max(nc // 2, 1) + 1, (B, 1, Hr, Wr), device=DEV, generator=g).clamp(max=nc - 1)
    if B > 1:
        gt[1] = 0                      # a sample with no weight at all
    return p, gt, ref


@pytest.mark.parametrize("nc,B,H,W,Hr,Wr", [(151, 3, 256, 256, 256, 256), (2, 2, 64, 64, 64, 64), (256, 2, 70, 66, 70, 66), (19, 1, 64, 48, 32, 40)])
def test_mask_nll_against_fp64_and_framework(nc, B, H, W, Hr, Wr, hip_lib):
    from cocosnet_amd import losses, ops
    p, gt, ref = _mask_inputs(nc, B, H, W, Hr, Wr, 5)
    pk = p.clone().requires_grad_(True)
    out = ops.mask_nll_loss(pk, gt, ref)
    assert out.shape == () and torch.equal(out, ops.mask_nll_loss(pk, gt, ref))
    grad, = torch.autograd.grad(out * 100.0, pk)
    assert torch.equal(grad, torch.autograd.grad(ops.mask_nll_loss(pk, gt, ref) * 100.0, pk)[0])
    pf = p.clone().requires_grad_(True)
    fw = losses._mask_loss_torch(pf, gt, ref)
    grad_f, = torch.autograd.grad(fw * 100.0, pf)
    # fp64 restatement: the fp32 rounding of p + 1e-10 belongs to the reference's arithmetic, the log and the sums are fp64
    gt_s = F.interpolate(gt.float(), scale_factor=0.25, mode="nearest").long().squeeze(1)
    ref_s = F.interpolate(ref.float(), scale_factor=0.25, mode="nearest").long().squeeze(1)
    present = torch.zeros(B, nc, dtype=torch.bool, device=DEV)
    present.scatter_(1, ref_s.view(B, -1), True)
    wgt = (present.gather(1, gt_s.view(B, -1)).view_as(gt_s) & (gt_s != 0)).double()
    logs = -torch.log((p + 1e-10).double().gather(1, gt_s.unsqueeze(1)).squeeze(1))
    want = (logs * wgt).sum() / (wgt.sum() + 1e-5)
    wmean = float((logs.abs() * wgt).sum() / wgt.sum().clamp_min(1))
    assert float(wgt.sum()) > 0
    _check_value(out, want, fw, 1 + wmean, E21, f"mask nc={nc}")
    _check_grad(grad, grad_f, f"mask nc={nc}")
    assert bool((grad[1] == 0).all()) if B > 1 else True


def test_mask_nll_without_any_weight_is_zero(hip_lib):
    from cocosnet_amd import ops
    p, gt, ref = _mask_inputs(7, 2, 32, 32, 32, 32, 9)
    gt.zero_()
    pk = p.requires_grad_(True)
    out = ops.mask_nll_loss(pk, gt, ref)
    out.backward()
    assert float(out) == 0 and bool((pk.grad == 0).all())


# ---- the block ----------------------------------------------------------------------------------------------------------------------
def _gpu_model(name, losses, **over):
    inputs = loss_case.require_grad(loss_case.to_device(loss_case.make_inputs(name), DEV))
    return loss_case.StubModel(loss_case.options(name, **over), inputs, losses.GANLoss, losses.L1Loss, float_tensor=torch.cuda.FloatTensor), inputs


def _gan_bound(opt, preds, target_is_real, for_discriminator):
    """item-5 bound of a GANLoss key: 2^-22 x the loss with every term replaced by its absolute value (hinge / ls / w), 2^-21 x
    (1 + mean |term|) for 'original'; the key is that loss times weight_gan"""
    from cocosnet_amd import losses
    mode, label = losses._gan_case(opt.gan_mode, 1.0, 0.0, target_is_real, for_discriminator)
    scale = _gan_abs(preds, mode, label)
    return (E21 * (1 + scale) if mode == "bce" else E22 * scale) * opt.weight_gan


@pytest.mark.parametrize("name", sorted(loss_case.CASES))
def test_block_against_the_reference_goldens(name, hip_lib):
    from cocosnet_amd import losses
    g = np.load(os.path.join(GOLDEN, f"loss_block_{name}.npz"))
    model, inputs = _gpu_model(name, losses)
    G, _ = loss_case.run_generator(losses.compute_generator_loss, model)
    loss_case.total(G).backward()
    assert ["G." + k for k in G] == [k for k in g.files if k.startswith("G.")]
    # the goldens are the reference's own fp32 CPU results (the framework's op sequence and its autograd): every key within the
    # kernel bounds of the module docstring, every input gradient within 2^-22 per element
    opt, last = model.opt, [d[-1].detach() for d in inputs["pred_fake"]]
    last_real = [d[-1].detach() for d in inputs["pred_real"]]
    bounds = {"GAN": _gan_bound(opt, last, True, False), "D_Fake": _gan_bound(opt, last, False, True),
              "D_real": _gan_bound(opt, last_real, True, True)}

    def check_key(k, v, want):
        assert tuple(v.shape) == want.shape, k
        err = float(np.abs(v.detach().cpu().numpy().astype(np.float64) - want).max())
        if k in bounds:
            bound = bounds[k]
        elif k == "mask":          # weighted mean of |log| = the loss itself before * weight_mask (every term is positive)
            bound = E21 * (opt.weight_mask + float(np.abs(want).max()))
        else:                      # L1 / MSE groups: every term is non-negative
            bound = E22 * float(np.abs(want).max())
        print(f"{name} {k}: {float(v.sum()):.9g} golden {float(want.sum()):.9g} err {err:.3g} bound {bound:.3g}")
        assert err <= bound, (k, err, bound)

    def check_grad(k, got, want, bce, count):
        if bce:                    # see the module docstring: 2^-22 of the factor weight_gan / (n T), absolute
            scale = opt.weight_gan / (want.numel() * count)
            err = float((got.double() - want.double()).abs().max())
            print(f"{name} d {k}: worst gradient error {err:.3g}, bound {E22 * scale:.3g}")
            assert err <= E22 * scale, (k, err)
        else:
            _check_grad(got, want, f"{name} d {k}")

    for k, v in G.items():
        check_key(k, v, g["G." + k])
    n_d, per_d = len(inputs["pred_fake"]), len(inputs["pred_fake"][0])
    for k, t in loss_case.leaves(inputs):
        got = (t.grad if t.grad is not None else torch.zeros_like(t)).cpu()
        is_last = k.startswith("pred_fake.") and (int(k.split(".")[1]) + 1) % per_d == 0
        check_grad(k, got, torch.from_numpy(g["dG." + k]), opt.gan_mode == "original" and is_last, n_d)
    loss_case.require_grad(inputs)
    D = loss_case.run_discriminator(losses.compute_discriminator_loss, model)
    heads = [d[-1] for d in inputs["pred_fake"]]
    grads = torch.autograd.grad(loss_case.total(D), heads)
    for k, v in D.items():
        check_key(k, v, g["D." + k])
    for i, gr in enumerate(grads):
        check_grad(f"D pred_fake_last.{i}", gr.cpu(), torch.from_numpy(g[f"dD.pred_fake_last.{i}"]), opt.gan_mode == "original", n_d)


def test_block_is_deterministic_and_fused_equals_unfused(hip_lib, monkeypatch):
    from cocosnet_amd import losses
    runs = []
    for fused in (True, True, False):
        monkeypatch.setattr(losses, "FUSED", fused)
        model, inputs = _gpu_model("ade20k", losses)
        G, _ = loss_case.run_generator(losses.compute_generator_loss, model)
        loss_case.total(G).backward()
        runs.append((G, [t.grad for _, t in loss_case.leaves(inputs)]))
    for k in runs[0][0]:
        assert torch.equal(runs[0][0][k], runs[1][0][k]), k
        assert abs(float(runs[0][0][k].sum()) - float(runs[2][0][k].sum())) <= 1e-5 * (1 + abs(float(runs[2][0][k].sum()))), k
    for a, b in zip(runs[0][1], runs[1][1]):
        assert (a is None and b is None) or torch.equal(a, b)


def test_no_host_synchronisation(hip_lib, monkeypatch):
    from cocosnet_amd import losses
    model, inputs = _gpu_model("ade20k", losses)
    loss_case.run_generator(losses.compute_generator_loss, model)          # warm-up: library load, allocator
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            G, _ = loss_case.run_generator(losses.compute_generator_loss, model)
            loss_case.total(G).backward()
            D = loss_case.run_discriminator(losses.compute_discriminator_loss, model)
            loss_case.total(D).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if honoured:
        print("sync debug mode 'error' is honoured: the fused block ran under it")
        assert "mask" in G
        return
    print("sync debug mode is not honoured on this build: counting the host-reading calls instead")
    counts = {}
    for owner, attr in ((torch, "unique"), (torch.Tensor, "item"), (torch.Tensor, "__contains__"), (torch.Tensor, "tolist")):
        real = getattr(owner, attr)
        monkeypatch.setattr(owner, attr, lambda *a, _r=real, _n=attr, **k: (counts.__setitem__(_n, counts.get(_n, 0) + 1), _r(*a, **k))[1])
    G, _ = loss_case.run_generator(losses.compute_generator_loss, model)
    loss_case.total(G).backward()
    D = loss_case.run_discriminator(losses.compute_discriminator_loss, model)
    loss_case.total(D).backward()
    assert "mask" in G and not counts, counts


def test_launch_budget_of_the_generator_block(hip_lib, monkeypatch):
    """at most one forward C-ABI call per group: warp terms, GAN, GAN_Feat, fm + perc, mask"""
    from cocosnet_amd import _lib, losses
    model, _ = _gpu_model("ade20k", losses, warp_cycle_w=1.0, warp_self_w=10.0)
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    G, _ = loss_case.run_generator(losses.compute_generator_loss, model)
    fwd = sorted(calls)
    assert fwd == sorted(["cocos_pair_loss_fwd"] * 3 + ["cocos_gan_loss_fwd", "cocos_mask_nll_fwd"]), fwd
    calls.clear()
    loss_case.total(G).backward()
    assert sorted(calls) == sorted(["cocos_pair_loss_bwd"] * 3 + ["cocos_gan_loss_bwd", "cocos_mask_nll_bwd"]), calls
    calls.clear()
    loss_case.run_discriminator(losses.compute_discriminator_loss, model)
    assert calls == ["cocos_gan_loss_fwd"] * 2


def test_memory_budget_of_the_fm_perc_group(hip_lib, monkeypatch):
    from cocosnet_amd import losses
    g = torch.Generator(device=DEV).manual_seed(1)
    shapes = [(4, 64, 128, 128), (4, 128, 64, 64), (4, 256, 32, 32), (4, 512, 16, 16), (4, 512, 8, 8)]
    fake = [torch.randn(*s, device=DEV, generator=g).requires_grad_(True) for s in shapes]
    real = [torch.randn(*s, device=DEV, generator=g) for s in shapes]
    self_ref = torch.tensor([1.0, 0.0, 1.0, 1.0], device=DEV).view(4, 1, 1, 1)
    model = loss_case.StubModel(loss_case.options("ade20k"), {}, losses.GANLoss, losses.L1Loss, float_tensor=torch.cuda.FloatTensor)
    level = fake[0].numel() * 4
    inputs_and_grads = 3 * sum(t.numel() * 4 for t in fake)           # fake, real, d fake

    def peak(fused):
        monkeypatch.setattr(losses, "FUSED", fused)
        for t in fake:
            t.grad = None
        G = {}
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        losses._vgg_losses(G, model, model.opt, fake, real, losses._sample_weights(self_ref))
        (G["fm"] + G["perc"]).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base + 2 * inputs_and_grads // 3      # the inputs were allocated before `base`

    fused, unfused = peak(True), peak(False)
    print(f"fm + perc peak: fused {fused / 2**20:.1f} MiB, unfused {unfused / 2**20:.1f} MiB, inputs + gradients {inputs_and_grads / 2**20:.1f} MiB")
    assert fused < inputs_and_grads + (1 << 20)
    assert unfused >= inputs_and_grads + (1 << 20) + level


# ---- live pointers ------------------------------------------------------------------------------------------------------------------
def _live_blocks():
    blocks = []
    for seg in torch.cuda.memory_snapshot():
        addr = seg["address"]
        for b in seg["blocks"]:
            blocks.append((addr, b["size"], b["state"] == "active_allocated"))
            addr += b["size"]
    blocks.sort()
    return blocks


def test_loss_ops_hand_over_live_buffers_only(hip_lib, monkeypatch):
    """Every device pointer — direct arguments and the entries of the host-side tables — lies inside a live allocation at call time."""
    from cocosnet_amd import _lib, losses
    seen, dead, real = [0, 0], [], _lib.call

    def checked_call(name, *args):
        blocks = _live_blocks()
        starts = [b[0] for b in blocks]
        ptrs = []
        for i, a in enumerate(args):
            if isinstance(a, int) and _lib._SIGNATURES[name][1][i] is ctypes.c_void_p:
                ptrs.append((i, a))
            elif isinstance(a, ctypes.Array) and a._type_ is ctypes.c_void_p:
                ptrs += [(i, v) for v in a if v]
        for i, a in ptrs:
            j = bisect.bisect_right(starts, a) - 1
            if a == 0 or j < 0 or a >= blocks[j][0] + blocks[j][1]:
                continue
            seen[1] += 1
            if not blocks[j][2]:
                dead.append((name, i, hex(a)))
        seen[0] += 1
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", checked_call)
    for name in ("ade20k", "celebahq"):
        model, inputs = _gpu_model(name, losses)
        # non-contiguous predictions: the op's contiguous copies must outlive the launch
        inputs["pred_fake"][0][0] = inputs["pred_fake"][0][0].detach().transpose(2, 3).requires_grad_(True)
        inputs["pred_real"][0][0] = inputs["pred_real"][0][0].transpose(2, 3)
        G, _ = loss_case.run_generator(losses.compute_generator_loss, model)
        loss_case.total(G).backward()
        D = loss_case.run_discriminator(losses.compute_discriminator_loss, model)
        loss_case.total(D).backward()
    torch.cuda.synchronize()
    assert seen[0] >= 16 and seen[1] >= 60, seen
    assert not dead, dead[:8]
