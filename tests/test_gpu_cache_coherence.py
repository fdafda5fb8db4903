"""The version-keyed caches inside composed steps (tests/cache_audit.py does the checking).

(a) Composed forward + backward steps run three times: caches live (under the audit), every consumer taking its own pass
    (`cache_audit.caches_off`), caches live again.  A consumer that measures for itself finds the same maximum, hence the same
    power-of-two scale: outputs and every gradient of the two arms must be torch.equal, and so must the first and third run.
(b) `test_every_site_was_reached` (last in the file): every `_remember_amax` site of the source was reached and verified, every
    `_recall_amax` site returned a verified cell at least once (EXEMPT_CONSUMERS: at most two, with the code's own reason).
(c) Wrappers of ops.py that write, through raw pointers, into a tensor they did not allocate:
      spectral_weight            weight_u, weight_v (power iteration)
      adam_multi_step            every p, exp_avg, exp_avg_sq
      ema_multi_update           every shadow
      _Box3SoftmaxWarp.backward  the shared gradient buffer of a Box3GradSink (an accumulating pass adds into the first pass's G)
      _Box3CorrXbox.backward     T's storage lent to the dC planes (only above ops.BOX3_ALIAS_T_BYTES: 2 GiB — bumped in the same
                                 branch, next to the comment that says why; no tensor of that size is made here)
    (norm_spade updates its running buffers with framework ops, which count for themselves.)  For each: if the bytes changed,
    `_version` rose; a cell remembered before the call is no longer recalled; OperandPlanes.get re-splits the tensor, and raises
    for producer-made planes.
(d) The frozen-record scenario of inference.PreparedWeight under spectral norm: freeze -> eval forward -> train() forward (the power
    iteration moves u, v) -> eval forward must use W / sigma(u_new, v_new) and count one repreparation."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import cache_audit
from test_gpu_grad_subsets import PAIR_NAMES, _dev, _hot_path_case

pytestmark = pytest.mark.gpu
DEV = "cuda"

AUDIT = []          # the one Audit of the module (made by the first test that needs it)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


@pytest.fixture(autouse=True)
def precision(monkeypatch):
    """the flavours that HAVE the caches (the exact-fp32 / bf16 flavours derive no scale from a maximum)"""
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    monkeypatch.setattr(ops, "PROJ_PRECISION", "f16x3")
    monkeypatch.setattr(ops, "CONV_PRECISION", "f16x3")


def _audit():
    if not AUDIT:
        from cocosnet_amd import inference, ops
        AUDIT.append(cache_audit.Audit(ops, inference))
    return AUDIT[0]


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, device=DEV, generator=g) * scale


# ---------------------------------------------------------------------------------------------------------------- the driver
def _run(workload):
    """one step from an empty table: (outputs, gradients of the leaves), detached copies"""
    cache_audit.clear_caches()
    outs, leaves = workload()
    outs = [o for o in outs if o is not None]
    diff = [o for o in outs if o.requires_grad]
    if diff:
        g = torch.Generator(device=DEV).manual_seed(20240611)
        torch.autograd.backward(diff, [_rand(g, *o.shape) for o in diff])
    torch.cuda.synchronize()
    for n, l in enumerate(leaves):
        assert l.grad is not None, f"leaf {n} received no gradient"
    res = [o.detach().clone() for o in outs] + [l.grad.detach().clone() for l in leaves]
    assert all(bool(torch.isfinite(r).all()) for r in res)
    return res


def _three_arms(workload, monkeypatch, what):
    a = _audit()
    with monkeypatch.context() as mp:
        a.install(mp)
        live = _run(workload)
    with monkeypatch.context() as mp:
        cache_audit.caches_off(mp)
        off = _run(workload)
    with monkeypatch.context() as mp:
        a.install(mp)
        again = _run(workload)
    assert len(live) == len(off) == len(again)
    for k, (x, y) in enumerate(zip(live, again)):
        assert torch.equal(x, y), f"{what}: result {k} is not bitwise repeatable run to run (max diff {float((x - y).abs().max()):.3g})"
    for k, (x, y) in enumerate(zip(live, off)):
        assert torch.equal(x, y), (f"{what}: result {k} differs between the cached and the self-measured arm "
                                   f"(max diff {float((x - y).abs().max()):.3g} of {float(x.abs().max()):.3g})")


# ---------------------------------------------------------------------------------------------------------------- the hot path
DIRECT = dict(warp_mask_losstype="direct")
HOT = {
    # name: (mk, fh, fw, flags, inputs that need gradients, route, module switches)
    # route "lazy": LazyProj1x1 pairs; "raw": the projections made by K0 first; "norm": the features come out of K13 (their cell
    # is there when the projections ask); "frozen": "norm" + frozen records on both projections, no_grad
    "mk1_direct": (1, 8, 16, DIRECT, PAIR_NAMES, "lazy", {}),
    "mk3_direct": (3, 4, 64, DIRECT, PAIR_NAMES, "lazy", {}),
    "mk1_cycle_mask": (1, 8, 16, dict(warp_mask_losstype="cycle"), PAIR_NAMES, "lazy", {}),
    "mk3_cycle_mask": (3, 4, 64, dict(warp_mask_losstype="cycle"), PAIR_NAMES, "lazy", {}),
    "mk1_two_cycle": (1, 8, 16, dict(warp_mask_losstype="direct", warp_cycle_w=1.0, two_cycle=True), PAIR_NAMES, "lazy", {}),
    "mk3_two_cycle": (3, 4, 64, dict(warp_mask_losstype="direct", warp_cycle_w=1.0, two_cycle=True), PAIR_NAMES, "lazy", {}),
    "mk1_bilinear": (1, 8, 16, dict(warp_mask_losstype="direct", warp_bilinear=True), PAIR_NAMES, "lazy", {}),
    "mk3_bilinear": (3, 4, 64, dict(warp_mask_losstype="direct", warp_bilinear=True), PAIR_NAMES, "lazy", {}),
    "mk1_patch_cycle": (1, 8, 16, dict(warp_mask_losstype="direct", warp_patch=True, warp_cycle_w=1.0), PAIR_NAMES, "lazy", {}),
    "mk3_patch_cycle": (3, 4, 64, dict(warp_mask_losstype="direct", warp_patch=True, warp_cycle_w=1.0), PAIR_NAMES, "lazy", {}),
    # mixed subsets: K23 with round 5's chain backward (weights only) / match_kernel 3 off K25 (features only: prefetch_amax + K0 + K12)
    "mk1_weights_only": (1, 8, 16, DIRECT, ("w_theta", "b_theta", "w_phi", "b_phi"), "lazy", {}),
    "mk3_features_only": (3, 4, 64, DIRECT, ("x_theta", "x_phi"), "norm", {}),
    # K23 / K25 in a training step whose features arrive with K13's cells (plain leaves bring none: the pair kernels measure them)
    "mk1_features_from_k13": (1, 8, 16, DIRECT, PAIR_NAMES, "norm", {}),
    "mk3_features_from_k13": (3, 4, 64, DIRECT, PAIR_NAMES, "norm", {}),
    # the projections as tensors: K1's planes flavour / K1 itself (no PONO_C) / K12 on its own / the materialised family (8 x 16 is
    # no grid of the fused match_kernel-3 family: K3 -> K6 -> K7)
    "mk1_raw": (1, 8, 16, DIRECT, PAIR_NAMES, "raw", {}),
    "mk1_raw_no_pono": (1, 8, 16, dict(warp_mask_losstype="direct", PONO_C=False), PAIR_NAMES, "raw", {}),
    "mk3_raw": (3, 4, 64, DIRECT, PAIR_NAMES, "raw", {}),
    "mk3_materialised": (3, 8, 16, DIRECT, PAIR_NAMES, "raw", {}),
    # round 6's head (ops.WARP_HEAD_MODES off): the nearest ops.warp_head, and the framework route whose backward concatenates (concat_channels_amax)
    "mk1_head_r6": (1, 8, 16, DIRECT, PAIR_NAMES, "lazy", dict(WARP_HEAD_MODES=False)),
    "mk1_concat_r6": (1, 8, 16, dict(warp_mask_losstype="direct", warp_bilinear=True), PAIR_NAMES, "lazy", dict(WARP_HEAD_MODES=False)),
    # the backward that recomputes its logits
    "mk1_recompute": (1, 8, 16, DIRECT, PAIR_NAMES, "lazy", dict(MAX_SAVED_LOGITS_BYTES=0)),
    # frozen records on the projections (inference.PreparedWeight): the weights' cells are the records', the features' K13's
    "mk1_frozen": (1, 8, 16, DIRECT, (), "frozen", {}),
    "mk3_frozen": (3, 4, 64, DIRECT, (), "frozen", {}),
}


def _hot_workload(mk, fh, fw, flags, needs, route):
    from cocosnet_amd import inference, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_hot_path

    def workload():
        inputs, base = _hot_path_case(mk, 2, 64 + 7, fh, fw, seed=21 + mk)
        cfg = HotPathConfig(**{**base, **flags})
        lv = {n: (t.detach().clone().requires_grad_(n in needs) if n in PAIR_NAMES else t) for n, t in inputs.items()}
        feats = {s: lv["x_" + s] for s in ("theta", "phi")}
        if route in ("norm", "frozen"):
            slope = torch.full((1,), 0.25, device=DEV)
            feats = {s: ops.instnorm_prelu(x, None, slope) for s, x in feats.items()}
        if route == "frozen":
            recs = {}
            for s in ("theta", "phi"):
                m = nn.Conv2d(64 + 7, 256, 1).to(DEV)
                with torch.no_grad():
                    m.weight.copy_(lv["w_" + s])
                    m.bias.copy_(lv["b_" + s])
                m.requires_grad_(False)
                recs[s] = (m, inference.PreparedWeight(m.eval()).ensure())
            th, ph = (ops.LazyProj1x1(feats[s], recs[s][0].weight, recs[s][0].bias, recs[s][1]) for s in ("theta", "phi"))
        elif route == "raw":
            th, ph = (ops.proj1x1(feats[s], lv["w_" + s], lv["b_" + s]) for s in ("theta", "phi"))
        else:
            th, ph = (ops.LazyProj1x1(feats[s], lv["w_" + s], lv["b_" + s]) for s in ("theta", "phi"))
        out = correspondence_hot_path(th, ph, lv["ref_img"], lv["ref_img"], lv["seg"], lv["seg"], cfg)
        return [out[k] for k in sorted(out)], [lv[n] for n in PAIR_NAMES if n in needs]
    return workload


@pytest.mark.parametrize("case", sorted(HOT))
def test_hot_path_step(case, monkeypatch):
    from cocosnet_amd import ops
    mk, fh, fw, flags, needs, route, switches = HOT[case]
    for k, v in switches.items():
        monkeypatch.setattr(ops, k, v)
    wl = _hot_workload(mk, fh, fw, flags, needs, route)
    if route == "frozen":
        with torch.no_grad():
            _three_arms(wl, monkeypatch, case)
    else:
        _three_arms(wl, monkeypatch, case)


# ---------------------------------------------------------------------------------------------------------------- K19 / K20
def test_box3_pair_with_one_sink_and_two_passes(monkeypatch):
    """test_box3_corr_xbox_and_softmax_warp's 4 x 64 case with a row pass and a column pass (transposed=True) over one T: the second
    pass's backward ADDS into the first one's G and replaces its max|G| cell (ops._Box3SoftmaxWarp.backward)."""
    from cocosnet_amd import ops
    B, fh, fw, Cv, kc, scale = 1, 4, 64, 5, 256.0 * 9, 100.0
    N = fh * fw

    def workload():
        g = torch.Generator(device=DEV).manual_seed(104)
        q = (_rand(g, B, 256, fh, fw) + 0.15).requires_grad_(True)
        k = (0.05 * q.detach().roll((1, 5), (2, 3)) + _rand(g, B, 256, fh, fw) - 0.1).requires_grad_(True)
        v1 = (torch.rand(B, Cv, N, device=DEV, generator=g) * 2 - 1).requires_grad_(True)
        v2 = (torch.rand(B, 3, N, device=DEV, generator=g) * 2 - 1).requires_grad_(True)
        (mu, a), (nu, b) = ops.unfold3_stats(q, kc), ops.unfold3_stats(k, kc)
        sink = ops.Box3GradSink()
        T = ops.box3_corr_xbox(q, k, sink)
        rows = ops.box3_softmax_warp(T, mu, a, nu, b, v1, fh, fw, kc, scale, False, sink)
        cols = ops.box3_softmax_warp(T, nu, b, mu, a, v2, fh, fw, kc, scale, True, sink)
        return [rows, cols], [q, k, v1, v2]
    _three_arms(workload, monkeypatch, "box3 pair")


# ---------------------------------------------------------------------------------------------------------------- K16 / K13 / K29
def _conv_chain_leaves(seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = _rand(g, 2, 128, 32, 32).requires_grad_(True)
    w1 = (_rand(g, 128, 128, 3, 3) * 0.05).requires_grad_(True)
    w2 = (_rand(g, 128, 128, 3, 3) * 0.05).requires_grad_(True)
    a = torch.tensor([0.25], device=DEV, requires_grad=True)
    return x, w1, w2, a


def _conv_chain(x, w1, w2, a):
    from cocosnet_amd import ops
    return ops.conv2d(ops.instnorm_prelu(ops.conv2d(x, w1, None, 1, 1), None, a), w2, None, 1, 1)


def test_conv_instnorm_conv(monkeypatch):
    """the chain and shape of test_the_next_convolution_finds_the_cell"""
    def workload():
        x, w1, w2, a = _conv_chain_leaves()
        return [_conv_chain(x, w1, w2, a)], [x, w1, w2, a]
    _three_arms(workload, monkeypatch, "conv -> K13 -> conv")


def test_two_steps_with_adam_between(monkeypatch):
    """two consecutive steps of the chain with adam_multi_step on the weights in between: the second step's convolutions must measure
    the UPDATED weights (no cell survives an in-place parameter update)."""
    from cocosnet_amd import ops

    def workload():
        x, w1, w2, a = _conv_chain_leaves()
        y1 = _conv_chain(x, w1, w2, a)
        g = torch.Generator(device=DEV).manual_seed(5)
        y1.backward(_rand(g, *y1.shape))
        ps = [w1, w2]
        ops.prefetch_amax([p.detach() for p in ps])          # cells of the weights as they are BEFORE the update
        ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
        lr, b1, b2 = 1e-2, 0.5, 0.999
        row = (lr / (1 - b1), (1 - b2) ** 0.5, b1, 1 - b1, b2, 1 - b2, 1e-8, 0.0)
        with torch.no_grad():
            ops.adam_multi_step([p.detach() for p in ps], [p.grad for p in ps], ms, vs, [row], [0, 0])
        first = [t.grad.detach().clone() for t in (x, w1, w2, a)]
        for t in (x, w1, w2, a):
            t.grad = None
        y2 = _conv_chain(x, w1, w2, a)
        return [y2, y1.detach(), *first], [x, w1, w2, a]
    _three_arms(workload, monkeypatch, "two steps with Adam between")


# ---------------------------------------------------------------------------------------------------------------- K21 / K9 / K26
def _spade_pair(label_nc, norm_nc, seed):
    """SPADE's mlp_gamma / mlp_beta: two producers.Conv2d under hip_spectral_norm, in train() mode (power iteration per forward)"""
    from cocosnet_amd import producers
    torch.manual_seed(seed)
    convs = [producers.hip_spectral_norm(producers.Conv2d(label_nc, norm_nc, 3, padding=1)) for _ in range(2)]
    return [c.to(DEV).train() for c in convs]


@pytest.mark.parametrize("kind,shape,label_nc", [("pono", (2, 128, 4, 32), 32), ("batch", (2, 16, 12, 12), 8), ("instance", (2, 16, 12, 12), 8),
                                                 ("batch", (1, 5, 7, 9), 3), ("instance", (1, 5, 7, 9), 3)])
def test_spade_block(kind, shape, label_nc, monkeypatch):
    """two spectral-normed convolutions reading ONE label map (the second finds the cell the first one measured, both find K21's
    weight cells) into K9 / K26, whose backward leaves max|d gamma|, max|d beta| for the convolutions' backward.  (2, 128, 4, 32)
    from 32 channels is on the NHWC route (Cin >= 32, Cout >= 128, OW % 32 == 0); the small shapes are test_norm_spade's."""
    from cocosnet_amd import ops
    B, C, h, w = shape

    def workload():
        mg, mb = _spade_pair(label_nc, C, seed=11)
        g = torch.Generator(device=DEV).manual_seed(C + h)
        seg = _rand(g, B, label_nc, h, w).requires_grad_(True)
        x = (_rand(g, *shape, scale=1.5) + 0.3).requires_grad_(True)
        gamma, beta = mg(seg), mb(seg)
        if kind == "pono":
            y = ops.pono_spade(x, gamma, beta, 0.2)
        else:
            y = ops.norm_spade(x, gamma, beta, kind, training=True, slope=0.2)
        return [y], [x, seg, mg.weight_orig, mb.weight_orig, mg.bias, mb.bias]
    _three_arms(workload, monkeypatch, f"SPADE[{kind}]")


def test_discriminator_stub_real_then_fake(monkeypatch):
    """two spectral-normed layers run on real, then on fake, then ONE backward: two power iterations per layer and step, the first
    call's backward must use the u, v (and sigma) of ITS forward"""
    from cocosnet_amd import producers

    def workload():
        torch.manual_seed(17)
        l1 = producers.hip_spectral_norm(producers.Conv2d(3, 16, 4, stride=2, padding=1)).to(DEV).train()
        l2 = producers.hip_spectral_norm(producers.Conv2d(16, 1, 4, stride=1, padding=1)).to(DEV).train()
        g = torch.Generator(device=DEV).manual_seed(18)
        real, fake = _rand(g, 2, 3, 16, 16), _rand(g, 2, 3, 16, 16).requires_grad_(True)
        d = lambda t: l2(F.leaky_relu(l1(t), 0.2))
        return [d(real), d(fake)], [fake, l1.weight_orig, l2.weight_orig, l1.bias, l2.bias]
    _three_arms(workload, monkeypatch, "discriminator stub")


# ---------------------------------------------------------------------------------------------------------------- K2 / K22 / K27 / K28
def test_softmax_attention(monkeypatch):
    from cocosnet_amd import ops
    K, Nq, Nk = 64, 1024, 128

    def workload():
        rs = np.random.RandomState(K + Nq)
        q, k, v = rs.standard_normal((1, K, Nq)) * 1.5, rs.standard_normal((1, K, Nk)), rs.uniform(-1, 1, (1, 70, Nk))
        lv = [_dev(t).requires_grad_(True) for t in (q, k, v)]
        return [ops.softmax_attention(*lv, float(1.0 / np.sqrt(K)))], lv
    _three_arms(workload, monkeypatch, "softmax_attention")


def test_contextual_cx(monkeypatch):
    from cocosnet_amd import ops

    def workload():
        g = torch.Generator(device=DEV).manual_seed(2200)
        nrm = lambda t: t / (t.norm(dim=1, keepdim=True) + 2.2e-16)
        xn, yn = nrm(_rand(g, 2, 40, 200)).requires_grad_(True), nrm(_rand(g, 2, 40, 330))
        return [ops.contextual_cx(xn, yn, 0.1, 1e-3)], [xn]
    _three_arms(workload, monkeypatch, "contextual_cx")


def test_vgg_first_block_into_pair_loss(monkeypatch):
    """vgg_preprocess -> conv1_1 -> ReLU -> conv1_2 -> ReLU + pool -> conv2_1 -> pair_loss against fixed features: every K27 output
    arrives at its convolution with its cell, every K27 backward leaves one for the convolution behind it"""
    from cocosnet_amd import ops

    def workload():
        g = torch.Generator(device=DEV).manual_seed(27)
        x = torch.rand(2, 3, 16, 16, device=DEV, generator=g).requires_grad_(True)
        w11, w12, w21 = _rand(g, 64, 3, 3, 3, scale=0.01), _rand(g, 64, 64, 3, 3, scale=0.05), _rand(g, 128, 64, 3, 3, scale=0.05)
        r11 = ops.relu(ops.conv2d(ops.vgg_preprocess(x, False), w11, None, 1, 1))
        r12, p1 = ops.relu_pool2(ops.conv2d(r11, w12, None, 1, 1), "max", True)
        r21 = ops.relu(ops.conv2d(p1, w21, None, 1, 1))
        real = [_rand(g, *t.shape) for t in (r12, r21)]
        loss = ops.pair_loss([(r12, real[0], None, 1.0 / 32, 0.0), (r21, real[1], None, 1.0 / 16, 0.0)])
        return [loss], [x]
    _three_arms(workload, monkeypatch, "VGG block -> pair_loss")


# ---------------------------------------------------------------------------------------------------------------- (c)
def _writers():
    """name -> (tensors it writes, call): each call writes into tensors made here, by the test"""
    from cocosnet_amd import ops
    g = torch.Generator(device=DEV).manual_seed(41)

    def spectral():
        w = _rand(g, 6, 5, 3, 3)
        u, v = F.normalize(_rand(g, 6), dim=0), F.normalize(_rand(g, 45), dim=0)
        return [u, v], lambda: ops.spectral_weight(w, u, v, True)

    def adam():
        p, gr = _rand(g, 7, 5), _rand(g, 7, 5)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        row = (1e-2 / 0.5, (1 - 0.999) ** 0.5, 0.5, 0.5, 0.999, 1 - 0.999, 1e-8, 0.0)
        return [p, m, v], lambda: ops.adam_multi_step([p], [gr], [m], [v], [row], [0])

    def ema():
        s, p = _rand(g, 7, 5), _rand(g, 7, 5)
        return [s], lambda: ops.ema_multi_update([s], [p], 0.9)
    return dict(spectral_weight=spectral, adam_multi_step=adam, ema_multi_update=ema)


@pytest.mark.parametrize("name", ["spectral_weight", "adam_multi_step", "ema_multi_update"])
def test_raw_pointer_writes_are_visible(name):
    from cocosnet_amd import _lib, ops
    cache_audit.clear_caches()
    tensors, call = _writers()[name]()
    before = [(t.clone(), t._version) for t in tensors]
    planes, made = ops.OperandPlanes(), ops.OperandPlanes()
    views = [t.view(1, 1, -1) for t in tensors]          # (a view shares the version counter; split_f16 wants three dimensions)
    old = []
    for t, v3 in zip(tensors, views):
        ops._remember_amax(t, ops.absmax(t))
        assert ops._recall_amax(t, consume=False) is not None
        hi, lo = planes.get(v3, False, 1.0)
        old.append((hi.clone(), lo.clone()))
        made.put(v3, False, 1.0, hi, lo)
    with torch.no_grad():
        call()
    torch.cuda.synchronize()
    for k, (t, v3, (was, version)) in enumerate(zip(tensors, views, before)):
        assert not torch.equal(t, was), f"{name}: tensor {k} did not change: the case does not test anything"
        assert t._version > version, f"{name}: wrote tensor {k} through a raw pointer and left its _version at {version}"
        assert ops._recall_amax(t, consume=False) is None, f"{name}: the max|.| cell of tensor {k} from before the call is still recalled"
        hi, lo = planes.get(v3, False, 1.0)
        ref_hi, ref_lo = ops.split_f16(v3, False, 1.0)
        assert torch.equal(hi, ref_hi) and torch.equal(lo, ref_lo) and not (torch.equal(hi, old[k][0]) and torch.equal(lo, old[k][1])), (
            f"{name}: OperandPlanes.get returned the planes of tensor {k} as it was before the call")
        with pytest.raises(_lib.CocosHipError):
            made.get(v3, False, 1.0)


def test_an_accumulating_box3_pass_bumps_the_shared_buffer(monkeypatch):
    """the sink buffer: the second pass's backward adds into the first one's G — its bytes change, so its _version must rise, and
    T's node must be handed the cell of the SUM"""
    from cocosnet_amd import ops
    B, fh, fw, kc, scale = 1, 4, 64, 256.0 * 9, 100.0
    N = fh * fw
    g = torch.Generator(device=DEV).manual_seed(104)
    q = (_rand(g, B, 256, fh, fw) + 0.15).requires_grad_(True)
    k = (0.05 * q.detach().roll((1, 5), (2, 3)) + _rand(g, B, 256, fh, fw) - 0.1).requires_grad_(True)
    v1, v2 = (torch.rand(B, 3, N, device=DEV, generator=g) * 2 - 1 for _ in range(2))
    (mu, a), (nu, b) = ops.unfold3_stats(q, kc), ops.unfold3_stats(k, kc)
    sink = ops.Box3GradSink()
    T = ops.box3_corr_xbox(q, k, sink)
    rows = ops.box3_softmax_warp(T, mu, a, nu, b, v1, fh, fw, kc, scale, False, sink)
    cols = ops.box3_softmax_warp(T, nu, b, mu, a, v2, fh, fw, kc, scale, True, sink)
    seen = []
    real = ops._remember_amax

    def remember(t, cell, weak=False):
        if t.numel() == B * N * N:
            seen.append((t, t._version, t.clone(), float(cell)))
        return real(t, cell, weak)
    monkeypatch.setattr(ops, "_remember_amax", remember)
    torch.autograd.backward([rows, cols], [_rand(g, *rows.shape), _rand(g, *cols.shape)])
    assert len(seen) == 2 and seen[0][0] is seen[1][0], "two passes, one buffer"
    (_, v_first, bytes_first, _), (buf, v_second, bytes_second, cell) = seen
    assert not torch.equal(bytes_first, bytes_second)
    assert v_second > v_first, "the accumulating pass changed the shared gradient buffer and left its _version alone"
    assert cell == float(bytes_second.abs().max())


# ---------------------------------------------------------------------------------------------------------------- (d)
def _sigma64(m):
    w = m.weight_orig.detach().double().cpu()
    u, v = m.weight_u.detach().double().cpu(), m.weight_v.detach().double().cpu()
    return w, torch.dot(u, w.reshape(w.shape[0], -1) @ v)


@pytest.mark.parametrize("hook", ["hip", "framework"])
def test_frozen_record_follows_the_power_iteration(hook, monkeypatch):
    from cocosnet_amd import inference, producers
    monkeypatch.setattr(inference, "FROZEN", True)
    torch.manual_seed(8)
    conv = producers.Conv2d(8, 16, 4, stride=2, padding=1)
    m = (producers.hip_spectral_norm(conv) if hook == "hip" else torch.nn.utils.spectral_norm(conv)).to(DEV).eval()
    x = _rand(torch.Generator(device=DEV).manual_seed(9), 2, 8, 16, 16)
    a = _audit()
    with torch.no_grad(), monkeypatch.context() as mp:
        a.install(mp)
        cache_audit.clear_caches()
        report = inference.freeze(m)
        assert report.layers == 1 and report.spectral == 1 and report.skipped == []
        m(x)
        assert report.repreparations == 0
        u_old = m.weight_u.clone()
        m.train()
        m(x)                                     # the power iteration runs: u, v move
        m.eval()
        assert not torch.equal(m.weight_u, u_old), "the train() forward did not change weight_u"
        frozen = m(x)
        monkeypatch.setattr(inference, "FROZEN", False)
        unfrozen, unfrozen2 = m(x), m(x)
        monkeypatch.setattr(inference, "FROZEN", True)
    assert report.repreparations == 1, f"repreparations = {report.repreparations} after a power iteration moved weight_u / weight_v"
    assert torch.equal(frozen, unfrozen), (
        f"the frozen forward differs from the unfrozen one by {float((frozen - unfrozen).abs().max()):.3g} "
        f"(range {float(unfrozen.abs().max()):.3g}): the record holds W / sigma of the u, v from before the power iteration")
    # ... and both are the convolution with W / sigma(u_new, v_new): the bound of test_frozen_forward_equals_the_unfrozen_forward
    # (frozen error <= unfrozen error + the unfrozen arm's run-to-run difference), the unfrozen arm itself within test_conv2d_matches_fp64's 1e-5
    w64, sigma = _sigma64(m)
    ref = F.conv2d(x.double().cpu(), w64 / sigma, m.bias.detach().double().cpu(), stride=2, padding=1)
    rel = lambda t, r: float((t.double().cpu() - r.double().cpu()).abs().max() / (r.double().abs().max().cpu() + 1e-30))
    e_un, e_fr, spread = rel(unfrozen, ref), rel(frozen, ref), rel(unfrozen, unfrozen2)
    print(f"frozen record after a power iteration [{hook}]: error against fp64: unfrozen {e_un:.3e}, frozen {e_fr:.3e}; run-to-run {spread:.3e}")
    assert e_un <= 1e-5 and e_fr <= e_un + spread


# ---------------------------------------------------------------------------------------------------------------- (b)
#: consumer sites that may stay without a verified hit: (file, qualified name) -> the code's own reason.  At most two.
EXEMPT_CONSUMERS = {}


def test_every_site_was_reached():
    a = _audit()
    line = a.report()
    assert len(EXEMPT_CONSUMERS) <= 2
    print("pairs:", *sorted(f"{a.label(p)} -> {a.label(c)}" for p, c in a.pairs), sep="\n  ")
    missing_p = [a.label(s) for s in a.uncovered_producers()]
    missing_c = [a.label(s) for s in a.uncovered_consumers() if (s[0], a.consumers[s]) not in EXEMPT_CONSUMERS]
    assert a.rowdot_hits > 0, "no softmax backward ever took the D that warp_head's backward left"
    assert not missing_p, f"{line}: _remember_amax sites no workload reached: {missing_p}"
    assert not missing_c, f"{line}: _recall_amax sites that never returned a cell: {missing_c}"
