"""Frozen-weight inference on the GPU (cocosnet_amd/inference.py, K32 = csrc/weight_prepare_multi.hip).

1. plane bytes: cocos_weight_planes_multi / cocos_weight_absmax_multi against the single-tensor routines, bitwise, every layout;
2. launch accounting: the second and third frozen forward launch NO weight preparation (derived: weights are constant, so 0);
3. the frozen forward equals the unfrozen one (bitwise where the unfrozen forward reproduces itself, else within the unfrozen arm's own
   run-to-run difference on top of its error against an fp64 copy of the module);
4. load_state_dict invalidates the records: one re-preparation per layer, results those of the new weights;
5. every pointer a frozen forward hands to the library lies in a live allocation (the records hold their planes);
6. without freeze() a forward launches, name for name, what it launches with COCOS_FROZEN=0.
"""
import bisect
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

PREP_NAMES = ("cocos_conv2d_weight_planes", "cocos_split_f16_rows", "cocos_spectral_weight_fwd")
PREP_PREFIXES = ("cocos_proj_weight_",)


class _CallLog:
    """`_lib.call` wrapped (a wrapper of this file's own): the (name, args) of every entry-point call, and — with `guard` — the
    pointer-liveness check of tests/test_gpu_live_buffers.py."""

    def __init__(self, monkeypatch, guard=False):
        from cocosnet_amd import _lib
        self.calls, self.dead, self.pointers = [], [], 0
        real_call, sigs = _lib.call, _lib._SIGNATURES

        def logged(name, *args):
            if guard:
                blocks = []
                for seg in torch.cuda.memory_snapshot():
                    addr = seg["address"]
                    for b in seg["blocks"]:
                        blocks.append((addr, b["size"], b["state"] == "active_allocated"))
                        addr += b["size"]
                blocks.sort()
                starts = [b[0] for b in blocks]
                for i, (a, ty) in enumerate(zip(args, sigs[name][1])):
                    if ty is not ctypes.c_void_p or not isinstance(a, int) or a == 0:
                        continue
                    j = bisect.bisect_right(starts, a) - 1
                    if j < 0 or a >= blocks[j][0] + blocks[j][1]:
                        continue
                    self.pointers += 1
                    if not blocks[j][2]:
                        self.dead.append((name, i, hex(a), blocks[j][1]))
            self.calls.append((name, args))
            return real_call(name, *args)

        monkeypatch.setattr(_lib, "call", logged)

    def names(self):
        return [n for n, _ in self.calls]

    def clear(self):
        self.calls = []


def _weight_pointers(*modules):
    """data_ptr of every parameter and buffer, and of the records' effective weights (W / sigma of spectral layers)"""
    from cocosnet_amd import inference
    ptrs = set()
    for m in modules:
        for t in list(m.parameters()) + list(m.buffers()):
            ptrs.add(t.data_ptr())
        for sub in m.modules():
            rec = inference.record_of(sub)
            if rec is not None and rec.weight is not None:
                ptrs.add(rec.weight.data_ptr())
    return ptrs


def _weight_preparation_calls(calls, ptrs):
    bad = []
    for name, args in calls:
        if name in PREP_NAMES or name.startswith(PREP_PREFIXES):
            bad.append(name)
        elif name.startswith("cocos_absmax"):
            where = args[0:12:3] if name == "cocos_absmax4" else args[0:1]
            if any(isinstance(a, int) and a in ptrs for a in where):
                bad.append(name)
    return bad


# ---- 1. plane bytes -------------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(64, 3, 3, 3), (128, 64, 4, 4), (256, 256, 3, 3), (407, 407, 3, 3), (512, 512, 3, 3), (128, 151, 3, 3), (13, 7, 3, 3),
               (3, 64, 7, 7), (151, 128, 3, 3)]
PROJ_SHAPES = [(256, 407, 1, 1), (256, 448, 1, 1), (256, 71, 1, 1), (256, 263, 1, 1), (256, 64, 1, 1)]


def _weights(shapes, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(*s, device=DEV, generator=g) * (0.02 + 0.3 * (i % 5)) for i, s in enumerate(shapes)]


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8).flatten(), b.view(torch.uint8).flatten())


def test_absmax_multi_equals_the_single_tensor_pass_bitwise(hip_lib):
    from cocosnet_amd import ops
    ws = _weights(CONV_SHAPES + PROJ_SHAPES, 1)
    g = torch.Generator(device=DEV).manual_seed(2)
    flat = torch.randn(40000, device=DEV, generator=g)
    ws += [flat[1:1 + 8193], flat[9000:9003], flat[10000:10001], flat[12001:12001 + 16390]]      # 4-byte aligned only; n % 4 != 0; one element
    ws += [torch.randn(5, 3, 3, 3, device=DEV, generator=g) * 10.0 ** (k % 7 - 3) for k in range(60)]      # > 64 entries: 78
    ws.append(torch.zeros(33, device=DEV))
    assert len(ws) > ops.weight_prepare_constants()["TABLE_ENTRIES"] == 64
    cells, launches = ops.weight_absmax_multi(ws)
    assert launches == 2 * -(-len(ws) // 64)
    for w, c in zip(ws, cells):
        want = ops.absmax(w)
        assert torch.equal(c.view(torch.int32), want.view(torch.int32)), (tuple(w.shape), float(c), float(want))
        assert float(c) == float(w.abs().max())


def test_planes_multi_equals_the_single_tensor_routines_bitwise(hip_lib):
    from cocosnet_amd import ops
    lib = hip_lib
    convs, projs = _weights(CONV_SHAPES, 3), _weights(PROJ_SHAPES, 4)
    cells, _ = ops.weight_absmax_multi(convs + projs)
    amax = {id(w): c for w, c in zip(convs + projs, cells)}
    reqs = []
    for w in convs:
        reqs += [(w, amax[id(w)], "conv_fwd", 0), (w, None, "conv_fwd_bf16", 0)]
        if w.shape[2] == w.shape[3]:
            reqs += [(w, amax[id(w)], "conv_dgrad", 0), (w, None, "conv_dgrad_bf16", 0)]
    for w in projs:
        kp = lib.cocos_proj1x1_stream_kpad(w.shape[1]) or (w.shape[1] + 15) // 16 * 16      # (0: beyond the streaming kernel's channels)
        reqs += [(w, amax[id(w)], "frag", 0), (w, amax[id(w)], "rows", kp), (w, amax[id(w)], "conv_fwd", 0)]
    for w in convs[:4]:      # rows of a k x k weight (cols = Cin * KH * KW, not a multiple of 8)
        cols = w[0].numel()
        reqs.append((w, amax[id(w)], "rows", (cols + 15) // 16 * 16))
    while len(reqs) <= 64:
        reqs.append(reqs[len(reqs) % 7])
    assert len(reqs) > 64
    got, launches = ops.weight_planes_multi(reqs)
    assert launches == -(-len(reqs) // 64)
    for (w, cell, layout, aux), (hi, lo, sc) in zip(reqs, got):
        what = (tuple(w.shape), layout, aux)
        if layout.startswith("conv_"):
            eh, el, es = ops._conv_weight_planes(w, cell, 1 if "dgrad" in layout else 0)
            assert _same_bytes(hi, eh), what
            if cell is None:
                assert lo is None and sc is None and el is None
            else:
                assert _same_bytes(lo, el) and _same_bytes(sc, es), what
        elif layout == "rows":
            rows, cols = w.shape[0], w[0].numel()
            eh, el = torch.empty((rows, aux), device=DEV, dtype=torch.float16), torch.empty((rows, aux), device=DEV, dtype=torch.float16)
            es = torch.empty(1, device=DEV)
            ops._call("t", "cocos_split_f16_rows", w.data_ptr(), eh.data_ptr(), el.data_ptr(), rows, cols, aux, 1.0, cell.data_ptr(),
                      es.data_ptr(), ops._stream())
            assert _same_bytes(hi, eh) and _same_bytes(lo, el) and _same_bytes(sc, es), what
        else:
            Cin = w.shape[1]
            ef = torch.empty(lib.cocos_proj_weight_frag_bytes(Cin), device=DEV, dtype=torch.uint8)
            es = torch.empty(1, device=DEV)
            ops._call("t", "cocos_proj_weight_frag_planes", w.reshape(256, Cin).data_ptr(), cell.data_ptr(), ef.data_ptr(), es.data_ptr(),
                      None, None, 256, Cin, ops._stream())
            assert lo is None and _same_bytes(hi, ef) and _same_bytes(sc, es), what


def test_planes_multi_rejects_what_it_cannot_lay_out(hip_lib):
    from cocosnet_amd import _lib, ops
    w = torch.randn(128, 64, 1, 1, device=DEV)
    (cell,), _ = ops.weight_absmax_multi([w])
    with pytest.raises(_lib.CocosHipError):
        ops.weight_planes_multi([(w, cell, "frag", 0)])          # the fragment order is for 256 output channels
    with pytest.raises(_lib.CocosHipError):
        ops.weight_planes_multi([(w, cell, "rows", 60)])         # rows shorter than the columns
    with pytest.raises(ValueError):
        ops.weight_planes_multi([(w, None, "conv_fwd", 0)])      # a split layout without its max|w| cell


# ---- the networks of 2. - 6. ------------------------------------------------------------------------------------------------------
def _corr_case(mk):
    from cocosnet_amd import correspondence as cc
    opt = cc.ade20k_options(semantic_nc=7, match_kernel=mk)
    torch.manual_seed(0)
    net = cc.NoVGGCorrespondence(opt).to(DEV)
    net.init_weights(opt.init_type, opt.init_variance)
    net.eval()
    g = torch.Generator(device=DEV).manual_seed(4)
    S = 256 if mk == 3 else 64                    # (the fused match_kernel-3 family takes 64-wide grids)
    img = torch.rand(2, 3, S, S, device=DEV, generator=g) * 2 - 1
    real = torch.rand(2, 3, S, S, device=DEV, generator=g) * 2 - 1
    lab = torch.randint(0, 7, (2, 1, S, S), device=DEV, generator=g)
    seg = torch.zeros(2, 7, S, S, device=DEV).scatter_(1, lab, 1.0)
    inputs = (img, real, seg, seg.flip(0))

    def run(n=net, inputs=inputs):
        out = n(*inputs, alpha=1.0)
        return [out["warp_out"], out["warp_mask"]]

    def run64():      # an fp64 CPU copy of the module up to the projections, oracle/torch_ref.py's fp64 hot path from there on
        from cocosnet_amd import inference
        from cocosnet_amd.hot_path import HotPathConfig
        from oracle import torch_ref as tr
        n64 = copy.deepcopy(net)
        inference.unfreeze(n64)
        n64 = n64.double().cpu()
        in64 = [t.double().cpu() for t in inputs]
        theta, phi = n64.project(*in64)
        out = tr.hot_path(theta, phi, *in64, HotPathConfig.from_opt(opt, down=opt.down))
        return [out["warp_out"], out["warp_mask"]]
    return net, run, run, run64


def _generator_case():
    from cocosnet_amd import translation as tl
    opt = tl.celebahq_edge_train_options()
    g = torch.Generator(device=DEV).manual_seed(77)
    seg = torch.rand(2, 15, 256, 256, device=DEV, generator=g)
    cbn = torch.cat((torch.rand(2, 3, 256, 256, device=DEV, generator=g) * 2 - 1, seg), 1)
    torch.manual_seed(0)
    G = tl.SPADEGenerator(opt).to(DEV)
    G.init_weights(opt.init_type, opt.init_variance)
    G.eval()

    def run():
        return [G(seg, warp_out=cbn)]

    def run64():
        from cocosnet_amd import inference
        G64 = copy.deepcopy(G)
        inference.unfreeze(G64)
        return [G64.double().cpu()(seg.double().cpu(), warp_out=cbn.double().cpu())]
    return G, run, run, run64


VGG_KEYS = ["r12", "r22", "r32", "r42", "r52"]


def _vgg_case(B=2, S=64):
    from cocosnet_amd import vgg
    torch.manual_seed(3)
    v = vgg.VGG19_feature_color_torchversion().to(DEV).eval()
    with torch.no_grad():
        for m in v.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
                m.bias.normal_(0.0, 0.05)
    for p in v.parameters():
        p.requires_grad_(False)
    g = torch.Generator(device=DEV).manual_seed(8)
    x = torch.rand(B, 3, S, S, device=DEV, generator=g)

    def run():
        return v(x, VGG_KEYS, preprocess=True)

    def run64():
        from cocosnet_amd import inference
        v64 = copy.deepcopy(v)
        inference.unfreeze(v64)
        return v64.double().cpu()(x.double().cpu(), VGG_KEYS, preprocess=True)
    return v, run, run, run64


def _vgg_grad(v, x, seeds):
    xi = x.clone().requires_grad_(True)
    feats = v(xi, VGG_KEYS, preprocess=True)
    torch.autograd.backward(feats, seeds)
    return xi.grad


CASES = {"netCorr_mk1": lambda: _corr_case(1), "netCorr_mk3": lambda: _corr_case(3), "SPADEGenerator": _generator_case, "VGG19": _vgg_case}


# ---- 2. launch accounting ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_second_and_third_frozen_forward_prepare_no_weight(case, hip_lib, monkeypatch):
    from cocosnet_amd import inference
    net, run, _, _ = CASES[case]()
    log = _CallLog(monkeypatch)
    with torch.no_grad():
        run()
        unfrozen = _weight_preparation_calls(log.calls, _weight_pointers(net))
        assert unfrozen, "the unfrozen forward prepares weights: the check below would be vacuous otherwise"
        n_unfrozen = len(log.calls)
        report = inference.freeze(net)
        assert report.layers > 0
        log.clear()
        run()                                      # first frozen forward: may prepare the layouts freeze() could not foresee
        for k in (2, 3):
            log.clear()
            run()
            bad = _weight_preparation_calls(log.calls, _weight_pointers(net))
            print(f"{case}: forward {k} frozen: {len(log.calls)} entry-point calls (unfrozen {n_unfrozen}, of which weight preparation "
                  f"{len(unfrozen)}); weight-preparation calls left: {len(bad)}")
            assert bad == [], (case, k, sorted(set(bad)))
            assert "cocos_weight_planes_multi" not in log.names() and "cocos_weight_absmax_multi" not in log.names()
    assert report.repreparations == 0


def test_frozen_vgg_inside_a_grad_enabled_step_prepares_no_weight(hip_lib, monkeypatch):
    from cocosnet_amd import inference
    v, run, _, _ = _vgg_case()
    x = torch.rand(2, 3, 64, 64, device=DEV)
    with torch.no_grad():
        seeds = [torch.randn_like(f) for f in run()]
    log = _CallLog(monkeypatch)
    report = inference.freeze(v)
    assert report.layers == 16 and all(r.keep_dgrad for r in report.records)
    assert torch.is_grad_enabled()
    for k in (1, 2, 3):
        log.clear()
        g = _vgg_grad(v, x, seeds)
        assert g is not None and torch.isfinite(g).all()
        bad = _weight_preparation_calls(log.calls, _weight_pointers(v))
        print(f"VGG19 forward + backward {k} frozen: {len(log.calls)} entry-point calls, weight-preparation calls left: {len(bad)}")
        assert bad == [] and not any(n.startswith("cocos_weight_") for n in log.names()), (k, sorted(set(bad)))
    assert report.repreparations == 0


# ---- 3. equality with the unfrozen route ------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / (b.double().abs().max().cpu() + 1e-30))


def _assert_frozen_matches(what, a, b, frozen_runs, run64):
    """`a`, `b`: two unfrozen runs; bitwise reproducible -> every frozen run equals them bitwise.  Otherwise, per output, against the
    fp64 copy (`run64`): frozen error <= unfrozen error + the unfrozen arm's own run-to-run difference.  Returns `reproducible`."""
    reproducible = all(torch.equal(x, y) for x, y in zip(a, b))
    print(f"{what}: unfrozen eval() forward bitwise reproducible: {reproducible}")
    if reproducible:
        for n, f in enumerate(frozen_runs):
            for k, (x, y) in enumerate(zip(a, f)):
                assert torch.equal(x, y), (what, n, k, _rel(y, x))
        return True
    ref = run64()
    for k, (x, y, r) in enumerate(zip(a, b, ref)):
        e_un, spread = _rel(x, r), _rel(x, y)
        for n, f in enumerate(frozen_runs):
            e_fr = _rel(f[k], r)
            print(f"{what}[{k}] frozen run {n}: error against fp64: unfrozen {e_un:.3e}, frozen {e_fr:.3e}; unfrozen run-to-run {spread:.3e}")
            assert e_fr <= e_un + spread, (what, k, n, e_fr, e_un, spread)
    return False


@pytest.mark.parametrize("case", list(CASES))
def test_frozen_forward_equals_the_unfrozen_forward(case, hip_lib):
    from cocosnet_amd import inference
    net, run, _, run64 = CASES[case]()
    with torch.no_grad():
        a, b = run(), run()
        report = inference.freeze(net)
        if case == "SPADEGenerator":      # its Attention block sits under the framework's own spectral_norm hook: frozen too
            from cocosnet_amd import producers
            hooks = [r.hook for r in report.records if r.hook is not None]
            assert sum(type(h) is producers._SpectralNormRecord for h in hooks) == 4 and report.skipped == []
        _assert_frozen_matches(case, a, b, [run(), run()], run64)


def test_frozen_vgg_input_gradient_equals_the_unfrozen_one(hip_lib):
    from cocosnet_amd import inference
    v, run, _, _ = _vgg_case()
    x = torch.rand(2, 3, 64, 64, device=DEV)
    with torch.no_grad():
        seeds = [torch.randn_like(f) for f in run()]
    a, b = _vgg_grad(v, x, seeds), _vgg_grad(v, x, seeds)
    reproducible = torch.equal(a, b)
    print(f"VGG19 input gradient: unfrozen bitwise reproducible: {reproducible}")
    inference.freeze(v)
    f = _vgg_grad(v, x, seeds)
    if reproducible:
        assert torch.equal(f, a), _rel(f, a)
        return
    v64 = copy.deepcopy(v)
    inference.unfreeze(v64)
    r = _vgg_grad(v64.double().cpu(), x.double().cpu(), [s.double().cpu() for s in seeds])
    e_un, spread, e_fr = _rel(a, r), _rel(a, b), _rel(f, r)
    print(f"VGG19 input gradient: error against fp64: unfrozen {e_un:.3e}, frozen {e_fr:.3e}; unfrozen run-to-run {spread:.3e}")
    assert e_fr <= e_un + spread


# ---- 4. invalidation on the device ------------------------------------------------------------------------------------------------
def test_load_state_dict_reprepares_every_layer_once(hip_lib):
    from cocosnet_amd import inference
    net, run, _, run64 = _corr_case(1)
    with torch.no_grad():
        report = inference.freeze(net)
        first = run()
        assert report.repreparations == 0
        g = torch.Generator(device=DEV).manual_seed(21)
        new = {k: (v * (1.0 + 0.2 * torch.rand(v.shape, device=v.device, generator=g)) if v.is_floating_point() and v.dim() > 1 else v.clone())
               for k, v in net.state_dict().items()}
        net.load_state_dict(new)
        second = run()
        assert report.repreparations == report.layers, (report.repreparations, report.layers)
        third = run()
        assert report.repreparations == report.layers
        assert not torch.equal(second[0], first[0])
        inference.FROZEN = False
        try:
            u1, u2 = run(), run()
        finally:
            inference.FROZEN = True
        _assert_frozen_matches("netCorr_mk1 after load_state_dict", u1, u2, [second, third], run64)


# ---- 5. live buffers --------------------------------------------------------------------------------------------------------------
def test_a_frozen_forward_hands_over_live_buffers_only(hip_lib, monkeypatch):
    from cocosnet_amd import inference
    net, run, _, _ = _corr_case(3)
    with torch.no_grad():
        report = inference.freeze(net)
        run()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        guard = _CallLog(monkeypatch, guard=True)
        run()
        torch.cuda.synchronize()
    assert len(guard.calls) >= 100 and guard.pointers >= 500, (len(guard.calls), guard.pointers)
    assert not guard.dead, f"pointers into freed blocks at call time (entry point, argument index, address, block size): {guard.dead[:8]}"
    for rec in report.records:      # the records hold their planes
        assert rec.weight is not None and rec.amax is not None
        for hi, lo, sc in rec._layouts.values():
            assert hi.is_cuda and hi.numel() > 0


# ---- 6. default unchanged ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["netCorr_mk1", "netCorr_mk3", "VGG19"])
def test_without_freeze_the_call_sequence_is_the_parent_route(case, hip_lib, monkeypatch):
    from cocosnet_amd import inference
    net, run, _, _ = CASES[case]()
    log = _CallLog(monkeypatch)
    with torch.no_grad():
        run()                                      # (warm: caches of the first call)
        log.clear()
        run()
        default = log.names()
        monkeypatch.setattr(inference, "FROZEN", False)      # = COCOS_FROZEN=0: records ignored, the parent's route
        log.clear()
        run()
        expected = log.names()
        assert default == expected and len(default) > 10
        assert not any(n.startswith("cocos_weight_") for n in default)
        # ... and a FROZEN module under the switch takes the same route again
        inference.freeze(net)
        log.clear()
        run()
        assert log.names() == expected
