"""Every autograd.Function of cocosnet_amd.ops that reads ctx.needs_input_grad, run with `requires_grad` on PROPER SUBSETS of its
differentiable inputs — the way the GAN steps run them (D step: detached fake image, need_x = False; G step: frozen discriminator /
VGG, need_w = need_b = False) — against the same fp64 reference and the same bound as the op's existing all-gradients test.

`check_subsets` does, per subset S: forward vs fp64, .grad of every name in S vs fp64 autograd and finite (COCOS_POISON_EMPTY=1 turns
an output nobody wrote into NaN), .grad is None outside S; once per case: a no_grad forward vs fp64 and a second backward over a
retained graph (same gradients again, or RuntimeError — never a silently different value).  Where `ops._call` tags make it visible,
the launches a subset must NOT make are asserted too.

Functions of ops.py that read needs_input_grad and have no case here:
  _Relu, _ReluPool2, _MaskNll (and every other single-input Function): one differentiable input, no proper subset;
  _CorrSoftmaxWarp with operand_amax: reached through softmax_attention below."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import contextual_ref as cr
from oracle import corr_oracle as co

pytestmark = pytest.mark.gpu
DEV = "cuda"
E22 = 2.0 ** -22


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


@pytest.fixture(params=["f16x3", "fp32"])
def precision(request, monkeypatch):
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "PRECISION", request.param)
    monkeypatch.setattr(ops, "PROJ_PRECISION", request.param)
    return request.param


# ---------------------------------------------------------------------------------------------------------------- bounds
# A bound is a callable (got fp32 tensor, ref fp64 tensor) -> error / limit; the check is ratio < 1 (<= 1 where the test it is taken
# from asserts <=).  None of them is a new number: each case names the test it copies its measure and limit from.
def rel(tol, floor=1e-30):
    """max|x - ref| / (max|ref| + floor) < tol — `rel` of test_gpu_parity.py / test_gpu_baseline_sizes.py / test_gpu_mk3_sizes.py"""
    def f(got, ref):
        return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + floor)) / tol, True
    return f


def relmax(tol, least=1e-30):
    """max|x - ref| <= tol * max(max|ref|, least) — `close` of test_gpu_conv.py"""
    def f(got, ref):
        return float((got.double().cpu() - ref).abs().max()) / (tol * max(float(ref.abs().max()), least)), False
    return f


def elem(tol, least=1.0):
    """max(|x - ref| / max(|ref|, least)) <= tol — `_close` of test_gpu_norm_spade.py"""
    def f(got, ref):
        return float(((got.double().cpu() - ref).abs() / ref.abs().clamp_min(least)).max()) / tol, False
    return f


def elem_rel(tol):
    """|x - ref| <= tol * |ref| element by element, exact zeros where ref is zero — `_check_grad` / `_check_value` of test_gpu_losses.py"""
    def f(got, ref):
        g = got.double().cpu()
        if not bool((g[ref == 0] == 0).all()):
            return float("inf"), False
        nz = ref != 0
        return (float(((g[nz] - ref[nz]).abs() / ref[nz].abs()).max()) / tol if bool(nz.any()) else 0.0), False
    return f


RATIOS = {}      # op -> [cases, largest error / bound]


def _judge(op, b, got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio, strict = b(got, ref)
    ent = RATIOS.setdefault(op, [0, 0.0])
    ent[1] = max(ent[1], ratio)
    assert (ratio < 1.0) if strict else (ratio <= 1.0), f"{op} {what}: error / bound = {ratio:.3g}"


# ---------------------------------------------------------------------------------------------------------------- the driver
class Out:
    """What `fn` may return when the tensors that are differentiated (`outs`) are not the ones that hold the values (`values`):
    K23 / K25 hand back autograd handles whose memory is never written, the values sit in operand planes."""

    def __init__(self, outs, values):
        self.outs, self.values = list(outs), list(values)


def _unpack(res):
    if isinstance(res, Out):
        return res.outs, res.values
    outs = [res] if torch.is_tensor(res) else list(res)
    return outs, outs


def all_subsets(names):
    names = list(names)
    return [set(c) for r in range(1, len(names) + 1) for c in itertools.combinations(names, r)]


#: the fixed list for the six-input pair ops (63 subsets otherwise)
PAIR_NAMES = ("x_theta", "w_theta", "b_theta", "x_phi", "w_phi", "b_phi")
PAIR_SUBSETS = [{n} for n in PAIR_NAMES] + [{"x_theta", "x_phi"}, {"w_theta", "w_phi", "b_theta", "b_phi"},
                                            {"x_theta", "x_phi", "w_phi", "b_phi"}, set(PAIR_NAMES)]


def autograd_ref(f):
    """ref_fn from the operation written in plain torch: f(dict of fp64 CPU tensors, fp32 values of the op) -> output(s)"""
    def ref(inp, douts, vals32, diff_names):
        for n in diff_names:
            inp[n].requires_grad_(True)
        res = f(inp, vals32)
        outs = [res] if torch.is_tensor(res) else list(res)
        torch.autograd.backward(outs, douts)
        return [o.detach() for o in outs], {n: inp[n].grad for n in diff_names}
    return ref


def _leaves(inputs, S):
    return {n: (t.detach().clone().requires_grad_(n in S) if torch.is_tensor(t) and t.is_floating_point() else t) for n, t in inputs.items()}


def check_subsets(fn, inputs, diff_names, ref_fn, bound, subsets=None, op="op", dout_scale=1.0, amax_names=(), on_tags=None,
                  second_backward=True, max_subsets=7, dout_abs=False):
    """See the module docstring.  `inputs`: name -> fp32 device tensor (or anything else, handed through); `bound`: {"out": bound or
    list of bounds per output, name: bound}; `amax_names`: inputs whose gradient must arrive with its max|.| cell
    (ops._recall_amax(grad, consume=False) == grad.abs().max(), exactly); `on_tags(S, tags)`: the ops._call tags of forward + backward."""
    from cocosnet_amd import ops
    diff_names = [n for n in diff_names if inputs[n] is not None]
    subsets = all_subsets(diff_names) if subsets is None else [set(s) & set(diff_names) for s in subsets]
    subsets = [s for i, s in enumerate(subsets) if s and s not in subsets[:i]]
    assert 0 < len(subsets) <= max_subsets, len(subsets)
    out_bounds = bound["out"]
    # ---- the no_grad forward (keep = False / want_chan = False forwards), the fixed dout and the fp64 reference — once
    with torch.no_grad():
        _, vals0 = _unpack(fn(_leaves(inputs, set())))
    g = torch.Generator(device=DEV).manual_seed(20240607)
    douts = [(torch.randn(v.shape, device=DEV, generator=g) * dout_scale).contiguous() for v in vals0]
    if dout_abs:        # (the loss kernels' 2^-22 is a bound for terms of one sign: no cancellation between a cell and the sum cell)
        douts = [d.abs() for d in douts]
    inp64 = {n: (t.detach().double().cpu() if torch.is_tensor(t) and t.is_floating_point() else
                 (t.detach().cpu() if torch.is_tensor(t) else t)) for n, t in inputs.items()}
    ref_vals, ref_grads = ref_fn(inp64, [d.double().cpu() for d in douts], [v.detach() for v in vals0], diff_names)
    ref_vals = [torch.as_tensor(np.asarray(v)) if not torch.is_tensor(v) else v for v in ref_vals]
    ref_grads = {n: (torch.as_tensor(np.asarray(v)) if not torch.is_tensor(v) else v) for n, v in ref_grads.items()}
    if not isinstance(out_bounds, (list, tuple)):
        out_bounds = [out_bounds] * len(ref_vals)
    assert len(vals0) == len(ref_vals)

    def judge_values(vals, what):
        for i, (v, r, b) in enumerate(zip(vals, ref_vals, out_bounds)):
            _judge(op, b, v.detach(), r, f"{what} output {i}")

    judge_values(vals0, "no_grad")
    # ---- every subset
    for S in subsets:
        tag = "{" + ",".join(sorted(S)) + "}"
        lv = _leaves(inputs, S)
        seen = {}
        for n in set(amax_names) & S:
            lv[n].register_hook(lambda gr, n=n: seen.__setitem__(n, (ops._recall_amax(gr, consume=False), gr.abs().max())))
        with ops.KernelTimer() as kt:
            outs, vals = _unpack(fn(lv))
            torch.autograd.backward(outs, douts)
        tags = set(kt.summary())
        judge_values(vals, tag)
        for n in diff_names:
            if n not in S:
                assert lv[n].grad is None, f"{op} {tag}: {n} received a gradient nobody asked for"
                continue
            assert lv[n].grad is not None, f"{op} {tag}: no gradient for {n}"
            assert bool(torch.isfinite(lv[n].grad).all()), f"{op} {tag}: d {n} is not finite"
            _judge(op, bound[n], lv[n].grad, ref_grads[n], f"{tag} d {n}")
        for n in set(amax_names) & S:
            cell, mx = seen[n]
            assert cell is not None and float(cell) == float(mx), f"{op} {tag}: max|d {n}| cell {cell} vs {float(mx)}"
        if on_tags is not None:
            on_tags(S, tags)
        RATIOS.setdefault(op, [0, 0.0])[0] += 1
    # ---- a second backward over the retained graph: the same gradients again, or RuntimeError
    if second_backward:
        lv = _leaves(inputs, set(diff_names))
        outs, _ = _unpack(fn(lv))
        wrt = [lv[n] for n in diff_names]
        first = torch.autograd.grad(outs, wrt, douts, retain_graph=True)
        try:
            second = torch.autograd.grad(outs, wrt, douts, retain_graph=True)
        except RuntimeError:
            second = None
        for which, grads in (("first", first), ("second", second)):
            for n, gr in zip(diff_names, grads or ()):
                assert bool(torch.isfinite(gr).all()), f"{op} {which} backward: d {n} is not finite"
                _judge(op, bound[n], gr, ref_grads[n], f"{which} backward over a retained graph, d {n}")
    torch.cuda.synchronize()
    print("GRAD_SUBSETS", op, "cases", RATIOS[op][0], "largest error/bound %.3g" % RATIOS[op][1])


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, device=DEV, generator=g) * scale


# ---------------------------------------------------------------------------------------------------------------- conv2d
CONV_LAYERS = {
    # x shape, Cout, k, stride, pad, reflect, bias, on K16b / K16c (ops._conv_nhwc_ok: Cin >= 32, Cout >= 128; OW % 32 == 0 keeps xp)
    "k3_nhwc": ((2, 128, 4, 32), 128, 3, 1, 1, 0, True, True),
    "k3_gather_ragged": ((3, 5, 9, 7), 7, 3, 1, 1, 0, True, False),              # test_conv2d_matches_fp64 "everything ragged"
    "k4_s2_strided_dgrad": ((1, 16, 18, 22), 40, 4, 2, 1, 0, True, False),       # ... "adaptor down-sampling"
    "reflect_fold": ((1, 128, 4, 32), 128, 3, 1, 0, 1, True, True),              # test_conv2d_reflect_fused_equals_pad_then_conv
    "reflect_fused_no_fold": ((1, 128, 3, 32), 128, 3, 1, 0, 1, True, True),     # padded H - 2 = 3 < 4: K18's backward gather
    "reflect_5x5_unfused": ((2, 6, 5, 5), 7, 3, 1, 0, 1, True, False),           # reflect_pad2d + the plain layer
    "no_bias": ((3, 5, 9, 7), 7, 3, 1, 1, 0, False, False),
}


@pytest.mark.parametrize("flavour,tol", [("f16x3", 1e-5), ("bf16", 1.5e-2)])
@pytest.mark.parametrize("layer", sorted(CONV_LAYERS))
def test_conv2d(layer, flavour, tol, monkeypatch):
    """bounds: test_conv2d_matches_fp64 (f16x3: 1e-5 of the range) / test_conv2d_bf16_flavour_error_vs_fp64 (1.5e-2)"""
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", flavour)
    xs, Cout, k, stride, pad, reflect, bias, nhwc = CONV_LAYERS[layer]
    g = torch.Generator(device=DEV).manual_seed(11)
    Cin = xs[1]
    inputs = dict(x=_rand(g, *xs), w=_rand(g, Cout, Cin, k, k) / (Cin * k * k) ** 0.5, b=_rand(g, Cout) if bias else None)
    fn = lambda t: ops.conv2d(t["x"], t["w"], t["b"], stride, pad, 1, reflect=reflect)
    ref = autograd_ref(lambda t, _: F.conv2d(F.pad(t["x"], (reflect,) * 4, mode="reflect") if reflect else t["x"], t["w"], t["b"],
                                             stride=stride, padding=pad))
    fold = reflect == 1 and nhwc and xs[2] + 2 - 2 >= 4

    def on_tags(S, tags):
        assert ("conv2d_nhwc_prep" in tags) == nhwc, (layer, S, sorted(tags))                 # the route the case is named after
        assert ("conv2d_wgrad" in tags) == ("w" in S), (S, sorted(tags))                       # no weight gradient nobody asked for
        assert ("channel_sum" in tags) == ("b" in S and bias), (S, sorted(tags))               # ... and no bias gradient
        if reflect and "x" in S:
            assert ("reflect_pad2d_bwd" in tags) == (not fold), (S, sorted(tags))
        if reflect:
            assert ("reflect_pad2d_fwd" in tags) == (not nhwc), (S, sorted(tags))
    b = relmax(tol)
    check_subsets(fn, inputs, ("x", "w", "b"), ref, dict(out=b, x=b, w=b, b=b), op=f"conv2d[{flavour}]", on_tags=on_tags)
    if flavour != "bf16":
        return
    # ... and against the flavour's own operands (tests/conv_bf16_case.py): fp64 of the bf16-rounded x, w, dy, the bound being
    # factor x the error of the framework's fp32 convolution on the same operands — four decades below the 1.5e-2 above
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import accuracy_case as ac
    import conv_bf16_case as cb
    case =cb.Case(layer, xs, Cout, k, stride, pad, 1, reflect, bias, "normal")
    factor, names, arms = cb.factors(cb.routes(case)), dict(out="y", x="dx", w="dw", b="db"), {}

    def ref_exact(inp, douts, vals32, diff_names):
        args = (inp["x"], inp["w"], inp["b"], douts[0], stride, pad, 1, reflect)
        got = dict(zip(cb.TENSORS, cb.reference(*args)))
        arms.update(zip(cb.TENSORS, cb.fp32_arm(*args)))
        return [got["y"]], {n: got[names[n]] for n in diff_names}

    def exact(n):
        t = names[n]

        def f(got, want):
            as3 = cb._AS3[t]
            ek, ea = ac.rel_max(as3(got), as3(want)), ac.rel_max(as3(arms[t]), as3(want))
            limit = ac.bound(ea, factor[(t, "rel_max")])
            assert limit <= cb.CEILING, (t, limit)
            return ek / limit, False
        return f
    check_subsets(fn, inputs, ("x", "w", "b"), ref_exact, {n: exact(n) for n in names}, op="conv2d[bf16-exact]", on_tags=on_tags)


# ---------------------------------------------------------------------------------------------------------------- proj1x1
@pytest.mark.parametrize("shape,stream", [((2, 407, 256, 8, 8), True), ((2, 407, 256, 8, 8), False), ((1, 130, 70, 23, 29), True)])
def test_proj1x1(shape, stream, precision, monkeypatch):
    """shapes and the 1e-5 of test_proj1x1_equals_conv2d; PROJ_STREAM off = the GEMM form (test_proj1x1_streaming_and_gemm_forms_agree)"""
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "PROJ_STREAM", stream)
    B, Cin, Cout, h, w = shape
    g = torch.Generator(device=DEV).manual_seed(Cin)
    inputs = dict(x=_rand(g, B, Cin, h, w), w=_rand(g, Cout, Cin, 1, 1, scale=0.1), b=_rand(g, Cout))
    fn = lambda t: ops.proj1x1(t["x"], t["w"], t["b"])
    ref = autograd_ref(lambda t, _: F.conv2d(t["x"], t["w"], t["b"]))
    b = rel(1e-5)
    check_subsets(fn, inputs, ("x", "w", "b"), ref, dict(out=b, x=b, w=b, b=b), op=f"proj1x1[{precision}]")


# ---------------------------------------------------------------------------------------------------------------- K23 / K24 / K25
def _proj_case(B, Cin, h, w, seed, bias=True):
    """tests/test_gpu_proj_norm.py `_case`"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x1 = _rand(g, B, Cin, h, w)
    x2 = 0.3 * x1 + _rand(g, B, Cin, h, w)
    d = dict(x_theta=x1, w_theta=_rand(g, 256, Cin, 1, 1) / Cin ** 0.5, b_theta=None,
             x_phi=x2, w_phi=_rand(g, 256, Cin, 1, 1) / Cin ** 0.5, b_phi=None)
    if bias:
        d["b_theta"], d["b_phi"] = _rand(g, 256, scale=0.1), _rand(g, 256, scale=0.1)
    return d


def _lazy(t, side):
    from cocosnet_amd import ops
    return ops.LazyProj1x1(t["x_" + side], t["w_" + side], t["b_" + side])


def _proj64(t, side):
    return F.conv2d(t["x_" + side], t["w_" + side], t["b_" + side])


@pytest.mark.parametrize("fused_bwd", [True, False])
@pytest.mark.parametrize("B,Cin,h,w,bias", [(1, 256, 8, 16, True), (2, 19, 8, 16, False)])
def test_proj_center_l2norm_planes_pair(B, Cin, h, w, bias, fused_bwd, monkeypatch):
    """K23 forward (planes within 4e-6 absolute: test_k23_planes_match_fp64_projection_centring_normalisation) and K24 mode 0 /
    round 5's chain backward (2e-5: test_k24_mode0_gradients_of_the_fused_projection_match_fp64, whose G1 / G2 scales are kept)"""
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    monkeypatch.setattr(ops, "PROJ_PRECISION", "f16x3")
    monkeypatch.setattr(ops, "PROJ_BWD_FUSED", fused_bwd)
    inputs = _proj_case(B, Cin, h, w, seed=3 * Cin + h, bias=bias)
    N, S = h * w, ops.SPLIT_OPERAND_SCALE

    def fn(t):
        planes = ops.OperandPlanes()
        want_chan = torch.is_grad_enabled() and any(torch.is_tensor(v) and v.requires_grad for v in t.values())
        qn, kn = ops.proj_center_l2norm_planes_pair(_lazy(t, "theta"), _lazy(t, "phi"), 1, planes, want_chan=want_chan)
        vals = []
        for hd in (qn, kn):
            ph, pl = planes.get(hd, True, S)
            vals.append(((ph.double() + pl.double()) / S).transpose(1, 2).float())
        # (the second handle's gradient is 1e-3 of the first's, as in the test the bound comes from)
        return Out([qn, kn * 1e-3], [vals[0], vals[1] * 1e-3])

    def ref(t, _):
        res = []
        for side, sc in (("theta", 1.0), ("phi", 1e-3)):
            th = _proj64(t, side).reshape(B, 256, N)
            thc = th - th.mean(dim=1, keepdim=True)
            res.append(thc / (thc.norm(dim=1, keepdim=True) + co.EPS) * sc)
        return res

    def on_tags(Sub, tags):
        if not ({"x_theta", "x_phi"} & Sub):          # need_x = False on both sides: K24's input-gradient kernel must not run
            assert "proj_bwd_input" not in tags, (Sub, sorted(tags))
    absb = lambda lim: (lambda got, r: (float((got.double().cpu() - r).abs().max()) / lim, True))
    gb = rel(2e-5, floor=1e-300)
    bound = dict(out=[absb(4e-6), absb(4e-9)], **{n: gb for n in PAIR_NAMES})
    check_subsets(fn, inputs, PAIR_NAMES, autograd_ref(ref), bound, subsets=PAIR_SUBSETS, op=f"proj_center_l2norm_planes_pair[fused_bwd={fused_bwd}]",
                  on_tags=on_tags, max_subsets=len(PAIR_SUBSETS))


@pytest.mark.parametrize("fused_bwd", [True, False])
@pytest.mark.parametrize("B,Cin,h,w", [(1, 256, 8, 64), (2, 33, 2, 64)])
def test_proj_unfold3_stats(B, Cin, h, w, fused_bwd, monkeypatch):
    """test_k24_mode1_projection_plus_unfold_statistics_gradients_match_fp64: values 5e-6, gradients 2e-5, its gradient scales"""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import _unfold3_stats
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    monkeypatch.setattr(ops, "PROJ_PRECISION", "f16x3")
    monkeypatch.setattr(ops, "PROJ_BWD_FUSED", fused_bwd)
    c = _proj_case(B, Cin, h, w, seed=Cin)
    inputs = dict(x=c["x_theta"], w=c["w_theta"], b=c["b_theta"])
    kc = 256.0 * 9

    def fn(t):
        th, mu, a = ops.proj_unfold3_stats(ops.LazyProj1x1(t["x"], t["w"], t["b"]), kc)
        return th, mu, a * 0.1

    def ref(t, _):
        th = F.conv2d(t["x"], t["w"], t["b"])
        mu, a = _unfold3_stats(th, kc)
        return th, mu, a * 0.1
    vb, gb = rel(5e-6, floor=1e-300), rel(2e-5, floor=1e-300)
    check_subsets(fn, inputs, ("x", "w", "b"), autograd_ref(ref), dict(out=vb, x=gb, w=gb, b=gb), op=f"proj_unfold3_stats[fused_bwd={fused_bwd}]")


@pytest.mark.parametrize("B,Cin,h,w,bias", [(1, 256, 8, 64, True), (2, 33, 2, 64, False)])
def test_proj_raw_planes_stats_pair(B, Cin, h, w, bias, monkeypatch):
    """K25 takes "all or none" (ops.proj_raw_fused_ok gates it): the node itself is run with every input differentiated and under
    no_grad — planes 2^-20 of the range, statistics 5e-6 (test_k25_planes_sums_and_statistics_match_fp64), gradients 2e-5 with the
    gradient scales of test_k25_gradients_match_fp64 — and every mixed subset must be REFUSED by the gate (the hot path then takes
    the unfused route, which test_hot_path_match_kernel3_lazy_projections checks)."""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import _unfold3_stats
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    monkeypatch.setattr(ops, "PROJ_PRECISION", "f16x3")
    inputs = _proj_case(B, Cin, h, w, seed=Cin + 1, bias=bias)
    N, kc = h * w, 256.0 * 9
    scales = (1.0, 1.0, 0.1, 1e-3, 1.0, 0.1)

    def fn(t):
        holder = ops.Box3RawPlanes()
        th_l, ph_l = _lazy(t, "theta"), _lazy(t, "phi")
        assert ops.proj_raw_fused_ok(th_l, ph_l)
        (th, mu, a), (ph, nu, b) = ops.proj_raw_planes_stats_pair(th_l, ph_l, kc, holder)
        vals = []
        for hd in (th, ph):
            phh, pll, _, _, sc = holder.get(hd)
            vals.append(((phh.double() + pll.double()) / sc.double()).transpose(1, 2).reshape(B, 256, h, w).float())
        outs = [th, mu, a, ph, nu, b]
        return Out([o * s for o, s in zip(outs, scales)], [v * s for v, s in zip([vals[0], mu, a, vals[1], nu, b], scales)])

    def ref(t, _):
        res = []
        for side in ("theta", "phi"):
            y = _proj64(t, side)
            res += [y, *_unfold3_stats(y, kc)]
        return [r * s for r, s in zip(res, scales)]
    pb, sb, gb = relmax(2.0 ** -20), rel(5e-6, floor=1e-300), rel(2e-5, floor=1e-300)
    names = [n for n in PAIR_NAMES if inputs[n] is not None]
    check_subsets(fn, inputs, PAIR_NAMES, autograd_ref(ref), dict(out=[pb, sb, sb, pb, sb, sb], **{n: gb for n in PAIR_NAMES}),
                  subsets=[set(names)], op="proj_raw_planes_stats_pair")
    for Sub in PAIR_SUBSETS[:-1]:
        lv = _leaves(inputs, Sub & set(names))
        if Sub & set(names):
            assert not ops.proj_raw_fused_ok(_lazy(lv, "theta"), _lazy(lv, "phi")), Sub


def _hot_path_case(mk, B, Cin, fh, fw, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    inputs = _proj_case(B, Cin, fh, fw, seed=seed)
    down, nc = 4, 7
    H, W = fh * down, fw * down
    inputs["ref_img"] = torch.rand(B, 3, H, W, device=DEV, generator=g) * 2 - 1
    lab = torch.randint(0, nc, (B, 1, H, W), device=DEV, generator=g)
    inputs["seg"] = torch.zeros(B, nc, H, W, device=DEV).scatter_(1, lab, 1.0)
    return inputs, dict(match_kernel=mk, PONO_C=True, down=down, warp_mask_losstype="direct", isTrain=True)


@pytest.mark.parametrize("mk,fh,fw", [(1, 8, 16), (3, 4, 64)])
def test_hot_path_with_lazy_projections(mk, fh, fw, precision):
    """correspondence_hot_path on LazyProj1x1 pairs with mixed subsets: match_kernel 3 is where ops.proj_raw_fused_ok is false and the
    FALLBACK route (proj_unfold3_stats per side, or K0 + K12) is what runs; match_kernel 1 takes K23 with per-projection th / tl / wtf.
    Reference: oracle/torch_ref.py on fp64 projections; bound: the 2e-4 of test_box3_fused_family_on_small_grids_vs_fp64_... /
    test_hot_path_matches_reference_fixtures (OUT_TOL) for outputs and gradients alike (__graft_entry__.smoke holds the same)."""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_hot_path
    from oracle import torch_ref as tr
    inputs, flags = _hot_path_case(mk, 2, 64 + 7, fh, fw, seed=21 + mk)
    cfg = HotPathConfig(**flags)

    def fn(t):
        out = correspondence_hot_path(_lazy(t, "theta"), _lazy(t, "phi"), t["ref_img"], t["ref_img"], t["seg"], t["seg"], cfg)
        return [out["warp_mask"], out["warp_out"]]

    def ref(t, _):
        out = tr.hot_path(_proj64(t, "theta"), _proj64(t, "phi"), t["ref_img"], t["ref_img"], t["seg"], t["seg"], cfg)
        return [out["warp_mask"], out["warp_out"]]
    b = rel(2e-4)
    check_subsets(fn, inputs, PAIR_NAMES, autograd_ref(ref), dict(out=b, **{n: b for n in PAIR_NAMES}), subsets=PAIR_SUBSETS,
                  op=f"hot_path[mk{mk},{precision}]", max_subsets=len(PAIR_SUBSETS))


# ---------------------------------------------------------------------------------------------------------------- K2 and the materialised family
def _qkv(B, Nq, Nk, Cv, seed, K=256):
    rs = np.random.RandomState(seed)
    q, k = rs.standard_normal((B, K, Nq)), rs.standard_normal((B, K, Nk))
    v = rs.uniform(-1, 1, (B, Cv, Nk))
    return co.center_l2norm(q, True), co.center_l2norm(k, True), v


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _attention_ref(inv_t):
    """oracle/corr_oracle.py: corr_softmax_warp and its hand-written backward, in numpy fp64"""
    def ref(inp, douts, _vals, diff_names):
        q, k, v = (inp[n].numpy() for n in ("q", "k", "v"))
        dq, dk, dv = co.corr_softmax_warp_bwd(q, k, v, douts[0].numpy(), inv_t)
        return [co.corr_softmax_warp(q, k, v, inv_t)], dict(q=dq, k=dk, v=dv)
    return ref


@pytest.mark.parametrize("B,Nq,Nk,Cv,route", [(2, 64, 128, 3, "saved"), (1, 64, 128, 33, "recompute"), (1, 200, 177, 5, "ragged")])
def test_corr_softmax_warp(B, Nq, Nk, Cv, route, precision, monkeypatch):
    """test_fused_forward_backward_vs_oracle: 2e-4 with its floors (0.5 for d qn / d kn, 0.05 for d v).  `saved` / `recompute`: the
    two sides of ops._saves_logits (split flavour); `ragged`: Nk % 4 != 0, the exact-fp32 kernels under either flavour."""
    from cocosnet_amd import ops
    if route == "recompute":
        monkeypatch.setattr(ops, "MAX_SAVED_LOGITS_BYTES", 0)
    qn, kn, v = _qkv(B, Nq, Nk, Cv, seed=Nq * 7 + Nk)
    inputs = dict(q=_dev(qn), k=_dev(kn), v=_dev(v))
    fn = lambda t: ops.corr_softmax_warp(t["q"], t["k"], t["v"], 100.0)
    split = precision == "f16x3" and route != "ragged"

    def on_tags(S, tags):
        if split and S & {"q", "k"}:
            assert ("corr_softmax_warp_recompute" in tags) == (route == "recompute"), (S, sorted(tags))
        if not S & {"k", "v"}:          # need_k = False (and no d v, which shares the key side): no key-side GEMM or key kernel
            assert not tags & {"corr_softmax_warp_bwd_key_from_ds", "corr_softmax_warp_bwd_key"}, (S, sorted(tags))
    check_subsets(fn, inputs, ("q", "k", "v"), _attention_ref(100.0),
                  dict(out=rel(2e-4), q=rel(2e-4, 0.5), k=rel(2e-4, 0.5), v=rel(2e-4, 0.05)), op=f"corr_softmax_warp[{precision}]", on_tags=on_tags)


@pytest.mark.parametrize("K,Nq,Nk", [(64, 1024, 128), (64, 520, 36)])
def test_softmax_attention(K, Nq, Nk, precision):
    """test_softmax_attention_channel_counts_and_split_reductions: its fused (blocked) and materialised (Nk % 8 != 0) shapes, 2e-4"""
    from cocosnet_amd import ops
    rs = np.random.RandomState(K + Nq)
    q, k, v = rs.standard_normal((1, K, Nq)) * 1.5, rs.standard_normal((1, K, Nk)), rs.uniform(-1, 1, (1, 70, Nk))
    sc = float(1.0 / np.sqrt(K))
    inputs = dict(q=_dev(q), k=_dev(k), v=_dev(v))
    fn = lambda t: ops.softmax_attention(t["q"], t["k"], t["v"], sc)
    b = rel(2e-4)
    check_subsets(fn, inputs, ("q", "k", "v"), _attention_ref(sc), dict(out=b, q=b, k=b, v=b), op=f"softmax_attention[{precision}]")


@pytest.mark.parametrize("B,K,Nq,Nk", [(2, 256, 200, 300), (1, 17, 129, 127)])
def test_corr_materialize(B, K, Nq, Nk, precision):
    """test_materialised_path_vs_oracle: f within 1e-5, d qn / d kn within 2e-4; K % 8 == 0 takes the planes GEMM, 17 the split GEMM"""
    from cocosnet_amd import ops
    rs = np.random.RandomState(K + Nq + Nk)
    inputs = dict(q=_dev(rs.standard_normal((B, K, Nq))), k=_dev(rs.standard_normal((B, K, Nk))))
    fn = lambda t: ops.corr_materialize(t["q"], t["k"], 0.37)
    ref = autograd_ref(lambda t, _: torch.einsum("bci,bcj->bij", t["q"], t["k"]) * 0.37)
    check_subsets(fn, inputs, ("q", "k"), ref, dict(out=rel(1e-5), q=rel(2e-4), k=rel(2e-4)), op=f"corr_materialize[{precision}]")


@pytest.mark.parametrize("B,Nq,Nk,Cv", [(2, 200, 300, 5), (1, 129, 127, 154)])
def test_warp_materialized(B, Nq, Nk, Cv):
    """test_materialised_path_vs_oracle: o within 1e-4, gradients within 2e-4"""
    from cocosnet_amd import ops
    rs = np.random.RandomState(Nq + Nk)
    inputs = dict(p=_dev(co.softmax(rs.standard_normal((B, Nq, Nk)) * 3.0)), v=_dev(rs.standard_normal((B, Cv, Nk))))
    fn = lambda t: ops.warp_materialized(t["p"], t["v"])
    ref = autograd_ref(lambda t, _: torch.einsum("bij,bcj->bci", t["p"], t["v"]))
    check_subsets(fn, inputs, ("p", "v"), ref, dict(out=rel(1e-4), p=rel(2e-4), v=rel(2e-4)), op="warp_materialized")


@pytest.mark.parametrize("B,Nq,Nk,Cv", [(2, 64, 64, 3), (1, 129, 33, 5)])
def test_logits_softmax_warp(B, Nq, Nk, Cv, precision):
    """test_logits_softmax_warp_vs_oracle: 2e-4, floor 1e-3 for d logits; its data (sigma 6 logits, some peaked rows)"""
    from cocosnet_amd import ops
    rs = np.random.RandomState(Nq + 3 * Nk)
    f = rs.standard_normal((B, Nq, Nk)) * 6.0
    f[:, :, 0] += 25.0 * (rs.uniform(size=(B, Nq)) < 0.3)
    inputs = dict(logits=_dev(f.transpose(0, 2, 1)), v=_dev(rs.uniform(-1, 1, (B, Cv, Nk))))
    fn = lambda t: ops.logits_softmax_warp(t["logits"], t["v"])
    ref = autograd_ref(lambda t, _: torch.einsum("bji,bcj->bci", torch.softmax(t["logits"], dim=1), t["v"]))
    check_subsets(fn, inputs, ("logits", "v"), ref, dict(out=rel(2e-4), logits=rel(2e-4, 1e-3), v=rel(2e-4)), op=f"logits_softmax_warp[{precision}]")


@pytest.mark.parametrize("B,C,Nq,Nk,h", [(2, 40, 200, 330, 0.1), (1, 64, 513, 129, 0.5)])
def test_contextual_cx(B, C, Nq, Nk, h):
    """test_contextual_cx_rectangular_and_other_bandwidths: cx 2e-5, gradients 5e-5, oracle/contextual_ref.py"""
    from cocosnet_amd import ops
    g = torch.Generator(device=DEV).manual_seed(B * 1000 + Nq)
    nrm = lambda t: t / (t.norm(dim=1, keepdim=True) + 2.2e-16)
    inputs = dict(xn=nrm(_rand(g, B, C, Nq)), yn=nrm(_rand(g, B, C, Nk)))
    fn = lambda t: ops.contextual_cx(t["xn"], t["yn"], h, 1e-3)
    ref = autograd_ref(lambda t, _: cr.cx_rows(t["xn"], t["yn"], h, 1e-3))
    check_subsets(fn, inputs, ("xn", "yn"), ref, dict(out=rel(2e-5), xn=rel(5e-5), yn=rel(5e-5)), op="contextual_cx")


# ---------------------------------------------------------------------------------------------------------------- K19 / K20
@pytest.mark.parametrize("fh", [4, 8])
def test_box3_corr_xbox_and_softmax_warp(fh, monkeypatch):
    """box3_corr_xbox -> box3_softmax_warp as the pair they are (T is an opaque blocked layout, the gradient T's node receives a
    private contract between the two): the smallest grids of test_box3_fused_family_on_small_grids_vs_fp64_and_vs_the_materialised_chain
    (4 x 64: two of four rows are border rows; 8 x 64), its 2e-4, far below ops.BOX3_ALIAS_T_BYTES.  Reference: the unfolded
    formulation in torch fp64 — box(C) = unfold3(q)^T unfold3(k)."""
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    B, fw, Cv, kc, scale = 1, 64, 5, 256.0 * 9, 100.0
    N = fh * fw
    assert ops.box3_fused_ok(B, 256, fh, fw, Cv) and B * N * N * 4 < ops.BOX3_ALIAS_T_BYTES
    g = torch.Generator(device=DEV).manual_seed(100 + fh)
    q = _rand(g, B, 256, fh, fw) + 0.15
    # (a weak copy, as in __graft_entry__.smoke: with the 0.4 of test_box3_fused_family_... the nine-tap match saturates the softmax
    #  when mu / a / nu / b are inputs of their own, the gradients vanish by cancellation — |d q_raw| ~ 1e-5 — and what is left is fp32
    #  rounding: d q_raw measured 1.6x (4 x 64) and 2.75x (8 x 64) the bound.  The data was changed, not the bound.)
    k = 0.05 * q.roll((1, 5), (2, 3)) + _rand(g, B, 256, fh, fw) - 0.1
    with torch.no_grad():
        (mu, a), (nu, b) = ops.unfold3_stats(q, kc), ops.unfold3_stats(k, kc)
    inputs = dict(q_raw=q, k_raw=k, mu=mu.clone(), a=a.clone(), nu=nu.clone(), b=b.clone(), v=torch.rand(B, Cv, N, device=DEV, generator=g) * 2 - 1)

    def fn(t):
        sink = ops.Box3GradSink()
        T = ops.box3_corr_xbox(t["q_raw"], t["k_raw"], sink)
        return ops.box3_softmax_warp(T, t["mu"], t["a"], t["nu"], t["b"], t["v"], fh, fw, kc, scale, False, sink)

    def ref(t, _):
        uq, uk = F.unfold(t["q_raw"], 3, padding=1), F.unfold(t["k_raw"], 3, padding=1)
        box = torch.einsum("bcp,bcq->bpq", uq, uk)
        z = scale * t["a"][:, :, None] * t["b"][:, None, :] * (box - kc * t["mu"][:, :, None] * t["nu"][:, None, :])
        return torch.einsum("bpq,bcq->bcp", torch.softmax(z, dim=2), t["v"])
    tb = rel(2e-4)
    names = ("q_raw", "k_raw", "mu", "a", "nu", "b", "v")
    subsets = [{"q_raw"}, {"k_raw"}, {"v"}, {"mu", "a", "nu", "b"}, {"q_raw", "k_raw"}, {"q_raw", "v"}, set(names)]
    check_subsets(fn, inputs, names, autograd_ref(ref), dict(out=tb, **{n: tb for n in names}), subsets=subsets, op="box3")


# ---------------------------------------------------------------------------------------------------------------- K9 / K17 / K26 / K13
@pytest.mark.parametrize("flavour", ["f16x3", "bf16"])
@pytest.mark.parametrize("B,C,h,w,slope", [(1, 64, 8, 12, 1.0), (2, 96, 7, 5, 0.2)])
def test_pono_spade(B, C, h, w, slope, flavour, monkeypatch):
    """test_pono_spade_equals_torch_chain: 1e-5, d x 2e-5 with floor 0.1.  (1, 64, 8, 12): the register kernel (C % 32 == 0, N % 4 == 0);
    (2, 96, 7, 5): the generic one.  f16x3: the `_amax` entry points, and d gamma / d beta arrive with their max|.| cells."""
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", flavour)
    rs = np.random.RandomState(C + h)
    inputs = dict(x=_dev(rs.standard_normal((B, C, h, w))), gamma=_dev(rs.standard_normal((B, C, h, w))), beta=_dev(rs.standard_normal((B, C, h, w))))
    fn = lambda t: ops.pono_spade(t["x"], t["gamma"], t["beta"], slope)

    def ref(t, _):
        x = t["x"]
        xn = (x - x.mean(1, keepdim=True)) / (x.var(1, keepdim=True) + 1e-5).sqrt()
        return F.leaky_relu(xn * (1 + t["gamma"]) + t["beta"], slope)
    check_subsets(fn, inputs, ("x", "gamma", "beta"), autograd_ref(ref), dict(out=rel(1e-5), x=rel(2e-5, 0.1), gamma=rel(1e-5), beta=rel(1e-5)),
                  op=f"pono_spade[{flavour}]", amax_names=("gamma", "beta") if flavour == "f16x3" else ())


@pytest.mark.parametrize("flavour", ["f16x3", "bf16"])
@pytest.mark.parametrize("shape,slope", [((2, 16, 12, 12), 0.2), ((1, 5, 7, 9), 1.0)])
def test_spade_modulate(shape, slope, flavour, monkeypatch):
    """test_spade_modulate_matches_torch_fp64: 1e-5 * max(range, 1); 4608 elements (whole float4s) and 315 (the tail)"""
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", flavour)
    g = torch.Generator(device=DEV).manual_seed(9)
    inputs = dict(x=_rand(g, *shape), gamma=_rand(g, *shape), beta=_rand(g, *shape))
    fn = lambda t: ops.spade_modulate(t["x"], t["gamma"], t["beta"], slope)
    ref = autograd_ref(lambda t, _: F.leaky_relu(t["x"] * (1 + t["gamma"]) + t["beta"], slope))
    b = relmax(1e-5, 1.0)
    check_subsets(fn, inputs, ("x", "gamma", "beta"), ref, dict(out=b, x=b, gamma=b, beta=b), op=f"spade_modulate[{flavour}]")


@pytest.mark.parametrize("flavour", ["f16x3", "bf16"])
@pytest.mark.parametrize("kind", ["batch", "instance"])
@pytest.mark.parametrize("shape", [(2, 16, 12, 12), (1, 5, 7, 9)])
def test_norm_spade(shape, kind, flavour, monkeypatch):
    """test_operator_matches_fp64 (test_gpu_norm_spade.py): training mode, slope 0.2, 1e-5 element by element against the framework
    formulation in fp64 on the fp32 arm's branch pattern.  f16x3: d gamma / d beta arrive with their max|.| cells."""
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", flavour)
    g = torch.Generator(device=DEV).manual_seed(3)
    slope = 0.2
    inputs = dict(x=_rand(g, *shape, scale=1.5) + 0.3, gamma=_rand(g, *shape, scale=0.5), beta=_rand(g, *shape, scale=0.5))
    fn = lambda t: ops.norm_spade(t["x"], t["gamma"], t["beta"], kind, training=True, slope=slope)

    def ref(t, vals32):
        xh = F.instance_norm(t["x"], eps=1e-5) if kind == "instance" else F.batch_norm(t["x"], None, None, training=True, momentum=0.0, eps=1e-5)
        return (xh * (1 + t["gamma"]) + t["beta"]) * torch.where(vals32[0].cpu() > 0, 1.0, slope).double()
    b = elem(1e-5)
    check_subsets(fn, inputs, ("x", "gamma", "beta"), autograd_ref(ref), dict(out=b, x=b, gamma=b, beta=b), op=f"norm_spade[{flavour}]",
                  amax_names=("gamma", "beta") if flavour == "f16x3" else ())


@pytest.mark.parametrize("flavour", ["f16x3", "bf16"])
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("B,C,h,w", [(2, 8, 64, 64), (1, 5, 7, 3)])
def test_instnorm_prelu(B, C, h, w, with_res, flavour, monkeypatch):
    """test_instnorm_prelu_equals_torch_chain: y 1e-5, d x 5e-5 (floor 0.05), d weight 5e-5 (floor 1.0), d residual 1e-5.  The three
    backward entry points (`_amax` when d x is wanted under f16x3, `_f64` when d weight is, the plain one) are picked by the subset."""
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", flavour)
    rs = np.random.RandomState(C + h)
    inputs = dict(x=_dev(rs.standard_normal((B, C, h, w))), residual=_dev(rs.standard_normal((B, C, h, w))) if with_res else None,
                  weight=_dev(np.array([0.25])))
    fn = lambda t: ops.instnorm_prelu(t["x"], t["residual"], t["weight"])
    ref = autograd_ref(lambda t, _: F.prelu(F.instance_norm(t["x"], eps=1e-5) + (t["residual"] if with_res else 0.0), t["weight"]))
    check_subsets(fn, inputs, ("x", "residual", "weight"), ref,
                  dict(out=rel(1e-5), x=rel(5e-5, 0.05), residual=rel(1e-5), weight=rel(5e-5, 1.0)), op=f"instnorm_prelu[{flavour}]")


# ---------------------------------------------------------------------------------------------------------------- K28
def _loss_tensors():
    import loss_case
    return loss_case.to_device(loss_case.make_inputs("celebahq"), DEV)


def test_pair_loss():
    """The feature-matching / perceptual table of tests/loss_case.py's `celebahq` case (five fake-vs-real feature pairs with exact
    ties, sample weights on one, a b-less MSE segment): values and gradients element by element within 2^-22 of fp64
    (test_pair_loss_against_fp64_and_framework).  Subsets: each single tensor, alternating tensors, all."""
    from cocosnet_amd import ops
    li = _loss_tensors()
    fake, real = li["fake_features"], li["real_features"]
    wts = li["self_ref"].reshape(-1).contiguous()
    names = [f"a{i}" for i in range(5)]
    inputs = {n: t for n, t in zip(names, fake)}
    coef = [(1.0 / 32, 0.0), (1.0 / 16, 0.0), (1.0 / 8, 1.0), (1.0 / 4, 0.0), (0.0, 1.0)]

    def table(t):
        return [(t[n], None if i == 4 else real[i].to(t[n].dtype).to(t[n].device), (wts.to(t[n].dtype).to(t[n].device) if i == 1 else None), *coef[i])
                for i, n in enumerate(names)]
    fn = lambda t: ops.pair_loss(table(t))

    def ref(t, _):
        rows = []
        for a, b, w, c1, c2 in table(t):
            d = a - b if b is not None else a
            l1 = d.abs() if w is None else d.abs() * w.view(-1, 1, 1, 1)
            rows.append(torch.stack([c1 * l1.mean(), c2 * (d ** 2).mean()]))
        rows = torch.stack(rows)
        return torch.cat([rows, rows.sum(0, keepdim=True)])
    b = elem_rel(E22)
    subsets = [{n} for n in names] + [{"a0", "a2", "a4"}, set(names)]
    check_subsets(fn, inputs, names, autograd_ref(ref), dict(out=b, **{n: b for n in names}), subsets=subsets, op="pair_loss", dout_abs=True)


@pytest.mark.parametrize("mode,label", [("hinge_d_fake", 0.0), ("ls", 1.0)])
def test_gan_loss(mode, label):
    """The discriminator predictions of tests/loss_case.py's `celebahq` case (two scales' last maps + two inner ones);
    test_gan_loss_against_fp64_and_framework: value within 2^-22 of sum|term|, gradients element by element within 2^-22."""
    from cocosnet_amd import ops
    li = _loss_tensors()
    xs = [li["pred_fake"][0][-1], li["pred_fake"][1][-1], li["pred_fake"][0][1], li["pred_fake"][1][2]]
    names = [f"x{i}" for i in range(4)]
    inputs = dict(zip(names, xs))
    fn = lambda t: ops.gan_loss([t[n] for n in names], mode, label)

    def term(x):
        return -torch.clamp(-x - 1, max=0.0) if mode == "hinge_d_fake" else (x - label) ** 2

    ref = autograd_ref(lambda t, _: (sum(term(t[n]).mean() for n in names) / len(names)).reshape(1))
    scale = float(sum(term(x.double()).abs().mean() for x in xs) / len(xs))
    vb = lambda got, r: (abs(float(got) - float(r)) / (E22 * scale), False)
    gb = elem_rel(E22)
    subsets = [{n} for n in names] + [{"x0", "x2"}, {"x1", "x3"}, set(names)]
    check_subsets(fn, inputs, names, ref, dict(out=vb, **{n: gb for n in names}), subsets=subsets, op=f"gan_loss[{mode}]", dout_abs=True)
