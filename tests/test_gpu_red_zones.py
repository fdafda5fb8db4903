"""Red zones: every op of cocosnet_amd run with each buffer it is handed, and each buffer it allocates, between two 64 KiB guards of
0xFF bytes (tests/guarded_alloc.py).  Per case:

  (a) no guard byte changed (a kernel wrote outside a buffer): the message names entry point, allocation site, side, offset, bytes;
  (b) every returned value and every gradient is finite — guards and unwritten interiors are NaN, so an out-of-bounds or uninitialised
      read that reaches a result shows; where an op hands back autograd handles whose memory holds nothing (`Out`), the tensors that
      hold the values are judged;
  (c) at least one guarded allocation and one `_lib.call` (a case cannot pass empty);
  (d) no allocation inside cocosnet_amd/ went past the guard (out=, pinned, a memory format ...).

Carved tensors sit at a non-zero storage offset: `untyped_storage().data_ptr()` handed over for `data_ptr()` lands in the front guard.
The shapes are the raggedest member of each existing parametrisation (tile tails, float4 tails, odd planes, size 1).  Nothing here
under-sizes a buffer: the detector itself is proven on the host (tests/test_guarded_alloc_cpu.py).

The last test asserts that every `cocos_*` entry point the package invokes through `_lib.call` was reached by a case, and writes
profiles/red_zone_coverage.txt."""
import ast
import glob
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded_alloc import guarded  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: entry points of the coverage condition that no case has to reach — the only accepted reason: the entry writes no device memory
EXCLUDED = {}

COVERAGE = {}      # case id -> (sorted entry points, guarded allocations, pass-throughs inside the package, _lib.call count)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


class Out:
    """outs: what is differentiated; values: the tensors that hold the values (see test_gpu_grad_subsets.Out)"""

    def __init__(self, outs, values):
        self.outs, self.values = list(outs), list(values)


class Ctx:
    """what a case body gets: `leaf` / `data` place a host tensor under guard (with / without requires_grad)"""

    def __init__(self, g):
        self.g, self.leaves = g, []

    def leaf(self, t):
        if t is None:
            return None
        p = self.g.place(t.float()).requires_grad_(True)
        self.leaves.append(p)
        return p

    def data(self, t):
        return None if t is None else self.g.place(t)


class _ClearTls(torch.autograd.Function):
    """its backward runs in autograd's device thread: the per-thread pools of THAT thread are cleared there"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        _clear_pools()
        return g


def _clear_pools():
    from cocosnet_amd import ops
    ops._tls.zero_pool.clear()
    ops._tls.known_amax.clear()
    ops._tls.known_rowdot = None
    if getattr(ops._tls, "nhwc_ws", None):
        ops._tls.nhwc_ws.clear()


def _flat(res):
    if res is None:
        return []
    if torch.is_tensor(res):
        return [res]
    return [t for r in res for t in _flat(r)]


def run_guarded(name, body):
    with guarded() as g:
        c = Ctx(g)
        _clear_pools()
        _ClearTls.apply(torch.ones(1, device=DEV, requires_grad=True)).sum().backward()
        res = body(c)
        outs, values = (res.outs, res.values) if isinstance(res, Out) else (_flat(res), _flat(res))
        todo = [o for o in outs if o.requires_grad]
        if todo:
            gen = torch.Generator().manual_seed(20241018)
            douts = [g.place(torch.randn(o.shape, generator=gen) * 0.5) for o in todo]
            torch.autograd.backward(todo, douts)
        g.check()
        torch.cuda.synchronize()
        values = [v.detach() for v in values] + [p.grad for p in c.leaves if p.grad is not None]
        finite = [bool(torch.isfinite(v).all()) if v.is_floating_point() else True for v in values]      # (integers hold no NaN)
        missing = [i for i, p in enumerate(c.leaves) if p.grad is None] if todo else []
    inside = g.passthroughs_inside_package()
    COVERAGE[name] = (sorted(g.entries), g.guarded_count, sum(inside.values()), g.calls)
    assert not g.violations, f"{name}: guard bytes changed:\n" + g.report()                                                    # (a)
    assert finite and all(finite), f"{name}: returned tensors / gradients (in order) finite: {finite}"                          # (b)
    assert not missing, f"{name}: no gradient arrived for leaf number {missing}"
    assert g.guarded_count >= 1 and g.calls >= 1, (name, g.guarded_count, g.calls)                                             # (c)
    assert not inside, f"{name}: allocations inside cocosnet_amd/ that the helper could not carve: {dict(inside)}"             # (d)


# ---------------------------------------------------------------------------------------------------------------- data
def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def uni(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def unit(B, K, N, seed):
    x = rnd(B, K, N, seed=seed).double()
    x = x - x.mean(1, keepdim=True)
    return (x / x.norm(dim=1, keepdim=True)).float()


def labels(B, nc, H, W, seed):
    return torch.randint(0, nc, (B, 1, H, W), generator=torch.Generator().manual_seed(seed))


def onehot(lab, nc):
    B, _, H, W = lab.shape
    return torch.zeros(B, nc, H, W).scatter_(1, lab, 1.0)


CASES = {}      # id -> (module attributes to set: {module name: {attribute: value}}, body)


def case(name, attrs=None, **mods):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = (dict(ops=dict(attrs or {}), **mods), fn)
        return fn
    return deco


def each(name, flavours, attrs=None):
    """one case per flavour: 'prec' = PRECISION / PROJ_PRECISION f16x3 | fp32, 'conv' = CONV_PRECISION f16x3 | bf16"""
    table = {"prec": [("f16x3", dict(PRECISION="f16x3", PROJ_PRECISION="f16x3")), ("fp32", dict(PRECISION="fp32", PROJ_PRECISION="fp32"))],
             "conv": [("f16x3", dict(CONV_PRECISION="f16x3")), ("bf16", dict(CONV_PRECISION="bf16"))]}[flavours]

    def deco(fn):
        for tag, a in table:
            case(f"{name}[{tag}]", dict(a, **(attrs or {})))(fn)
        return fn
    return deco


def _ops():
    from cocosnet_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------- correlation
def _csw(B, Nq, Nk, Cv, dv=True):
    def body(c):
        q, k = c.leaf(unit(B, 256, Nq, 1)), c.leaf(unit(B, 256, Nk, 2))
        v = (c.leaf if dv else c.data)(uni(B, Cv, Nk, seed=3))
        return _ops().corr_softmax_warp(q, k, v, 100.0)
    return body


each("corr_softmax_warp-1x200x176x5", "prec")(_csw(1, 200, 176, 5))
each("corr_softmax_warp-1x200x176x5-no_dv", "prec")(_csw(1, 200, 176, 5, dv=False))
each("corr_softmax_warp-1x129x33x5", "prec")(_csw(1, 129, 33, 5))
each("corr_softmax_warp-1x129x33x5-no_dv", "prec")(_csw(1, 129, 33, 5, dv=False))
each("corr_softmax_warp-1x64x128x40-lo_mask", "prec")(_csw(1, 64, 128, 40))
case("corr_softmax_warp-1x64x128x40-VALUE_LO_SKIP_off", dict(PRECISION="f16x3", VALUE_LO_SKIP=False))(_csw(1, 64, 128, 40))
case("corr_softmax_warp-1x200x176x5-BWD_D_PRECOMPUTED_off", dict(PRECISION="f16x3", BWD_D_PRECOMPUTED=False))(_csw(1, 200, 176, 5))
case("corr_softmax_warp-1x64x256x33-chunked_recompute",
     dict(PRECISION="f16x3", MAX_SAVED_LOGITS_BYTES=0, RECOMPUTE_CHUNK_BYTES=64 * 128 * 4))(_csw(1, 64, 256, 33))
case("corr_softmax_warp-1x64x256x170-two_value_chunks", dict(PRECISION="f16x3"))(_csw(1, 64, 256, 170))


def _attention(K, Nq, Nk, Cv):
    def body(c):
        q, k, v = c.leaf(rnd(1, K, Nq, seed=4, scale=1.5)), c.leaf(rnd(1, K, Nk, seed=5)), c.leaf(uni(1, Cv, Nk, seed=6))
        return _ops().softmax_attention(q, k, v, K ** -0.5)
    return body


each("softmax_attention-K32-operand_amax", "prec")(_attention(32, 72, 40, 7))
each("softmax_attention-K64-materialised", "prec")(_attention(64, 52, 36, 7))


@each("materialised_chain-1x64x130x257x3", "prec")
def _materialised(c):
    ops = _ops()
    q, k, v = c.leaf(rnd(1, 64, 130, seed=7)), c.leaf(rnd(1, 64, 257, seed=8)), c.leaf(uni(1, 3, 257, seed=9))
    return ops.warp_materialized(ops.row_softmax(ops.corr_materialize(q, k, 0.37)), v)


@each("materialised_chain-K17", "prec")
def _materialised17(c):
    ops = _ops()
    q, k, v = c.leaf(rnd(1, 17, 129, seed=7)), c.leaf(rnd(1, 17, 127, seed=8)), c.leaf(uni(1, 5, 127, seed=9))
    return ops.warp_materialized(ops.row_softmax(ops.corr_materialize(q, k, 0.37)), v)


def _lsw(B, Nq, Nk, Cv):
    def body(c):
        f = rnd(B, Nk, Nq, seed=Nq + 3 * Nk, scale=6.0)
        return _ops().logits_softmax_warp(c.leaf(f), c.leaf(uni(B, Cv, Nk, seed=10)))
    return body


each("logits_softmax_warp-1x129x33x5", "prec")(_lsw(1, 129, 33, 5))
each("logits_softmax_warp-1x1x1x1", "prec")(_lsw(1, 1, 1, 1))
each("logits_softmax_warp-2x64x64x3", "prec")(_lsw(2, 64, 64, 3))


@case("corr_softmax_warp_shared-Be1", dict(PRECISION="f16x3"))
def _shared(c):
    ops = _ops()
    B, Nq, Nk, Cv = 2, 200, 176, 5
    q, k, v = c.data(rnd(B, 256, Nq, seed=11)), c.data(rnd(1, 256, Nk, seed=12)), c.data(uni(1, Cv, Nk, seed=13))
    with torch.no_grad():
        qh, ql, _ = ops.center_l2norm_planes_fwd(q, True)
        keys = ops.PreparedKeys(1, (1, 256, 16, 11), (64, 44), None, lambda: ops.center_l2norm_planes_fwd(k, True), None, None)
        return ops.corr_softmax_warp_shared(qh, ql, keys, ops.PreparedValues(v, 3), 100.0)


# ---------------------------------------------------------------------------------------------------------------- norms
for _mode in (0, 1, 2):
    each(f"center_l2norm-mode{_mode}-2x37x50", "prec")(lambda c, m=_mode: _ops().center_l2norm(c.leaf(rnd(2, 37, 50, seed=14)), m))
each("center_l2norm-mode1-1x256x100", "prec")(lambda c: _ops().center_l2norm(c.leaf(rnd(1, 256, 100, seed=14)), 1))
each("feature_normalize-1x7x5x3", "prec")(lambda c: _ops().feature_normalize(c.leaf(rnd(1, 7, 5, 3, seed=15))))


@each("center_l2norm_planes-2x256x36", "prec")
def _cl2_planes(c):
    ops = _ops()
    planes = ops.OperandPlanes()
    x = c.leaf(rnd(2, 256, 36, seed=16))
    h = ops.center_l2norm_planes(x, 1, planes, want_chan=True)
    S = ops.SPLIT_OPERAND_SCALE
    return Out([h], [*planes.get(h, True, S), *planes.get(h, False, S)])


def _triple(shape, seed, **kw):
    return lambda c: (c.leaf(rnd(*shape, seed=seed, **kw)), c.leaf(rnd(*shape, seed=seed + 1, scale=0.5)), c.leaf(rnd(*shape, seed=seed + 2, scale=0.5)))


each("pono_spade-2x96x7x5", "conv")(lambda c: _ops().pono_spade(*_triple((2, 96, 7, 5), 17)(c), 0.2))
each("pono_spade-1x64x8x12-register_kernel", "conv")(lambda c: _ops().pono_spade(*_triple((1, 64, 8, 12), 17)(c), 1.0))
each("spade_modulate-315", "conv")(lambda c: _ops().spade_modulate(*_triple((1, 5, 7, 9), 20)(c), 1.0))
each("spade_modulate-4608", "conv")(lambda c: _ops().spade_modulate(*_triple((2, 16, 12, 12), 20)(c), 0.2))


def _norm_spade(kind, training, shape):
    def body(c):
        x, gamma, beta = _triple(shape, 23, scale=1.5)(c)
        rm = rv = nbt = None
        if kind != "instance":
            C = shape[1]
            rm, rv = c.data(rnd(C, seed=26, scale=0.3)), c.data(torch.rand(C, generator=torch.Generator().manual_seed(27)) * 1.5 + 0.5)
            nbt = c.data(torch.zeros((), dtype=torch.int64))
        y = _ops().norm_spade(x, gamma, beta, kind, rm, rv, nbt, training=training, momentum=0.1, slope=0.2)
        return Out([y], [y] + [t for t in (rm, rv) if t is not None])
    return body


for _kind, _training in (("batch", True), ("batch", False), ("syncbatch", True), ("syncbatch", False), ("instance", True)):
    for _shape in ((1, 5, 7, 9), (2, 16, 12, 12)):
        each(f"norm_spade-{_kind}-{'train' if _training else 'eval'}-{'x'.join(map(str, _shape))}", "conv")(_norm_spade(_kind, _training, _shape))


def _instnorm(shape, with_res, split, w_grad=True):
    def body(c):
        ops = _ops()
        x = c.leaf(rnd(*shape, seed=28, scale=3.0) + 0.5)
        res = c.leaf(rnd(*shape, seed=29, scale=3.0)) if with_res else None
        w = (c.leaf if w_grad else c.data)(torch.tensor([0.25]))
        return (ops.instnorm_prelu_split if split else ops.instnorm_prelu)(x, res, w)
    return body


for _res in (True, False):
    each(f"instnorm_prelu-1x5x7x3-res{int(_res)}", "conv")(_instnorm((1, 5, 7, 3), _res, False))
    each(f"instnorm_prelu_split-1x2x10x10-res{int(_res)}", "conv")(_instnorm((1, 2, 10, 10), _res, True))
    each(f"instnorm_prelu_split-1x3x2x8194-two_slices-res{int(_res)}", "conv")(_instnorm((1, 3, 2, 8194), _res, True))


each("instnorm_prelu-1x5x7x3-frozen_weight", "conv")(_instnorm((1, 5, 7, 3), True, False, w_grad=False))
each("instnorm_prelu_split-1x2x10x10-frozen_weight", "conv")(_instnorm((1, 2, 10, 10), True, True, w_grad=False))


@each("unfold3_stats-1x5x3x7", "prec")
def _unfold3(c):
    return _ops().unfold3_stats(c.leaf(rnd(1, 5, 3, 7, seed=30)), 45.0)


# ---------------------------------------------------------------------------------------------------------------- projections
def _proj(shape, stream):
    def body(c):
        B, Cin, Cout, h, w = shape
        return _ops().proj1x1(c.leaf(rnd(B, Cin, h, w, seed=31)), c.leaf(rnd(Cout, Cin, 1, 1, seed=32, scale=0.1)), c.leaf(rnd(Cout, seed=33)))
    return body


each("proj1x1-1x5x3x3x7", "prec")(_proj((1, 5, 3, 3, 7), True))
each("proj1x1-2x271x256x16x9-stream", "prec", dict(PROJ_STREAM=True))(_proj((2, 271, 256, 16, 9), True))
each("proj1x1-2x271x256x16x9-gemm", "prec", dict(PROJ_STREAM=False))(_proj((2, 271, 256, 16, 9), False))
each("proj1x1-2x407x256x8x8-stream", "prec", dict(PROJ_STREAM=True))(_proj((2, 407, 256, 8, 8), True))


def _pair(c, B, Cin, h, w, bias, seed, leaf=True):
    put = c.leaf if leaf else c.data
    x1 = rnd(B, Cin, h, w, seed=seed)
    x2 = 0.3 * x1 + rnd(B, Cin, h, w, seed=seed + 1)
    ops = _ops()
    mk = lambda x, s: ops.LazyProj1x1(put(x), put(rnd(256, Cin, 1, 1, seed=s) / Cin ** 0.5), put(rnd(256, seed=s + 1, scale=0.1)) if bias else None)
    return mk(x1, seed + 2), mk(x2, seed + 4)


def _k23_pair(B, Cin, h, w, bias, fused_bwd, grad=True):
    def body(c):
        ops = _ops()
        theta, phi = _pair(c, B, Cin, h, w, bias, 34, leaf=grad)
        planes = ops.OperandPlanes()
        S = ops.SPLIT_OPERAND_SCALE
        with torch.set_grad_enabled(grad):
            qn, kn = ops.proj_center_l2norm_planes_pair(theta, phi, 1, planes, want_chan=grad)
        vals = [t for hd in (qn, kn) for t in planes.get(hd, True, S)]
        return Out([qn, kn], vals)
    return body


_F16 = dict(PRECISION="f16x3", PROJ_PRECISION="f16x3")
for _fb in (True, False):
    case(f"proj_center_l2norm_planes_pair-2x19x8x16-fused_bwd{int(_fb)}", dict(_F16, PROJ_BWD_FUSED=_fb))(_k23_pair(2, 19, 8, 16, False, _fb))
    case(f"proj_center_l2norm_planes_pair-1x256x8x16-bias-fused_bwd{int(_fb)}", dict(_F16, PROJ_BWD_FUSED=_fb))(_k23_pair(1, 256, 8, 16, True, _fb))
case("proj_center_l2norm_planes_pair-1x3x16x8-no_grad", _F16)(_k23_pair(1, 3, 16, 8, True, True, grad=False))


@case("proj_center_l2norm_planes_one-1x3x16x8", _F16)
def _k23_one(c):
    theta, _ = _pair(c, 1, 3, 16, 8, True, 40, leaf=False)
    return _ops().proj_center_l2norm_planes_one(theta, 1)


def _k25_pair(B, Cin, h, w, bias):
    def body(c):
        ops = _ops()
        theta, phi = _pair(c, B, Cin, h, w, bias, 41)
        holder = ops.Box3RawPlanes()
        assert ops.proj_raw_fused_ok(theta, phi)
        (th, mu, a), (ph, nu, b) = ops.proj_raw_planes_stats_pair(theta, phi, 2304.0, holder)
        vals = [mu, a, nu, b]
        for hd in (th, ph):
            vals += [t for t in holder.get(hd) if torch.is_tensor(t)]
        return Out([th, mu, a * 0.1, ph, nu, b * 0.1], vals)
    return body


case("proj_raw_planes_stats_pair-2x33x2x64", _F16)(_k25_pair(2, 33, 2, 64, False))
case("proj_raw_planes_stats_pair-1x256x8x64-bias", _F16)(_k25_pair(1, 256, 8, 64, True))


def _k24_unfold(B, Cin, h, w):
    def body(c):
        theta, _ = _pair(c, B, Cin, h, w, True, 47)
        del c.leaves[3:]                                   # (phi is not part of this op)
        th, mu, a = _ops().proj_unfold3_stats(theta, 2304.0)
        return th, mu, a * 0.1
    return body


for _fb in (True, False):
    case(f"proj_unfold3_stats-2x33x2x64-fused_bwd{int(_fb)}", dict(_F16, PROJ_BWD_FUSED=_fb))(_k24_unfold(2, 33, 2, 64))


# ---------------------------------------------------------------------------------------------------------------- convolution
CONV_LAYERS = {
    # x shape, Cout, k, stride, pad, reflect, bias   (the table of tests/test_gpu_grad_subsets.py)
    "k3_nhwc": ((2, 128, 4, 32), 128, 3, 1, 1, 0, True),
    "k3_gather_ragged": ((3, 5, 9, 7), 7, 3, 1, 1, 0, True),
    "k4_s2_strided_dgrad": ((1, 16, 18, 22), 40, 4, 2, 1, 0, True),
    "reflect_fold": ((1, 128, 4, 32), 128, 3, 1, 0, 1, True),
    "reflect_fused_no_fold": ((1, 128, 3, 32), 128, 3, 1, 0, 1, True),
    "reflect_5x5_unfused": ((2, 6, 5, 5), 7, 3, 1, 0, 1, True),
    "no_bias": ((3, 5, 9, 7), 7, 3, 1, 1, 0, False),
    # test_conv2d_bf16_nhwc_stream_k_equals_one_tile_per_workgroup's layer (288 output channels: 256 x 256 tiles), batch 8 kept: the
    # tile count has to pass one round of the CUs for the route to be taken
    "stream_k": ((8, 32, 68, 68), 288, 3, 1, 0, 0, True),
}


def _conv(layer):
    def body(c):
        xs, Cout, k, stride, pad, reflect, bias = CONV_LAYERS[layer]
        Cin = xs[1]
        x, w = c.leaf(rnd(*xs, seed=11)), c.leaf(rnd(Cout, Cin, k, k, seed=12) / (Cin * k * k) ** 0.5)
        b = c.leaf(rnd(Cout, seed=13)) if bias else None
        return _ops().conv2d(x, w, b, stride, pad, 1, reflect=reflect)
    return body


for _layer in CONV_LAYERS:
    each(f"conv2d-{_layer}", "conv", dict(CONV_NHWC_STREAMK=True, CONV_NHWC_STREAMK_SPLIT=True) if _layer == "stream_k" else None)(_conv(_layer))

case("conv_nhwc_prep-2x37x9x70-reflect")(lambda c: _ops().conv_nhwc_prep(c.data(rnd(2, 37, 9, 70, seed=50)), 1, True))
case("conv_nhwc_prep-1x64x5x5-zero_pad2")(lambda c: _ops().conv_nhwc_prep(c.data(rnd(1, 64, 5, 5, seed=50)), 2, False))


@case("conv_nhwc_prep_split-2x37x9x70-reflect")
def _prep_split(c):
    ops = _ops()
    x = c.data(rnd(2, 37, 9, 70, seed=51))
    return ops.conv_nhwc_prep_split(x, 1, True, ops.absmax(x))


case("reflect_pad2d-1x2x7x5-pad2")(lambda c: _ops().reflect_pad2d(c.leaf(rnd(1, 2, 7, 5, seed=52)), 2))
case("reflect_pad2d-1x3x4x4-pad3")(lambda c: _ops().reflect_pad2d(c.leaf(rnd(1, 3, 4, 4, seed=52)), 3))
case("upsample_nearest-1x5x7x6x2")(lambda c: _ops().upsample_nearest(c.leaf(rnd(1, 5, 7, 6, seed=53)), 2))


def _spectral(shape, power):
    def body(c):
        R, K = shape[0], shape[1] * shape[2] * shape[3]
        nrm = lambda t: t / t.norm()
        w, u, v = c.leaf(rnd(*shape, seed=54, scale=0.2)), c.data(nrm(rnd(R, seed=55))), c.data(nrm(rnd(K, seed=56)))
        y = _ops().spectral_weight(w, u, v, power)
        return Out([y], [y, u, v])
    return body


for _shape in ((5, 3, 4, 4), (64, 151, 3, 3)):
    for _power in (True, False):
        each(f"spectral_weight-{'x'.join(map(str, _shape))}-power{int(_power)}", "conv")(_spectral(_shape, _power))


# ---------------------------------------------------------------------------------------------------------------- match_kernel 3
def _box3_logits(B, h, w):
    def body(c):
        N = h * w
        cr = c.leaf(rnd(B, N, N, seed=57))
        mu, nu = c.leaf(rnd(B, N, seed=58, scale=0.1)), c.leaf(rnd(B, N, seed=59, scale=0.1))
        a, b = c.leaf(torch.rand(B, N, generator=torch.Generator().manual_seed(60)) * 1.5 + 0.5), c.leaf(torch.rand(B, N, generator=torch.Generator().manual_seed(61)) * 1.5 + 0.5)
        return _ops().box3_logits(cr, mu, nu, a, b, h, w, 2304.0, 100.0)
    return body


each("box3_logits-2x33x31", "prec")(_box3_logits(2, 33, 31))
each("box3_logits-1x1x1", "prec")(_box3_logits(1, 1, 1))


def _box3_fused(fh, transposed=False):
    def body(c):
        ops = _ops()
        B, fw, Cv, kc = 1, 64, 5, 2304.0
        N = fh * fw
        assert ops.box3_fused_ok(B, 256, fh, fw, Cv)
        qh = rnd(B, 256, fh, fw, seed=62) + 0.15
        kh = 0.05 * qh.roll((1, 5), (2, 3)) + rnd(B, 256, fh, fw, seed=63) - 0.1
        q, k = c.leaf(qh), c.leaf(kh)
        with torch.no_grad():
            (mu, a), (nu, b) = ops.unfold3_stats(q, kc), ops.unfold3_stats(k, kc)
        mu, a, nu, b = (c.leaf(t.cpu()) for t in (mu, a, nu, b))
        v = c.leaf(uni(B, Cv, N, seed=64))
        sink = ops.Box3GradSink()
        T = ops.box3_corr_xbox(q, k, sink)
        return ops.box3_softmax_warp(T, mu, a, nu, b, v, fh, fw, kc, 100.0, False, sink)
    return body


case("box3_corr_xbox+box3_softmax_warp-sink-4x64", _F16)(_box3_fused(4))
case("box3_corr_xbox+box3_softmax_warp-sink-8x64-T_aliased", dict(_F16, BOX3_ALIAS_T_BYTES=0))(_box3_fused(8))


# ---------------------------------------------------------------------------------------------------------------- head and glue
HEAD_GRID = (1, 2, 1, 5, 8, 3)      # B, Ci, Cs, h, w, d: the smallest grid of test_gpu_warp_head_modes.SHAPES with a mask channel


def _head(mode, **kw):
    def body(c):
        ops = _ops()
        B, Ci, Cs, h, w, d = HEAD_GRID
        if mode == "patch":
            Ci = Ci * d * d
        o = c.leaf(rnd(B, Ci + Cs, h * w, seed=65))
        assert ops.warp_head_ok(o, Ci, h, w, d, mode)
        return [t for t in ops.warp_head(o, Ci, h, w, d, mode=mode, **kw) if t is not None]
    return body


each("warp_head-nearest", "prec")(_head("nearest"))
each("warp_head-nearest-want_bi", "prec")(_head("nearest", want_bi=True))
each("warp_head-nearest-want_y", "prec")(_head("nearest", want_y=True))
each("warp_head-bilinear", "prec")(_head("bilinear"))
each("warp_head-bilinear-want_y", "prec")(_head("bilinear", want_y=True))
each("warp_head-patch-want_y", "prec")(_head("patch", want_y=True))


def _warp_values(B, Ci, Cs, H, W, d, patch):
    def body(c):
        seg = c.data(onehot(labels(B, Cs, H, W, 66), Cs)) if Cs else None
        return _ops().warp_values(c.data(uni(B, Ci, H, W, seed=67)), seg, d, patch)
    return body


for _patch in (False, True):
    each(f"warp_values-1x3x5x12x20x2-patch{int(_patch)}", "prec")(_warp_values(1, 3, 5, 12, 20, 2, _patch))
    each(f"warp_values-1x3x0x12x20x2-patch{int(_patch)}", "prec")(_warp_values(1, 3, 0, 12, 20, 2, _patch))
each("warp_values-1x2x1x9x6x3-patch1", "prec")(_warp_values(1, 2, 1, 9, 6, 3, True))

case("wta_scale-5x333")(lambda c: _ops().wta_scale(c.leaf(rnd(1, 5, 333, seed=68)), 0.5, 100.0))
case("wta_scale-2x1")(lambda c: _ops().wta_scale(c.leaf(rnd(1, 2, 1, seed=68)), 0.5, 100.0))
each("concat_channels_amax", "prec")(lambda c: _ops().concat_channels_amax(c.data(rnd(2, 3, 2, 6, seed=69)), c.data(rnd(2, 1, 2, 6, seed=70))))


def _split(transpose, **kw):
    def body(c):
        ops = _ops()
        x = c.data(rnd(1, 154, 100, seed=71))
        if kw.pop("amax", False):
            kw["amax"] = ops.absmax(x)
        return ops.split_f16(x, transpose, 16.0, **kw)
    return body


case("split_f16-1x154x100")(_split(False))
case("split_f16-1x154x100-transposed")(_split(True))
case("split_f16-1x154x100-transposed-cpad256-amax")(_split(True, cpad=256, amax=True))
case("split_f16-1x154x100-amax")(_split(False, amax=True))


@case("cocos_split_f16_rows-3x5-pad16")
def _split_rows(c):
    ops = _ops()
    w = c.data(rnd(3, 5, seed=72))
    hi, lo = torch.empty((3, 16), device=DEV, dtype=torch.float16), torch.empty((3, 16), device=DEV, dtype=torch.float16)
    sc = torch.empty(1, device=DEV)
    ops._call("t", "cocos_split_f16_rows", w.data_ptr(), hi.data_ptr(), lo.data_ptr(), 3, 5, 16, 1.0, ops.absmax(w).data_ptr(), sc.data_ptr(), ops._stream())
    return hi, lo, sc


def _chan_mask(N, want):
    def body(c):
        ops = _ops()
        x = c.data(rnd(1, 40, N, seed=73))
        return ops.split_f16_chan_mask(x, ops.absmax(x), want)
    return body


case("split_f16_chan_mask-1x40x100-mask")(_chan_mask(100, True))
case("split_f16_chan_mask-1x40x100-no_mask")(_chan_mask(100, False))
case("split_f16_chan_mask-1x40x99-two_launches")(_chan_mask(99, True))
case("f16_plane_block_mask-1x40x99")(lambda c: _ops().f16_plane_block_mask(c.data(rnd(1, 40, 99, seed=74).half())).view(torch.int32))
for _n in (1, 3, 4097):
    case(f"absmax-n{_n}")(lambda c, n=_n: _ops().absmax(c.data(rnd(n, seed=75))))
case("absmax_many-5")(lambda c: _ops().absmax_many([c.data(rnd(n, seed=76 + n)) for n in (1, 3, 4097, 70000, 5)]))


@case("prefetch_amax+cocos_absmax")
def _absmax_plain(c):
    ops = _ops()
    x = c.data(rnd(4097, seed=77))
    ops.prefetch_amax([x, c.data(rnd(3, seed=78))])
    cell = torch.empty(1, device=DEV)
    ops._call("t", "cocos_absmax", x.data_ptr(), x.numel(), cell.data_ptr(), ops._stream())
    return cell, ops._recall_amax(x, consume=False)


case("sum_leading-3x5x7")(lambda c: _ops().sum_leading(c.data(rnd(3, 5, 7, seed=79))))
case("sum_leading-1x1")(lambda c: _ops().sum_leading(c.data(rnd(1, 1, seed=79))))
case("channel_sum-3x7x9x7")(lambda c: _ops().channel_sum(c.data(rnd(3, 7, 9, 7, seed=80))))
case("channel_sum-2x3x130x130-sliced")(lambda c: _ops().channel_sum(c.data(rnd(2, 3, 130, 130, seed=80))))
case("mfma_probe")(lambda c: _ops().mfma_probe())


# ---------------------------------------------------------------------------------------------------------------- loss side
def _nrm(t):
    return t / (t.norm(dim=1, keepdim=True) + 2.2e-16)


case("contextual_cx-1x40x131x67")(lambda c: _ops().contextual_cx(c.leaf(_nrm(rnd(1, 40, 131, seed=81))), c.leaf(_nrm(rnd(1, 40, 67, seed=82))), 0.1, 1e-3))
case("contextual_cx-2x64x513x129-h0.5")(lambda c: _ops().contextual_cx(c.leaf(_nrm(rnd(2, 64, 513, seed=81))), c.leaf(_nrm(rnd(2, 64, 129, seed=82))), 0.5, 1e-3))
case("contextual_rows-2x33x131")(lambda c: _ops().contextual_rows(c.leaf(uni(2, 33, 131, seed=83)), 0.1, 1e-3))
for _nc in (False, True):
    each(f"vgg_preprocess-2x3x7x9-normal_correct{int(_nc)}", "conv")(lambda c, nc=_nc: _ops().vgg_preprocess(c.leaf(uni(2, 3, 7, 9, seed=84)), nc))
each("relu-315", "conv")(lambda c: _ops().relu(c.leaf(rnd(1, 5, 7, 9, seed=85))))
for _mode in ("max", "avg"):
    for _keep in (False, True):
        each(f"relu_pool2-{_mode}-keep_r{int(_keep)}-2x3x7x9", "conv")(lambda c, m=_mode, k=_keep: _ops().relu_pool2(c.leaf(rnd(2, 3, 7, 9, seed=86)), m, k))


@case("pair_loss-5_segments-odd_sizes")
def _pair_loss(c):
    shapes = [(3, 5, 7, 3), (3, 2, 9, 5), (3, 1, 1, 1), (3, 4, 33, 31), (3, 7)]
    coef = [(1.0 / 32, 0.0), (1.0 / 16, 0.0), (1.0 / 8, 1.0), (1.0 / 4, 0.0), (0.0, 1.0)]
    segs = []
    for i, s in enumerate(shapes):
        a = c.leaf(rnd(*s, seed=87 + i))
        b = None if i == 4 else c.data(rnd(*s, seed=97 + i))
        w = c.data(torch.tensor([1.0, 0.0, 0.5])) if i == 1 else None
        segs.append((a, b, w, *coef[i]))
    return _ops().pair_loss(segs)


def _gan(mode, label):
    def body(c):
        xs = [c.leaf(rnd(*s, seed=107 + i)) for i, s in enumerate([(2, 1, 7, 5), (2, 1, 3, 3), (1, 1, 1, 1), (2, 1, 35, 33), (3,)])]
        return _ops().gan_loss(xs, mode, label)
    return body


for _gmode, _label in (("hinge_d_real", 0.0), ("hinge_d_fake", 0.0), ("neg_mean", 0.0), ("mean", 0.0), ("ls", 1.0), ("bce", 1.0)):
    case(f"gan_loss-{_gmode}")(_gan(_gmode, _label))


def _mask_nll(nc, B, H, W, Hr, Wr):
    def body(c):
        p = torch.softmax(rnd(B, nc, H // 4, W // 4, seed=112, scale=3.0), dim=1)
        return _ops().mask_nll_loss(c.leaf(p), c.data(labels(B, nc, H, W, 113)), c.data(labels(B, nc // 2 + 1, Hr, Wr, 114)))
    return body


case("mask_nll_loss-nc151-2x70x66")(_mask_nll(151, 2, 70, 66, 70, 66))
case("mask_nll_loss-nc19-1x64x48-ref32x40")(_mask_nll(19, 1, 64, 48, 32, 40))
case("mask_nll_loss-nc2-3x9x5")(_mask_nll(2, 3, 9, 5, 9, 5))


# ---------------------------------------------------------------------------------------------------------------- step and inference
STEP_SIZES = (1, 3, 4097, 70000)


@case("adam_multi_step-1-3-4097-70000")
def _adam(c):
    ps = [c.data(rnd(n, seed=115 + i)) for i, n in enumerate(STEP_SIZES)]
    gs = [c.data(rnd(n, seed=120 + i)) for i, n in enumerate(STEP_SIZES)]
    ms = [c.data(rnd(n, seed=125 + i, scale=0.1)) for i, n in enumerate(STEP_SIZES)]
    vs = [c.data(rnd(n, seed=130 + i).square()) for i, n in enumerate(STEP_SIZES)]
    rows = [(1e-3, 0.3, 0.0, 1.0, 0.9, 0.1, 1e-3, 0.0), (2e-3, 0.5, 0.5, 0.5, 0.999, 0.001, 1e-8, 1e-4)]
    _ops().adam_multi_step(ps, gs, ms, vs, rows, [0, 1, 0, 1])
    return ps + ms + vs + gs


@case("ema_multi_update-1-3-4097-70000")
def _ema(c):
    ss = [c.data(rnd(n, seed=135 + i)) for i, n in enumerate(STEP_SIZES)]
    ps = [c.data(rnd(n, seed=140 + i)) for i, n in enumerate(STEP_SIZES)]
    _ops().ema_multi_update(ss, ps, 0.999)
    return ss + ps


@case("weight_absmax_multi+weight_planes_multi-more_than_one_table")
def _wprep(c):
    ops = _ops()
    n = ops.weight_prepare_constants()["TABLE_ENTRIES"] + 1
    ws = [c.data(rnd(5, 3, 3, 3, seed=145 + i) * 10.0 ** (i % 7 - 3)) for i in range(n - 3)]
    ws += [c.data(rnd(256, 71, 1, 1, seed=300)), c.data(rnd(7, 5, 4, 4, seed=301)), c.data(rnd(4099, seed=302)).view(4099, 1)]
    cells, launches = ops.weight_absmax_multi(ws)
    assert launches == 2 * -(-n // (n - 1))
    layouts = ("conv_fwd", "conv_dgrad", "conv_fwd_bf16", "conv_dgrad_bf16")
    reqs = [(w, None if layouts[i % 4].endswith("bf16") else cells[i], layouts[i % 4], 0) for i, w in enumerate(ws[:n - 2])]
    proj = ws[n - 3]
    reqs += [(proj, cells[n - 3], "frag", 0), (proj, cells[n - 3], "rows", 80), (ws[n - 2], cells[n - 2], "rows", 96)]
    assert len(reqs) > n - 1
    got, launches = ops.weight_planes_multi(reqs)
    assert launches == -(-len(reqs) // (n - 1))
    return cells, [t for tup in got for t in tup if t is not None]


# ---------------------------------------------------------------------------------------------------------------- whole path
def _hot_path(mk, fh, fw, lazy, Cin=71, img=None, **flags):
    def body(c):
        from cocosnet_amd.hot_path import HotPathConfig, correspondence_hot_path
        B, down, nc = 2, 4, 7
        H, W = img or (fh * down, fw * down)
        if lazy:
            theta, phi = _pair(c, B, Cin, fh, fw, True, 150)
        else:
            th = rnd(B, 256, fh, fw, seed=156)
            theta, phi = c.leaf(th), c.leaf(0.05 * th.roll(3, 3) + rnd(B, 256, fh, fw, seed=157))
        ref_img = c.data(uni(B, 3, H, W, seed=158))
        seg = c.data(onehot(labels(B, nc, H, W, 159), nc))
        cfg = HotPathConfig(**dict(dict(match_kernel=mk, PONO_C=True, down=down, warp_mask_losstype="direct", isTrain=True), **flags))
        out = correspondence_hot_path(theta, phi, ref_img, ref_img, seg, seg, cfg)
        return [v for v in out.values() if torch.is_tensor(v)]
    return body


for _mk in (1, 3):
    each(f"correspondence_hot_path-mk{_mk}-2x256x8x8-img32", "prec")(_hot_path(_mk, 8, 8, False))
each("correspondence_hot_path-mk1-lazy-8x16", "prec")(_hot_path(1, 8, 16, True))
each("correspondence_hot_path-mk3-lazy-4x64", "prec")(_hot_path(3, 4, 64, True))
case("correspondence_hot_path-mk3-lazy-4x64-unfused_bwd", dict(_F16, PROJ_BWD_FUSED=False, PROJ_DW_PAIR=False))(_hot_path(3, 4, 64, True))
case("correspondence_hot_path-mk1-lazy-8x16-unfused_bwd", dict(_F16, PROJ_BWD_FUSED=False, PROJ_DW_PAIR=False))(_hot_path(1, 8, 16, True))


# ---------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name", list(CASES))
def test_red_zones(name, monkeypatch):
    import importlib
    attrs, body = CASES[name]
    for mod, table in attrs.items():
        m = importlib.import_module("cocosnet_amd." + mod)
        for k, v in table.items():
            assert hasattr(m, k), (mod, k)
            monkeypatch.setattr(m, k, v)
    run_guarded(name, body)


def entry_points_invoked_through_lib_call():
    """every `cocos_*` string literal of cocosnet_amd/*.py that names an exported symbol: the names handed to `_lib.call` (the query
    functions are reached as attributes of the loaded library, not through string literals; _lib.py itself is the table of symbols)"""
    from cocosnet_amd import _lib
    exported, found = set(_lib.EXPORTED_SYMBOLS), set()
    for path in glob.glob(os.path.join(REPO, "cocosnet_amd", "*.py")):
        if os.path.basename(path) == "_lib.py":
            continue
        with open(path) as fh:
            tree = ast.parse(fh.read())
        found |= {n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str) and n.value in exported}
    return found


def test_every_entry_point_was_reached():
    from cocosnet_amd import _lib
    assert set(COVERAGE) == set(CASES), f"cases that did not run: {sorted(set(CASES) - set(COVERAGE))}"
    wanted = entry_points_invoked_through_lib_call()
    assert len(wanted) > 100 and set(EXCLUDED) <= set(_lib.EXPORTED_SYMBOLS)
    reached = set().union(*(set(e) for e, *_ in COVERAGE.values()))
    lines = ["# tests/test_gpu_red_zones.py: per case, the entry points reached, guarded allocations and pass-throughs inside cocosnet_amd/",
             f"# {len(COVERAGE)} cases, {len(reached & wanted)} of {len(wanted)} entry points, "
             f"{sum(v[1] for v in COVERAGE.values())} guarded allocations, {sum(v[3] for v in COVERAGE.values())} calls, "
             f"{sum(v[2] for v in COVERAGE.values())} pass-throughs"]
    for name in CASES:
        entries, n_alloc, n_pass, n_calls = COVERAGE[name]
        lines.append(f"{name}: guarded {n_alloc} passthrough {n_pass} calls {n_calls}: {' '.join(entries)}")
    lines.append("# exclusions (entry points that write no device memory)")
    lines += [f"{k}: {v}" for k, v in sorted(EXCLUDED.items())] or ["(none)"]
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "red_zone_coverage.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    missing = sorted(wanted - reached - set(EXCLUDED))
    assert not missing, f"entry points no case reached: {missing}"
