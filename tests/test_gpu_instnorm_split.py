"""K34 (`ops.instnorm_prelu_split`, csrc/instnorm_split.hip): InstanceNorm (+ residual) + PReLU with a plane spread over several
workgroups, against `F.prelu(F.instance_norm(x, eps=1e-5) (+ residual), weight)` in torch fp64.  The bounds are K13's
(tests/test_gpu_grad_subsets.py::test_instnorm_prelu): y rel 1e-5, d x rel 5e-5 (floor 0.05), d residual rel 1e-5, d weight rel 5e-5
(floor 1.0), `rel` = max|got - ref| / (max|ref| + floor).  Shapes: one slice (partly and exactly full), a second slice of 4 elements, an
odd plane (unaligned plane bases: the 4-byte route), 4 slices (the adaptors' own plane) and 16."""
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLICE = 16384
SHAPES = [(1, 2, 10, 10), (2, 3, 128, 128), (1, 3, 2, 8194), (1, 3, 129, 129), (2, 3, 256, 256), (1, 2, 512, 512)]
BOUNDS = dict(out=(1e-5, 1e-30), x=(5e-5, 0.05), residual=(1e-5, 1e-30), weight=(5e-5, 1.0))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def _rel(got, ref, what):
    tol, floor = BOUNDS[what]
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + floor)) / tol


_CASES = {}


def _case(shape, with_res, a):
    """Seeded fp32 inputs on the device and the fp64 arbiter's output and gradients (all three inputs), computed once per case."""
    key = (shape, with_res, a)
    if key not in _CASES:
        g = torch.Generator().manual_seed(sum(shape) + 7 * with_res)
        x = torch.randn(*shape, generator=g) * 3 + 0.5
        res = torch.randn(*shape, generator=g) * 3 + 0.5 if with_res else None
        w = torch.tensor([a])
        dy = torch.randn(*shape, generator=g)
        xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
        rd = res.double().requires_grad_(True) if with_res else None
        z = F.instance_norm(xd, eps=1e-5)
        y = F.prelu(z + rd if with_res else z, wd)
        y.backward(dy.double())
        ref = dict(out=y.detach(), x=xd.grad, weight=wd.grad, residual=rd.grad if with_res else None)
        dev = dict(x=x.to(DEV), residual=res.to(DEV) if with_res else None, weight=w.to(DEV), dy=dy.to(DEV))
        _CASES[key] = (dev, ref)
    return _CASES[key]


def _leaves(dev, S):
    return {n: (None if dev[n] is None else dev[n].clone().requires_grad_(n in S)) for n in ("x", "residual", "weight")}


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [0.2, 0.25])                 # the LeakyReLU use (adaptors, PatchGAN) and nn.PReLU()'s initial weight
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("flavour", ["f16x3", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_every_gradient_against_fp64(shape, flavour, with_res, a, monkeypatch):
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", flavour)
    dev, ref = _case(shape, with_res, a)
    names = [n for n in ("x", "residual", "weight") if dev[n] is not None]
    t = _leaves(dev, set(names))
    y = ops.instnorm_prelu_split(t["x"], t["residual"], t["weight"])
    assert y.shape == ref["out"].shape and y.dtype == torch.float32
    if flavour == "f16x3":                                                            # max|y| leaves with y, exactly
        cell = ops._recall_amax(y, consume=False)
        assert cell is not None and float(cell) == float(y.detach().abs().max())
    else:
        assert ops._recall_amax(y, consume=False) is None
    y.backward(dev["dy"])
    ratios = {"out": _rel(y.detach(), ref["out"], "out")}
    ratios.update({n: _rel(t[n].grad, ref[n], n) for n in names})
    print("K34_ERR_OVER_BOUND", shape, flavour, with_res, a, {k: round(v, 4) for k, v in ratios.items()})
    for n in names:
        assert t[n].grad.shape == t[n].shape and bool(torch.isfinite(t[n].grad).all()), n
    assert all(v < 1.0 for v in ratios.values()), ratios


# ---- 2. gradient subsets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["f16x3", "fp32"])
@pytest.mark.parametrize("shape", [(1, 3, 2, 8194), (2, 3, 256, 256)], ids=lambda s: "x".join(map(str, s)))
def test_every_subset_of_inputs_that_need_gradients(shape, flavour, monkeypatch):
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", flavour)
    dev, ref = _case(shape, True, 0.25)
    names = ("x", "residual", "weight")
    for r in range(1, 4):
        for S in map(set, itertools.combinations(names, r)):
            t = _leaves(dev, S)
            y = ops.instnorm_prelu_split(t["x"], t["residual"], t["weight"])
            assert _rel(y.detach(), ref["out"], "out") < 1.0, S
            y.backward(dev["dy"], retain_graph=True)
            first = {n: t[n].grad.clone() for n in S}
            for n in names:
                if n in S:
                    assert _rel(t[n].grad, ref[n], n) < 1.0, (S, n, _rel(t[n].grad, ref[n], n))
                    t[n].grad = None
                else:
                    assert t[n].grad is None, (S, n)
            y.backward(dev["dy"])                                                      # the same backward again: the same bits
            for n in S:
                assert torch.equal(t[n].grad, first[n]), (S, n)


# ---- 3. maxima ------------------------------------------------------------------------------------------------------------------------
def _raw(dev, cell_y=None, cell_dx=None):
    """Forward + backward through the C entry points; returns (y, dx, dres, da)."""
    from cocosnet_amd import _lib
    x, res, w, dy = dev["x"], dev["residual"], dev["weight"], dev["dy"]
    planes, N = x.shape[0] * x.shape[1], x.shape[2] * x.shape[3]
    ptr = lambda t: 0 if t is None else t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    floats = _lib.load().cocos_instnorm_prelu_split_workspace_floats(planes, N)
    assert floats >= 7 * planes * -(-N // SLICE)
    ws = torch.full(((floats + 1) // 2,), float("nan"), device=DEV, dtype=torch.float64)       # (never read before written)
    y, dx, dr = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    stats, da = torch.empty(planes, 2, device=DEV), torch.empty(1, device=DEV)
    _lib.call("cocos_instnorm_prelu_split_fwd", x.data_ptr(), ptr(res), w.data_ptr(), y.data_ptr(), stats.data_ptr(), ws.data_ptr(), ptr(cell_y),
              planes, N, 1e-5, s)
    ws.fill_(float("nan"))
    _lib.call("cocos_instnorm_prelu_split_bwd", x.data_ptr(), ptr(res), w.data_ptr(), dy.data_ptr(), stats.data_ptr(), dx.data_ptr(), dr.data_ptr(),
              da.data_ptr(), ws.data_ptr(), ptr(cell_dx), planes, N, 1e-5, s)
    torch.cuda.synchronize()
    return y, dx, dr, da, stats


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("shape", [(1, 3, 2, 8194), (1, 3, 129, 129), (2, 3, 256, 256)], ids=lambda s: "x".join(map(str, s)))
def test_maxima_leave_with_the_outputs(shape, with_res):
    dev, ref = _case(shape, with_res, 0.2)
    y0, dx0, dr0, da0, st0 = _raw(dev)
    cy, cdx = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    y1, dx1, dr1, da1, st1 = _raw(dev, cy, cdx)
    assert float(cy) == float(y1.abs().max()) and float(cdx) == float(dx1.abs().max())
    for u, v in ((y0, y1), (dx0, dx1), (dr0, dr1), (da0, da1), (st0, st1)):
        assert torch.equal(u, v)
    big_y, big_dx = torch.full((1,), 1e9, device=DEV), torch.full((1,), 1e9, device=DEV)
    y2, dx2, _, _, _ = _raw(dev, big_y, big_dx)
    assert float(big_y) == 1e9 and float(big_dx) == 1e9 and torch.equal(y2, y0) and torch.equal(dx2, dx0)
    # the statistics the backward takes are the plane's own
    xd = dev["x"].double().flatten(2)
    assert float((st0[:, 0].double() - xd.mean(2).flatten()).abs().max()) < 1e-5
    rstd = 1.0 / torch.sqrt(xd.var(2, unbiased=False) + 1e-5).flatten()
    assert float(((st0[:, 1].double() - rstd) / rstd).abs().max()) < 1e-5
    assert _rel(y0, ref["out"], "out") < 1.0 and _rel(dx0, ref["x"], "x") < 1.0 and _rel(da0, ref["weight"], "weight") < 1.0


# ---- 4. statistics under an offset ----------------------------------------------------------------------------------------------------
def test_statistics_under_an_offset_are_no_worse_than_the_register_kernel():
    """x = 20 + randn: a sum of squares about zero would lose the variance (400 against 1).  The yardstick is K13's register kernel at
    128 x 128 (its own mean-then-centred-squares); the split kernel at 256 x 256 differs from it in the order of the sums only and must
    stay within twice its error against fp64, on y and on d x."""
    from cocosnet_amd import ops
    w = torch.full((1,), 0.2, device=DEV)

    def errors(fn, side):
        g = torch.Generator().manual_seed(side)
        x, dy = 20 + torch.randn(1, 2, side, side, generator=g), torch.randn(1, 2, side, side, generator=g)
        xd = x.double().requires_grad_(True)
        yd = F.prelu(F.instance_norm(xd, eps=1e-5), w.double().cpu())
        yd.backward(dy.double())
        xg = x.to(DEV).requires_grad_(True)
        y = fn(xg, None, w)
        y.backward(dy.to(DEV))
        e = lambda got, ref: float((got.double().cpu() - ref).abs().max() / ref.abs().max())
        return e(y.detach(), yd.detach()), e(xg.grad, xd.grad)
    yard = errors(ops.instnorm_prelu, 128)
    split = errors(ops.instnorm_prelu_split, 256)
    print("K34_OFFSET_STATS rel err vs fp64 (y, dx): register kernel 128x128", yard, "split kernel 256x256", split)
    assert split[0] <= 2 * yard[0] and split[1] <= 2 * yard[1], (split, yard)


# ---- 5. live buffers ------------------------------------------------------------------------------------------------------------------
def test_every_pointer_argument_is_a_live_allocation(monkeypatch):
    from test_gpu_live_buffers import _Guard
    from cocosnet_amd import ops
    dev, _ = _case((2, 3, 256, 256), True, 0.25)
    t = _leaves(dev, {"x", "residual", "weight"})
    guard = _Guard(monkeypatch)
    y = ops.instnorm_prelu_split(t["x"], t["residual"], t["weight"])
    y.backward(dev["dy"])
    guard.check(2, 6 + 10)                 # fwd: x, res, w, y, stats, workspace; bwd: ten pointers (+ a max|.| cell each under f16x3)


# ---- 6. routing -----------------------------------------------------------------------------------------------------------------------
class _Count:
    def __init__(self, monkeypatch):
        from cocosnet_amd import _lib
        self.names = []
        real = _lib.call

        def counted(name, *args):
            self.names.append(name)
            return real(name, *args)
        monkeypatch.setattr(_lib, "call", counted)

    def split(self, which=""):
        return sum(1 for n in self.names if n.startswith("cocos_instnorm_prelu_split") and n.endswith(which))


def _adaptor_arms(monkeypatch, smooth):
    """AdaptiveFeatureGenerator (ngf 8, spade_ic 3, PONO) on a [1, 3, 256, 256] input with the switch off and on: ((split forward calls,
    split backward calls) per arm, {name: relative max-norm difference of the two arms} for the output and every parameter gradient).
    smooth: every kink of the module taken out in both arms, as tests/test_gpu_conv.py's `smooth_adaptors` does (LeakyReLU slopes at 1,
    SPADE's ReLU the identity; every kernel still runs, K34 with a = 1)."""
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd import ops, producers
    opt = cc.base_options(semantic_nc=3, ngf=8, PONO=True, PONO_C=True)
    opt.spade_ic = 3
    torch.manual_seed(0)
    net = producers.AdaptiveFeatureGenerator(opt).to(DEV).eval()        # eval: the spectral norm's u is not advanced between the arms
    if smooth:
        net.actvn.negative_slope = 1.0
        for m in net.modules():
            if isinstance(m, producers.SPADEResnetBlock):
                m.slope = 1.0
            elif isinstance(m, producers.SPADE):
                m.mlp_shared[2] = torch.nn.Identity()
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.rand(1, 3, 256, 256, device=DEV, generator=g) * 2 - 1
    count = _Count(monkeypatch)
    go = None

    def arm(on):
        nonlocal go
        monkeypatch.setattr(ops, "INSTNORM_SPLIT", on)
        net.zero_grad()
        count.names.clear()
        out = net(x, x)
        if go is None:
            go = torch.randn(out.shape, device=DEV, generator=g)
        out.backward(go)
        got = {"out": out.detach()}
        got.update({"d " + n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
        return (count.split("_fwd"), count.split("_bwd")), got
    c_off, r_off = arm(False)
    c_on, r_on = arm(True)
    assert sorted(r_on) == sorted(r_off) and len(r_on) > 10
    assert all(bool(torch.isfinite(v).all()) for v in r_on.values())
    return c_off, c_on, {k: float((r_on[k] - r_off[k]).abs().max() / (r_off[k].abs().max() + 1e-30)) for k in r_off}


def test_the_adaptor_takes_the_split_kernel_for_layer1_under_the_switch(monkeypatch):
    """layer1 (stride 1) is the one plane above 128 x 128: one split forward and one split backward call with the switch on, none with
    it off.  The tolerances are those of the module tests of tests/test_gpu_conv.py: 1e-3 of the largest entry for what is a continuous
    function of the features — here the output — while the parameter gradients, which sit upstream of InstanceNorm -> LeakyReLU /
    ReLU kinks, are required finite (one element within rounding of zero taking the other branch moves them by 1e-3 .. 6e-2 of their
    range for any two fp32 evaluations: test_module_end_to_end_against_an_fp64_copy_of_itself) and are HELD to 1e-3 with the kinks
    taken out in both arms (test_module_end_to_end_against_fp64_every_gradient_without_the_adaptor_kinks): the test below."""
    c_off, c_on, diff = _adaptor_arms(monkeypatch, smooth=False)
    print("K34_ROUTING adaptor, relative difference of the two arms:", {k: float(f"{v:.3g}") for k, v in diff.items()})
    assert c_off == (0, 0) and c_on == (1, 1), (c_off, c_on)
    assert diff["out"] < 1e-3, diff


def test_the_adaptor_arms_agree_on_every_gradient_without_the_kinks(monkeypatch):
    c_off, c_on, diff = _adaptor_arms(monkeypatch, smooth=True)
    print("K34_ROUTING adaptor without kinks, relative difference of the two arms:", {k: float(f"{v:.3g}") for k, v in diff.items()})
    assert c_off == (0, 0) and c_on == (1, 1), (c_off, c_on)
    bad = {k: v for k, v in diff.items() if not v < 1e-3}
    assert not bad, bad


def test_the_patchgan_block_takes_the_split_kernel_under_the_switch(monkeypatch):
    from cocosnet_amd import ops, producers, translation
    torch.manual_seed(0)
    blk = translation._ConvNormAct(torch.nn.Sequential(producers.Conv2d(3, 4, 3, stride=1, padding=1), torch.nn.InstanceNorm2d(4)),
                                   torch.nn.LeakyReLU(0.2, False)).to(DEV)
    x = torch.randn(1, 3, 256, 256, device=DEV)
    outs = {}
    count = _Count(monkeypatch)
    for on in (False, True):
        monkeypatch.setattr(ops, "INSTNORM_SPLIT", on)
        blk.zero_grad()
        count.names.clear()
        y = blk(x)
        y.square().mean().backward()
        outs[on] = (y.detach(), blk[0][0].weight.grad.clone())
        assert y.shape == (1, 4, 256, 256)
        assert (count.split("_fwd"), count.split("_bwd")) == ((1, 1) if on else (0, 0)), count.names
    for a, r in zip(outs[True], outs[False]):
        assert float((a - r).abs().max() / r.abs().max()) < 1e-3
