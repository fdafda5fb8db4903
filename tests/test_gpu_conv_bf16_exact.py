"""The one-term bf16 convolution flavour (ops.CONV_PRECISION = "bf16") held to a reference ON ITS OWN OPERANDS: fp64 of the
bf16-rounded x, w, dy (tests/conv_bf16_case.py), against which a kernel differs by fp32 accumulation only.  The bound is
accuracy_case's: E_kernel <= factor * max(E_arm, eps), the arm being the framework's fp32 convolution on the CPU on the same rounded
operands, under rel_max and rel_slice; never above 1e-5 rel_max.  The older tests of the flavour allow 1.5e-2 of the range: that is
the rounding of the operands, four decades above what the kernels deliver.

What this catches that 1.5e-2 lets through: a wrong rounding mode in an operand preparation, an operand rounded twice, partials or
stream-K hand-overs kept in 16 bits, db taken from the rounded dy, a stale accumulator at a k-tail, a race that perturbs one partial sum.

Every case runs inside red zones with the live-buffer check, asserts the ENTRY POINTS it reached, in order (the route it is named after:
a case cannot drift to another kernel unnoticed), and prints `CONV_BF16_EXACT <route> <shape> <tensor> <metric> E_kernel E_arm ratio`;
profiles/conv_bf16_exact.txt is one run.  Twins judge the same kernel output against an arbiter built on slightly different operands
(truncated instead of rounded to nearest even; db of the rounded dy; a frozen record's weight rounded before its scaling instead of
after): they must miss at least TEETH times over.  Nothing deliberately wrong is launched."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy_case as ac  # noqa: E402
import conv_bf16_case as cb  # noqa: E402
from guarded_alloc import guarded  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


@pytest.fixture(autouse=True)
def _bf16_flavour(monkeypatch):
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", "bf16")
    monkeypatch.setattr(ops, "CONV_NHWC", True)
    monkeypatch.setattr(ops, "CONV_NHWC_STREAMK", False)


class _Run:
    """launch trace + live-buffer check + red zones around one case.  `trace`: [(entry point, its arguments)] of the convolution
    entry points (cb.CONV_ENTRIES), `split()` cuts it where `mark()` was called (forward | backward)."""

    def __init__(self, monkeypatch):
        import test_gpu_live_buffers as lb
        from cocosnet_amd import _lib
        self.trace, self._mark = [], None
        real = _lib.call

        def recorder(name, *args):
            if name in cb.CONV_ENTRIES:
                self.trace.append((name, args))
            return real(name, *args)

        monkeypatch.setattr(_lib, "call", recorder)
        self.live = lb._Guard(monkeypatch)
        self.g = guarded()

    def __enter__(self):
        self.g.__enter__()
        return self

    def place(self, t):
        return self.g.place(t)

    def mark(self):
        self._mark = len(self.trace)

    def split(self):
        names = [n for n, _ in self.trace]
        return names[:self._mark], names[self._mark:]

    def __exit__(self, et, ev, tb):
        try:
            bad = self.g.check() if et is None else []
        finally:
            self.g.__exit__(et, ev, tb)
        if et is None:
            assert bad == [] and self.g.violations == [], self.g.report()
            self.live.check(1, 1)
        return False


_ARB = {}


def _arb(c):
    """(inputs, reference, arm) on the CPU: once per case, shared, never written"""
    if c.name not in _ARB:
        _ARB[c.name] = cb.arbiter(c)
    return _ARB[c.name]


def _run(c, monkeypatch, inputs, need=("x", "w", "b"), prepared=None, repeat=1):
    """ops.conv2d forward and backward on guarded copies of `inputs` -> ([{"y", "dx", "dw", "db"} per repeat], the _Run)"""
    from cocosnet_amd import ops
    x, w, b, dy = inputs
    res = []
    with _Run(monkeypatch) as r:
        for _ in range(repeat):
            xd = r.place(x.to(DEV).requires_grad_("x" in need))
            wd = r.place(w.to(DEV).requires_grad_("w" in need))
            bd = None if b is None else r.place(b.to(DEV).requires_grad_("b" in need))
            gd = r.place(dy.to(DEV))
            y = ops.conv2d(xd, wd, bd, c.stride, c.pad, c.dil, reflect=c.reflect, prepared=prepared)
            if r._mark is None:
                r.mark()
            y.backward(gd)
            res.append({"y": y.detach().cpu(), "dx": None if xd.grad is None else xd.grad.cpu(),
                        "dw": None if wd.grad is None else wd.grad.cpu(), "db": None if bd is None or bd.grad is None else bd.grad.cpu()})
    return res, r


def _route_label(rt, nhwc=True):
    return f"fwd:{rt['fwd']},dx:{rt['dx']}{'+fold' if rt['fold'] else ''},dw:{rt['dw']}" + ("" if nhwc else ",CONV_NHWC=0")


def _check_trace(c, r, nhwc=True, need=("x", "w", "b")):
    fwd, bwd = cb.expected_trace(c, nhwc, need)
    got_f, got_b = r.split()
    assert got_f == fwd and got_b == bwd, f"{c.name}: reached {got_f} | {got_b}, the case is there for {fwd} | {bwd}"


def test_dispatch_limits_are_the_library_s():
    """conv_bf16_case restates cocos_conv2d_nhwc_bf16_supported and the slice rule of the K16b weight gradient: compared here"""
    from cocosnet_amd import _lib
    lib = _lib.load()
    for cin in (3, 31, 32, 33, 127, 128, 130):
        for cout in (7, 96, 127, 128, 129, 300):
            for k, s in ((1, 1), (3, 1), (3, 2), (4, 2), (5, 1), (7, 1), (8, 1), (3, 5)):
                assert bool(lib.cocos_conv2d_nhwc_bf16_supported(cin, cout, k, k, s)) == cb.nhwc_supported(cin, cout, k, s), (cin, cout, k, s)
    # "cin130-cout300-ow64": 12 k-steps of 32 positions -> ONE slice per tile; "one-kstep": 32 k-steps -> 4; "s2-ow32": 16 -> 2
    assert lib.cocos_conv2d_nhwc_wgrad_bf16_slices(1, 6, 64, 160, 300, 3, 3) == 1
    assert lib.cocos_conv2d_nhwc_wgrad_bf16_slices(2, 16, 32, 32, 128, 1, 1) == 4
    assert lib.cocos_conv2d_nhwc_wgrad_bf16_slices(2, 8, 32, 64, 160, 3, 3) == 2


@pytest.mark.parametrize("c", cb.GATHER + cb.NHWC + cb.MIXED + cb.REFLECT, ids=cb.case_id)
def test_layer_in_class(c, monkeypatch):
    """y, dx, dw, db of every layer of the list, on the default routes"""
    inputs, ref, arm = _arb(c)
    (got,), r = _run(c, monkeypatch, inputs)
    _check_trace(c, r)
    rt = cb.routes(c)
    cb.judge(cb.Judge(_route_label(rt), cb.shape_str(c) + ":" + c.regime), got, arm, ref, factor=cb.factors(rt)).assert_in_class()


#: CONV_NHWC = False: the gather layers again (nothing may change for them) and K16b's layers on conv_f16x3.hip's one-term kernels
GATHER_FORCED = cb.GATHER[:6] + [cb.BY_NAME[n] for n in ("cin33-cout129-ow33", "cin130-cout300-ow64", "s2-ow32", "fwd-gather-dx-nhwc")]


@pytest.mark.parametrize("c", GATHER_FORCED, ids=cb.case_id)
def test_layer_in_class_on_the_gather_kernels(c, monkeypatch):
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "CONV_NHWC", False)
    inputs, ref, arm = _arb(c)
    (got,), r = _run(c, monkeypatch, inputs)
    _check_trace(c, r, nhwc=False)
    rt = cb.routes(c, nhwc=False)
    assert "K16b" not in rt.values()
    cb.judge(cb.Judge(_route_label(rt, False), cb.shape_str(c) + ":" + c.regime), got, arm, ref, factor=cb.factors(rt)).assert_in_class()


@pytest.mark.parametrize("need", [("x",), ("w",)], ids=["x-only", "w-only-xp-saved"])
def test_gradient_subsets_in_class(need, monkeypatch):
    """x only (the G step against a fixed network: no xp kept, no weight gradient) and the weight only with the forward's NHWC operand
    saved for it (the D step on a detached image) — two subsets; the lattice is tests/test_gpu_grad_subsets.py's"""
    c = cb.BY_NAME["square128-no-bias"]
    inputs, ref, arm = _arb(c)
    (got,), r = _run(c, monkeypatch, inputs, need=need)
    _check_trace(c, r, need=need)
    assert (got["dx"] is None) == ("x" not in need) and (got["dw"] is None) == ("w" not in need) and got["db"] is None
    rt = cb.routes(c)
    cb.judge(cb.Judge(_route_label(rt) + ":need=" + "+".join(need), cb.shape_str(c)), got, arm, ref, factor=cb.factors(rt)).assert_in_class()


def test_stream_k_on_and_off(monkeypatch):
    """the smallest layer the host-side rule runs as stream-K (cb.streamk_rule quotes it: on 256 compute units 258 tiles of 2 k-steps,
    3 k-steps per workgroup, so tiles are cut and meet through the parked fp32 partials), with the workspace and without: both held to
    the arbiter; with it, twice on the same workspace, and every flag back to zero"""
    from cocosnet_amd import ops
    c = cb.STREAMK
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    taken, tiles, nsteps, units = cb.streamk_rule(c, cus)
    assert taken and nsteps > 1 and units % nsteps != 0, (cus, tiles, nsteps, units)
    inputs, ref, arm = _arb(c)
    rt = cb.routes(c)
    out = {}
    for on in (False, True):
        monkeypatch.setattr(ops, "CONV_NHWC_STREAMK", on)
        ws = ops._conv_nhwc_workspace(DEV)                   # (allocated outside the red zones: it outlives the case)
        assert (ws is not None) == on
        res, r = _run(c, monkeypatch, inputs, repeat=2 if on else 1)
        fwd = [a for n, a in r.trace if n == "cocos_conv2d_nhwc_bf16"]
        assert len(fwd) == len(res) and all((a[5] == ws.data_ptr()) if on else not a[5] for a in fwd)
        for i, got in enumerate(res):
            j = cb.Judge(f"{_route_label(rt)}:stream-K={'on' if on else 'off'}:run{i}", f"{cb.shape_str(c)}:tiles={tiles}:cus={cus}")
            cb.judge(j, got, arm, ref, factor=cb.factors(rt)).assert_in_class()
        if on:
            assert int(ws[:1024].abs().sum()) == 0, "stream-K flags left set"
            assert torch.equal(res[0]["y"], res[1]["y"])
        out[on] = res[0]["y"]
    # cut tiles add their two k-steps as partial + partial instead of in one accumulator: the stream-K kernel really ran
    assert not torch.equal(out[True], out[False]), "stream-K on and off agree bit for bit: the stream-K kernel did not run"


@pytest.mark.parametrize("name", cb.TWIN_CASES)
def test_twins_miss_on_the_hardware(name, monkeypatch):
    """K16b forward / input gradient / weight gradient ("cin130-cout300-ow64", "square128") and the gather kernels ("ragged", "cout96"):
    the kernel's own output is in class against the arbiter and out of class, TEETH times, against each twin's"""
    c = cb.BY_NAME[name]
    inputs, ref, arm = _arb(c)
    (got,), r = _run(c, monkeypatch, inputs)
    _check_trace(c, r)
    rt = cb.routes(c)
    cb.judge(cb.Judge(_route_label(rt) + ":twin:intact", cb.shape_str(c)), got, arm, ref, factor=cb.factors(rt)).assert_in_class()
    for twin, (kw, damaged) in sorted(cb.TWINS.items()):
        _, tref, tarm = cb.arbiter(c, inputs, **kw)
        j = cb.judge(cb.Judge(f"{_route_label(rt)}:twin:{twin}", cb.shape_str(c)), got, tarm, tref, factor=cb.factors(rt))
        j.assert_out_of_class(damaged)
        for t in set(cb.TENSORS) - set(damaged):
            assert j.over(t) <= 1.0, (twin, t, j.over(t))


def test_frozen_record_is_the_unprepared_call(monkeypatch):
    """prepared= with the conv_fwd_bf16 and conv_dgrad_bf16 layouts of a cocosnet_amd.inference record whose effective weight is
    W / sigma: bit for bit the unprepared call on that weight, in class, and out of class against the twin that rounds W BEFORE the
    scaling"""
    from cocosnet_amd import inference, ops, producers
    c = cb.BY_NAME["square128"]
    x, w, b, dy = cb.make_inputs(c)
    wf = cb.frozen_weight(w)
    conv = producers.Conv2d(c.x[1], c.Cout, c.k, padding=c.pad).to(DEV).eval()
    with torch.no_grad():
        conv.weight.copy_(w.to(DEV))
    conv.weight.requires_grad_(False)

    def prepare(rec):
        rec.weight = wf.to(DEV)
        rec.amax = ops.absmax(rec.weight)
    rec = inference.PreparedWeight(conv, keep_dgrad=True, prepare=prepare).ensure()
    inputs, ref, arm = cb.arbiter(c, (x, wf, b, dy))
    (got,), r = _run(c, monkeypatch, inputs, need=("x",), prepared=rec)
    _check_trace(c, r, need=("x",))
    assert set(k[0] for k in rec._layouts) == {"conv_fwd_bf16", "conv_dgrad_bf16"}, sorted(rec._layouts)
    (plain,), _ = _run(c, monkeypatch, inputs, need=("x",))
    assert torch.equal(got["y"], plain["y"]) and torch.equal(got["dx"], plain["dx"])
    rt = cb.routes(c)
    cb.judge(cb.Judge(_route_label(rt) + ":frozen-record", cb.shape_str(c)), got, arm, ref, factor=cb.factors(rt)).assert_in_class()
    tref, tarm = cb.arbiter_frozen_twin(c, (x, w, b, dy))
    j = cb.judge(cb.Judge(_route_label(rt) + ":twin:scaled-after-rounding", cb.shape_str(c)), got, tarm, tref, factor=cb.factors(rt))
    j.assert_out_of_class(("y", "dx"))
