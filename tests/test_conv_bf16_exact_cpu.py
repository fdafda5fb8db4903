"""The exact-operand arbiter of the bf16 convolution flavour (tests/conv_bf16_case.py), checked on the CPU before it is trusted on
the hardware:
    the arbiter against an independent formulation (unfold + fp64 matmul, the mirror by index arithmetic) for y, dx, dw, db;
    the fp32 arm is in class by construction (E_arm is printed: of the order of 1e-7);
    each twin, judged with the ARM in place of the kernel, misses the bound at least TEETH times: the bound discriminates;
    rel_slice leaves out at most EXCLUDED_MAX of the slices of every reference in the case list."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy_case as ac  # noqa: E402
import conv_bf16_case as cb  # noqa: E402

#: the largest layer of the list costs a second in fp64; it is the GPU file's (its properties are those of every 1x1 layer)
CPU_CASES = [c for c in cb.CASES if c is not cb.STREAMK]


def _mirror_index(n, r):
    return torch.tensor([abs(i) if i < n else 2 * (n - 1) - i for i in range(-r, n + r)])


def _unfold_formulation(x, w, b, dy, stride, pad, dil, reflect):
    """y, dx, dw, db of conv(mirror(rn x), rn w) + b in fp64 without the framework's convolution: columns by F.unfold, three matmuls,
    F.fold as the transpose of unfold, the mirror and its transpose by index_select / index_add"""
    xr, wr, gr = cb.rn_bf16(x), cb.rn_bf16(w), cb.rn_bf16(dy)
    B, Cin, H, W = xr.shape
    Cout, _, KH, KW = wr.shape
    ih, iw = _mirror_index(H, reflect), _mirror_index(W, reflect)
    xm = xr.index_select(2, ih).index_select(3, iw)
    cols = F.unfold(xm, (KH, KW), dilation=dil, padding=pad, stride=stride)            # [B, K, L]
    w2 = wr.reshape(Cout, -1)
    OH, OW = dy.shape[2:]
    y = torch.matmul(w2, cols).reshape(B, Cout, OH, OW)
    if b is not None:
        y = y + b.double().view(1, -1, 1, 1)
    g2 = gr.reshape(B, Cout, OH * OW)
    dw = torch.einsum("bol,bkl->ok", g2, cols).reshape(wr.shape)
    dxm = F.fold(torch.matmul(w2.t(), g2), xm.shape[2:], (KH, KW), dilation=dil, padding=pad, stride=stride)
    dx = torch.zeros(B, Cin, H, xm.shape[3], dtype=torch.float64).index_add_(2, ih, dxm)
    dx = torch.zeros(B, Cin, H, W, dtype=torch.float64).index_add_(3, iw, dx)
    return y, dx, dw, dy.double().sum((0, 2, 3))


#: (x shape, Cout, k, stride, pad, dil, reflect): stride 1 and 2, dilation 2, padding 0 / same / full, reflect 1 and 3
INDEPENDENT = [((2, 5, 9, 7), 6, 3, 1, 0, 1, 0), ((2, 5, 9, 7), 6, 3, 1, 1, 1, 0), ((1, 4, 8, 10), 3, 3, 1, 2, 1, 0),
               ((2, 3, 11, 9), 5, 4, 2, 2, 1, 0), ((1, 6, 12, 10), 4, 3, 2, 1, 1, 0), ((2, 4, 10, 12), 5, 3, 1, 2, 2, 0),
               ((1, 3, 9, 9), 4, 3, 1, 4, 2, 0), ((2, 4, 6, 8), 5, 3, 1, 0, 1, 1), ((1, 3, 5, 6), 4, 7, 1, 0, 1, 3),
               ((1, 2, 6, 5), 3, 3, 2, 1, 1, 1), ((1, 7, 5, 5), 2, 1, 1, 0, 1, 0)]


@pytest.mark.parametrize("case", INDEPENDENT, ids=lambda c: "-".join(map(str, c[0])) + "-" + "-".join(map(str, c[1:])))
def test_arbiter_matches_the_unfold_formulation(case):
    xs, Cout, k, stride, pad, dil, reflect = case
    c = cb.Case("independent", xs, Cout, k, stride, pad, dil, reflect, True, "normal")
    x, w, b, dy = cb.make_inputs(c)
    got = cb.reference(x, w, b, dy, stride, pad, dil, reflect)
    want = _unfold_formulation(x, w, b, dy, stride, pad, dil, reflect)
    for name, a, r in zip(cb.TENSORS, got, want):
        assert a.dtype == torch.float64 and a.shape == r.shape, (name, a.shape, r.shape)
        e = float((a - r).abs().max() / r.abs().max())
        assert e <= 1e-13, f"{name}: {e:.3e}"                 # two fp64 summation orders of at most 147 terms
    # the operands are what the flavour rounds to: bf16 values, and not the inputs themselves
    assert torch.equal(cb.rn_bf16(x).to(torch.bfloat16).double(), cb.rn_bf16(x)) and not torch.equal(cb.rn_bf16(x), x.double())
    assert bool((cb.trunc_bf16(x).abs() <= x.double().abs()).all()) and not torch.equal(cb.trunc_bf16(x), cb.rn_bf16(x))


_ARB = {}


def _arb(c):
    if c.name not in _ARB:
        _ARB[c.name] = cb.arbiter(c)
    return _ARB[c.name]


@pytest.mark.parametrize("c", CPU_CASES, ids=cb.case_id)
def test_case_list_routes_arm_and_slices(c):
    """every case: a route this arbiter covers (routes() raises for a dx handed to the framework), the fp32 arm in class against
    itself with an fp32-class error, the slice rule within EXCLUDED_MAX on the reference alone"""
    for nhwc in (True, False):
        rt = cb.routes(c, nhwc)
        assert rt["dx"] in ("K16b", "K16", "parity") and (nhwc or "K16b" not in (rt["fwd"], rt["dx"], rt["dw"]))
        cb.expected_trace(c, nhwc)
    _, ref, arm = _arb(c)
    j = cb.judge(cb.Judge("cpu-arm", cb.shape_str(c) + ":" + c.regime), arm, arm, ref)
    j.assert_in_class()
    for t, m, ek, ea, _ in j.rows:
        assert ek == ea
        if m == "rel_max":
            assert ea <= 1e-6, (t, ea)             # E_arm of the order of 1e-7
    for t in cb.TENSORS:
        if ref[t] is not None:
            share = ac.excluded_share(cb._AS3[t](ref[t]))
            assert share <= ac.EXCLUDED_MAX, (t, share)


def test_the_case_list_names_what_the_host_code_decides():
    """the route each group of the list is there for (restated from the branch conditions, compared with the library on the GPU)"""
    for c in cb.GATHER:
        assert cb.routes(c)["fwd"] == "K16" and cb.routes(c)["dw"] == "K16" and cb.routes(c)["dx"] in ("K16", "parity")
    assert all(cb.routes(c)["fwd"] == "K16b" for c in cb.NHWC + cb.REFLECT + [cb.STREAMK])
    r = {c.name: cb.routes(c) for c in cb.CASES}
    assert r["cin130-cout300-ow64"] == dict(fwd="K16b", dx="K16b", dw="K16b", fused_reflect=False, fold=False)
    assert r["one-kstep"]["dx"] == "K16" and r["one-kstep"]["dw"] == "K16b"
    for name in ("cin33-cout129-ow33", "cin47-cout255-ow40", "cin127-cout257-ow7", "k4s2-ragged"):
        assert r[name]["dw"] == "K16", name                                  # OW % 32 != 0: the weight gradient falls back to K16
    assert r["s2-ow32"]["dx"] == r["k4s2-ragged"]["dx"] == r["k4s2-odd"]["dx"] == "parity"
    assert r["fwd-gather-dx-nhwc"] == dict(fwd="K16", dx="K16b", dw="K16", fused_reflect=False, fold=False)
    assert r["reflect1-fold"]["fold"] and not r["reflect1-no-fold"]["fold"] and r["reflect1-no-fold"]["dx"] == "K16b"
    assert r["reflect2-k5"]["fused_reflect"] and r["reflect2-k5"]["dx"] == "K16" and not r["reflect2-k5"]["fold"]
    # stream-K on 256 compute units: 258 tiles of 2 k-steps, 3 k-steps per workgroup (tiles are cut); not on a smaller batch
    assert cb.streamk_rule(cb.STREAMK, 256) == (True, 258, 2, 3)
    assert not cb.streamk_rule(cb.STREAMK._replace(x=(1, 64, 128, 129)), 256)[0]
    # the layer whose dx goes to the framework is refused
    with pytest.raises(ValueError):
        cb.routes(cb.Case("strided-dilated", (1, 8, 12, 12), 8, 3, 2, 2, 2, 0, True, "normal"))


@pytest.mark.parametrize("twin", sorted(cb.TWINS))
@pytest.mark.parametrize("name", cb.TWIN_CASES)
def test_twins_miss_the_bound(name, twin):
    """the fp32 arm of the TRUE operands (what a correct kernel delivers at best) judged against the arbiter of the twin's operands:
    out of class by at least TEETH in every tensor the twin touches, in class in the others"""
    c = cb.BY_NAME[name]
    inputs, ref, arm = _arb(c)
    kw, damaged = cb.TWINS[twin]
    _, tref, tarm = cb.arbiter(c, inputs, **kw)
    j = cb.judge(cb.Judge(f"cpu-twin:{twin}", cb.shape_str(c)), arm, tarm, tref)
    j.assert_out_of_class(damaged)
    for t in set(cb.TENSORS) - set(damaged):
        assert j.over(t) <= 1.0, (twin, t, j.over(t))
    cb.check_ceiling(j)


def test_frozen_record_twin_misses_the_bound():
    """w rounded after the 1/sigma-style scaling (what the record does) against rounded before it: y, dx out of class"""
    c = cb.BY_NAME["square128"]
    x, w, b, dy = cb.make_inputs(c)
    _, ref, arm = cb.arbiter(c, (x, cb.frozen_weight(w), b, dy))
    tref, tarm = cb.arbiter_frozen_twin(c, (x, w, b, dy))
    cb.judge(cb.Judge("cpu-arm:frozen", cb.shape_str(c)), arm, arm, ref).assert_in_class()
    j = cb.judge(cb.Judge("cpu-twin:scaled-after-rounding", cb.shape_str(c)), arm, tarm, tref)
    j.assert_out_of_class(("y", "dx"))
    assert j.over("dw") <= 1.0 and j.over("db") <= 1.0
