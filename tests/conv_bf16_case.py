"""The exact-operand arbiter of the one-term bf16 convolution flavour (ops.CONV_PRECISION = "bf16").  A plain helper like
tests/accuracy_case.py (no fixtures, no conftest), plain torch on the CPU, imported by tests/test_conv_bf16_exact_cpu.py and
tests/test_gpu_conv_bf16_exact.py.

The flavour's kernels round their operands deterministically to nearest even (cv_pack_bf16, cocos_conv2d_nhwc_prep_bf16,
cocos_conv2d_weight_planes with mode | 2) and accumulate in fp32.  So the operands can be reproduced on the host, and against THEM the
kernel differs from fp64 by fp32 accumulation only — the 1.5e-2 of the older tests measures the rounding of the operands, not the kernel:

    y  = conv64(rn(x), rn(w)) + b             dx = conv_input64(rn(dy), rn(w))
    dw = conv_weight64(rn(x), rn(dy))         db = sum64(dy) of the UNROUNDED dy (ops.channel_sum reads fp32)

With `reflect` the mirror is applied before the convolution (rounding and mirroring commute).

The yardstick is the framework's fp32 convolution and gradients ON THE CPU on the same rounded operands held as fp32 (fp32_arm): it
does not move with MIOpen's algorithm choice.  Judgement is tests/accuracy_case.py's: E_kernel <= FACTOR * max(E_arm, eps) per tensor
under rel_max and rel_slice, EXCLUDED_MAX of the slices at most left out, a twin must miss by TEETH.  CEILING: the f16x3 flavour is
held at 1e-5 with the same fp32 accumulation in the same kernels and one term rounds less than three, so no bound asserted with this
arbiter may exceed 1e-5 rel_max, whatever the factor (`check_ceiling`).

The route that hands dx to the framework (the last branch of ops._Conv2d.backward: stride > 1 together with dilation > 1, or a
parity class that would need negative padding) is KEPT OUT of the case list: `routes()` raises for such a layer.  torch's
conv2d_input on unrounded operands is not this flavour's arithmetic and is not judged here.

Twins perturb the REFERENCE, never the kernel: the same output judged against an arbiter (reference and arm) built on slightly different
operands must miss the bound at least TEETH times over."""
import collections
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy_case as ac  # noqa: E402

CEILING = 1e-5           # rel_max: the f16x3 flavour's bound on the same data paths
SIGMA = 1.37             # the 1/sigma-style scaling of a frozen record's weight (no power of two: the two roundings differ)


# ------------------------------------------------------------------------------------------------------------------ roundings
def rn_bf16(t):
    return t.to(torch.bfloat16).to(torch.float64)


def trunc_bf16(t):
    """round towards zero: the low 16 bits of the fp32 pattern dropped"""
    bits = t.detach().to(torch.float32).contiguous().view(torch.int32)
    return (bits & -65536).view(torch.float32).to(torch.float64)


# ------------------------------------------------------------------------------------------------------------------ reference, arm
def _chain(x, w, b, dy, stride, pad, dil, reflect):
    """y, dx, dw of the operation in the dtype of the operands, by the framework's convolution and autograd on the CPU"""
    x, w = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    xin = F.pad(x, (reflect,) * 4, mode="reflect") if reflect else x
    y = F.conv2d(xin, w, None, stride=stride, padding=pad, dilation=dil)
    y.backward(dy)
    if b is not None:
        y = y + b.view(1, -1, 1, 1)
    return y.detach(), x.grad, w.grad


def reference(x, w, b, dy, stride, pad, dil, reflect=0, rnd=rn_bf16, db_rounded=False):
    """fp64 (y, dx, dw, db) of the operation as the flavour defines it.  x, w, b, dy: CPU tensors of fp32-representable values.
    `rnd`, `db_rounded`: the twins' perturbations (another rounding of the operands; db taken from the rounded dy)."""
    xr, wr, gr = rnd(x), rnd(w), rnd(dy)
    y, dx, dw = _chain(xr, wr, None if b is None else b.double(), gr, stride, pad, dil, reflect)
    db = (gr if db_rounded else dy.double()).sum((0, 2, 3))
    return y, dx, dw, db


def fp32_arm(x, w, b, dy, stride, pad, dil, reflect=0, rnd=rn_bf16, db_rounded=False):
    """the framework's fp32 convolution and gradients on the same rounded operands held as fp32, on the CPU"""
    f = torch.float32
    xr, wr, gr = rnd(x).to(f), rnd(w).to(f), rnd(dy).to(f)
    y, dx, dw = _chain(xr, wr, None if b is None else b.to(f), gr, stride, pad, dil, reflect)
    db = (gr if db_rounded else dy.to(f)).sum((0, 2, 3))
    assert all(t.dtype == f for t in (y, dx, dw, db))
    return y, dx, dw, db


# ------------------------------------------------------------------------------------------------------------------ cases
#: x = (B, Cin, H, W); k: square kernel; regime: "normal" | "chanscale" (x scaled per input channel by 2^-6 .. 2^6) | "small-dy" (1e-3)
Case = collections.namedtuple("Case", "name x Cout k stride pad dil reflect bias regime")


def _c(name, x, Cout, k, stride=1, pad=0, dil=1, reflect=0, bias=True, regime="normal"):
    return Case(name, tuple(x), Cout, k, stride, pad, dil, reflect, bias, regime)


#: the gather flavour (conv_f16x3.hip's one-term kernels): every gradient
GATHER = [
    _c("cout96", (2, 64, 12, 20), 96, 3, pad=1),                    # Cout < 128
    _c("cin3", (2, 3, 13, 17), 16, 3, pad=1),                       # Cin < 32: element gather
    _c("cin8-cout130", (1, 8, 12, 12), 130, 1),                     # Cin < 32 keeps a wide layer off K16b
    _c("k4s2-odd", (2, 3, 33, 37), 16, 4, stride=2, pad=2),         # 17 x 19 outputs, parity-class input gradient
    _c("ragged", (3, 5, 9, 7), 7, 3, pad=1),
    _c("dil2", (2, 12, 20, 24), 10, 3, pad=2, dil=2),
    _c("full-pad", (2, 20, 10, 16), 24, 3, pad=2),                  # output larger than the input
    _c("ragged-chanscale", (3, 5, 9, 7), 7, 3, pad=1, regime="chanscale"),
    _c("ragged-small-dy", (3, 5, 9, 7), 7, 3, pad=1, regime="small-dy"),
    _c("ragged-no-bias", (3, 5, 9, 7), 7, 3, pad=1, bias=False),
]
#: K16b (conv_nhwc_bf16.hip) forward: Cout >= 128 and Cin >= 32 (cocos_conv2d_nhwc_bf16_supported).  Its weight gradient needs
#: OW % 32 == 0 (else K16's), its input gradient stride 1, q = dil (k - 1) - pad >= 0 and Cin >= 128, Cout >= 32 (roles swapped)
NHWC = [
    _c("one-kstep", (2, 32, 16, 32), 128, 1),                       # Cin = 32, 1x1: the prologue is everything; wgrad: 4 slices
    _c("cin33-cout129-ow33", (1, 33, 6, 33), 129, 3, pad=1),        # channel padding, row tile tail, 198 positions
    _c("cin47-cout255-ow40", (2, 47, 5, 40), 255, 3, pad=1),
    _c("cin127-cout257-ow7", (1, 127, 7, 7), 257, 3, pad=1),        # second row tile of ONE row, 49 positions
    _c("cin130-cout300-ow64", (1, 130, 6, 64), 300, 3, pad=1),      # forward, input and weight gradient on K16b; wgrad: one slice
    _c("k5", (1, 64, 6, 64), 160, 5, pad=2),
    _c("dil2-ow32", (2, 32, 12, 32), 256, 3, pad=2, dil=2),
    _c("s2-ow32", (2, 64, 16, 64), 160, 3, stride=2, pad=1),        # forward + weight gradient on K16b, parity-class input gradient
    _c("k4s2-ragged", (2, 32, 33, 37), 128, 4, stride=2, pad=2),    # 17 x 19 outputs
    _c("square128", (2, 128, 4, 32), 128, 3, pad=1),                # all three on K16b, 256 positions
    _c("cin130-chanscale", (1, 130, 6, 64), 300, 3, pad=1, regime="chanscale"),
    _c("cin130-small-dy", (1, 130, 6, 64), 300, 3, pad=1, regime="small-dy"),
    _c("square128-no-bias", (2, 128, 4, 32), 128, 3, pad=1, bias=False),
]
#: forward on K16 (Cout < 128), input gradient on K16b (Cin >= 128): the reverse of "one-kstep" and its kind
MIXED = [_c("fwd-gather-dx-nhwc", (2, 128, 8, 32), 64, 3, pad=1)]
#: the fused reflect border (ops.conv2d: stride 1, padding 0, OW % 32 == 0, on K16b)
REFLECT = [
    _c("reflect1-fold", (1, 128, 4, 32), 128, 3, reflect=1),        # padded H - 2 = 4 >= 4: the GEMM folds the border back
    _c("reflect1-no-fold", (1, 128, 3, 32), 128, 3, reflect=1),     # padded H - 2 = 3: cocos_reflect_pad2d_bwd
    _c("reflect2-k5", (1, 40, 6, 32), 128, 5, reflect=2),           # reflect > 1; input gradient on K16, then the gather
]
#: the smallest layer the host-side rule of cocos_nhwc_gemm_impl runs as stream-K on 256 CUs (the rule is quoted at streamk_rule)
STREAMK = _c("streamk", (2, 64, 128, 129), 257, 1)
CASES = GATHER + NHWC + MIXED + REFLECT + [STREAMK]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def case_id(c):
    return c.name


def shape_str(c):
    B, Cin, H, W = c.x
    return f"{B}x{Cin}x{H}x{W}->{c.Cout}k{c.k}s{c.stride}p{c.pad}d{c.dil}r{c.reflect}"


def out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def make_inputs(c, seed=2027):
    """(x, w, b or None, dy): CPU fp32 tensors.  Unit-normal x, w / sqrt(K) as the suite's convolution tests build them."""
    B, Cin, H, W = c.x
    g = torch.Generator().manual_seed(seed + 131 * Cin + 7 * c.Cout + H * W + c.k)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(c.Cout, Cin, c.k, c.k, generator=g) / (Cin * c.k * c.k) ** 0.5
    b = torch.randn(c.Cout, generator=g) if c.bias else None
    r = c.reflect
    dy = torch.randn(B, c.Cout, out_size(H + 2 * r, c.k, c.stride, c.pad, c.dil), out_size(W + 2 * r, c.k, c.stride, c.pad, c.dil),
                     generator=g)
    if c.regime == "chanscale":
        x = x * torch.exp2(torch.linspace(-6.0, 6.0, Cin).round()).view(1, Cin, 1, 1)
    elif c.regime == "small-dy":
        dy = dy * 1e-3
    elif c.regime != "normal":
        raise ValueError(c.regime)
    return x, w, b, dy


# ------------------------------------------------------------------------------------------------------------------ routes
def nhwc_supported(Cin, Cout, k, stride):
    """cocos_conv2d_nhwc_bf16_supported, restated (the GPU test compares it with the library's answer)"""
    return 1 <= stride <= 4 and Cout >= 128 and Cin >= 32 and k >= 1 and k * k <= 49


def _parity_classes_ok(H, W, k, s, p):
    """ops._conv_dgrad_strided returns None when a parity class would need negative padding"""
    for n in (H, W):
        for r in range(s):
            J = len(range(r, k, s))
            u0 = max(0, -((r - p) // s))
            U = (n - 1 + p - r) // s + 1 - u0 if n - 1 + p - r >= 0 else 0
            if U > 0 and J > 0 and J - 1 - u0 < 0:
                return False
    return True


def routes(c, nhwc=True):
    """{"fwd", "dx", "dw": "K16b" | "K16" | "parity", "fused_reflect", "fold": bool} from the branch conditions of ops.conv2d and
    ops._Conv2d — pinned here, not asked of the code under test.  Raises for a layer whose dx goes to the framework."""
    B, Cin, H, W = c.x
    k, s, r = c.k, c.stride, c.reflect
    ow = out_size(W + 2 * r, k, s, c.pad, c.dil)
    fused = bool(r) and nhwc and s == 1 and c.pad == 0 and r < min(H, W) and ow >= 32 and ow % 32 == 0 and nhwc_supported(Cin, c.Cout, k, 1)
    fwd = "K16b" if nhwc and nhwc_supported(Cin, c.Cout, k, s) else "K16"
    assert not r or fused or fwd == "K16"
    dw = "K16b" if fwd == "K16b" and ow % 32 == 0 else "K16"
    q = c.dil * (k - 1) - c.pad
    Hk, Wk = (H + 2 * r, W + 2 * r) if fused else (H, W)      # (unfused: reflect_pad2d in front of the plain layer, same sizes)
    if s == 1 and q >= 0:
        dx = "K16b" if nhwc and nhwc_supported(c.Cout, Cin, k, 1) else "K16"
    elif s > 1 and c.dil == 1 and _parity_classes_ok(H + 2 * r, W + 2 * r, k, s, c.pad):
        dx = "parity"
    else:
        raise ValueError(f"{c.name}: dx is handed to the framework (ops._Conv2d.backward, last branch): not a case of this arbiter")
    fold = fused and dx == "K16b" and r == 1 and Hk - 2 >= 4 and Wk - 2 >= 4
    return dict(fwd=fwd, dx=dx, dw=dw, fused_reflect=fused, fold=fold)


FWD_ENTRY = {"K16b": "cocos_conv2d_nhwc_bf16", "K16": "cocos_conv2d_fwd_f16x3"}
DX_ENTRY = {"K16b": "cocos_conv2d_nhwc_bf16", "K16": "cocos_conv2d_fwd_f16x3", "parity": "cocos_conv2d_fwd_scatter_f16x3"}
DW_ENTRY = {"K16b": "cocos_conv2d_nhwc_wgrad_bf16", "K16": "cocos_conv2d_wgrad_bf16"}
CONV_ENTRIES = set(FWD_ENTRY.values()) | set(DX_ENTRY.values()) | set(DW_ENTRY.values()) | {
    "cocos_conv2d_nhwc_f16x3", "cocos_conv2d_nhwc_wgrad_f16x3", "cocos_conv2d_wgrad_f16x3", "cocos_conv2d_wgrad_reduce",
    "cocos_reflect_pad2d_fwd", "cocos_reflect_pad2d_bwd", "cocos_channel_sum"}


def expected_trace(c, nhwc=True, need=("x", "w", "b")):
    """(forward, backward): the convolution entry points each phase must reach, in order, operand preparations left out"""
    rt = routes(c, nhwc)
    fwd = ([] if rt["fused_reflect"] or not c.reflect else ["cocos_reflect_pad2d_fwd"]) + [FWD_ENTRY[rt["fwd"]]]
    bwd = []
    if "x" in need:
        n = 1
        if rt["dx"] == "parity":        # one launch per parity class that has pixels and taps
            n = sum(1 for ry in range(c.stride) for rx in range(c.stride) if len(range(ry, c.k, c.stride)) and len(range(rx, c.k, c.stride)))
        bwd += [DX_ENTRY[rt["dx"]]] * n
    if "w" in need:
        bwd += [DW_ENTRY[rt["dw"]], "cocos_conv2d_wgrad_reduce"]
    if "b" in need and c.bias:
        bwd.append("cocos_channel_sum")
    if c.reflect and "x" in need and not rt["fold"]:
        bwd.append("cocos_reflect_pad2d_bwd")
    return fwd, bwd


def streamk_rule(c, cus):
    """cocos_nhwc_gemm_impl (conv_nhwc_bf16.hip), restated for the forward of `c` on `cus` compute units:
        bm = Cout <= 128 ? 128 : 256;  ntm = ceil(Cout / bm);  cols = ceil(B OH OW / 256)
        bn = (bm == 128 ? cols >= 100 : ntm * cols >= 200) ? 256 : 128;  tiles = ntm * ceil(B OH OW / bn);  rounds = ceil(tiles / cus)
        stream-K  <=>  workspace given and tiles > cus and 5 tiles < 4 rounds cus and bm == 256 and bn == 256
    -> (taken, tiles, k-steps per tile, k-steps per workgroup)"""
    B, Cin, H, W = c.x
    ntot = B * out_size(H + 2 * c.reflect, c.k, c.stride, c.pad, c.dil) * out_size(W + 2 * c.reflect, c.k, c.stride, c.pad, c.dil)
    bm = 128 if c.Cout <= 128 else 256
    ntm, cols = -(-c.Cout // bm), -(-ntot // 256)
    bn = 256 if (cols >= 100 if bm == 128 else ntm * cols >= 200) else 128
    tiles = ntm * -(-ntot // bn)
    rounds = -(-tiles // cus)
    nsteps = c.k * c.k * -(-Cin // 32)
    taken = tiles > cus and tiles * 5 < rounds * cus * 4 and bm == 256 and bn == 256
    return taken, tiles, nsteps, -(-tiles * nsteps // cus)


# ------------------------------------------------------------------------------------------------------------------ judgement
def as3(t):
    """[B, C, positions] for accuracy_case's slice metric: y and dx flattened over the pixels (a slice is a pixel, over the channels);
    dw [Cout, Cin, KH, KW] as ONE sample of Cout slices (a slice is an output channel's filter, over K = Cin KH KW — so the per-channel
    scales of the "chanscale" regime, 2^12 apart, stay inside every slice and none falls below SLICE_MIN); db [Cout] is one slice:
    an entry that cancels to 1e-3 of the largest carries 1000 x the rounding of its sum, in arm and kernel alike."""
    t = t.detach().double().cpu()
    if t.dim() == 1:
        return t.reshape(1, -1, 1).numpy()
    return t.reshape(t.shape[0], t.shape[1], -1).numpy()


def as3_weight(t):
    t = t.detach().double().cpu()
    return t.reshape(1, t.shape[0], -1).transpose(1, 2).numpy()


#: (tensor, route of that tensor, metric) -> factor, for a route the hardware puts outside FACTOR x the arm but inside the ceiling:
#: twice the largest measured ratio (profiles/conv_bf16_exact.txt), the cause stated next to it.  Everything else: FACTOR.
#:
#: The input gradient, on K16 and on K16b alike: measured on an MI355X 5.17 / 4.95 (K16: rel_max / rel_slice) and 5.16 / 4.72 (K16b),
#: E_kernel 4.9e-7 .. 9.1e-7 against an arm of 1.2e-7 .. 1.8e-7.  Cause: summation depth.  dx sums over K = Cout KH KW, the deepest
#: sum of a layer here — 4000 for "k5" (160 x 25), 2700 for "cin130-cout300-ow64", 2313 for "cin127-cout257-ow7", 1152 plus the
#: mirrored border's two to four addends for "reflect1-fold" — and both kernels carry it in ONE fp32 accumulator per output over
#: K / 16 MFMA k-steps (250 for "k5") with no slices and, stream-K off, no splits, so the rounding grows with sqrt(K / 16); the
#: framework's CPU convolution blocks the same sum and stays at 1.2e-7 .. 1.8e-7.  The same layers' y (K = Cin KH KW <= 1600) and
#: dw (slices of at most a few hundred positions, summed by cocos_conv2d_wgrad_reduce) stay inside FACTOR, as does the parity-class
#: dx (K / 4 per class).  The largest bound this gives is 10.4 x 2.0e-7 = 2.1e-6 rel_max, a fifth of the ceiling; a twin measures
#: 5.5e3 .. 6.0e4 x the arm on the same hardware run.
ROUTE_FACTOR = {("dx", "K16", "rel_max"): 10.4, ("dx", "K16", "rel_slice"): 9.9,
                ("dx", "K16b", "rel_max"): 10.4, ("dx", "K16b", "rel_slice"): 9.5}


def factors(rt):
    """{(tensor, metric): factor} of a layer with the routes `rt`"""
    of = {"y": rt["fwd"], "dx": rt["dx"], "dw": rt["dw"], "db": "channel_sum"}
    return {(t, m): ROUTE_FACTOR.get((t, of[t], m), ac.FACTOR) for t in of for m in ac.METRICS}


TENSORS = ("y", "dx", "dw", "db")
_AS3 = {"y": as3, "dx": as3, "dw": as3_weight, "db": as3}


class Judge(ac.Judge):
    """accuracy_case.Judge with this file's line format: `CONV_BF16_EXACT <route> <shape> <tensor> <metric> E_kernel E_arm ratio`"""

    def __init__(self, route, shape):
        self.head = f"CONV_BF16_EXACT {route} {shape}"
        self.rows = []

    def add(self, tensor, got, arm, ref, floor=0.0, factor=ac.FACTOR, excluded=ac.EXCLUDED_MAX):
        ek, ea = ac.errors(got, ref, floor, excluded), ac.errors(arm, ref, floor, excluded)
        for m in ac.METRICS:
            f = factor.get((tensor, m), ac.FACTOR) if isinstance(factor, dict) else factor
            self.rows.append((tensor, m, ek[m], ea[m], f))
            print(f"{self.head} {tensor} {m} {ek[m]:.3e} {ea[m]:.3e} {ek[m] / max(ea[m], ac.FP32_EPS):.2f}", flush=True)
        return self

    def assert_in_class(self):
        super().assert_in_class()
        check_ceiling(self)


def check_ceiling(j):
    """no bound asserted with this arbiter exceeds CEILING under rel_max"""
    over = [(t, f"{ac.bound(ea, f):.3e}") for t, m, _, ea, f in j.rows if m == "rel_max" and ac.bound(ea, f) > CEILING]
    assert not over, f"{j.head}: bound above the ceiling of {CEILING} rel_max: {over}"


def judge(j, got, arm, ref, tensors=TENSORS, factor=ac.FACTOR):
    """got / arm / ref: {"y", "dx", "dw", "db"} (absent or None: not judged)"""
    for t in tensors:
        if got.get(t) is not None:
            j.add(t, _AS3[t](got[t]), _AS3[t](arm[t]), _AS3[t](ref[t]), factor=factor)
    return j


def arbiter(c, inputs=None, **twin):
    """(inputs, ref, arm) of a case: {"y", "dx", "dw", "db"} each; `twin`: rnd= / db_rounded= of reference and fp32_arm"""
    x, w, b, dy = make_inputs(c) if inputs is None else inputs
    args = (x, w, b, dy, c.stride, c.pad, c.dil, c.reflect)
    ref = dict(zip(TENSORS, reference(*args, **twin)))
    arm = dict(zip(TENSORS, fp32_arm(*args, **twin)))
    if b is None:
        ref["db"] = arm["db"] = None
    return (x, w, b, dy), ref, arm


#: twin -> (keywords of the perturbed arbiter, the tensors it must throw out of class)
TWINS = {"truncated-operands": (dict(rnd=trunc_bf16), ("y", "dx", "dw")), "db-of-rounded-dy": (dict(db_rounded=True), ("db",))}
#: the cases whose kernel output is judged against the twins on the GPU: K16b forward / input gradient / weight gradient, gather forward
TWIN_CASES = ["cin130-cout300-ow64", "square128", "ragged", "cout96"]


def frozen_weight(w):
    """the effective weight of a frozen record under a 1/sigma-style scaling, as the record forms it: scaled in fp32, THEN rounded"""
    return (w / SIGMA).contiguous()


def frozen_twin_weight(w):
    """... and its twin: rounded first, scaled afterwards (fp64; in general no bf16 value)"""
    return rn_bf16(w) / SIGMA


def arbiter_frozen_twin(c, inputs):
    """(ref, arm) on rn(x), rn(W) / SIGMA, rn(dy), W = the layer's parameter BEFORE the scaling: the weight operand is used as it
    stands (rounded to fp32 in the arm), not rounded to bf16 again"""
    x, w, b, dy = inputs
    wt = frozen_twin_weight(w)
    res = []
    for dt in (torch.float64, torch.float32):
        y, dx, dw = _chain(rn_bf16(x).to(dt), wt.to(dt), None if b is None else b.to(dt), rn_bf16(dy).to(dt), c.stride, c.pad, c.dil, c.reflect)
        res.append(dict(y=y, dx=dx, dw=dw, db=dy.to(dt).sum((0, 2, 3))))
    return res[0], res[1]
