"""Accuracy-class cases: inputs, two metrics and the yardstick that hold the split-precision (f16x3) kernels to the error of fp32
arithmetic itself, not to a fixed 2e-4.  A plain helper like tests/loss_case.py (no fixtures, no conftest).

The claim under test: a three-term f16 hi/lo product with fp32 accumulation is not coarser than fp32.  So the bound is never a constant:
it is the error E_fp32 of the same operation in plain fp32 (numpy here, torch on the device in the GPU tests) on the same inputs against
the same fp64 reference, under the same metric:

    E_kernel <= FACTOR * max(E_fp32, eps_fp32)            FACTOR = 4: another accumulation and merge order (tests/test_gpu_match.py)

Metrics (both against fp64, both with the suite's absolute `floor` added to the denominator where a gradient vanishes by cancellation):
    rel_max     max|x - ref| / max|ref| over the tensor: the suite's metric
    rel_slice   the same per position (a query column of out / dq, a key column of dk / dv), then the largest over the positions whose
                reference maximum exceeds SLICE_MIN of the tensor's: an error confined to one position cannot hide behind the largest
                element elsewhere.  At most EXCLUDED_MAX of the positions may be left out (asserted on the reference).

Input regimes, K = 256 channels, centred and L2-normalised over the channels as center_l2norm does, then rounded to fp32 (the reference is
computed from exactly what the kernels are handed):
    diffuse     independent q and k: tests/test_gpu_parity.py's _qkv(peaked=False)
    semi        k[:, :, :n] = q[:, :, :n] + sigma * noise with sigma such that at least SEMI_SHARE_MIN of ALL rows of the reference P have
                their largest weight in [0.1, 0.9]: few competing keys, the cancellation in dS = P (dP - D) is live.  (The suite's "peaked"
                inputs use sigma = 0.05: every row one-hot to 1e-40, every gradient 1e-35.)

Lost planes (`hi_plane`): an operand rounded to its f16 hi plane across the whole tensor — the planes of a slightly different tensor, what
a kernel computes when a lo plane is dropped, mis-indexed or skipped by a wrong mask.  tests/test_accuracy_class_cpu.py shows in numpy that
every such loss exceeds the bound at least twofold; the GPU file repeats it on the kernels wherever the planes are reachable."""
import contextlib

import numpy as np

from oracle import corr_oracle as co

INV_T = 100.0
K = 256
FACTOR = 4.0
FP32_EPS = float(np.finfo(np.float32).eps)
SLICE_MIN = 1e-3
EXCLUDED_MAX = 0.05
SEMI_SHARE_MIN = 1.0 / 3.0
TEETH = 2.0                      # a lost plane must miss the bound at least this many times over
#: the suite's floors (tests/test_gpu_parity.py) for g ~ N(0, 1): gradients that vanish by cancellation are judged on the operands' scale
FLOORS = {"out": 0.0, "dq": 0.5, "dk": 0.5, "dv": 0.05}

#: (B, Nq, Nk, Cv): partial query and key tiles, a last tile of 4 keys, Cv on either side of a 32-block, the ADE20k width
K2_SHAPES = [(2, 64, 64, 3), (2, 132, 68, 33), (2, 36, 260, 5), (2, 256, 128, 154), (2, 384, 384, 40), (2, 8, 8, 1)]
#: sigma of the semi regime per (Nq, Nk): chosen on the CPU (a scan over sigma of the share of rows with max weight in [0.1, 0.9]);
#: tests/test_accuracy_class_cpu.py asserts the share for every committed shape and seed.  (8, 8) has no semi case.
SEMI_SIGMA = {(64, 64): 10.0, (132, 68): 12.0, (36, 260): 10.0, (256, 128): 10.0, (384, 384): 8.0}
SEED = 2026
#: (8, 8): with SEED three of the sixteen reference rows are one-hot (dq slices below SLICE_MIN); 2031 is the first seed with none
SHAPE_SEED = {(8, 8): 2031}
#: The one place the 5 % cannot be met by ANY input of the shape: (Nq, Nk) = (36, 260) has 72 query rows to spread over 520 key columns
#: at inv_t = 100, so about a quarter of the key columns carry no weight in either regime (reference: dk 0.21 / 0.24, dv 0.23 / 0.26 for
#: diffuse / semi).  Those columns are left out as the rule says; the share is still asserted, against this ceiling.
EXCLUDED_ALLOW = {(36, 260): {"dk": 0.30, "dv": 0.30}}


#: K7 (ops.logits_softmax_warp) is correct but coarser than 4 x fp32 WHEN ITS LOGITS ARE EXACT INPUTS, so it carries factors of its own:
#: twice the largest ratio E_kernel / E_fp32 measured on an MI355X over the eleven K2 cases (profiles/accuracy_class.txt), rounded up.
#:     measured   out rel_slice 5.52   d logits rel_max 7.47, rel_slice 26.59   dv rel_max 10.76, rel_slice 16.14   (out rel_max 0.87: stays 4)
#: Reason: the kernels keep the row statistics flash-style, in the log2 domain — x = l * log2(e), lse = (m + log2 s) * ln 2, and in the
#: backward P = exp2(l * log2(e) - lse * log2(e)).  Each of those numbers is of magnitude 2^5 at |logit| ~ 30, so each rounding is worth
#: up to 2^-19 = 1.9e-6 in log2 units = 1.3e-6 RELATIVE in every P of the row: E(P) ~ 1e-6 .. 3e-6, which is what d logits and dv show
#: (2.2e-6 .. 2.6e-6).  The framework's softmax subtracts the row maximum before anything is scaled, and reaches 1e-7 .. 4e-7.  In K2 the
#: same arithmetic is NOT coarser than its arm: there the logits come out of an fp32 product at 100 x and carry that rounding in both.
#: Measured, not only argued: torch fp32 on the device with the SAME row statistics (the `torch-fp32-log2-domain` lines of
#: tests/test_gpu_accuracy_class.py) is 6.6 x .. 11.6 x coarser than torch's softmax on these cases (out 10.0 / 6.6, d logits 8.9 / 11.6,
#: dv 8.1 / 8.6 for rel_max / rel_slice), i.e. where the kernel is, except d logits' rel_slice (26.6 against 11.6).  That remainder comes
#: from ONE case, (64, 64, 3) diffuse (the other ten measure 0.4 .. 2.8), and its explanation is a hypothesis:
#: d logits' rel_slice: in a row with largest weight P* the difference dP - D is (1 - P*) times its terms, and a column just above
#: SLICE_MIN has 1 - P* ~ 2e-3: the three-term product's 2^-22 per term (the lo x lo term is dropped) against fp32's 2^-24 shows 500-fold.
#: The widened bound still discriminates: a lost lo plane of V, dO or P measures 230 x .. 790 x the fp32 arm on these cases
#: (tests/test_accuracy_class_cpu.py asserts at least twice the factor for every tensor and metric).  K7's planes are made inside the op,
#: so it has no twin on the GPU: that the widened bounds discriminate is shown by the numpy emulation only.
K7_FACTORS = {("out", "rel_slice"): 12.0, ("dlogits_t", "rel_max"): 15.0, ("dlogits_t", "rel_slice"): 54.0,
              ("dv", "rel_max"): 22.0, ("dv", "rel_slice"): 33.0}
K7_FLOORS = {"out": 0.0, "dlogits_t": 1e-3, "dv": 0.05}       # tests/test_gpu_parity.py's


def k7_reference(qn, kn, v, g, inv_t=INV_T):
    """K7 on the K2 cases' own logits, fp32-rounded: (logits [B,Nq,Nk] fp64, {"out", "dlogits_t" [B,Nk,Nq], "dv", "p"} fp64)"""
    f = as_f32(co.correlation(qn, kn) * inv_t)
    p = co.softmax(f)
    dp = np.matmul(g.transpose(0, 2, 1), v)
    return f, {"out": np.matmul(p, v.transpose(0, 2, 1)).transpose(0, 2, 1), "dv": np.matmul(g, p), "p": p,
               "dlogits_t": (p * (dp - (p * dp).sum(-1, keepdims=True))).transpose(0, 2, 1)}


def excluded_max(Nq, Nk, tensor):
    return EXCLUDED_ALLOW.get((Nq, Nk), {}).get(tensor, EXCLUDED_MAX)


def k2_cases():
    """[(B, Nq, Nk, Cv, regime)] of the K2 rows"""
    out = []
    for B, Nq, Nk, Cv in K2_SHAPES:
        out.append((B, Nq, Nk, Cv, "diffuse"))
        if (Nq, Nk) in SEMI_SIGMA:
            out.append((B, Nq, Nk, Cv, "semi"))
    return out


def case_id(c):
    return "-".join(str(x) for x in c)


def as_f32(a):
    """fp64 array holding fp32-representable values"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def make_qkv(B, Nq, Nk, Cv, regime, seed=None, sigma=None):
    """(qn [B,256,Nq], kn [B,256,Nk], v [B,Cv,Nk], g [B,Cv,Nq]) as fp64 arrays of fp32-representable values"""
    seed = SHAPE_SEED.get((Nq, Nk), SEED) if seed is None else seed
    rs = np.random.RandomState(seed + 7 * Nq + Nk)
    q = rs.standard_normal((B, K, Nq))
    k = rs.standard_normal((B, K, Nk))
    if regime == "semi":
        n = min(Nq, Nk)
        s = SEMI_SIGMA[(Nq, Nk)] if sigma is None else sigma
        k[:, :, :n] = q[:, :, :n] + s * rs.standard_normal((B, K, n))
    elif regime != "diffuse":
        raise ValueError(regime)
    v = rs.uniform(-1, 1, (B, Cv, Nk))
    g = rs.standard_normal((B, Cv, Nq))
    return as_f32(co.center_l2norm(q, True)), as_f32(co.center_l2norm(k, True)), as_f32(v), as_f32(g)


# ------------------------------------------------------------------------------------------------------------------ the reference
def reference(qn, kn, v, g, inv_t=INV_T):
    """fp64: {"out", "dq", "dk", "dv", "p"}"""
    p = co.softmax(co.correlation(qn, kn) * inv_t)
    out = np.matmul(p, v.transpose(0, 2, 1)).transpose(0, 2, 1)
    dq, dk, dv = co.corr_softmax_warp_bwd(qn, kn, v, g, inv_t)
    return {"out": out, "dq": dq, "dk": dk, "dv": dv, "p": p}


def semi_share(p):
    """share of the rows of P [B,Nq,Nk] whose largest weight lies in [0.1, 0.9]"""
    m = np.asarray(p).max(axis=-1)
    return float(((m >= 0.1) & (m <= 0.9)).mean())


def check_regime(regime, p):
    """the semi regime is what it says: asserted on the REFERENCE P, so inputs that drift out of range fail loudly"""
    if regime == "semi":
        share = semi_share(p)
        assert share >= SEMI_SHARE_MIN, f"semi regime: only {share:.3f} of the rows have their largest weight in [0.1, 0.9]"


# ------------------------------------------------------------------------------------------------------------------ the metrics
def _np64(x):
    if hasattr(x, "detach"):
        x = x.detach().double().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def rel_max(x, ref, floor=0.0):
    x, ref = _np64(x), _np64(ref)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    assert np.isfinite(x).all(), "non-finite values"
    return float(np.abs(x - ref).max() / (np.abs(ref).max() + floor))


def slice_maxima(ref):
    """ref [..., C, N] (or [B, N] when `ref` has no channel axis to reduce: then every element is its own slice) -> per-position maxima"""
    ref = _np64(ref)
    return np.abs(ref).max(axis=-2) if ref.ndim >= 3 else np.abs(ref)


def excluded_share(ref):
    m = slice_maxima(ref)
    return float((m <= SLICE_MIN * m.max()).mean())


def rel_slice(x, ref, floor=0.0, excluded=EXCLUDED_MAX):
    """max over the judged positions of max_c|x - ref| / (max_c|ref| + floor); the position axis is the last, the axis before it is
    reduced per slice"""
    x, ref = _np64(x), _np64(ref)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    assert np.isfinite(x).all(), "non-finite values"
    m = slice_maxima(ref)
    keep = m > SLICE_MIN * m.max()
    assert (~keep).mean() <= excluded, f"{(~keep).mean():.3f} of the positions fall below {SLICE_MIN} of the tensor's maximum"
    err = np.abs(x - ref).max(axis=-2) if ref.ndim >= 3 else np.abs(x - ref)
    return float((err[keep] / (m[keep] + floor)).max())


METRICS = {"rel_max": rel_max, "rel_slice": rel_slice}


def errors(x, ref, floor=0.0, excluded=EXCLUDED_MAX):
    return {"rel_max": rel_max(x, ref, floor), "rel_slice": rel_slice(x, ref, floor, excluded)}


def bound(e_fp32, factor=FACTOR):
    return factor * max(e_fp32, FP32_EPS)


class Judge:
    """One case: collects `ACC_CLASS <kernel> <route> <shape> <regime> <tensor> <metric> E_kernel E_fp32 ratio` lines (ratio = E_kernel
    / E_fp32, the floor of eps applied), prints them, and asserts the class bound — or, for a lost-plane twin, that it is missed."""

    def __init__(self, kernel, route, shape, regime):
        self.head = f"ACC_CLASS {kernel} {route} {'x'.join(str(s) for s in shape)} {regime}"
        self.rows = []                      # (tensor, metric, e_kernel, e_fp32, factor)

    def add(self, tensor, got, arm, ref, floor=0.0, factor=FACTOR, excluded=EXCLUDED_MAX):
        """`factor`: a number, or {(tensor, metric): number} for a kernel with measured factors of its own (FACTOR where it has none)"""
        ek, ea = errors(got, ref, floor, excluded), errors(arm, ref, floor, excluded)
        for m in METRICS:
            self.rows.append((tensor, m, ek[m], ea[m], factor.get((tensor, m), FACTOR) if isinstance(factor, dict) else factor))
            print(f"{self.head} {tensor} {m} {ek[m]:.3e} {ea[m]:.3e} {ek[m] / max(ea[m], FP32_EPS):.2f}", flush=True)
        return self

    def over(self, tensor=None, metric=None):
        """largest E_kernel / bound among the rows of `tensor` / `metric` (None: all)"""
        sel = [r for r in self.rows if tensor in (None, r[0]) and metric in (None, r[1])]
        assert sel, (tensor, metric)
        return max(ek / bound(ea, f) for _, _, ek, ea, f in sel)

    def assert_in_class(self):
        bad = [(t, m, f"{ek:.3e}", f"{ea:.3e}", f) for t, m, ek, ea, f in self.rows if not ek <= bound(ea, f)]
        assert not bad, f"{self.head}: coarser than factor x fp32 (tensor, metric, E_kernel, E_fp32, factor): {bad}"
        # the fp32 arm is the yardstick: it must itself be an fp32-class result, or the bound means nothing
        # (under the suite's metric; a slice just above SLICE_MIN carries up to 1 / SLICE_MIN times the tensor-wide relative error)
        assert all(ea <= 1e-4 for _, m, _, ea, _ in self.rows if m == "rel_max"), f"{self.head}: the fp32 arm is not an fp32-class result: {self.rows}"

    def assert_out_of_class(self, tensors):
        """a lost-plane twin: every tensor the plane feeds misses the bound at least TEETH times, under the suite's own metric"""
        for t in tensors:
            r = self.over(t, "rel_max")
            assert r >= TEETH, f"{self.head}: the lost plane leaves {t} at {r:.2f} x the bound: the bound does not discriminate"


# ------------------------------------------------------------------------------------------------------------------ lost planes (numpy)
def hi_plane(x, scale=None):
    """x rounded to the f16 hi plane of the split: f16(x * scale) / scale.  scale None: the device-side power of two that takes
    max|x| into [2^9, 2^10) (cocos_split_f16_ex with a max|x| cell)"""
    x = np.asarray(x, dtype=np.float64)
    if scale is None:
        amax = np.abs(x).max()
        scale = 2.0 ** (9 - np.floor(np.log2(amax))) if amax > 0 else 1.0
    return (x * scale).astype(np.float16).astype(np.float64) / scale


#: name -> (which tensors it damages)
LOST_PLANES = {"v_lo_fwd": ("out",), "v_lo_bwd": ("dq", "dk"), "k_lo_dqn": ("dq",), "ds_lo_keygemm": ("dk",), "q_lo_keygemm": ("dk",)}


def lost_plane(which, qn, kn, v, g, inv_t=INV_T):
    """fp64 arithmetic with ONE operand of ONE product rounded to its hi plane -> {"out", "dq", "dk", "dv"}"""
    p = co.softmax(co.correlation(qn, kn) * inv_t)
    vf = hi_plane(v) if which == "v_lo_fwd" else v
    out = np.matmul(p, vf.transpose(0, 2, 1)).transpose(0, 2, 1)
    vb = hi_plane(v) if which == "v_lo_bwd" else v
    dp = np.matmul(g.transpose(0, 2, 1), vb)
    ds = p * (dp - (p * dp).sum(axis=-1, keepdims=True)) * inv_t
    dq = np.matmul(hi_plane(kn, 16.0) if which == "k_lo_dqn" else kn, ds.transpose(0, 2, 1))
    dk = np.matmul(hi_plane(qn, 16.0) if which == "q_lo_keygemm" else qn, hi_plane(ds) if which == "ds_lo_keygemm" else ds)
    return {"out": out, "dq": dq, "dk": dk, "dv": np.matmul(g, p)}


def fp32_arm_numpy(qn, kn, v, g, inv_t=INV_T):
    """the same chain in numpy fp32: the CPU stand-in of the device's torch-fp32 arm"""
    f = np.float32
    qn, kn, v, g = (np.asarray(t, dtype=f) for t in (qn, kn, v, g))
    s = np.matmul(qn.transpose(0, 2, 1), kn) * f(inv_t)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    out = np.matmul(p, v.transpose(0, 2, 1)).transpose(0, 2, 1)
    dp = np.matmul(g.transpose(0, 2, 1), v)
    ds = p * (dp - (p * dp).sum(axis=-1, keepdims=True)) * f(inv_t)
    res = {"out": out, "dq": np.matmul(kn, ds.transpose(0, 2, 1)), "dk": np.matmul(qn, ds), "dv": np.matmul(g, p)}
    assert all(t.dtype == f for t in res.values())
    return res


# ------------------------------------------------------------------------------------------------------------------ the fp32 arm (torch)
@contextlib.contextmanager
def plain_fp32():
    """torch's own fp32 (no TF32) for the duration of the yardstick's computation"""
    import torch
    saved = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    try:
        yield
    finally:
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = saved


def fp32_arm_torch(q, k, v, g, inv_t=INV_T, need_v=True):
    """plain torch fp32 ops + autograd on the tensors' device: {"out", "dq", "dk"[, "dv"]}"""
    import torch
    with plain_fp32():
        q, k = q.detach().clone().requires_grad_(True), k.detach().clone().requires_grad_(True)
        v = v.detach().clone().requires_grad_(need_v)
        p = torch.softmax(torch.matmul(q.transpose(1, 2), k) * inv_t, dim=-1)
        out = torch.matmul(p, v.transpose(1, 2)).transpose(1, 2)
        out.backward(g)
    res = {"out": out.detach(), "dq": q.grad, "dk": k.grad}
    if need_v:
        res["dv"] = v.grad
    return res
