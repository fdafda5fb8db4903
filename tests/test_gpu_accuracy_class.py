"""Accuracy class of the split-precision (f16x3) kernels on the GPU: every output and gradient is held to the error of the framework's own
fp32 arithmetic on the same inputs (tests/accuracy_case.py: E_kernel <= 4 * max(E_fp32, eps), two metrics, fp64 reference), not to 2e-4.

What each group would catch that the 2e-4 max-norm asserts let through:
    K2 routes, shared keys        a lost or mis-indexed lo plane of q, k, V, dO or dS'' (1.2e-4 .. 3e-4 under the suite's metric), in the
                                  saved-logits and the recompute backward, with and without the P planes / dv GEMM
    semi regime                   a softmax-backward cancellation error in rows that are neither flat nor one-hot
    VALUE_LO_SKIP                 a lo-skip mask that skips a block holding one non-zero lo element
    logits_softmax_warp, match    the same for K7 and for K36a's lse
    hgemm                         a device-side scale that costs bits, a lost A / B plane
    attention                     the magnitude-free flavour (device-side operand scales) at partial tiles
    hot path                      one whole call per match kernel: the chain K1 -> K2 / K19 -> K20 -> heads against torch fp32 of the same chain
Twins ("teeth"): the same launch with an operand's lo plane zeroed (the planes of a slightly different tensor) must MISS the bound at
least twice over — the bound discriminates on the hardware, not only in tests/test_accuracy_class_cpu.py.

Every case prints `ACC_CLASS <kernel> <route> <shape> <regime> <tensor> <metric> E_kernel E_fp32 ratio`; profiles/accuracy_class.txt is one run.
Every case runs inside red zones (guarded_alloc) with the live-buffer check of tests/test_gpu_live_buffers.py on each entry-point call."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy_case as ac  # noqa: E402
from guarded_alloc import guarded  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SPLIT_FWD = "cocos_corr_softmax_warp_fwd_f16x3_ex"
SPLIT_BWD = "cocos_corr_softmax_warp_bwd_query_f16x3_ex"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


@pytest.fixture(autouse=True)
def _split_flavour(monkeypatch):
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    monkeypatch.setattr(ops, "PROJ_PRECISION", "f16x3")


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).requires_grad_(grad)


class _Run:
    """red zones + live-buffer check around one case: `with _Run(monkeypatch) as r: x = r.place(x) ...`; on exit both are asserted"""

    def __init__(self, monkeypatch):
        import test_gpu_live_buffers as lb
        self.live = lb._Guard(monkeypatch)
        self.g = guarded()

    def __enter__(self):
        self.g.__enter__()
        return self

    def place(self, t):
        return self.g.place(t)

    @property
    def entries(self):
        return self.g.entries

    def __exit__(self, et, ev, tb):
        try:
            bad = self.g.check() if et is None else []
        finally:
            self.g.__exit__(et, ev, tb)
        if et is None:
            assert bad == [] and self.g.violations == [], self.g.report()
            self.live.check(1, 1)
        return False


# ---------------------------------------------------------------------------------------------------------------- K2
_K2 = {}


def _k2(c):
    """(inputs fp64, reference fp64, torch-fp32 arm as numpy): once per case, shared, never written"""
    if c not in _K2:
        inp = ac.make_qkv(*c)
        ref = ac.reference(*inp)
        ac.check_regime(c[4], ref["p"])
        arm = ac.fp32_arm_torch(*(dev(t) for t in inp))
        _K2[c] = (inp, ref, {k: v.double().cpu().numpy() for k, v in arm.items()})
    return _K2[c]


def _judge_k2(j, c, got, ref, arm, tensors):
    _, Nq, Nk, _, _ = c
    for t in tensors:
        j.add(t, got[t], arm[t], ref[t], ac.FLOORS[t], excluded=ac.excluded_max(Nq, Nk, t))
    return j


def _run_k2(c, monkeypatch, need_v, train=True, planes=None, recompute=False):
    from cocosnet_amd import ops
    if recompute:
        monkeypatch.setattr(ops, "MAX_SAVED_LOGITS_BYTES", 0)
    (qn, kn, v, g), ref, arm = _k2(c)
    with _Run(monkeypatch) as r:
        q, k, vv, gg = r.place(dev(qn, train)), r.place(dev(kn, train)), r.place(dev(v, train and need_v)), r.place(dev(g))
        pl = planes(ops, q, k) if planes else None
        got = {}
        if train:
            out = ops.corr_softmax_warp(q, k, vv, ac.INV_T, pl)
            out.backward(gg)
            got.update(dq=q.grad, dk=k.grad)
            if need_v:
                got["dv"] = vv.grad
        else:
            with torch.no_grad():
                out = ops.corr_softmax_warp(q, k, vv, ac.INV_T, pl)
        got["out"] = out.detach()
        got = {t: x.double().cpu().numpy() for t, x in got.items()}
        entries = set(r.entries)
    return got, ref, arm, entries


K2_ROUTES = ["forward", "saved", "saved-noV", "recompute", "recompute-noV"]
K2_SPLIT_SAVED = {(64, 64), (256, 128), (384, 384), (8, 8)}
K2_SPLIT_RECOMPUTE = {(256, 128), (384, 384)}


@pytest.mark.parametrize("route", K2_ROUTES)
@pytest.mark.parametrize("c", ac.k2_cases(), ids=ac.case_id)
def test_k2_routes(c, route, monkeypatch):
    """ops.corr_softmax_warp forward only, and differentiated with saved logits / by recomputing them, with the V gradient (P planes + the
    dv GEMM) and without (the theta / phi-only route).  A shape the split backward does not take (Nq or Nk not a multiple of 8; without
    saved logits: Nk % 128, Nq % 32) runs the exact-fp32 kernels when differentiated — the route column says which ran — and is held to
    the same bound."""
    from cocosnet_amd import ops
    B, Nq, Nk, Cv, regime = c
    train, need_v, recompute = route != "forward", not route.endswith("noV") and route != "forward", route.startswith("recompute")
    with ops.KernelTimer(tags=("corr_softmax_warp_recompute",)) as kt:
        got, ref, arm, entries = _run_k2(c, monkeypatch, need_v, train, recompute=recompute)
    split = SPLIT_FWD in entries
    # the expected route, pinned here (not asked of the code under test): the split forward takes every shape of the table; the split
    # backward the four with Nq and Nk multiples of 8, by recomputing only the two with Nk % 128 == 0 and Nq % 32 == 0
    want = not train or (Nq, Nk) in (K2_SPLIT_RECOMPUTE if recompute else K2_SPLIT_SAVED)
    assert split == want and (not train or (SPLIT_BWD in entries) == want), sorted(entries)
    n_recompute = kt.summary().get("corr_softmax_warp_recompute", {}).get("calls", 0)
    assert (n_recompute >= 1) == (split and recompute), (route, n_recompute)
    if split and recompute:
        assert ops._saves_logits(B, Nq, Nk) is False
    j = ac.Judge("corr_softmax_warp", f"{route}:{'f16x3' if split else 'fp32-kernels'}", c[:4], regime)
    _judge_k2(j, c, got, ref, arm, [t for t in ("out", "dq", "dk", "dv") if t in got]).assert_in_class()


def _twin_planes(zero):
    """OperandPlanes filled by hand: the kernel's own split of q / k in both orientations, the lo plane of `zero` = (operand, transposed)
    replaced by zeros"""
    def make(ops, q, k):
        pl = ops.OperandPlanes()
        for name, x in (("q", q), ("k", k)):
            for transposed in (True, False):
                hi, lo = ops.split_f16(x, transposed, ops.SPLIT_OPERAND_SCALE)
                pl.put(x, transposed, ops.SPLIT_OPERAND_SCALE, hi, torch.zeros_like(lo) if (name, transposed) == zero else lo)
        return pl
    return make


#: twin -> ((operand, position-major?), the tensors it feeds in the saved-logits route): the position-major planes make the logits
#: (everything follows), k's channel-major planes are the B operand of d qn, q's the A operand of the key GEMM
K2_TWINS = {"k-lo-logits": (("k", True), ("out", "dq", "dk", "dv")), "q-lo-logits": (("q", True), ("out", "dq", "dk", "dv")),
            "k-lo-dqn": (("k", False), ("dq",)), "q-lo-keygemm": (("q", False), ("dk",))}
K2_TRAIN_SPLIT = [c for c in ac.k2_cases() if c[1] % 8 == 0 and c[2] % 8 == 0]


@pytest.mark.parametrize("twin", ["intact"] + sorted(K2_TWINS))
@pytest.mark.parametrize("c", K2_TRAIN_SPLIT, ids=ac.case_id)
def test_k2_lost_plane_twins(c, twin, monkeypatch):
    """the saved-logits route on hand-made operand planes: intact they are in class (the harness hands over what the op would make);
    with one lo plane zeroed the tensors it feeds miss the bound at least TEETH times, the others stay in class"""
    zero, damaged = K2_TWINS.get(twin, (None, ()))
    got, ref, arm, entries = _run_k2(c, monkeypatch, True, planes=_twin_planes(zero))
    assert SPLIT_FWD in entries and SPLIT_BWD in entries
    j = ac.Judge("corr_softmax_warp", f"twin:{twin}", c[:4], c[4])
    _judge_k2(j, c, got, ref, arm, ("out", "dq", "dk", "dv"))
    if twin == "intact":
        j.assert_in_class()
        return
    j.assert_out_of_class(damaged)
    for t in set(("out", "dq", "dk", "dv")) - set(damaged):
        assert j.over(t) <= 1.0, (twin, t, j.over(t))


@pytest.mark.parametrize("c", [c for c in ac.k2_cases() if c[2] % 4 == 0 and (c[1] % 8 or c[2] % 8)], ids=ac.case_id)
def test_k2_forward_lost_plane_twin(c, monkeypatch):
    """the shapes only the split FORWARD takes: k's lo plane zeroed in the logits"""
    got, ref, arm, entries = _run_k2(c, monkeypatch, False, train=False, planes=_twin_planes(("k", True)))
    assert SPLIT_FWD in entries
    j = ac.Judge("corr_softmax_warp", "twin:k-lo-logits:forward", c[:4], c[4])
    _judge_k2(j, c, got, ref, arm, ("out",)).assert_out_of_class(("out",))


# ---------------------------------------------------------------------------------------------------------------- shared keys / values
def _shared_reference(c, Be):
    (qn, kn, v, g), ref, arm = _k2(c)
    if Be != 1:
        return (qn, kn, v), ref["out"], arm["out"]
    kn1, v1 = np.repeat(kn[:1], c[0], axis=0), np.repeat(v[:1], c[0], axis=0)
    a = ac.fp32_arm_torch(dev(qn), dev(kn1), dev(v1), dev(g))["out"].double().cpu().numpy()
    return (qn, kn[:1], v[:1]), ac.reference(qn, kn1, v1, g)["out"], a


SHARED_TWINS = {"intact": None, "V-lo": "v", "K-lo": "k", "lo-mask-all-skipped": "mask"}


#: (the lo-skip mask exists above 32 value channels only: the mask twin is made for those cases)
SHARED_CASES = [(c, Be, twin) for c in ac.k2_cases() if c[2] % 4 == 0 for Be in ("dense", "one") for twin in SHARED_TWINS
                if twin != "lo-mask-all-skipped" or c[3] > 32]


@pytest.mark.parametrize("c,Be,twin", SHARED_CASES, ids=lambda x: ac.case_id(x) if isinstance(x, tuple) else x)
def test_shared_keys_and_values(c, Be, twin, monkeypatch):
    """ops.corr_softmax_warp_shared with PreparedKeys / PreparedValues (batch B, and ONE exemplar read by every query batch), and its twins:
    V's lo plane zeroed, K's lo plane zeroed, and a lo-skip mask that claims every block's lo plane is zero while it is not"""
    from cocosnet_amd import ops
    B, Nq, Nk, Cv, regime = c
    (qn, kn, v), ref, arm = _shared_reference(c, 1 if Be == "one" else B)
    with _Run(monkeypatch) as r, torch.no_grad():
        q, k, vv = r.place(dev(qn)), r.place(dev(kn)), r.place(dev(v))
        qh, ql = ops.split_f16(q, True, ops.SPLIT_OPERAND_SCALE)
        kh, kl = ops.split_f16(k, True, ops.SPLIT_OPERAND_SCALE)
        if SHARED_TWINS[twin] == "k":
            kl = torch.zeros_like(kl)
        keys = ops.PreparedKeys(Be=k.shape[0], shape=(k.shape[0], 256, 1, Nk), image_size=(1, Nk), make_phi_raw=None,
                                make_split=lambda: (kh, kl, None), make_box=None, make_values=None)
        values = ops.PreparedValues(vv, 0)
        vh, vl, vs, mask = values.split()
        assert (mask is not None) == (Cv > 32)
        if SHARED_TWINS[twin] == "v":
            values._split = (vh, torch.zeros_like(vl), vs, mask)
        elif SHARED_TWINS[twin] == "mask":
            assert int(mask.view(torch.int32)) != 0
            values._split = (vh, vl, vs, torch.zeros(1, device=DEV, dtype=torch.float32))
        out = ops.corr_softmax_warp_shared(qh, ql, keys, values, ac.INV_T).double().cpu().numpy()
        assert "cocos_corr_softmax_warp_fwd_f16x3_shared" in r.entries
    j = ac.Judge("corr_softmax_warp_shared", f"{Be}:{twin}", c[:4], regime).add("out", out, arm, ref)
    if twin == "intact":
        j.assert_in_class()
    else:
        j.assert_out_of_class(("out",))


# ---------------------------------------------------------------------------------------------------------------- VALUE_LO_SKIP
#: fp32-exact, and halfway between two f16 values after the device-side scale 2^9 (max|v| = 1): the largest lo-plane element there is
ODD_ONE = 153.5625 / 512.0


def _label_values(c, kind, p):
    """V [B,Cv,Nk]: channels 0..2 an image in (-1, 1), the rest one-hot labels (exact in f16: their lo plane is zero).  kind "one-odd":
    ALL channels labels, except ONE element of the second 32-channel block — at the key with the largest weight in the reference P"""
    B, Nq, Nk, Cv, _ = c
    rs = np.random.RandomState(Cv + Nk)
    lab = rs.randint(0, Cv - 3, (B, Nk))
    v = np.zeros((B, Cv, Nk))
    if kind == "labels":
        v[:, :3] = rs.uniform(-1, 1, (B, 3, Nk))
        np.put_along_axis(v[:, 3:], lab[:, None], 1.0, axis=1)
        return ac.as_f32(v), None
    np.put_along_axis(v, rs.randint(0, Cv, (B, 1, Nk)), 1.0, axis=1)
    b, i, jk = np.unravel_index(np.argmax(p), p.shape)
    v[b, 35, jk] = ODD_ONE
    return v, (b, 35, i)


@pytest.mark.parametrize("kind", ["labels", "one-odd"])
@pytest.mark.parametrize("c", [(2, 384, 384, 40, "semi"), (2, 256, 128, 154, "diffuse")], ids=ac.case_id)
def test_value_lo_skip(c, kind, monkeypatch):
    """labels: the mask says "only block 0 has a lo plane" and the skipped blocks lose nothing.  one-odd: the mask must keep the block with
    the single non-zero lo element — skipping it costs p * 2^-13 at that query's column (judged by rel_slice), 3x the bound at p ~ 0.9"""
    from cocosnet_amd import ops
    assert ops.VALUE_LO_SKIP
    B, Nq, Nk, Cv, regime = c
    (qn, kn, _, g), ref0, _ = _k2(c)
    v, odd = _label_values(c, kind, ref0["p"])
    ref = ac.reference(qn, kn, v, g)
    arm = {t: x.double().cpu().numpy() for t, x in ac.fp32_arm_torch(dev(qn), dev(kn), dev(v), dev(g), need_v=False).items()}
    with _Run(monkeypatch) as r:
        q, k, vv, gg = r.place(dev(qn, True)), r.place(dev(kn, True)), r.place(dev(v)), r.place(dev(g))
        _, lo, _, mask = ops.split_f16_chan_mask(vv, ops.absmax(vv), True)
        bits = int(mask.view(torch.int32))
        assert bits == (1 if kind == "labels" else 2), bin(bits)
        assert int((lo != 0).sum()) == (1 if kind == "one-odd" else int((lo[:, :3] != 0).sum()))
        out = ops.corr_softmax_warp(q, k, vv, ac.INV_T)
        out.backward(gg)
        got = {"out": out.detach(), "dq": q.grad, "dk": k.grad}
        assert SPLIT_FWD in r.entries and SPLIT_BWD in r.entries
    j = ac.Judge("corr_softmax_warp", f"lo-skip:{kind}", c[:4], regime)
    _judge_k2(j, c, got, ref, arm, ("out", "dq", "dk")).assert_in_class()
    if odd is not None:      # the one element itself: its lo part reaches the output
        b, ch, i = odd
        lo_part = abs(ODD_ONE - float(np.float16(ODD_ONE * 512.0)) / 512.0) * ref0["p"][b, i].max()
        err = abs(float(got["out"][b, ch, i]) - ref["out"][b, ch, i])
        print(f"{j.head} out[{b},{ch},{i}]: error {err:.3e}, the element's lo part there {lo_part:.3e}")
        assert err <= lo_part / 4


# ---------------------------------------------------------------------------------------------------------------- K7
@pytest.mark.parametrize("c", ac.k2_cases(), ids=ac.case_id)
def test_logits_softmax_warp(c, monkeypatch):
    """ops.logits_softmax_warp on the K2 cases' own logits (fp32-rounded 100 * cos), key-major: out, d logits, d v.  With exact logits
    the framework's arm is at 1e-7 .. 4e-7 and K7's log2-domain row statistics cost 1e-6 .. 3e-6 in P: the kernel carries its own measured
    factors, accuracy_case.K7_FACTORS (reason and figures there); a lost plane still misses them at least fourfold (the CPU test).
    The `torch-fp32-log2-domain` lines are the measurement behind the reason: torch fp32 with the kernel's row statistics."""
    from cocosnet_amd import ops
    B, Nq, Nk, Cv, regime = c
    (qn, kn, v, g), _, _ = _k2(c)
    f, ref = ac.k7_reference(qn, kn, v, g)
    ac.check_regime(regime, ref["p"])
    with ac.plain_fp32():
        lt, vd = dev(f.transpose(0, 2, 1), True), dev(v, True)
        o = torch.matmul(torch.softmax(lt.transpose(1, 2), dim=-1), vd.transpose(1, 2)).transpose(1, 2)
        o.backward(dev(g))
    arm = {"out": o.detach(), "dlogits_t": lt.grad, "dv": vd.grad}
    with _Run(monkeypatch) as r:
        lt2, v2, gg = r.place(dev(f.transpose(0, 2, 1), True)), r.place(dev(v, True)), r.place(dev(g))
        out = ops.logits_softmax_warp(lt2, v2)
        out.backward(gg)
        got = {"out": out.detach(), "dlogits_t": lt2.grad, "dv": v2.grad}
        flavour = "f16x3" if any("logits_softmax_warp" in e and "f16x3" in e for e in r.entries) else "fp32-kernels"
    # the measurement behind K7_FACTORS' reason: torch fp32 with the kernel's row statistics (log2 domain, lse saved, P rebuilt from it)
    with ac.plain_fp32(), torch.no_grad():
        log2e, ln2 = 1.4426950408889634, 0.6931471805599453
        l, vv, gg2 = dev(f), dev(v), dev(g)
        x = l * log2e
        m = x.max(dim=-1, keepdim=True).values
        lse = (m + torch.log2(torch.exp2(x - m).sum(dim=-1, keepdim=True))) * ln2
        pk = torch.exp2(l * log2e - lse * log2e)
        dpk = torch.matmul(gg2.transpose(1, 2), vv)
        outk = torch.matmul(pk, vv.transpose(1, 2)).transpose(1, 2)
        D = (gg2 * outk).sum(dim=1).unsqueeze(-1)
        log2_arm = {"out": outk, "dlogits_t": (pk * (dpk - D)).transpose(1, 2), "dv": torch.matmul(gg2, pk)}
    jl = ac.Judge("logits_softmax_warp", "torch-fp32-log2-domain", c[:4], regime)
    for t, floor in ac.K7_FLOORS.items():
        jl.add(t, log2_arm[t], arm[t], ref[t], floor, excluded=ac.excluded_max(Nq, Nk, t))
    j = ac.Judge("logits_softmax_warp", flavour, c[:4], regime)
    # floors: the suite's (tests/test_gpu_parity.py: 1e-3 for d logits); d logits' slices are query columns (over the keys)
    for t, floor in ac.K7_FLOORS.items():
        j.add(t, got[t], arm[t], ref[t], floor, factor=ac.K7_FACTORS, excluded=ac.excluded_max(Nq, Nk, t))
    j.assert_in_class()


# ---------------------------------------------------------------------------------------------------------------- K36a: lse
@pytest.mark.parametrize("twin", ["intact", "k-lo"])
@pytest.mark.parametrize("c", [c for c in ac.k2_cases() if c[2] % 4 == 0], ids=ac.case_id)
def test_corr_match_lse(c, twin, monkeypatch):
    """ops.corr_match's row log-sum-exp against logsumexp of the fp64 logits; the arm is torch.logsumexp of the fp32 matmul"""
    from cocosnet_amd import ops
    (qn, kn, _, _), ref, _ = _k2(c)
    want = np.log(np.exp(ac.co.correlation(qn, kn) * ac.INV_T - 100.0).sum(-1)) + 100.0
    with ac.plain_fp32(), torch.no_grad():
        arm = torch.logsumexp(torch.matmul(dev(qn).transpose(1, 2), dev(kn)) * ac.INV_T, dim=-1)
    with _Run(monkeypatch) as r, torch.no_grad():
        q, k = r.place(dev(qn)), r.place(dev(kn))
        pl = _twin_planes(("k", True) if twin == "k-lo" else None)(ops, q, k)
        _, _, lse = ops.corr_match(q, k, ac.INV_T, pl)
        assert "cocos_corr_match_f16x3" in r.entries
    j = ac.Judge("corr_match", f"lse:{twin}", c[:4], c[4]).add("lse", lse, arm, want)
    if twin == "intact":
        j.assert_in_class()
    else:
        j.assert_out_of_class(("lse",))


# ---------------------------------------------------------------------------------------------------------------- the split GEMM
@pytest.mark.parametrize("twin", ["intact", "A-lo", "B-lo"])
@pytest.mark.parametrize("batch,M,N,Kr", [(2, 256, 128, 64), (1, 100, 70, 40), (2, 300, 200, 8)])
def test_hgemm_planes(batch, M, N, Kr, twin, monkeypatch):
    """cocos_hgemm_f16x3 through the ABI (host scale and a device-side scale cell, as tests/test_gpu_parity.py calls it): C = A B^T"""
    from cocosnet_amd import _lib, ops
    rs = np.random.RandomState(M + Kr)
    a, b = ac.as_f32(rs.standard_normal((batch, M, Kr))), ac.as_f32(rs.standard_normal((batch, N, Kr)))
    ref = np.einsum("bmk,bnk->bmn", a, b)
    with ac.plain_fp32():
        arm = torch.matmul(dev(a), dev(b).transpose(1, 2))
    with _Run(monkeypatch) as r:
        ad, bd = r.place(dev(a)), r.place(dev(b))
        ah, al = ops.split_f16(ad, False, 4.0)
        bh, bl = ops.split_f16(bd, False, 2.0)
        if twin == "A-lo":
            al = torch.zeros_like(al)
        if twin == "B-lo":
            bl = torch.zeros_like(bl)
        cc = torch.empty((batch, M, N), device=DEV, dtype=torch.float32)
        sc = torch.full((1,), 2.0, device=DEV)
        _lib.call("cocos_hgemm_f16x3", ah.data_ptr(), al.data_ptr(), bh.data_ptr(), bl.data_ptr(), cc.data_ptr(), batch, M, N, Kr,
                  0.25, sc.data_ptr(), 0, 0, torch.cuda.current_stream().cuda_stream)
        got = cc.double().cpu().numpy()
    # [B, M, N]: a slice is an output column n (over m)
    j = ac.Judge("hgemm_f16x3", twin, (batch, M, N, Kr), "normal").add("c", got, arm, ref)
    if twin == "intact":
        j.assert_in_class()
    else:
        j.assert_out_of_class(("c",))


# ---------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("B,Kc,Nq,Nk,Cv", [(2, 32, 132, 68, 16), (1, 64, 513, 129, 8), (2, 64, 136, 72, 40)])
def test_softmax_attention(B, Kc, Nq, Nk, Cv, monkeypatch):
    """ops.softmax_attention, raw (not unit-norm) q / k with K < 256: the fused magnitude-free flavour where it takes the shape, the
    materialised family elsewhere (partial tiles either way); out and the three gradients"""
    from cocosnet_amd import ops
    rs = np.random.RandomState(Nq + Nk)
    q, k = ac.as_f32(rs.standard_normal((B, Kc, Nq)) * 1.5 * (32.0 / Kc) ** 0.5), ac.as_f32(rs.standard_normal((B, Kc, Nk)) * 0.7 + 0.1)
    v, g = ac.as_f32(rs.standard_normal((B, Cv, Nk))), ac.as_f32(rs.standard_normal((B, Cv, Nq)))
    ref = ac.reference(q, k, v, g, 1.0)
    arm = {t: x.double().cpu().numpy() for t, x in ac.fp32_arm_torch(dev(q), dev(k), dev(v), dev(g), 1.0).items()}
    with _Run(monkeypatch) as r:
        qd, kd, vd, gd = r.place(dev(q, True)), r.place(dev(k, True)), r.place(dev(v, True)), r.place(dev(g))
        out = ops.softmax_attention(qd, kd, vd, 1.0)
        out.backward(gd)
        got = {"out": out.detach(), "dq": qd.grad, "dk": kd.grad, "dv": vd.grad}
        fused = SPLIT_FWD in r.entries
    assert fused == (Nq % 8 == 0 and Nk % 8 == 0)
    j = ac.Judge("softmax_attention", "fused" if fused else "materialised", (B, Kc, Nq, Nk, Cv), "raw")
    for t in ("out", "dq", "dk", "dv"):
        j.add(t, got[t], arm[t], ref[t])
    j.assert_in_class()


# ---------------------------------------------------------------------------------------------------------------- one whole call
def _hot_path_inputs(fh, fw, seed, couple=0.05):
    """theta / phi as tests/test_gpu_parity.py builds them for the hot path (both far from unit norm), with a weaker copy of theta in
    phi: with 0.2 a quarter of the match_kernel-1 rows are one-hot and their d theta columns fall below SLICE_MIN"""
    rs = np.random.RandomState(seed)
    B, nc, down = 2, 6, 4
    theta = rs.standard_normal((B, 256, fh, fw))
    perm = rs.permutation(fh * fw)
    phi = couple * theta.reshape(B, 256, -1)[:, :, perm].reshape(theta.shape) + rs.standard_normal(theta.shape) + 0.1
    theta, phi = ac.as_f32(theta * 3.0 + 0.5), ac.as_f32(phi * 2.0 - 0.3)
    img = ac.as_f32(rs.uniform(-1, 1, (B, 3, fh * down, fw * down)))
    lab = rs.randint(0, nc, (B, fh * down, fw * down))
    seg = (lab[:, None] == np.arange(nc)[None, :, None, None]).astype(np.float64)
    G = {"warp_out": ac.as_f32(rs.standard_normal(img.shape)), "warp_mask": ac.as_f32(rs.standard_normal((B, nc, fh, fw)))}
    return theta, phi, img, seg, G


@pytest.mark.parametrize("mk,fh,fw,fused", [(1, 16, 16, True), (3, 4, 64, True), (3, 7, 9, False)],
                         ids=["mk1-16x16", "mk3-4x64-fused", "mk3-7x9-BOX3_FUSED-off"])
def test_whole_hot_path_call(mk, fh, fw, fused, monkeypatch):
    """correspondence_hot_path: warp_out, warp_mask, d theta, d phi against torch fp64 of the reference's formulation; the arm is the same
    torch code in fp32 on the device (match_kernel 3: the unfolded K = 2304 formulation)"""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_hot_path
    from oracle import torch_ref as tr
    monkeypatch.setattr(ops, "BOX3_FUSED", fused)
    if mk == 3 and fused:
        assert ops.box3_fused_ok(2, 256, fh, fw, 9)
    theta, phi, img, seg, G = _hot_path_inputs(fh, fw, 5 + mk)
    flags = dict(match_kernel=mk, PONO_C=True, down=4, warp_mask_losstype="direct", isTrain=True)
    opt = ac.co.default_opt(**flags)
    ref, dth, dph = tr.forward_backward(theta, phi, img, img, seg, seg, opt, G, device=DEV)
    with ac.plain_fp32():
        a_out, a_dth, a_dph = tr.forward_backward(theta, phi, img, img, seg, seg, opt, G, dtype=torch.float32, device=DEV)
    with _Run(monkeypatch) as r:
        th, ph = r.place(dev(theta, True)), r.place(dev(phi, True))
        im, sg = r.place(dev(img)), r.place(dev(seg))
        out = correspondence_hot_path(th, ph, im, im, sg, sg, HotPathConfig(**flags))
        torch.autograd.backward([out["warp_out"], out["warp_mask"]], [r.place(dev(G["warp_out"])), r.place(dev(G["warp_mask"]))])
        got = {"warp_out": out["warp_out"].detach(), "warp_mask": out["warp_mask"].detach(), "dtheta": th.grad, "dphi": ph.grad}
        got = {t: x.double().cpu().numpy() for t, x in got.items()}
    want = {"warp_out": ref["warp_out"], "warp_mask": ref["warp_mask"], "dtheta": dth, "dphi": dph}
    arm = {"warp_out": a_out["warp_out"], "warp_mask": a_out["warp_mask"], "dtheta": a_dth, "dphi": a_dph}
    flat = lambda x: np.asarray(x, dtype=np.float64).reshape(x.shape[0], x.shape[1], -1)
    j = ac.Judge("correspondence_hot_path", f"mk{mk}:{'fused' if fused else 'fallback'}", (2, fh, fw), "mixed")
    for t in want:
        j.add(t, flat(got[t]), flat(arm[t]), flat(want[t]))
    j.assert_in_class()


# ---------------------------------------------------------------------------------------------------------------- generic op cases
def _as3(x):
    """[B, C, positions] for the slice metric: images flattened, a weight [Cout, Cin, 1, 1] as one sample of Cin columns.  A bias
    gradient [Cout] has no position axis: it is ONE slice (rel_slice == rel_max) — judged element by element, an entry that cancels to
    1e-3 of the largest would carry 1000 x the rounding of its sum over B * N terms, in the arm and in the kernel alike, and the ratio of
    two such numbers is noise (measured at Cin = 5: 3.2e-5 against 4.4e-6 on one entry, rel_max 1.1)"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 4 and x.shape[2:] == (1, 1):
        return x.reshape(1, x.shape[0], x.shape[1])
    if x.ndim == 4:
        return x.reshape(x.shape[0], x.shape[1], -1)
    return x.reshape(1, -1, 1) if x.ndim == 1 else x


def _torch_arms(ref, inputs, seed):
    """`ref(t) -> [outputs]` in plain torch on `inputs` {name: CPU fp64 tensor}: run in fp64 (the reference) and in fp32 (the arm) on the
    device, differentiated with the same random cotangents -> (G, {dtype: (outputs, {name: gradient})})"""
    res, G = {}, None
    for dtype in (torch.float64, torch.float32):
        t = {k: v.detach().to(DEV, dtype).clone().requires_grad_(True) for k, v in inputs.items()}
        with ac.plain_fp32():
            outs = ref(t)
            if G is None:
                gen = torch.Generator().manual_seed(seed)
                G = [torch.randn(o.shape, generator=gen, dtype=torch.float64).float().double().to(DEV) for o in outs]
            torch.autograd.backward(outs, [g.to(dtype) for g in G])
        res[dtype] = ([o.detach().double().cpu().numpy() for o in outs], {k: t[k].grad.double().cpu().numpy() for k in t})
    return G, res


def _judge_op(j, fn, ref, inputs, out_names, monkeypatch, seed=1, factor=ac.FACTOR, floors=None):
    """kernel `fn(t) -> [outputs]` on guarded copies of `inputs`, every output and every input gradient judged against the torch arms"""
    floors = floors or {}
    G, arms = _torch_arms(ref, inputs, seed)
    with _Run(monkeypatch) as r:
        t = {k: r.place(v.detach().to(DEV, torch.float32).clone().requires_grad_(True)) for k, v in inputs.items()}
        outs = fn(t)
        torch.autograd.backward(outs, [r.place(g.float()) for g in G])
        got_o = [o.detach().double().cpu().numpy() for o in outs]
        got_g = {k: t[k].grad.double().cpu().numpy() for k in t}
        entries = set(r.entries)
    (ref_o, ref_g), (arm_o, arm_g) = arms[torch.float64], arms[torch.float32]
    for i, name in enumerate(out_names):
        j.add(name, _as3(got_o[i]), _as3(arm_o[i]), _as3(ref_o[i]), floors.get(name, 0.0), factor=factor)
    for k in inputs:
        j.add("d" + k, _as3(got_g[k]), _as3(arm_g[k]), _as3(ref_g[k]), floors.get("d" + k, 0.0), factor=factor)
    return entries


def _rs_t(rs, *shape, scale=1.0, shift=0.0):
    return torch.from_numpy(ac.as_f32(rs.standard_normal(shape) * scale + shift))


# ---------------------------------------------------------------------------------------------------------------- K23 / K24 / dW
def proj_pair_case(Cin, h, w, B=2):
    """the fused projections of both sides: x [B,Cin,h,w], W [256,Cin,1,1], b [256] each; phi's input a weak copy of theta's"""
    rs = np.random.RandomState(Cin + h * w)
    x1 = _rs_t(rs, B, Cin, h, w)
    inputs = dict(x_theta=x1, w_theta=_rs_t(rs, 256, Cin, 1, 1, scale=Cin ** -0.5), b_theta=_rs_t(rs, 256, scale=0.1),
                  x_phi=torch.from_numpy(ac.as_f32((0.3 * x1 + _rs_t(rs, B, Cin, h, w)).numpy())),
                  w_phi=_rs_t(rs, 256, Cin, 1, 1, scale=Cin ** -0.5), b_phi=_rs_t(rs, 256, scale=0.1))

    def ref(t):
        res = []
        for side in ("theta", "phi"):
            th = torch.nn.functional.conv2d(t["x_" + side], t["w_" + side], t["b_" + side]).reshape(B, 256, h * w)
            thc = th - th.mean(dim=1, keepdim=True)
            res.append(thc / (thc.norm(dim=1, keepdim=True) + ac.co.EPS))
        return res
    return inputs, ref


@pytest.mark.parametrize("fused_bwd", [True, False], ids=["K24", "chain-bwd"])
@pytest.mark.parametrize("h,w", [(8, 16), (16, 24)], ids=["N128", "N384"])
@pytest.mark.parametrize("Cin", [5, 271, 407])
def test_fused_projection_pair(Cin, h, w, fused_bwd, monkeypatch):
    """ops.proj_center_l2norm_planes_pair, forward (K23: the normalised planes, read back as (hi + lo) / scale) and backward (K24 or the
    chain, and the dW kernel): qn, kn, and dx, dW, db of both projections"""
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "PROJ_BWD_FUSED", fused_bwd)
    inputs, ref = proj_pair_case(Cin, h, w)
    S = ops.SPLIT_OPERAND_SCALE
    seen = {}

    def fn(t):
        planes = ops.OperandPlanes()
        lazy = lambda side: ops.LazyProj1x1(t["x_" + side], t["w_" + side], t["b_" + side])
        qn, kn = ops.proj_center_l2norm_planes_pair(lazy("theta"), lazy("phi"), 1, planes, want_chan=True)
        for name, hd in (("qn", qn), ("kn", kn)):
            ph, pl = planes.get(hd, True, S)
            seen[name] = ((ph.double() + pl.double()) / S).transpose(1, 2)
        return [qn, kn]

    j = ac.Judge("proj_center_l2norm_planes_pair", "K24" if fused_bwd else "chain-bwd", (2, Cin, h, w), "normal")
    G, arms = _torch_arms(ref, inputs, 1)
    with _Run(monkeypatch) as r:
        t = {k: r.place(v.detach().to(DEV, torch.float32).clone().requires_grad_(True)) for k, v in inputs.items()}
        outs = fn(t)
        torch.autograd.backward(outs, [r.place(g.float()) for g in G])
        got_g = {k: t[k].grad.double().cpu().numpy() for k in t}
    (ref_o, ref_g), (arm_o, arm_g) = arms[torch.float64], arms[torch.float32]
    for i, name in enumerate(("qn", "kn")):
        j.add(name, seen[name].cpu().numpy(), arm_o[i], ref_o[i])
    for k in inputs:
        j.add("d" + k, _as3(got_g[k]), _as3(arm_g[k]), _as3(ref_g[k]))
    j.assert_in_class()


# ---------------------------------------------------------------------------------------------------------------- K12 / K19 / K20
def box3_case(fh, fw, B=1, Cv=5):
    """match_kernel 3 on raw features: q, k [B,256,fh,fw] (k a weak copy: the nine-tap match saturates the softmax otherwise), v"""
    rs = np.random.RandomState(100 + fh)
    q = _rs_t(rs, B, 256, fh, fw, shift=0.15)
    k = torch.from_numpy(ac.as_f32((0.05 * q.roll((1, 5), (2, 3)) + _rs_t(rs, B, 256, fh, fw, shift=-0.1)).numpy()))
    v = torch.from_numpy(ac.as_f32(rs.uniform(-1, 1, (B, Cv, fh * fw))))

    def ref(t):
        def unit(x):
            u = torch.nn.functional.unfold(x, 3, padding=1)
            u = u - u.mean(dim=1, keepdim=True)
            return u / (u.norm(dim=1, keepdim=True) + ac.co.EPS)
        z = ac.INV_T * torch.einsum("bcp,bcq->bpq", unit(t["q"]), unit(t["k"]))
        return [torch.einsum("bpq,bcq->bcp", torch.softmax(z, dim=2), t["v"])]
    return dict(q=q, k=k, v=v), ref


@pytest.mark.parametrize("fh", [4, 8])
def test_box3_family_fused(fh, monkeypatch):
    """unfold3_stats -> box3_corr_xbox -> box3_softmax_warp (K12, K19, K20), forward and backward through all three, at the two smallest
    grids the fused family takes (4 x 64, 8 x 64); reference and arm: the unfolded K = 2304 formulation in torch"""
    from cocosnet_amd import ops
    fw, kc = 64, 256.0 * 9
    assert ops.box3_fused_ok(1, 256, fh, fw, 5) and not ops.box3_fused_ok(1, 256, 2, 64, 5)
    inputs, ref = box3_case(fh, fw)

    def fn(t):
        (mu, a), (nu, b) = ops.unfold3_stats(t["q"], kc), ops.unfold3_stats(t["k"], kc)
        sink = ops.Box3GradSink()
        T = ops.box3_corr_xbox(t["q"], t["k"], sink)
        return [ops.box3_softmax_warp(T, mu, a, nu, b, t["v"], fh, fw, kc, ac.INV_T, False, sink)]
    j = ac.Judge("box3_family", "fused", (1, fh, fw, 5), "weak-copy")
    entries = _judge_op(j, fn, ref, inputs, ("out",), monkeypatch)
    assert any("box3_softmax_warp_bwd" in e for e in entries), sorted(entries)
    j.assert_in_class()


def test_box3_family_fallback_ragged(monkeypatch):
    """BOX3_FUSED off at a ragged 7 x 9 grid: the materialised box logits (K6 + K12) -> logits_softmax_warp (K7), forward and backward.
    K7 runs behind a product here, so the plain factor applies."""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, _scaled_logits
    monkeypatch.setattr(ops, "BOX3_FUSED", False)
    fh, fw = 7, 9
    inputs, ref = box3_case(fh, fw, B=2)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True)

    def fn(t):
        f = _scaled_logits(t["q"], t["k"], cfg, ac.INV_T, False, 1)
        return [ops.logits_softmax_warp(f.transpose(1, 2).contiguous(), t["v"])]
    j = ac.Judge("box3_family", "fallback", (2, fh, fw, 5), "weak-copy")
    _judge_op(j, fn, ref, inputs, ("out",), monkeypatch)
    j.assert_in_class()


# ---------------------------------------------------------------------------------------------------------------- K22 / K15
def contextual_case(B, C, Nq, Nk):
    rs = np.random.RandomState(Nq + Nk)
    nrm = lambda x: torch.from_numpy(ac.as_f32((x / (x.norm(dim=1, keepdim=True) + 2.2e-16)).numpy()))
    return dict(xn=nrm(_rs_t(rs, B, C, Nq)), yn=nrm(_rs_t(rs, B, C, Nk)))


@pytest.mark.parametrize("route", ["fused", "materialised"])
@pytest.mark.parametrize("B,C,Nq,Nk,h", [(2, 40, 132, 68, 0.1), (1, 64, 513, 129, 0.5)])
def test_contextual_cx(B, C, Nq, Nk, h, route, monkeypatch):
    """ops.contextual_cx (K22, nothing [Nq, Nk]) and the materialised route (the cosine GEMM + ops.contextual_rows, K15) at partial tiles:
    cx and both gradients against oracle/contextual_ref.py in torch fp64; the arm is the same code in fp32"""
    from cocosnet_amd import ops
    from oracle import contextual_ref as cr
    inputs = contextual_case(B, C, Nq, Nk)
    ref = lambda t: [cr.cx_rows(t["xn"], t["yn"], h, 1e-3)]
    if route == "fused":
        fn = lambda t: [ops.contextual_cx(t["xn"], t["yn"], h, 1e-3)]
    else:
        fn = lambda t: [ops.contextual_rows(ops.corr_materialize(t["xn"], t["yn"], 1.0), h, 1e-3)]
    j = ac.Judge("contextual_cx", route, (B, C, Nq, Nk, h), "normal")
    entries = _judge_op(j, fn, ref, inputs, ("cx",), monkeypatch)
    assert ("cocos_contextual_cx_fwd_f16x3" in entries) == (route == "fused"), sorted(entries)
    j.assert_in_class()
