"""K53 on the GPU: cocos_box3_lse_bwd_f16x3 alone, ops.box3_lse / ops.box3_pair_logits / ops.box3_gather_keys,
hot_path.correspondence_nll_box3 and NoVGGCorrespondence.match_loss_box3 — the supervised match loss on the match_kernel-3 route.

The reference is tests/match_box3_nll_case.py's `arbiter` in torch fp64 (F.unfold -> centre -> normalise -> dot -> logsumexp over each
axis -> gather, gradients from autograd; evaluated on the device, in fp64).  Bounds are tests/test_gpu_parity.py's (imported): OUT_TOL =
2e-4 on outputs, GRAD_TOL = 1e-3 on gradients, its `rel` measure (max error over max reference).

Shapes: B = 2 on 4 x 64 and 2 x 128 (the smallest 64- and 128-wide grids cocos_box3_fused_supported takes: every cell is a y-border
cell), B = 2 on 64 x 64, B = 1 on 40 x 128 (5120 keys: the statistics ring and the 128-wide halo).

The file name sorts before test_gpu_red_zones.py: its red-zone case has run when that file's audit is collected."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_box3_nll_case as mc  # noqa: E402
import test_gpu_red_zones as rz  # noqa: E402
from test_gpu_live_buffers import _Guard  # noqa: E402
from test_gpu_match_box3 import TOL as BOX_LSE_TOL  # noqa: E402  (the readout's recorded lse tolerance at inv_t = 100)
from test_gpu_parity import GRAD_TOL, OUT_TOL, rel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KC = 9 * 256.0
SHAPES = [(2, 4, 64), (2, 2, 128), (2, 64, 64), (1, 40, 128)]
SMALL = [(2, 4, 64), (2, 2, 128)]
NEW_ENTRIES = {"cocos_box3_lse_bwd_f16x3", "cocos_box3_pair_logit_fwd", "cocos_box3_pair_logit_bwd_pair"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


@contextlib.contextmanager
def _poisoned_empty():
    """every torch.empty filled with NaN: an output nobody wrote shows up as a NaN"""
    det, fill = torch.are_deterministic_algorithms_enabled(), torch.utils.deterministic.fill_uninitialized_memory
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.utils.deterministic.fill_uninitialized_memory = True
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(det, warn_only=warn)
        torch.utils.deterministic.fill_uninitialized_memory = fill


def _sid(s):
    return f"{s[0]}x{s[1]}x{s[2]}"


def _cfg():
    from cocosnet_amd.hot_path import HotPathConfig
    return HotPathConfig(match_kernel=3, PONO_C=True, down=4)


_CASES = {}


def _case(shape, kind="diffuse"):
    """(theta, phi) on the device, made once per shape and kind, shared, never written"""
    if (shape, kind) not in _CASES:
        B, h, w = shape
        seed = 100 * h + w + B
        made = {"diffuse": mc.diffuse, "peaked": lambda *a: mc.peaked(*a)[:2], "identical": mc.identical}[kind](B, (h, w), seed)
        _CASES[shape, kind] = tuple(t.to(DEV) for t in made)
    return _CASES[shape, kind]


def _readout_inputs(shape, kind="diffuse"):
    """(T, mu, a, nu, b, row lse, col lse) of the case as the route makes them, detached"""
    from cocosnet_amd import ops
    B, h, w = shape
    theta, phi = _case(shape, kind)
    with torch.no_grad():
        (mu, a), (nu, b) = ops.unfold3_stats(theta, KC), ops.unfold3_stats(phi, KC)
        t = ops.box3_corr_xbox(theta, phi)
        row = ops.box3_match(t, mu, a, nu, b, h, w, KC, mc.INV_T)[2]
        col = ops.box3_match(t, nu, b, mu, a, h, w, KC, mc.INV_T, transposed=True)[2]
    return t, mu, a, nu, b, row, col


def _unblock(g, B, N):
    """the tile-blocked [B][N/32 key tiles][N/32 query blocks][g][lane][4] image -> [B, query, key]: register 4g + e of lane (h, c) of
    block (kt, qb) is key 32 kt + 8 g + 4 h + e, query 32 qb + c"""
    x = g.reshape(B, N // 32, N // 32, 4, 2, 32, 4)            # b, kt, qb, g, h, c, e
    return x.permute(0, 2, 5, 1, 3, 4, 6).reshape(B, N, N)      # b, (qb, c), (kt, g, h, e)


def _lse_bwd(t, q_stats, k_stats, lse, g_lse, shape, flags, g_init=None):
    """one call of the entry point on poisoned outputs -> (G blocked, dmu, da, dnu, db, gmax)"""
    from cocosnet_amd import _lib, ops
    B, h, w = shape
    N = h * w
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    G = nan(B * N * N) if g_init is None else g_init.clone()
    dmu, da, dnu, db = (nan(B, N) for _ in range(4))
    colpart = nan(_lib.load().cocos_box3_lse_bwd_colpart_bytes(B, N, N) // 4)
    gmax = nan(1)
    _lib.call("cocos_box3_lse_bwd_f16x3", t.data_ptr(), q_stats[0].data_ptr(), q_stats[1].data_ptr(), k_stats[0].data_ptr(),
              k_stats[1].data_ptr(), lse.data_ptr(), 0 if g_lse is None else g_lse.data_ptr(), G.data_ptr(), dmu.data_ptr(), da.data_ptr(),
              dnu.data_ptr(), db.data_ptr(), colpart.data_ptr(), gmax.data_ptr(), B, N, N, h, w, KC, mc.INV_T, flags, ops._stream())
    torch.cuda.synchronize()
    return G, dmu, da, dnu, db, gmax


def _upstreams(B, N):
    g = torch.Generator().manual_seed(N + B)
    mixed = torch.randn(B, N, generator=g)
    single = torch.zeros(B, N)
    single[B - 1, N // 3] = -2.5
    return {"mixed": mixed, "tiny": mixed * 1e-6, "huge": mixed * 1e6, "zero": torch.zeros(B, N), "single-row": single}


# ---------------------------------------------------------------------------------------------------------------- 1: forward identity
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_box3_lse_is_box3_match_lse_bitwise(shape):
    from cocosnet_amd import ops
    B, h, w = shape
    t, mu, a, nu, b, row, col = _readout_inputs(shape)
    with _poisoned_empty():
        got_row = ops.box3_lse(t, mu, a, nu, b, h, w, KC, mc.INV_T)
        got_col = ops.box3_lse(t, nu, b, mu, a, h, w, KC, mc.INV_T, transposed=True)
    assert torch.equal(got_row, row) and torch.equal(got_col, col)
    assert bool(torch.isfinite(row).all()) and bool(torch.isfinite(col).all())


# ---------------------------------------------------------------------------------------------------------------- 2: the kernel alone
@pytest.mark.parametrize("transposed", [False, True], ids=["rows", "transposed"])
@pytest.mark.parametrize("shape", SMALL + [(1, 40, 128)], ids=_sid)
def test_kernel_against_fp64(shape, transposed):
    """G (un-blocked on the host side of the test), dmu, da, dnu, db against fp64 for upstream gradients of mixed sign, of magnitude
    1e-6 and 1e+6, all zero, one non-zero row and a null pointer; then ACCUMULATE onto a pre-filled G: bitwise the sum"""
    T_FLAG, ACC_FLAG = 1, 2                                                    # COCOS_BOX3_T_TRANSPOSED, COCOS_BOX3_G_ACCUMULATE
    B, h, w = shape
    N = h * w
    theta, phi = _case(shape)
    t, mu, a, nu, b, row, col = _readout_inputs(shape)
    z = mc.logits(theta.double(), phi.double())                                # [B, p, q]
    (mu64, a64), (nu64, b64) = mc.stats(theta.double()), mc.stats(phi.double())
    if transposed:      # the column direction: the "queries" of the pass are the keys of the stored T
        z, qs, ks, lse = z.transpose(1, 2), (nu, b), (mu, a), col
        qs64, ks64 = (nu64, b64), (mu64, a64)
    else:
        qs, ks, lse = (mu, a), (nu, b), row
        qs64, ks64 = (mu64, a64), (nu64, b64)
    p64 = torch.softmax(z, dim=2)
    flags = T_FLAG if transposed else 0
    for tag, g_host in _upstreams(B, N).items():
        g_lse = g_host.to(DEV)
        G, dmu, da, dnu, db, gmax = _lse_bwd(t, qs, ks, lse, g_lse, shape, flags)
        wgt = g_lse.double().unsqueeze(2) * p64                               # d loss / d z
        G_ref = wgt * mc.INV_T * qs64[1].unsqueeze(2) * ks64[1].unsqueeze(1)
        ref = {"dmu": -(wgt * mc.INV_T * qs64[1].unsqueeze(2) * ks64[1].unsqueeze(1) * KC * ks64[0].unsqueeze(1)).sum(2),
               "da": (wgt * z).sum(2) / qs64[1], "db": (wgt * z).sum(1) / ks64[1],
               "dnu": -(wgt * mc.INV_T * qs64[1].unsqueeze(2) * ks64[1].unsqueeze(1) * KC * qs64[0].unsqueeze(2)).sum(1)}
        Gq = _unblock(G, B, N)                                                # [B, query of the stored T, key of the stored T]
        if transposed:
            Gq = Gq.transpose(1, 2)
        got = {"dmu": dmu, "da": da, "dnu": dnu, "db": db}
        assert all(bool(torch.isfinite(x).all()) for x in (G, dmu, da, dnu, db, gmax)), tag
        assert float(gmax) == float(G.abs().max()), tag
        if tag == "zero":
            assert not G.any() and not any(x.any() for x in got.values())
            Gn = _lse_bwd(t, qs, ks, lse, None, shape, flags)[0]            # a null g_lse: zeros as well
            assert not Gn.any()
            continue
        errs = {"G": rel(Gq, G_ref.cpu().numpy())}
        errs.update({n: rel(got[n], ref[n].cpu().numpy()) for n in got})
        print(f"[match_box3_nll] kernel {_sid(shape)} {'T' if transposed else 'R'} {tag}: " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
        assert max(errs.values()) < GRAD_TOL, (tag, errs)
        assert float(G.abs().max()) <= float((g_lse.abs().unsqueeze(2) * mc.INV_T * qs[1].unsqueeze(2) * ks[1].unsqueeze(1)).max()) * (1 + 1e-6)
        if tag == "mixed":
            again = _lse_bwd(t, qs, ks, lse, g_lse, shape, flags)
            assert all(torch.equal(x, y) for x, y in zip((G, dmu, da, dnu, db, gmax), again))      # run to run
            pre = torch.randn(B * N * N, generator=torch.Generator().manual_seed(N)).to(DEV)
            acc = _lse_bwd(t, qs, ks, lse, g_lse, shape, flags | ACC_FLAG, g_init=pre)
            assert torch.equal(acc[0], pre + G) and float(acc[5]) == float((pre + G).abs().max())
            assert all(torch.equal(x, y) for x, y in zip(acc[1:5], (dmu, da, dnu, db)))


# ---------------------------------------------------------------------------------------------------------------- 3: end to end
def _run(shape, kind, target, weight=None, symmetric=True, need=(True, True)):
    from cocosnet_amd.hot_path import correspondence_nll_box3
    theta, phi = _case(shape, kind)
    th, ph = theta.clone().requires_grad_(need[0]), phi.clone().requires_grad_(need[1])
    with _poisoned_empty():
        out = correspondence_nll_box3(th, ph, target, _cfg(), 1.0 / mc.INV_T, weight=weight, symmetric=symmetric)
        out["loss_match"].backward()
    torch.cuda.synchronize()
    return out, th.grad, ph.grad


def _ref(shape, kind, target, weight=None, symmetric=True):
    theta, phi = _case(shape, kind)
    th, ph = theta.double().requires_grad_(True), phi.double().requires_grad_(True)
    out = mc.arbiter(th, ph, target, weight=weight, symmetric=symmetric)
    out["loss_match"].backward()
    return out, th.grad, ph.grad


E2E = [(s, True, True) for s in SHAPES] + [((2, 4, 64), sym, wt) for sym, wt in ((True, False), (False, True), (False, False))]


@pytest.mark.parametrize("shape,symmetric,weighted", E2E, ids=[f"{_sid(s)}-{'sym' if sy else 'row'}-{'w' if wt else 'u'}" for s, sy, wt in E2E])
def test_loss_and_gradients_against_fp64_diffuse(shape, symmetric, weighted):
    B, h, w = shape
    target = mc.targets(B, (h, w), h + w).to(DEV)
    weight = mc.weights(B, (h, w), h).to(DEV) if weighted else None
    (out, dth, dph), (ref, dth_r, dph_r) = _run(shape, "diffuse", target, weight, symmetric), _ref(shape, "diffuse", target, weight, symmetric)
    errs = {n: rel(out[n].reshape(B, -1), ref[n].detach().cpu().numpy()) for n in ("match_nll", "back_nll", "match_lse", "back_lse")}
    errs["loss"] = abs(float(out["loss_match"].detach()) - float(ref["loss_match"].detach())) / abs(float(ref["loss_match"].detach()))
    gerrs = {"dtheta": rel(dth, dth_r.cpu().numpy()), "dphi": rel(dph, dph_r.cpu().numpy())}
    print(f"[match_box3_nll] e2e {_sid(shape)} sym={symmetric} weighted={weighted}: " + "  ".join(f"{n} {e:.2e}" for n, e in {**errs, **gerrs}.items())
          + f"  min match_nll {float(out['match_nll'].detach().min()):.3e}")
    flat = target.reshape(B, -1)
    assert not out["match_nll"].reshape(B, -1)[flat < 0].any() and not out["back_nll"].reshape(B, -1)[flat < 0].any()
    assert not out["match_target_prob"].requires_grad
    assert max(errs.values()) < OUT_TOL, errs
    assert max(gerrs.values()) < GRAD_TOL, gerrs


# ---------------------------------------------------------------------------------------------------------------- 5, 6: bits and launches
def test_run_to_run_and_gradient_subsets_bitwise():
    shape = (2, 4, 64)
    target, weight = mc.targets(2, (4, 64), 9).to(DEV), mc.weights(2, (4, 64), 8).to(DEV)
    out, dth, dph = _run(shape, "diffuse", target, weight)
    out2, dth2, dph2 = _run(shape, "diffuse", target, weight)
    assert torch.equal(dth, dth2) and torch.equal(dph, dph2) and torch.equal(out["loss_match"], out2["loss_match"])
    _, dth_only, none = _run(shape, "diffuse", target, weight, need=(True, False))
    assert none is None and torch.equal(dth_only, dth)
    none, dph_only = _run(shape, "diffuse", target, weight, need=(False, True))[1:]
    assert none is None and torch.equal(dph_only, dph)


def test_symmetric_loss_shares_one_gradient_of_t():
    """the launch log `ops._call` keeps (ops.KernelTimer: one entry per launch, by tag) over the backward: both lse passes write into
    one G — one box adjoint, two GEMMs"""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import correspondence_nll_box3
    theta, phi = _case((2, 4, 64))
    th, ph = theta.clone().requires_grad_(True), phi.clone().requires_grad_(True)
    out = correspondence_nll_box3(th, ph, mc.targets(2, (4, 64), 9).to(DEV), _cfg(), 1.0 / mc.INV_T)
    with ops.KernelTimer() as log:
        out["loss_match"].backward()
    torch.cuda.synchronize()
    counts = {tag: len(ev) for tag, ev in log.events.items()}
    print(f"[match_box3_nll] backward launches by tag: {counts!r}")
    assert counts.get("box3_lse_bwd") == 2 and counts.get("box3_adjoint_planes") == 1 and counts.get("box3_corr_grad") == 2
    assert counts.get("box3_pair_logit_bwd_pair") == 1


def test_row_only_loss_reports_a_detached_column_side():
    from cocosnet_amd.hot_path import correspondence_nll_box3
    theta, phi = _case((2, 4, 64))
    th, ph = theta.clone().requires_grad_(True), phi.clone().requires_grad_(True)
    out = correspondence_nll_box3(th, ph, mc.targets(2, (4, 64), 9).to(DEV), _cfg(), 1.0 / mc.INV_T, symmetric=False)
    assert not out["back_nll"].requires_grad and not out["back_lse"].requires_grad and out["match_nll"].requires_grad


def test_arbiter_logits_are_box3_logits():
    """the arbiter's z (fp64, unfold) against hot_path._box3_logits (K3 -> K6) on a 5 x 7 grid: the two state one function"""
    from cocosnet_amd.hot_path import _box3_logits
    theta, phi = (t.to(DEV) for t in mc.diffuse(2, (5, 7), 3))
    z = mc.logits(theta.double(), phi.double())
    assert rel(_box3_logits(theta, phi, mc.INV_T), z.cpu().numpy()) < OUT_TOL


# ---------------------------------------------------------------------------------------------------------------- 4: peaked rows
PEAKED = [(shape, tk, sym, wt) for shape in SMALL for tk in ("mixed", "planted") for sym in (True, False) for wt in (True, False)]
ALLOWED = []      # the cases judged under the allowance: peaked ones only, by construction (the diffuse test has no such arm)


@pytest.mark.parametrize("shape,tkind,symmetric,weighted", PEAKED,
                         ids=[f"{_sid(s)}-{tk}-{'sym' if sy else 'row'}-{'w' if wt else 'u'}" for s, tk, sy, wt in PEAKED])
def test_loss_and_gradients_against_fp64_peaked(shape, tkind, symmetric, weighted):
    """one-hot rows and columns (phi = theta permuted + noise), random targets and the planted permutation itself.  Outputs under
    OUT_TOL; d theta / d phi under GRAD_TOL where they meet it, else after match_box3_nll_case.lse_allowance at the readout's recorded
    lse tolerance (tests/test_gpu_match_box3.py's TOL) — what is left of the error after the allowance is held to GRAD_TOL.  The
    ratios are printed."""
    B, h, w = shape
    theta, phi = _case(shape, "peaked")
    if tkind == "planted":
        perm = mc.peaked(B, (h, w), 100 * h + w + B)[2]
        target = perm.repeat(B, 1).reshape(B, h, w).clone()
        target[:, 0, 1::6] = -1
        target = target.to(DEV)
    else:
        target = mc.targets(B, (h, w), h + w + 1).to(DEV)
    weight = mc.weights(B, (h, w), h + 2).to(DEV) if weighted else None
    (out, dth, dph), (ref, dth_r, dph_r) = _run(shape, "peaked", target, weight, symmetric), _ref(shape, "peaked", target, weight, symmetric)
    errs = {n: rel(out[n].reshape(B, -1), ref[n].detach().cpu().numpy()) for n in ("match_nll", "back_nll", "match_lse", "back_lse")}
    allow = mc.lse_allowance(theta.double(), phi.double(), *mc.lse_gradients(target, weight, symmetric), mc.INV_T, BOX_LSE_TOL)
    tag = f"peaked {_sid(shape)} {tkind} sym={symmetric} weighted={weighted}"
    line = [f"[match_box3_nll] {tag}: " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()) + f"  min match_nll {float(out['match_nll'].detach().min()):.3e}"]
    for name, got, want in (("dtheta", dth, dth_r), ("dphi", dph, dph_r)):
        err, scale = (got.double() - want).abs(), float(want.abs().max())
        plain = float(err.max()) / scale
        used = float((err / allow[name].clamp_min(1e-300)).max())                 # the largest share of its allowance an element uses
        left = float((err - allow[name]).clamp_min(0).max()) / scale
        line.append(f"{name}: plain {plain:.2e} (bound {GRAD_TOL:.0e})  err / allowance {used:.2e}  left after the allowance {left:.2e}")
        if plain >= GRAD_TOL:
            ALLOWED.append((tag, name))
            assert left < GRAD_TOL, (tag, name, plain, left)
    print("  ".join(line))
    assert bool(torch.isfinite(dth).all()) and bool(torch.isfinite(dph).all())
    assert max(errs.values()) < OUT_TOL, errs


def test_allowance_is_used_by_peaked_cases_only():
    print(f"[match_box3_nll] judged under the allowance: {len(ALLOWED)} of {2 * len(PEAKED)} peaked gradients, 0 of the diffuse ones: {ALLOWED!r}")
    assert all(tag.startswith("peaked") for tag, _ in ALLOWED)


# ---------------------------------------------------------------------------------------------------------------- 9: degenerate targets
def test_no_supervised_cell_gives_zero_loss_and_zero_gradients():
    out, dth, dph = _run((2, 4, 64), "diffuse", mc.targets(2, (4, 64), 0, "all_negative").to(DEV))
    assert float(out["loss_match"]) == 0.0 and not out["match_nll"].any() and not out["back_nll"].any()
    assert dth is not None and dph is not None and not dth.any() and not dph.any()


def test_identity_target_on_identical_features():
    """theta == phi, t_i = i: every row and column is one-hot at the target, match_target_prob -> 1.  match_nll is NOT clamped: the
    most negative value (fp32 target logit against the f16x3 lse) is printed"""
    shape = (2, 4, 64)
    out, dth, dph = _run(shape, "identical", mc.targets(2, (4, 64), 0, "identity").to(DEV))
    print(f"[match_box3_nll] identity: min prob {float(out['match_target_prob'].min()):.6f}  most negative match_nll "
          f"{float(out['match_nll'].min()):.3e}  back_nll {float(out['back_nll'].min()):.3e}")
    assert float(out["match_target_prob"].min()) > 0.99
    assert bool(torch.isfinite(dth).all()) and bool(torch.isfinite(dph).all())


# ---------------------------------------------------------------------------------------------------------------- the module
def test_module_match_loss_box3():
    """NoVGGCorrespondence.match_loss_box3 at a 256 crop (a 64 x 64 grid): the dictionary, match_lse / back_lse equal to
    correspondence_mutual's readouts on the same projections bit for bit, gradients at theta.weight and phi.weight"""
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_mutual
    from test_gpu_exemplar import _module_case
    net, ref_img, real, seg, ref_seg = _module_case("ade20k_options", 256, 1, 1, match_kernel=3)
    target = mc.targets(1, (64, 64), 5).to(DEV)
    out = net.match_loss_box3(ref_img, real, seg, ref_seg, target)
    assert {"match_nll", "back_nll", "match_lse", "back_lse", "match_target_prob", "loss_match"} <= set(out)
    assert all(out[n].shape == (1, 64, 64) for n in ("match_nll", "back_nll", "match_lse", "back_lse", "match_target_prob"))
    with torch.no_grad():
        theta_raw, phi_raw = net.project(ref_img, real, seg, ref_seg, {}, lazy=True)
        m = correspondence_mutual(theta_raw, phi_raw, HotPathConfig.from_opt(net.opt, down=net.opt.down), 0.01)
    assert torch.equal(out["match_lse"], m.rows.lse.reshape(1, 64, 64)) and torch.equal(out["back_lse"], m.cols.lse.reshape(1, 64, 64))
    out["loss_match"].backward()
    for p in (net.theta.weight, net.phi.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- 8: live buffers
def test_loss_hands_over_live_buffers_only(monkeypatch):
    """forward + backward of the symmetric loss with every pointer argument of every entry point checked against the allocator's live
    blocks (tests/test_gpu_live_buffers.py's guard): T, the shared G the second pass accumulates into, the colpart workspaces"""
    guard = _Guard(monkeypatch)
    _run((2, 4, 64), "diffuse", mc.targets(2, (4, 64), 9).to(DEV), mc.weights(2, (4, 64), 8).to(DEV))
    _run((2, 4, 64), "diffuse", mc.targets(2, (4, 64), 9).to(DEV), None, symmetric=False)
    guard.check(20, 120)


# ---------------------------------------------------------------------------------------------------------------- 10: memory
def test_peak_memory_stays_within_the_dense_steps():
    """B = 1 on 64 x 64: peak allocation above the inputs over forward + backward, against the dense correspondence_hot_path
    match_kernel-3 step measured here, on the same run.  Margin, from shapes: one set of [B,N] vectors (the two lse, z_t, c, the nll
    pair, g / hb / dmu / da / dnu / db, the statistics' gradients: 24 vectors allowed) plus the pair unit's rows — the position-major
    copies of theta and phi and their two gradients, and their transposes back: 6 x [B,N,256] fp32"""
    import gc
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_hot_path, correspondence_nll_box3
    B, h, w, down, nc = 1, 64, 64, 4, 7
    N = h * w
    g = torch.Generator().manual_seed(5)
    theta0, phi0 = (t.to(DEV) for t in mc.diffuse(B, (h, w), 77))
    ref_img, real = (torch.rand(B, 3, h * down, w * down, generator=g).to(DEV) * 2 - 1 for _ in range(2))
    seg = torch.zeros(B, nc, h * down, w * down).scatter_(1, torch.randint(0, nc, (B, 1, h * down, w * down), generator=g), 1.0).to(DEV)
    target = mc.targets(B, (h, w), 3).to(DEV)
    dense_cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=down, warp_mask_losstype="direct", isTrain=True)

    def peak(step):
        th, ph = theta0.clone().requires_grad_(True), phi0.clone().requires_grad_(True)
        rz._clear_pools()
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step(th, ph)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    def dense(th, ph):
        out = correspondence_hot_path(th, ph, ref_img, real, seg, seg, dense_cfg)
        (out["warp_out"].square().sum() + out["warp_mask"].square().sum()).backward()

    def loss(th, ph):
        correspondence_nll_box3(th, ph, target, _cfg(), 1.0 / mc.INV_T)["loss_match"].backward()

    peak(loss), peak(dense)                                   # warm: kernels loaded, pools filled
    p_dense, p_loss = peak(dense), peak(loss)
    margin = 24 * B * N * 4 + 6 * B * N * 256 * 4
    mib = 2 ** 20
    print(f"[match_box3_nll] peak above inputs, B = 1 on 64 x 64: loss {p_loss / mib:.1f} MiB  dense step {p_dense / mib:.1f} MiB  "
          f"margin {margin / mib:.1f} MiB  (one HW x HW fp32 tensor: {N * N * 4 / mib:.0f} MiB)")
    assert p_loss <= p_dense + margin, (p_loss, p_dense, margin)


# ---------------------------------------------------------------------------------------------------------------- 8: red zones
# The case joins tests/test_gpu_red_zones.py's table at import time, as the K36 - K52 files' cases do, so its "every entry point was
# reached" audit counts the three K53 entry points; this file runs it.
def _rz_hot(c):
    from cocosnet_amd.hot_path import correspondence_nll_box3
    theta, phi = mc.diffuse(1, (4, 64), 71)
    th, ph = c.leaf(theta), c.leaf(phi)
    out = correspondence_nll_box3(th, ph, c.data(mc.targets(1, (4, 64), 72)), _cfg(), 0.01, weight=c.data(mc.weights(1, (4, 64), 73)))
    return [out["loss_match"], out["match_nll"], out["back_nll"]]


def _rz_entry(c):
    """cocos_box3_lse_bwd_f16x3 called directly: the row pass, then COCOS_BOX3_T_TRANSPOSED | COCOS_BOX3_G_ACCUMULATE onto its G, on a
    128-wide grid; every buffer of the entry is carved between red zones"""
    from cocosnet_amd import _lib, ops
    B, h, w = 1, 2, 128
    N = h * w
    theta, phi = (c.data(t) for t in mc.diffuse(B, (h, w), 81))
    with torch.no_grad():
        (mu, a), (nu, b) = ops.unfold3_stats(theta, KC), ops.unfold3_stats(phi, KC)
        t = ops.box3_corr_xbox(theta, phi)
        row = ops.box3_match(t, mu, a, nu, b, h, w, KC, mc.INV_T)[2]
        col = ops.box3_match(t, nu, b, mu, a, h, w, KC, mc.INV_T, transposed=True)[2]
    gen = torch.Generator().manual_seed(82)
    g_row, g_col = c.data(torch.randn(B, N, generator=gen)), c.data(torch.randn(B, N, generator=gen))
    G = torch.empty(B * N * N, device=DEV)
    res = [G]
    for qs, ks, lse, gl, flags in (((mu, a), (nu, b), row, g_row, 0), ((nu, b), (mu, a), col, g_col, 3)):
        outs = [torch.empty(B, N, device=DEV) for _ in range(4)]
        colpart = torch.empty(_lib.load().cocos_box3_lse_bwd_colpart_bytes(B, N, N) // 4, device=DEV)
        gmax = torch.empty(1, device=DEV)
        _lib.call("cocos_box3_lse_bwd_f16x3", t.data_ptr(), qs[0].data_ptr(), qs[1].data_ptr(), ks[0].data_ptr(), ks[1].data_ptr(),
                  lse.data_ptr(), gl.data_ptr(), G.data_ptr(), *(o.data_ptr() for o in outs), colpart.data_ptr(), gmax.data_ptr(), B, N, N,
                  h, w, KC, mc.INV_T, flags, ops._stream())
        res += outs + [colpart, gmax]
    return res


RZ_CASES = {"correspondence_nll_box3-1x256x4x64": _rz_hot, "box3_lse_bwd-rows-then-transposed-accumulate-1x2x128": _rz_entry}
for _name, _body in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_loss_inside_red_zones(name, monkeypatch):
    """forward + backward under tests/guarded_alloc.guarded: no guard byte changes, every returned tensor and gradient is finite"""
    rz.test_red_zones(name, monkeypatch)
    assert (NEW_ENTRIES if name.startswith("correspondence") else {"cocos_box3_lse_bwd_f16x3"}) <= set(rz.COVERAGE[name][0])
