"""K51 on the GPU: ops.box3_sparse_softmax_warp (forward and every gradient), hot_path.correspondence_sparse_box3 and
NoVGGCorrespondence.sparse_warp_box3 — the trainable k-sparse warp on the match_kernel-3 route.

The reference is tests/box3_sparse_case.py's `arbiter`: torch fp64, F.unfold(3, padding=1) -> centre -> normalise -> gather the k logits
from the clamped idx -> softmax -> blend, gradients from autograd.  It shares no code with the kernels' tap formulation.  Bounds are
tests/test_gpu_parity.py's (imported): OUT_TOL = 2e-4 on out and w, GRAD_TOL = 1e-3 on every gradient, its `rel` measure.  No floor is
needed: with k = 1 the logit gradients are exactly zero on both sides (w = 1, dz = w (dw - w dw) = 0).

The gradients of theta and phi are TOTAL derivatives: the op's own (through R) plus the statistics' share (through mu, a, nu, b).  In
the op tests the statistics are made from the leaves by an fp64 torch chain (box3_sparse_case.stats), so what is judged there is the op
alone, its dmu / da / dnu / db outputs included; test_statistics_path makes them with ops.unfold3_stats (K12) as the hot path does.

The file name sorts before test_gpu_red_zones.py: its red-zone cases have run when that file's audit is collected."""
import contextlib
import gc
import itertools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box3_sparse_case as bc  # noqa: E402
import test_gpu_red_zones as rz  # noqa: E402
from test_gpu_parity import GRAD_TOL, OUT_TOL, rel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INV_T = 100.0
B = 2
KC = 9 * 256.0
GRIDS = [((2, 2), (2, 2)), ((1, 8), (8, 1)), ((6, 6), (6, 6)), ((5, 7), (4, 9))]
MIB = 2 ** 20


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


@contextlib.contextmanager
def _poisoned_empty():
    """every torch.empty filled with NaN (what COCOS_POISON_EMPTY=1 switches on for the whole suite, tests/conftest.py): an output row
    no wave wrote shows up as a NaN instead of whatever the allocator's block held"""
    det, fill = torch.are_deterministic_algorithms_enabled(), torch.utils.deterministic.fill_uninitialized_memory
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.utils.deterministic.fill_uninitialized_memory = True
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(det, warn_only=warn)
        torch.utils.deterministic.fill_uninitialized_memory = fill


def _gname(g):
    return f"{g[0]}x{g[1]}"


_CASES = {}


def _case(grid, kgrid, Cv):
    """(theta, phi, v, dout) on the device, made once per shape, shared, never written"""
    key = (grid, kgrid, Cv)
    if key not in _CASES:
        theta, phi = bc.features(B, grid, kgrid, 1000 * grid[0] + 10 * kgrid[1] + Cv)
        g = torch.Generator().manual_seed(Cv + grid[1])
        v = torch.randn(B, Cv, kgrid[0] * kgrid[1], generator=g)
        dout = torch.randn(B, Cv, grid[0] * grid[1], generator=g)
        _CASES[key] = tuple(t.to(DEV) for t in (theta, phi, v, dout))
    return _CASES[key]


def _stat_chain(x):
    """(mu, a) fp32 of x through an fp64 torch chain with autograd: exact inputs for the op, and the route the statistics' share of the
    gradient takes back to the leaf"""
    mu, a = bc.stats(x.double())
    return mu.float(), a.float()


def _run(theta, phi, v, idx, dout, need=(True, True, True), k12=False):
    """(out, w, [d theta, d phi, dv]) of the op; `k12`: the statistics come from ops.unfold3_stats instead of the torch chain"""
    from cocosnet_amd import ops
    leaves = [t.clone().requires_grad_(n) for t, n in zip((theta, phi, v), need)]
    th, ph, vv = leaves
    (mu, a), (nu, b) = (ops.unfold3_stats(th, KC), ops.unfold3_stats(ph, KC)) if k12 else (_stat_chain(th), _stat_chain(ph))
    out, w = ops.box3_sparse_softmax_warp(th, ph, mu, a, nu, b, vv, idx, INV_T, return_weights=True)
    assert not w.requires_grad
    out.backward(dout)
    torch.cuda.synchronize()
    return out.detach(), w, [t.grad for t in leaves]


def _ref(theta, phi, v, idx, dout):
    leaves = [t.double().clone().requires_grad_(True) for t in (theta, phi, v)]
    out, w = bc.arbiter(*leaves, idx, INV_T, weights=True)
    out.backward(dout.double())
    return out.detach(), w.detach(), [t.grad for t in leaves]


def _judge(tag, got, want):
    (out, w, grads), (out_r, w_r, grads_r) = got, want
    errs = [rel(out, out_r.cpu().numpy()), rel(w, w_r.cpu().numpy())] + [rel(g, r.cpu().numpy()) for g, r in zip(grads, grads_r)]
    print(f"[box3_sparse] {tag}: rel out {errs[0]:.3e}  w {errs[1]:.3e}  dtheta {errs[2]:.3e}  dphi {errs[3]:.3e}  dv {errs[4]:.3e}")
    assert all(bool(torch.isfinite(t).all()) for t in [out, w] + grads), tag
    assert max(errs[:2]) < OUT_TOL, (tag, errs)
    assert max(errs[2:]) < GRAD_TOL, (tag, errs)


# ---------------------------------------------------------------------------------------------------------------- the op against fp64
OP_CASES = [(grid, kgrid, Cv, k) for grid, kgrid in GRIDS for Cv in (3, 5, 154) for k in (1, 2, 3, 8) if k <= kgrid[0] * kgrid[1]]


@pytest.mark.parametrize("grid,kgrid,Cv,k", OP_CASES, ids=[f"{_gname(g)}-{_gname(kg)}-Cv{c}-k{k}" for g, kg, c, k in OP_CASES])
def test_op_against_fp64(grid, kgrid, Cv, k):
    """random tables with repeats, out-of-range values, a hub, a key nobody names and candidates on every border (index_table);
    outputs allocated poisoned, so a row or a key nobody wrote is a NaN"""
    theta, phi, v, dout = _case(grid, kgrid, Cv)
    Nq, Nk = grid[0] * grid[1], kgrid[0] * kgrid[1]
    idx, hub, dead = bc.index_table(B, Nq, Nk, k, 7 * Nq + k)
    idx = idx.to(DEV)
    with _poisoned_empty():
        got = _run(theta, phi, v, idx, dout)
    _judge(f"{_gname(grid)}/{_gname(kgrid)} Cv={Cv} k={k}", got, _ref(theta, phi, v, idx, dout))
    if dead is not None:      # the key nobody names: zeros from the kernel (its phi gradient may still be reached as a neighbour's tap)
        assert bool((got[2][2][:, :, dead] == 0).all())


def test_int32_and_int64_tables_agree_bitwise():
    theta, phi, v, dout = _case((5, 7), (4, 9), 5)
    idx = bc.index_table(B, 35, 36, 3, 5)[0].clamp(-5, 50).to(DEV)
    a, b = _run(theta, phi, v, idx, dout), _run(theta, phi, v, idx.to(torch.int32), dout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


# ---------------------------------------------------------------------------------------------------------------- subsets, determinism
@pytest.mark.parametrize("need", [s for s in itertools.product([False, True], repeat=3) if any(s)],
                         ids=lambda s: "".join(n for n, on in zip("tpv", s) if on))
def test_gradient_subsets(need):
    """each non-empty subset of {theta, phi, v}: None outside it, and inside it the all-three run's gradients, bit for bit (every
    gradient comes from the same launch whichever others are asked for)"""
    theta, phi, v, dout = _case((5, 7), (4, 9), 5)
    idx = bc.index_table(B, 35, 36, 3, 11)[0].to(DEV)
    out_all, w_all, grads_all = _run(theta, phi, v, idx, dout)
    out, w, grads = _run(theta, phi, v, idx, dout, need)
    assert torch.equal(out, out_all) and torch.equal(w, w_all)
    for g, g_all, on in zip(grads, grads_all, need):
        assert (g is None) if not on else torch.equal(g, g_all)


def test_same_call_twice_same_bits():
    """forward + backward twice, the hub table included (one key named by every query: the longest serial list)"""
    theta, phi, v, dout = _case((6, 6), (6, 6), 154)
    idx = bc.index_table(B, 36, 36, 8, 13)[0].to(DEV)
    assert bool((idx[:, :, 0] == 35).all())
    a = _run(theta, phi, v, idx, dout, k12=True)
    junk = [torch.full((n,), float("nan"), device=DEV) for n in (B * 36 * 256, B * 36 * 256, B * 36 * 154, B * 36 * 8)]      # another history
    del junk
    b = _run(theta, phi, v, idx, dout, k12=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


# ---------------------------------------------------------------------------------------------------------------- statistics path
def test_statistics_path():
    """theta and phi as leaves, (mu, a, nu, b) from ops.unfold3_stats of them: the gradients equal the arbiter's TOTAL derivative.  The
    share that travels through dmu / da / dnu / db is far above the bound (printed and asserted: the run with the statistics detached
    misses the arbiter), so this fails when those terms are dropped."""
    from cocosnet_amd import ops
    theta, phi, v, dout = _case((5, 7), (4, 9), 5)
    idx = bc.index_table(B, 35, 36, 3, 17)[0].to(DEV)
    want = _ref(theta, phi, v, idx, dout)
    _judge("statistics from K12", _run(theta, phi, v, idx, dout, k12=True), want)
    th, ph = theta.clone().requires_grad_(True), phi.clone().requires_grad_(True)
    with torch.no_grad():
        (mu, a), (nu, b) = ops.unfold3_stats(th, KC), ops.unfold3_stats(ph, KC)
    ops.box3_sparse_softmax_warp(th, ph, mu, a, nu, b, v, idx, INV_T).backward(dout)
    share = [rel(t.grad, r.cpu().numpy()) for t, r in zip((th, ph), want[2])]
    print(f"[box3_sparse] statistics detached: rel dtheta {share[0]:.3e}  dphi {share[1]:.3e} (the statistics' share of the gradient)")
    assert min(share) > GRAD_TOL, share      # (an fp64 host restatement on these features and this table: about 1e-2 and 4e-2)


# ---------------------------------------------------------------------------------------------------------------- dense limit
def test_full_support_is_the_materialised_route():
    """k = Nk = 8 on a 2 x 4 grid, idx = every key: out against _box3_logits -> softmax -> matmul on the same inputs"""
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import _box3_logits
    theta, phi = (t.to(DEV) for t in bc.features(B, (2, 4), (2, 4), 88))
    v = torch.randn(B, 5, 8, generator=torch.Generator().manual_seed(89)).to(DEV)
    idx = torch.arange(8, device=DEV).expand(B, 8, 8).contiguous()
    (mu, a), (nu, b) = ops.unfold3_stats(theta, KC), ops.unfold3_stats(phi, KC)
    out = ops.box3_sparse_softmax_warp(theta, phi, mu, a, nu, b, v, idx, INV_T)
    f = _box3_logits(theta, phi, INV_T)                                       # [B,Nq,Nk]
    want = torch.matmul(torch.softmax(f, dim=-1), v.transpose(1, 2)).transpose(1, 2)
    err = rel(out, want.cpu().numpy())
    print(f"[box3_sparse] full support against the materialised route: rel out {err:.3e}")
    assert err < OUT_TOL, err


# ---------------------------------------------------------------------------------------------------------------- hot path
def _hot_case(Bq, fh, seed, down=4, nc=5):
    g = torch.Generator().manual_seed(seed)
    theta, phi = bc.features(Bq, (fh, fh), (fh, fh), seed)
    H = fh * down
    onehot = lambda: torch.zeros(Bq, nc, H, H).scatter_(1, torch.randint(0, nc, (Bq, 1, H, H), generator=g), 1.0)
    ref_img = torch.rand(Bq, 3, H, H, generator=g) * 2 - 1
    return tuple(t.to(DEV) for t in (theta, phi, ref_img, onehot(), onehot()))


def _hot_ref(theta, phi, ref_img, ref_seg, idx, down):
    """fp64: the arbiter on `idx` with the values the hot path blends (pooled exemplar, sampled labels), then nearest up-sampling"""
    Bq, _, fh, fw = theta.shape
    vals = torch.cat([F.avg_pool2d(ref_img.double(), down).reshape(Bq, 3, -1),
                      F.interpolate(ref_seg.double(), scale_factor=1 / down, mode="nearest").reshape(Bq, ref_seg.shape[1], -1)], 1)
    o = bc.arbiter(theta, phi, vals, idx, INV_T)
    return F.interpolate(o[:, :3].reshape(Bq, 3, fh, fw), scale_factor=down, mode="nearest"), o[:, 3:].reshape(Bq, -1, fh, fw)


def _hot_check(tag, Bq, fh, k, seed):
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match, correspondence_sparse_box3
    theta0, phi0, ref_img, seg, ref_seg = _hot_case(Bq, fh, seed)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4, warp_mask_losstype="direct")
    theta, phi = theta0.clone().requires_grad_(True), phi0.clone().requires_grad_(True)
    out = correspondence_sparse_box3(theta, phi, ref_img, seg, ref_seg, cfg, 1.0 / INV_T, k)
    H = fh * 4
    assert set(out) == {"warp_out", "warp_mask", "match_index", "match_weight"}
    assert out["warp_out"].shape == (Bq, 3, H, H) and out["warp_mask"].shape == (Bq, 5, fh, fh)
    assert out["match_index"].shape == out["match_weight"].shape == (Bq, k, fh, fh)
    assert out["match_index"].dtype == torch.int64 and not out["match_weight"].requires_grad
    m = correspondence_match(theta0, phi0, cfg, 1.0 / INV_T, topk=k)
    assert torch.equal(out["match_index"], m.index)
    del m
    gen = torch.Generator().manual_seed(seed + 1)
    g_out, g_mask = torch.randn(Bq, 3, H, H, generator=gen).to(DEV), torch.randn(Bq, 5, fh, fh, generator=gen).to(DEV)
    ((out["warp_out"] * g_out).sum() + (out["warp_mask"] * g_mask).sum()).backward()
    idx = out["match_index"].permute(0, 2, 3, 1).reshape(Bq, fh * fh, k)
    th64, ph64 = theta0.double().requires_grad_(True), phi0.double().requires_grad_(True)
    warp_r, mask_r = _hot_ref(th64, ph64, ref_img, ref_seg, idx, 4)
    ((warp_r * g_out.double()).sum() + (mask_r * g_mask.double()).sum()).backward()
    errs = {"warp_out": rel(out["warp_out"], warp_r.detach().cpu().numpy()), "warp_mask": rel(out["warp_mask"], mask_r.detach().cpu().numpy()),
            "d theta": rel(theta.grad, th64.grad.cpu().numpy()), "d phi": rel(phi.grad, ph64.grad.cpu().numpy())}
    print(f"[box3_sparse] correspondence_sparse_box3 {tag}: " + "  ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    assert all(e < (GRAD_TOL if n.startswith("d ") else OUT_TOL) for n, e in errs.items()), errs
    assert float(out["match_weight"].sum(1).sub(1).abs().max()) < 1e-5


def test_hot_path_chain_selection():
    """B = 2, 8 x 8, k = 3: the selection is the materialised chain (the fused family does not take the grid)"""
    from cocosnet_amd import ops
    assert not ops.box3_fused_ok(2, 256, 8, 8)
    _hot_check("chain 2x8x8 k=3", 2, 8, 3, 41)


def test_hot_path_fused_selection():
    """B = 1, 64 x 64, k = 4: the smallest shape the fused family takes — the selection is K41 on T; the arbiter runs on the GPU"""
    from cocosnet_amd import ops
    assert ops.box3_fused_ok(1, 256, 64, 64) and ops.box3_topk_ok(4)
    _hot_check("fused 1x64x64 k=4", 1, 64, 4, 43)


def test_nothing_hw_by_hw_is_kept():
    """B = 1, 64 x 64, k = 4: what stays allocated after the forward — the result and everything saved for the backward, the
    selection's tensors released — above what was allocated before the call is below the size of ONE T (4096^2 x 4 bytes = 64 MiB).
    A condition, not a measurement: the saved state is a few 4 MiB tensors (theta^T, phi^T and the [B,N,k] tables)."""
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse_box3
    theta0, phi0, ref_img, seg, ref_seg = _hot_case(1, 64, 47)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4, warp_mask_losstype="direct")
    theta, phi = theta0.requires_grad_(True), phi0.requires_grad_(True)
    rz._clear_pools()      # (the per-thread max|x| table may still hold a few tensors of earlier tests: they are not this call's)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = correspondence_sparse_box3(theta, phi, ref_img, seg, ref_seg, cfg, 1.0 / INV_T, 4)
    torch.cuda.synchronize()
    held, peak = torch.cuda.memory_allocated() - before, torch.cuda.max_memory_allocated() - before
    print(f"[box3_sparse] held after the forward: {held / MIB:.1f} MiB (bound {4096 * 4096 * 4 / MIB:.0f} MiB); peak during it, the "
          f"selection's T included: {peak / MIB:.1f} MiB")
    assert held < 4096 * 4096 * 4, held
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    (out["warp_out"].square().sum() + out["warp_mask"].square().sum()).backward()
    torch.cuda.synchronize()
    print(f"[box3_sparse] peak during the backward: {(torch.cuda.max_memory_allocated() - before) / MIB:.1f} MiB")
    assert torch.cuda.max_memory_allocated() - before < 4096 * 4096 * 4
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0 for t in (theta, phi))


def test_module_sparse_warp_box3():
    """NoVGGCorrespondence.sparse_warp_box3 on ade20k_options(match_kernel=3) at the module tests' smallest crop: keys, shapes, finite
    values, gradients at theta.weight and phi.weight, and the same result as correspondence_sparse_box3 on project()'s outputs"""
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse_box3
    from test_gpu_exemplar import _module_case
    net, ref_img, real, seg, ref_seg = _module_case("ade20k_options", 64, 2, 2, match_kernel=3)
    out = net.sparse_warp_box3(ref_img, real, seg, ref_seg, topk=4)
    assert {"warp_out", "warp_mask", "match_index", "match_weight"} <= set(out)
    assert out["warp_out"].shape == (2, 3, 64, 64) and out["warp_mask"].shape == (2, 7, 16, 16)
    assert out["match_index"].shape == out["match_weight"].shape == (2, 4, 16, 16)
    assert all(bool(torch.isfinite(out[n]).all()) for n in ("warp_out", "warp_mask", "match_weight"))
    theta_raw, phi_raw = net.project(ref_img, real, seg, ref_seg, {}, lazy=True)
    want = correspondence_sparse_box3(theta_raw, phi_raw, ref_img, seg, ref_seg, HotPathConfig.from_opt(net.opt, down=net.opt.down), 0.01, 4)
    for n in ("warp_out", "warp_mask", "match_index", "match_weight"):
        assert torch.equal(out[n], want[n]), n
    (out["warp_out"].square().sum() + out["warp_mask"].square().sum()).backward()
    for p in (net.theta.weight, net.phi.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- red zones
# The cases join tests/test_gpu_red_zones.py's table at import time, as the K36 - K50 files' cases do, so its coverage report and its
# "every entry point was reached" audit count the four K51 entry points; this file runs them.
NEW_ENTRIES = {"cocos_box3_sparse_softmax_warp_fwd", "cocos_box3_sparse_softmax_warp_bwd_pair", "cocos_box3_sparse_softmax_warp_bwd_theta",
               "cocos_box3_sparse_softmax_warp_bwd_key"}


def _rz_op(c):
    """odd sizes, unequal grids, out-of-range entries, a hub; forward and backward with every gradient (the statistics from K12)"""
    from cocosnet_amd import ops
    theta, phi = bc.features(2, (5, 7), (4, 9), 61)
    th, ph, v = c.leaf(theta), c.leaf(phi), c.leaf(rz.rnd(2, 5, 36, seed=62))
    idx = bc.index_table(2, 35, 36, 3, 63)[0]
    (mu, a), (nu, b) = ops.unfold3_stats(th, KC), ops.unfold3_stats(ph, KC)
    return [ops.box3_sparse_softmax_warp(th, ph, mu, a, nu, b, v, c.data(idx), 100.0)]


def _rz_hot(c):
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse_box3
    theta, phi = bc.features(2, (8, 8), (8, 8), 64)
    th, ph = c.leaf(theta), c.leaf(phi)
    ref_img = c.data(rz.uni(2, 3, 32, 32, seed=65))
    seg = c.data(rz.onehot(rz.labels(2, 7, 32, 32, 66), 7))
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4, warp_mask_losstype="direct", isTrain=True)
    out = correspondence_sparse_box3(th, ph, ref_img, seg, seg, cfg, 0.01, 3)
    return [v for v in out.values() if torch.is_tensor(v)]


RZ_CASES = {"box3_sparse_softmax_warp-2x5x7-4x9-Cv5-k3": _rz_op, "correspondence_sparse_box3-2x256x8x8-img32-k3": _rz_hot}
for _name, _body in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_op_inside_red_zones(name, monkeypatch):
    """forward + backward under tests/guarded_alloc.guarded: no guard byte changes, every returned tensor and gradient is finite (a read
    outside a buffer, or of one nobody wrote, carries the guard's NaN), every leaf gets its gradient"""
    rz.test_red_zones(name, monkeypatch)
    assert NEW_ENTRIES | {"cocos_transpose_f32"} <= set(rz.COVERAGE[name][0])
