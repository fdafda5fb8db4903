"""K52 on the GPU: ops.box3_soft_match_offset (forward and every gradient), hot_path.correspondence_flow_box3 and
NoVGGCorrespondence.flow_warp_box3 — the trainable sub-cell flow warp on the match_kernel-3 route.

The reference is tests/match_box3_flow_case.py: torch fp64, F.unfold(3, padding=1) -> centre -> normalise -> dot, K44's window rules,
the soft-argmax and the limit; gradients from autograd.  It shares no code with the kernels' tap formulation.

The bound on an op tensor is K46's rule, not a constant: the same formulas run in plain fp32 torch ops on the device from the same fp32
inputs (the arbiter itself, in fp32), judged against the same fp64 reference; the kernel's error, relative to max |reference| of the
tensor, may be at most FACTOR = 4 x that arm's — the factor covers the different summation order — with a floor of 2^-21 of
max |reference| (4 ulps of fp32) for tensors where the fp32 arm happens to be exact.  In the op tests the statistics (mu, a), (nu, b)
are leaves of their own (made in fp64, rounded to fp32), so each of the six gradients the op returns has its own reference;
test_statistics_path makes them with ops.unfold3_stats (K12) as the hot path does and judges the TOTAL derivative.  The hot path's
outputs and gradients are judged by the family's bounds (tests/test_gpu_parity.py: OUT_TOL = 2e-4, GRAD_TOL = 1e-3).

The file name sorts before test_gpu_red_zones.py: its red-zone cases have run when that file's audit is collected."""
import contextlib
import gc
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box3_sparse_case as bc  # noqa: E402
import match_box3_flow_case as xc  # noqa: E402
import match_flow_case as fc  # noqa: E402
import test_gpu_red_zones as rz  # noqa: E402
from test_gpu_live_buffers import _Guard  # noqa: E402
from test_gpu_parity import GRAD_TOL, OUT_TOL, rel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
B = 2
KC = 9 * 256.0
GRIDS = [((2, 2), (2, 2)), ((1, 8), (8, 1)), ((5, 7), (3, 6)), ((6, 6), (8, 8))]
FLOOR = 2.0 ** -21
FACTOR = 4.0
MIB = 2 ** 20
NAMES = ("dtheta", "dphi", "dmu", "da", "dnu", "db")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


@contextlib.contextmanager
def _poisoned_empty():
    """every torch.empty filled with NaN: an output element no wave wrote shows up as a NaN instead of what the allocator's block held"""
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


def _bits(t):
    return t.contiguous().view(torch.int32)


_CASES = {}


def _case(grid, kgrid):
    """(theta, phi, mu, a, nu, b, idx, doff): fp32 on the device except idx (host, int64); the statistics are the fp64 definition rounded
    to fp32.  Made once per shape, shared, never written."""
    key = (grid, kgrid)
    if key not in _CASES:
        theta, phi = bc.features(B, grid, kgrid, 520 + 10 * grid[0] + kgrid[1])
        (mu, a), (nu, b) = bc.stats(theta.double()), bc.stats(phi.double())
        idx = xc.centre_table(B, grid, kgrid, 52 + grid[1])
        doff = torch.randn(B, grid[0] * grid[1], 2, generator=torch.Generator().manual_seed(grid[0] + kgrid[0]))
        _CASES[key] = tuple(t.float().to(DEV) for t in (theta, phi, mu, a, nu, b)) + (idx, doff.to(DEV))
    return _CASES[key]


_REFS = {}


def _ref(grid, kgrid, r, inv_rt):
    """(off, lse_win, six gradients) of the fp64 arbiter on the device, computed once per case"""
    key = (grid, kgrid, r, inv_rt)
    if key not in _REFS:
        *ops6, idx, doff = _case(grid, kgrid)
        leaves = [t.double().requires_grad_(True) for t in ops6]
        off, lse = xc.arbiter_stats(*leaves, idx.to(DEV), r, inv_rt)
        _REFS[key] = (off.detach(), lse.detach(), torch.autograd.grad(off, leaves, doff.double()))
    return _REFS[key]


def _arm(grid, kgrid, r, inv_rt):
    """the same formulas in fp32 torch ops on the device"""
    *ops6, idx, doff = _case(grid, kgrid)
    leaves = [t.clone().requires_grad_(True) for t in ops6]
    off, lse = xc.arbiter_stats(*leaves, idx.to(DEV), r, inv_rt)
    return off.detach(), lse.detach(), torch.autograd.grad(off, leaves, doff)


def _run(grid, kgrid, r, inv_rt, need=(True,) * 6, k12=False, table=None):
    """(off, lse_win, [six gradients]) of the op; `k12`: the statistics come from ops.unfold3_stats of the leaves"""
    from cocosnet_amd import ops
    *ops6, idx, doff = _case(grid, kgrid)
    leaves = [t.clone().requires_grad_(n) for t, n in zip(ops6, need)]
    th, ph = leaves[:2]
    stats = (*ops.unfold3_stats(th, KC), *ops.unfold3_stats(ph, KC)) if k12 else leaves[2:]
    off, lse = ops.box3_soft_match_offset(th, ph, *stats, (idx if table is None else table).to(DEV), grid, kgrid, inv_rt, r)
    assert off.requires_grad and not lse.requires_grad
    off.backward(doff)
    torch.cuda.synchronize()
    return off.detach(), lse, [t.grad for t in leaves]


def _judge(tag, name, got, arm, want):
    """the 4 x rule: both errors relative to max |reference|"""
    want = want.cpu().numpy()
    e_k, e_a = rel(got, want), rel(arm, want)
    bound = max(FACTOR * e_a, FLOOR)
    print(f"[match_box3_flow] {tag}: {name}: kernel {e_k:.3e}  fp32 torch arm {e_a:.3e}  bound {bound:.3e}  max |ref| {abs(want).max():.3e}")
    assert bool(torch.isfinite(got).all()), (tag, name)
    assert e_k <= bound, (tag, name, e_k, e_a)


# ---------------------------------------------------------------------------------------------------------------- the op against fp64
OP_CASES = [(grid, kgrid, r, inv_rt) for grid, kgrid in GRIDS for r in (1, 2, 3) for inv_rt in (10.0, 100.0)]


@pytest.mark.parametrize("grid,kgrid,r,inv_rt", OP_CASES, ids=[f"{_gname(g)}-{_gname(kg)}-r{r}-t{t:g}" for g, kg, r, t in OP_CASES])
def test_op_against_fp64(grid, kgrid, r, inv_rt):
    """off, lse_win and the six gradients, each within 4 x the fp32 arm's error; centres on corners, edges, the interior, out of range,
    one centre all queries of the last batch share; outputs allocated poisoned; the rows of keys outside every window exactly 0"""
    tag = f"{_gname(grid)}/{_gname(kgrid)} r={r} inv_rt={inv_rt:g}"
    with _poisoned_empty():
        off, lse, grads = _run(grid, kgrid, r, inv_rt)
    off_r, lse_r, grads_r = _ref(grid, kgrid, r, inv_rt)
    off_a, lse_a, grads_a = _arm(grid, kgrid, r, inv_rt)
    _judge(tag, "off", off, off_a, off_r)
    _judge(tag, "lse_win", lse, lse_a, lse_r)
    for name, g, g_a, g_r in zip(NAMES, grads, grads_a, grads_r):
        _judge(tag, name, g, g_a, g_r)
    assert float(off.abs().max()) <= r
    idx = _case(grid, kgrid)[6]
    Nk = kgrid[0] * kgrid[1]
    assert bool((idx[B - 1] == 0).all()) and bool(((idx[0] < 0) | (idx[0] >= Nk)).any())      # the hub; out-of-range entries
    window, reach = xc.touched(idx, kgrid, r), xc.touched(idx, kgrid, r, reach=1)
    dph, dnu, db = grads[1].reshape(B, 256, Nk).cpu(), grads[4].cpu(), grads[5].cpu()
    assert bool((dnu[~window] == 0).all()) and bool((db[~window] == 0).all())
    assert bool((dph.transpose(1, 2)[~reach] == 0).all())
    if kgrid == (8, 8):      # the hub's batch: key 0 is the only centre, everything further than the window is in nobody's
        assert not bool(window[B - 1].all()) and bool((dnu[window] != 0).any())
        if r < 3:
            assert not bool(reach[B - 1].all())


@pytest.mark.parametrize("r", [1, 2, 3])
def test_slots_outside_the_grid_are_zero(r):
    """the kernels themselves on NaN-filled outputs: c, g and hb are written in every slot, 0 where the slot lies outside the grid"""
    from cocosnet_amd import _lib, ops
    grid, kgrid = (5, 7), (3, 6)
    theta, phi, mu, a, nu, b, idx, doff = _case(grid, kgrid)
    Nq, Nk, W = 35, 18, (2 * r + 1) ** 2
    th_t, ph_t = ops._transpose(theta.reshape(B, 256, Nq)), ops._transpose(phi.reshape(B, 256, Nk))
    table = idx.clamp(0, Nk - 1).to(torch.int32).to(DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    off, lse, c, g, hb, dmu, da = nan(B, Nq, 2), nan(B, Nq), nan(B, Nq, W), nan(B, Nq, W), nan(B, Nq, W), nan(B, Nq), nan(B, Nq)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("cocos_box3_match_refine_fwd", th_t.data_ptr(), ph_t.data_ptr(), mu.data_ptr(), a.data_ptr(), nu.data_ptr(), b.data_ptr(),
              table.data_ptr(), off.data_ptr(), lse.data_ptr(), c.data_ptr(), B, 256, *grid, *kgrid, r, 100.0, st)
    _lib.call("cocos_box3_match_refine_bwd_pair", table.data_ptr(), c.data_ptr(), a.data_ptr(), nu.data_ptr(), b.data_ptr(),
              doff.data_ptr(), g.data_ptr(), hb.data_ptr(), dmu.data_ptr(), da.data_ptr(), B, 256, *grid, *kgrid, r, 100.0, st)
    torch.cuda.synchronize()
    inside = fc.t_window(idx, kgrid, r)[1].to(DEV)
    assert bool((~inside).any())
    for name, t in (("c", c), ("g", g), ("hb", hb)):
        assert bool(torch.isfinite(t).all()), name
        assert bool((t[~inside] == 0).all()), name
        assert bool((t[inside] != 0).any()), name
    assert all(bool(torch.isfinite(t).all()) for t in (off, lse, dmu, da))


def test_int32_and_int64_tables_agree_bitwise():
    idx = _case((5, 7), (3, 6))[6]
    x, y = _run((5, 7), (3, 6), 2, 100.0), _run((5, 7), (3, 6), 2, 100.0, table=idx.clamp(-5, 50).to(torch.int32))
    assert torch.equal(_bits(x[0]), _bits(y[0])) and torch.equal(_bits(x[1]), _bits(y[1]))
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(x[2], y[2]))


# ---------------------------------------------------------------------------------------------------------------- subsets, determinism
@pytest.mark.parametrize("need", [s for s in itertools.product([False, True], repeat=2) if any(s)],
                         ids=lambda s: "".join(n for n, on in zip("tp", s) if on))
def test_gradient_subsets(need):
    """each non-empty subset of {theta, phi} with the statistics from K12: None outside it, and inside it the full run's gradients, bit
    for bit; then the statistics alone as leaves"""
    full = _run((5, 7), (3, 6), 2, 100.0, k12=True)
    off, lse, grads = _run((5, 7), (3, 6), 2, 100.0, need + (False,) * 4, k12=True)
    assert torch.equal(_bits(off), _bits(full[0])) and torch.equal(_bits(lse), _bits(full[1]))
    for g, g_all, on in zip(grads[:2], full[2][:2], need):
        assert (g is None) if not on else torch.equal(_bits(g), _bits(g_all))
    leaves_all = _run((5, 7), (3, 6), 2, 100.0)
    for only in range(6):
        got = _run((5, 7), (3, 6), 2, 100.0, tuple(n == only for n in range(6)))
        assert all((g is None) if n != only else torch.equal(_bits(g), _bits(leaves_all[2][n])) for n, g in enumerate(got[2])), NAMES[only]


def test_same_call_twice_same_bits_and_a_retained_graph():
    """forward + backward twice on the table with the hub (one centre for every query of a batch: the longest serial list), with another
    allocator history in between; then the backward twice through one retained graph"""
    from cocosnet_amd import ops
    grid, kgrid, r = (6, 6), (8, 8), 3
    x = _run(grid, kgrid, r, 100.0, k12=True)
    junk = [torch.full((n,), float("nan"), device=DEV) for n in (B * 36 * 256, B * 64 * 256, B * 36 * 49, B * 36 * 49)]
    del junk
    y = _run(grid, kgrid, r, 100.0, k12=True)
    assert torch.equal(_bits(x[0]), _bits(y[0])) and torch.equal(_bits(x[1]), _bits(y[1]))
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(x[2][:2], y[2][:2]))
    theta, phi, _, _, _, _, idx, doff = _case(grid, kgrid)
    th, ph = theta.clone().requires_grad_(True), phi.clone().requires_grad_(True)
    off, _ = ops.box3_soft_match_offset(th, ph, *ops.unfold3_stats(th, KC), *ops.unfold3_stats(ph, KC), idx.to(DEV), grid, kgrid, 100.0, r)
    first = torch.autograd.grad(off, (th, ph), doff, retain_graph=True)
    second = torch.autograd.grad(off, (th, ph), doff)
    assert all(torch.equal(_bits(p), _bits(q)) and torch.equal(_bits(p), _bits(s)) for p, q, s in zip(first, second, x[2][:2]))


# ---------------------------------------------------------------------------------------------------------------- statistics path
def test_statistics_path():
    """theta and phi as leaves, (mu, a, nu, b) from ops.unfold3_stats of them: the gradients equal the arbiter's TOTAL derivative within
    the family's bound.  The share that travels through dmu / da / dnu / db is reported: the run with the statistics detached misses
    the arbiter by more than the bound, so this fails when those terms are dropped."""
    from cocosnet_amd import ops
    grid, kgrid, r, inv_rt = (5, 7), (3, 6), 2, 100.0
    theta, phi, _, _, _, _, idx, doff = _case(grid, kgrid)
    th64, ph64 = theta.double().requires_grad_(True), phi.double().requires_grad_(True)
    off_r, _ = xc.arbiter(th64, ph64, idx.to(DEV), r, inv_rt)
    want = torch.autograd.grad(off_r, (th64, ph64), doff.double())
    off, _, grads = _run(grid, kgrid, r, inv_rt, (True, True) + (False,) * 4, k12=True)
    errs = [rel(off, off_r.detach().cpu().numpy())] + [rel(g, w.cpu().numpy()) for g, w in zip(grads[:2], want)]
    print(f"[match_box3_flow] statistics from K12: rel off {errs[0]:.3e}  dtheta {errs[1]:.3e}  dphi {errs[2]:.3e}")
    assert errs[0] < OUT_TOL and max(errs[1:]) < GRAD_TOL, errs
    th, ph = theta.clone().requires_grad_(True), phi.clone().requires_grad_(True)
    with torch.no_grad():
        stats = (*ops.unfold3_stats(th, KC), *ops.unfold3_stats(ph, KC))
    ops.box3_soft_match_offset(th, ph, *stats, idx.to(DEV), grid, kgrid, inv_rt, r)[0].backward(doff)
    share = [rel(t.grad, w.cpu().numpy()) for t, w in zip((th, ph), want)]
    print(f"[match_box3_flow] statistics detached: rel dtheta {share[0]:.3e}  dphi {share[1]:.3e} (the statistics' share of the gradient)")
    assert min(share) > GRAD_TOL, share


# ---------------------------------------------------------------------------------------------------------------- hot path
def _hot_case(Bq, fh, seed, down=4):
    g = torch.Generator().manual_seed(seed)
    theta, phi = bc.features(Bq, (fh, fh), (fh, fh), seed)
    H = fh * down
    ref_img = torch.rand(Bq, 3, H, H, generator=g) * 2 - 1
    g_out, g_off = torch.randn(Bq, 3, H, H, generator=g), torch.randn(Bq, 2, fh, fh, generator=g)
    return tuple(t.to(DEV) for t in (theta, phi, ref_img, g_out, g_off))


def _hot_check(tag, Bq, fh, radius, refine_temperature, seed, memory=False):
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_flow_box3, correspondence_match
    theta0, phi0, ref_img, g_out, g_off = _hot_case(Bq, fh, seed)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    theta, phi = theta0.clone().requires_grad_(True), phi0.clone().requires_grad_(True)
    if memory:
        rz._clear_pools()
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
    out = correspondence_flow_box3(theta, phi, ref_img, cfg, 0.01, radius=radius, refine_temperature=refine_temperature)
    if memory:
        torch.cuda.synchronize()
        held, peak = torch.cuda.memory_allocated() - before, torch.cuda.max_memory_allocated() - before
        print(f"[match_box3_flow] {tag}: held after the forward {held / MIB:.1f} MiB (bound {4096 * 4096 * 4 / MIB:.0f} MiB); peak during "
              f"it, the selection's T included: {peak / MIB:.1f} MiB")
        assert held < 4096 * 4096 * 4, held
    H = fh * 4
    assert set(out) == {"warp_out", "match_index", "match_offset", "match_xy_sub", "match_window_prob"}
    assert out["warp_out"].shape == (Bq, 3, H, H) and out["match_index"].shape == out["match_window_prob"].shape == (Bq, fh, fh)
    assert out["match_offset"].shape == out["match_xy_sub"].shape == (Bq, 2, fh, fh) and out["match_index"].dtype == torch.int64
    assert out["match_offset"].requires_grad and out["match_xy_sub"].requires_grad and not out["match_window_prob"].requires_grad
    m = correspondence_match(theta0, phi0, cfg, 0.01)
    assert torch.equal(out["match_index"], m.index)
    del m
    assert bool(torch.isfinite(out["match_window_prob"]).all()) and float(out["match_window_prob"].min()) > 0
    loss = (out["warp_out"] * g_out).sum() + (out["match_offset"] * g_off).sum()
    if memory:
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
    loss.backward()
    torch.cuda.synchronize()
    if memory:
        peak = torch.cuda.max_memory_allocated() - before
        print(f"[match_box3_flow] {tag}: peak during the backward {peak / MIB:.1f} MiB")
        assert peak < 4096 * 4096 * 4, peak
    # torch fp64 autograd of the restated pipeline on the selected centres
    idx = out["match_index"].reshape(Bq, fh * fh)
    inv_rt = 100.0 if refine_temperature is None else 1.0 / refine_temperature
    th64, ph64 = theta0.double().requires_grad_(True), phi0.double().requires_grad_(True)
    off, _ = xc.arbiter(th64, ph64, idx, radius, inv_rt)
    warp = fc.t_gather_subcell(ref_img.double(), idx, off, (fh, fh), (fh, fh), 4)
    offset = off.reshape(Bq, fh, fh, 2).permute(0, 3, 1, 2)
    ((warp * g_out.double()).sum() + (offset * g_off.double()).sum()).backward()
    t = off.detach() * 4
    print(f"[match_box3_flow] {tag}: closest sample to a pixel boundary {float((t - t.round()).abs().min()):.2e} pixels")
    errs = {"warp_out": rel(out["warp_out"], warp.detach().cpu().numpy()), "match_offset": rel(out["match_offset"], offset.detach().cpu().numpy()),
            "d theta": rel(theta.grad, th64.grad.cpu().numpy()), "d phi": rel(phi.grad, ph64.grad.cpu().numpy())}
    print(f"[match_box3_flow] {tag}: " + "  ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    assert float(th64.grad.abs().max()) > 0 and float(ph64.grad.abs().max()) > 0
    assert all(e < (GRAD_TOL if n.startswith("d ") else OUT_TOL) for n, e in errs.items()), errs


@pytest.mark.parametrize("radius,refine_temperature", [(1, None), (2, 0.02)])
def test_hot_path_chain_selection(radius, refine_temperature):
    """B = 2, 8 x 8: the selection is the materialised chain (the fused family does not take the grid)"""
    from cocosnet_amd import ops
    assert not ops.box3_fused_ok(2, 256, 8, 8)
    _hot_check(f"chain 2x8x8 r={radius}", 2, 8, radius, refine_temperature, 52 + radius)


def test_hot_path_fused_selection_and_memory():
    """B = 1, 64 x 64, r = 1: the smallest shape the fused family takes — the selection is K37 on T; the arbiter runs on the GPU.  What
    stays allocated after the forward, and the backward's peak, stay below the size of ONE T (4096^2 x 4 bytes = 64 MiB)"""
    from cocosnet_amd import ops
    assert ops.box3_fused_ok(1, 256, 64, 64)
    _hot_check("fused 1x64x64 r=1", 1, 64, 1, None, 57, memory=True)


def test_module_flow_warp_box3(monkeypatch):
    """NoVGGCorrespondence.flow_warp_box3 on ade20k_options(match_kernel=3) at a 64 x 64 crop: keys and shapes, match_index is match()'s,
    the call under no_grad gives the differentiable call's bits, a zero offset gives gather_patches' copy, and a photometric loss
    reaches a theta-side and a phi-side convolution weight with finite, non-zero gradients (none reaches ref_img)"""
    from cocosnet_amd import ops
    from test_gpu_exemplar import _module_case
    net, ref_img, real, seg, ref_seg = _module_case("ade20k_options", 64, 2, 2, match_kernel=3)
    out = net.flow_warp_box3(ref_img, real, seg, ref_seg, radius=1)
    assert {"warp_out", "match_index", "match_offset", "match_xy_sub", "match_window_prob"} <= set(out)
    assert out["warp_out"].shape == (2, 3, 64, 64) and out["match_index"].shape == out["match_window_prob"].shape == (2, 16, 16)
    assert out["match_offset"].shape == out["match_xy_sub"].shape == (2, 2, 16, 16)
    assert all(bool(torch.isfinite(out[n]).all()) for n in ("warp_out", "match_offset", "match_xy_sub", "match_window_prob"))
    with torch.no_grad():
        m = net.match(ref_img, seg, ref_seg)
        plain = net.flow_warp_box3(ref_img, real, seg, ref_seg, radius=1)
    assert torch.equal(out["match_index"], m["match_index"])
    assert not plain["warp_out"].requires_grad and not plain["match_offset"].requires_grad
    for n in ("warp_out", "match_offset", "match_xy_sub", "match_window_prob"):
        assert torch.equal(_bits(plain[n]), _bits(out[n])), n
    assert torch.equal(plain["match_index"], out["match_index"])
    real_op = ops.box3_soft_match_offset

    def zero_offset(*args, **kw):
        off, lse_win = real_op(*args, **kw)
        return torch.zeros_like(off), lse_win

    monkeypatch.setattr(ops, "box3_soft_match_offset", zero_offset)
    with torch.no_grad():
        forced = net.flow_warp_box3(ref_img, real, seg, ref_seg, radius=1)
    monkeypatch.setattr(ops, "box3_soft_match_offset", real_op)
    assert torch.equal(forced["match_index"], out["match_index"]) and bool((forced["match_offset"] == 0).all())
    assert torch.equal(_bits(forced["warp_out"]), _bits(ops.gather_patches(ref_img, out["match_index"], 16, 16, 4)))
    (out["warp_out"] - real).square().mean().backward()
    for p in (net.theta.weight, net.phi.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    assert ref_img.grad is None


# ---------------------------------------------------------------------------------------------------------------- live buffers
def test_op_hands_over_live_buffers_only(monkeypatch):
    """one forward + backward of the op with every pointer argument of every entry point checked against the allocator's live blocks
    (tests/test_gpu_live_buffers.py's guard)"""
    guard = _Guard(monkeypatch)
    _run((5, 7), (3, 6), 2, 100.0, k12=True)
    guard.check(8, 30)


# ---------------------------------------------------------------------------------------------------------------- red zones
# The cases join tests/test_gpu_red_zones.py's table at import time, as the K36 - K51 files' cases do, so its coverage report and its
# "every entry point was reached" audit count the four K52 entry points; this file runs them.
NEW_ENTRIES = {"cocos_box3_match_refine_fwd", "cocos_box3_match_refine_bwd_pair", "cocos_box3_match_refine_bwd_theta",
               "cocos_box3_match_refine_bwd_key"}


def _rz_op(c):
    """odd sizes, unequal grids, out-of-range centres, a hub; forward and backward with every gradient (the statistics from K12)"""
    from cocosnet_amd import ops
    theta, phi = bc.features(2, (5, 7), (4, 9), 71)
    th, ph = c.leaf(theta), c.leaf(phi)
    idx = xc.centre_table(2, (5, 7), (4, 9), 72)
    (mu, a), (nu, b) = ops.unfold3_stats(th, KC), ops.unfold3_stats(ph, KC)
    return [*ops.box3_soft_match_offset(th, ph, mu, a, nu, b, c.data(idx), (5, 7), (4, 9), 100.0, 2)]


def _rz_hot(c):
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_flow_box3
    theta, phi = bc.features(2, (8, 8), (8, 8), 74)
    th, ph = c.leaf(theta), c.leaf(phi)
    ref_img = c.data(rz.uni(2, 3, 32, 32, seed=75))
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4, isTrain=True)
    out = correspondence_flow_box3(th, ph, ref_img, cfg, 0.01, radius=3)
    return [v for v in out.values() if torch.is_tensor(v)]


RZ_CASES = {"box3_soft_match_offset-2x5x7-4x9-r2": _rz_op, "correspondence_flow_box3-2x256x8x8-img32-r3": _rz_hot}
for _name, _body in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_op_inside_red_zones(name, monkeypatch):
    """forward + backward under tests/guarded_alloc.guarded: no guard byte changes, every returned tensor and gradient is finite (a read
    outside a buffer, or of one nobody wrote, carries the guard's NaN), every leaf gets its gradient"""
    rz.test_red_zones(name, monkeypatch)
    assert NEW_ENTRIES | {"cocos_transpose_f32"} <= set(rz.COVERAGE[name][0])
