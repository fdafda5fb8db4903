"""K46 on the GPU: ops.soft_match_offset, ops.subcell_warp, hot_path.correspondence_flow and NoVGGCorrespondence.flow_warp.

The reference is tests/match_flow_case.py: the three backward formulas restated in fp64 numpy, the scores from the values of the operand
planes the kernels read (tests/patchmatch_case.plane_values).  The bound on a kernel's tensor is not fixed in advance: the same formulas
are evaluated with plain fp32 torch ops on the device from the fp32 plane values (match_flow_case.t_refine_bwd / t_gather_bwd_off) and
judged against the same fp64 reference; the kernel's error, relative to max |reference| of the tensor, may be at most 4 x that arm's —
the factor covers the different summation order and the third term of the split operands — with a floor of FLOOR = 4 ulps of fp32
(2^-21 of max |reference|) for tensors where the fp32 arm happens to be exact: the kernels round a product, a sum and the final scaling
at least once each.  The hot path's gradients at theta / phi go through K1's backward as well and are judged by the project's bound
for gradients of the split-precision route (tests/test_gpu_parity.GRAD_TOL), as tests/test_gpu_sparse_warp.py judges K42's.

This file sorts before tests/test_gpu_red_zones.py: its red-zone cases (below) have run when that file's "every entry point was reached"
audit counts the three new `cocos_*` literals of cocosnet_amd/ops.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_flow_case as fc  # noqa: E402
import patchmatch_case as pc  # noqa: E402
import test_gpu_red_zones as rz  # noqa: E402
from test_gpu_parity import GRAD_TOL, rel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
B = 2
QGRID = (5, 7)
NQ = QGRID[0] * QGRID[1]
KGRIDS = [(3, 6), (8, 8)]
FLOOR = 2.0 ** -21
FACTOR = 4.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _unit(x):
    x = x.double()
    return (x / x.norm(dim=1, keepdim=True)).float().contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32)


_CASES = {}


def _case(kgrid):
    """(qn, kn, planes, qv, kv, idx, doff) as tests/test_gpu_match_refine.py makes its case: unit-norm columns on the device (every key a
    noisy copy of some query), their operand planes, the fp64 values of those planes, the centre table — random centres, the four
    corners, edges, the interior, out-of-range entries on both sides (so the centres 0 and Nk - 1 are each shared by several queries)
    and, on 8 x 8, no centre within one cell of key (3, 6): that key lies outside every window at r = 1 — and the incoming gradient of
    the offset.  Made once per key grid, never written."""
    from cocosnet_amd import ops
    if kgrid not in _CASES:
        hk, wk = kgrid
        Nk = hk * wk
        g = _gen(460 + Nk)
        q = _unit(torch.randn(B, 256, NQ, generator=g))
        src = torch.randint(0, NQ, (B, Nk), generator=g)
        noise = torch.rand(B, 1, Nk, generator=g) * 2.0
        k = _unit(torch.stack([q[b][:, src[b]] for b in range(B)]) + noise * torch.randn(B, 256, Nk, generator=g) / 16.0)
        q, k = q.to(DEV), k.to(DEV)
        planes = ops.OperandPlanes()
        with torch.no_grad():
            qv = pc.plane_values(*planes.get(q, True, ops.SPLIT_OPERAND_SCALE), ops.SPLIT_OPERAND_SCALE)
            kv = pc.plane_values(*planes.get(k, True, ops.SPLIT_OPERAND_SCALE), ops.SPLIT_OPERAND_SCALE)
        idx = torch.randint(0, Nk, (B, NQ), generator=g)
        if kgrid == (8, 8):
            near = ((idx // wk - 3).abs() <= 1) & ((idx % wk - 6).abs() <= 1)
            idx[near] = 0
        fixed = [0, wk - 1, Nk - wk, Nk - 1,                        # the corners
                 wk // 2, Nk - 1 - wk // 2, wk, 2 * wk - 1,         # the four edges
                 wk + 1, (hk // 2) * wk + wk // 2,                  # the interior
                 -1, Nk, 10 ** 9, -(2 ** 31)]                       # out of range: clamped
        idx[0, :len(fixed)] = torch.tensor(fixed)
        idx[1, NQ - len(fixed):] = torch.tensor(fixed)
        doff = torch.randn(B, NQ, 2, generator=g)
        _CASES[kgrid] = (q, k, planes, qv, kv, idx, doff)
    return _CASES[kgrid]


def _judge(tag, name, got, arm, want):
    """the 4 x rule: both errors relative to max |reference|"""
    e_k, e_a = rel(got, want), rel(arm, want)
    bound = max(FACTOR * e_a, FLOOR)
    print(f"[match_flow] {tag}: {name}: kernel {e_k:.3e}  fp32 torch arm {e_a:.3e}  bound {bound:.3e}  max |ref| {np.abs(want).max():.3e}")
    assert np.isfinite(got.detach().cpu().numpy()).all(), (tag, name)
    assert e_k <= bound, (tag, name, e_k, e_a)


def _kernel_backward(kgrid, r, inv_t, need=(True, True)):
    """(off, lse_win, dq, dk) of ops.soft_match_offset on the shared case, backward with the case's doff"""
    from cocosnet_amd import ops
    qn, kn, _, _, _, idx, doff = _case(kgrid)
    leaves = [t.clone().requires_grad_(n) for t, n in zip((qn, kn), need)]
    off, lse = ops.soft_match_offset(*leaves, idx.to(DEV), kgrid, inv_t, r)
    off.backward(doff.to(DEV))
    torch.cuda.synchronize()
    return off.detach(), lse, leaves[0].grad, leaves[1].grad


def _kernel_ds(kgrid, r, inv_t):
    """ds [B,NQ,W] of cocos_match_refine_bwd_query_f16x3 itself (the op keeps it to itself), dq_t null"""
    from cocosnet_amd import _lib, ops
    qn, kn, planes, _, _, idx, doff = _case(kgrid)
    hk, wk = kgrid
    with torch.no_grad():
        pl = (*planes.get(qn, True, ops.SPLIT_OPERAND_SCALE), *planes.get(kn, True, ops.SPLIT_OPERAND_SCALE))
    table = idx.clamp(0, hk * wk - 1).to(torch.int32).to(DEV)
    g = doff.to(DEV).contiguous()
    ds = torch.full((B, NQ, (2 * r + 1) ** 2), float("nan"), device=DEV)
    _lib.call("cocos_match_refine_bwd_query_f16x3", *(p.data_ptr() for p in pl), table.data_ptr(), g.data_ptr(), ds.data_ptr(), 0, B, 256,
              NQ, hk * wk, hk, wk, r, float(inv_t), ops.SPLIT_OPERAND_SCALE, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return ds


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("kgrid", KGRIDS)
def test_forward_is_the_forward_only_ops_bitwise(kgrid, r):
    from cocosnet_amd import ops
    qn, kn, planes, _, _, idx, _ = _case(kgrid)
    for inv_t in (10.0, 100.0):
        want = ops.match_refine(qn, kn, idx.to(DEV), kgrid, inv_t, r, planes)
        got = ops.soft_match_offset(qn.clone().requires_grad_(True), kn.clone().requires_grad_(True), idx.to(DEV), kgrid, inv_t, r)
        assert got[0].requires_grad and not got[1].requires_grad
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want))
        with torch.no_grad():
            shared = ops.soft_match_offset(qn, kn, idx.to(DEV), kgrid, inv_t, r, planes)
        assert not shared[0].requires_grad and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(shared, want))
    for down in (2, 4):
        img = (torch.rand(B, 3, kgrid[0] * down, kgrid[1] * down, generator=_gen(down)) * 2 - 1).to(DEV)
        hard = ops.gather_patches_subcell(img, idx.to(DEV), want[0], QGRID, kgrid, down)
        soft = ops.subcell_warp(img, idx.to(DEV), want[0].clone().requires_grad_(True), QGRID, kgrid, down)
        assert soft.requires_grad and torch.equal(_bits(soft), _bits(hard))


# ---------------------------------------------------------------------------------------------------------------- the window backward
@pytest.mark.parametrize("inv_t", [10.0, 100.0])
@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("kgrid", KGRIDS)
def test_window_backward_against_the_restatement(kgrid, r, inv_t):
    """ds (from the query kernel itself), dq and dk (through the op) against fp64, each within 4 x the error of the same formulas in
    fp32 torch ops; the slots outside the grid and the keys outside every window are exactly 0 (the buffers are NaN before the launch
    / come from an allocator history of NaN: an element the kernels did not write would show)"""
    _, _, _, qv, kv, idx, doff = _case(kgrid)
    tag = f"key {kgrid} r={r} inv_t={inv_t:g}"
    ds_r, dq_r, dk_r = fc.refine_bwd(qv, kv, idx.numpy(), kgrid, r, inv_t, doff.numpy())
    f32 = lambda t: torch.tensor(t, dtype=torch.float32, device=DEV)      # (the plane values are fp32 sums of two f16: exact here or one rounding)
    ds_a, dq_a, dk_a = fc.t_refine_bwd(f32(qv), f32(kv), idx.to(DEV), kgrid, r, inv_t, doff.to(DEV))
    junk = [torch.full((n,), float("nan"), device=DEV) for n in (B * NQ * 256, B * kgrid[0] * kgrid[1] * 256, B * NQ * 49)]
    del junk
    _, _, dq, dk = _kernel_backward(kgrid, r, inv_t)
    ds = _kernel_ds(kgrid, r, inv_t)
    _judge(tag, "ds", ds, ds_a, ds_r)
    _judge(tag, "dq", dq.transpose(1, 2), dq_a, dq_r)
    _judge(tag, "dk", dk.transpose(1, 2), dk_a, dk_r)
    _, inside, _, _ = fc.t_window(idx, kgrid, r)
    assert bool((ds.cpu()[~inside] == 0).all()) and bool((~inside).any())
    touched = torch.zeros(B, kgrid[0] * kgrid[1], dtype=torch.bool)
    keys, _, _, _ = fc.t_window(idx, kgrid, r)
    for b in range(B):
        touched[b, keys[b][inside[b]]] = True
    if kgrid == (8, 8) and r == 1:
        assert not bool(touched[:, 3 * 8 + 6].any())                      # the key the case keeps out of every window
    dk_rows = dk.transpose(1, 2).cpu()
    assert bool((dk_rows[~touched] == 0).all()) and bool((dk_rows[touched] != 0).any())
    shared = [int((idx[b].clamp(0, kgrid[0] * kgrid[1] - 1) == 0).sum()) for b in range(B)]
    assert min(shared) >= 3                                                # centre 0: named by 0, -1 and -(2^31)


# ---------------------------------------------------------------------------------------------------------------- the sampling backward
def _gather_case(kgrid, down, Be):
    hk, wk = kgrid
    Nk = hk * wk
    g = _gen(90 + down + hk + Be)
    img = torch.rand(Be, 3, hk * down, wk * down, generator=g) * 2 - 1
    idx = torch.randint(0, Nk, (B, NQ), generator=g)
    idx[0, 0], idx[0, 1], idx[1, 2], idx[1, 3] = -1, Nk, 10 ** 9, -(2 ** 31)
    off = (torch.rand(B, NQ, 2, generator=g) * 2 - 1) * 2.99
    # cells whose every sample is clamped at one border: left, right, top, bottom
    border = [(4, 0, (-1.3, 0.4), 0), (5, wk - 1, (1.3, 0.4), 0), (6, 0, (0.4, -1.3), 1), (7, Nk - 1, (0.4, 1.3), 1)]
    for cell, centre, o, _ in border:
        idx[0, cell], off[0, cell] = centre, torch.tensor(o)
    off = fc.away_from_kinks(off, down)
    assert float(off.abs().max()) < 3
    dout = torch.randn(B, 3, QGRID[0] * down, QGRID[1] * down, generator=g)
    return img, idx, off, dout, border


@pytest.mark.parametrize("Be", [B, 1])
@pytest.mark.parametrize("down", [2, 4])
@pytest.mark.parametrize("kgrid", [(3, 6), (5, 7)])
def test_sampling_backward_against_the_restatement(kgrid, down, Be):
    from cocosnet_amd import ops
    img, idx, off, dout, border = _gather_case(kgrid, down, Be)
    want = fc.gather_bwd_off(img.numpy(), idx.numpy(), off.numpy(), dout.numpy(), QGRID, kgrid, down)
    arm = fc.t_gather_bwd_off(img.to(DEV), idx.to(DEV), off.to(DEV), dout.to(DEV), QGRID, kgrid, down)
    leaf = off.to(DEV).requires_grad_(True)
    out = ops.subcell_warp(img.to(DEV), idx.to(DEV), leaf, QGRID, kgrid, down)
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    _judge(f"key {kgrid} down={down} Be={Be}", "doff", leaf.grad, arm, want)
    for cell, _, _, axis in border:
        assert float(leaf.grad[0, cell, axis]) == 0.0 and want[0, cell, axis] == 0.0, (cell, axis)
        assert float(leaf.grad[0, cell, 1 - axis]) != 0.0
    t = off.double() * down
    assert float((t - t.round()).abs().min()) >= 1e-3


# ---------------------------------------------------------------------------------------------------------------- determinism, subsets
def test_backward_twice_subsets_and_a_retained_graph():
    from cocosnet_amd import ops
    kgrid, r, inv_t = (8, 8), 2, 100.0
    a, b = _kernel_backward(kgrid, r, inv_t), _kernel_backward(kgrid, r, inv_t)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    only_q, only_k = _kernel_backward(kgrid, r, inv_t, (True, False)), _kernel_backward(kgrid, r, inv_t, (False, True))
    assert only_q[3] is None and torch.equal(_bits(only_q[2]), _bits(a[2]))
    assert only_k[2] is None and torch.equal(_bits(only_k[3]), _bits(a[3]))
    qn, kn, _, _, _, idx, doff = _case(kgrid)
    q, k = qn.clone().requires_grad_(True), kn.clone().requires_grad_(True)
    off, _ = ops.soft_match_offset(q, k, idx.to(DEV), kgrid, inv_t, r)
    first = torch.autograd.grad(off, (q, k), doff.to(DEV), retain_graph=True)
    second = torch.autograd.grad(off, (q, k), doff.to(DEV))
    assert all(torch.equal(_bits(x), _bits(y)) and torch.equal(_bits(x), _bits(z)) for x, y, z in zip(first, second, a[2:]))
    img, gidx, goff, dout, _ = _gather_case((3, 6), 2, B)
    grads = []
    for _ in range(2):
        leaf = goff.to(DEV).requires_grad_(True)
        out = ops.subcell_warp(img.to(DEV), gidx.to(DEV), leaf, QGRID, (3, 6), 2)
        g1 = torch.autograd.grad(out, leaf, dout.to(DEV), retain_graph=True)[0]
        g2 = torch.autograd.grad(out, leaf, dout.to(DEV))[0]
        assert torch.equal(_bits(g1), _bits(g2))
        grads.append(g1)
    assert torch.equal(_bits(grads[0]), _bits(grads[1]))
    with pytest.raises(ValueError, match="not built"):
        ops.subcell_warp(img.to(DEV).requires_grad_(True), gidx.to(DEV), goff.to(DEV), QGRID, (3, 6), 2)


# ---------------------------------------------------------------------------------------------------------------- hot path and module
@pytest.mark.parametrize("radius,refine_temperature", [(1, None), (2, 0.02)])
def test_correspondence_flow_against_fp64(radius, refine_temperature):
    """2 x 256 x 8 x 8: outputs, and the gradients of a photometric term on warp_out plus a regression term on match_offset at
    theta_raw / phi_raw, against torch-fp64 autograd of the restated pipeline (centre over channels + L2 norm as oracle/torch_ref.py
    states them, the window soft-argmax, the bilinear gather) on the centres the kernel selected"""
    from oracle.torch_ref import _unit_columns
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_flow, correspondence_match
    g = _gen(46 + radius)
    theta0, phi0 = torch.randn(2, 256, 8, 8, generator=g).to(DEV), torch.randn(2, 256, 8, 8, generator=g).to(DEV)
    ref_img = (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).to(DEV)
    g_out, g_off = torch.randn(2, 3, 32, 32, generator=g).to(DEV), torch.randn(2, 2, 8, 8, generator=g).to(DEV)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    theta, phi = theta0.clone().requires_grad_(True), phi0.clone().requires_grad_(True)
    out = correspondence_flow(theta, phi, ref_img, cfg, 0.01, radius=radius, refine_temperature=refine_temperature)
    assert set(out) == {"warp_out", "match_index", "match_offset", "match_xy_sub", "match_window_prob"}
    assert out["warp_out"].shape == (2, 3, 32, 32) and out["match_index"].shape == out["match_window_prob"].shape == (2, 8, 8)
    assert out["match_offset"].shape == out["match_xy_sub"].shape == (2, 2, 8, 8) and out["match_index"].dtype == torch.int64
    assert out["match_offset"].requires_grad and out["match_xy_sub"].requires_grad and not out["match_window_prob"].requires_grad
    m = correspondence_match(theta0, phi0, cfg, 0.01, refine=radius, refine_temperature=refine_temperature)
    assert torch.equal(out["match_index"], m.index) and torch.equal(_bits(out["match_offset"]), _bits(m.offset))
    assert torch.equal(_bits(out["match_window_prob"]), _bits(m.window_prob)) and torch.equal(_bits(out["match_xy_sub"]), _bits(m.xy_sub()))
    ((out["warp_out"] * g_out).sum() + (out["match_offset"] * g_off).sum()).backward()
    torch.cuda.synchronize()
    # fp64
    idx = out["match_index"].reshape(2, 64)
    inv_rt = 100.0 if refine_temperature is None else 1.0 / refine_temperature
    th64, ph64 = theta0.double().requires_grad_(True), phi0.double().requires_grad_(True)
    qn, kn = _unit_columns(th64.reshape(2, 256, -1), True), _unit_columns(ph64.reshape(2, 256, -1), True)
    off = fc.t_refine_off(qn.transpose(1, 2), kn.transpose(1, 2), idx, (8, 8), radius, inv_rt)
    warp = fc.t_gather_subcell(ref_img.double(), idx, off, (8, 8), (8, 8), 4)
    offset = off.reshape(2, 8, 8, 2).permute(0, 3, 1, 2)
    ((warp * g_out.double()).sum() + (offset * g_off.double()).sum()).backward()
    t = off.detach() * 4
    print(f"[match_flow] correspondence_flow r={radius}: closest sample to a pixel boundary {float((t - t.round()).abs().min()):.2e} pixels")
    errs = {"warp_out": rel(out["warp_out"], warp.detach().cpu().numpy()), "match_offset": rel(out["match_offset"], offset.detach().cpu().numpy()),
            "d theta": rel(theta.grad, th64.grad.cpu().numpy()), "d phi": rel(phi.grad, ph64.grad.cpu().numpy())}
    print(f"[match_flow] correspondence_flow r={radius}: " + "  ".join(f"{n} {e:.3e}" for n, e in errs.items()) + f"  (bound {GRAD_TOL:.0e})")
    assert float(th64.grad.abs().max()) > 0 and float(ph64.grad.abs().max()) > 0
    assert all(e < GRAD_TOL for e in errs.values()), errs


def test_module_flow_warp():
    """NoVGGCorrespondence.flow_warp on ade20k_options(match_kernel=1) at a 64 x 64 crop: keys and shapes, match_index / match_offset
    are match(refine=1)'s bit for bit, gradients reach a theta-side and a phi-side convolution weight, none reaches ref_img"""
    from test_gpu_exemplar import _module_case
    net, ref_img, real, seg, ref_seg = _module_case("ade20k_options", 64, 2, 2, match_kernel=1)
    out = net.flow_warp(ref_img, real, seg, ref_seg, radius=1)
    assert {"warp_out", "match_index", "match_offset", "match_xy_sub", "match_window_prob"} <= set(out)
    assert out["warp_out"].shape == (2, 3, 64, 64) and out["match_index"].shape == out["match_window_prob"].shape == (2, 16, 16)
    assert out["match_offset"].shape == out["match_xy_sub"].shape == (2, 2, 16, 16)
    assert all(bool(torch.isfinite(out[n]).all()) for n in ("warp_out", "match_offset", "match_xy_sub", "match_window_prob"))
    with torch.no_grad():
        m = net.match(ref_img, seg, ref_seg, refine=1, hard_warp=True)
    assert torch.equal(out["match_index"], m["match_index"]) and torch.equal(_bits(out["match_offset"]), _bits(m["match_offset"]))
    assert torch.equal(_bits(out["warp_out"]), _bits(m["warp_sub"]))
    (out["warp_out"].square().sum() + out["match_offset"].square().sum()).backward()
    for p in (net.theta.weight, net.phi.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    assert ref_img.grad is None


# ---------------------------------------------------------------------------------------------------------------- red zones
# The cases join tests/test_gpu_red_zones.py's table at import time, as tests/test_gpu_match_refine.py's do.
def _rz_table(seed):
    return torch.randint(-2, 21, (2, 35), generator=torch.Generator().manual_seed(seed))      # 18 keys: out-of-range entries on both sides


def _rz_soft_match_offset(need_k):
    def body(c):
        from cocosnet_amd import ops
        q = c.leaf(rz.unit(2, 256, 35, 71))
        k = (c.leaf if need_k else c.data)(rz.unit(2, 256, 18, 72))
        return [*ops.soft_match_offset(q, k, c.data(_rz_table(73)), (3, 6), 100.0, 2)]
    return body


def _rz_subcell_warp(c):
    from cocosnet_amd import ops
    img, off = c.data(rz.uni(2, 3, 6, 12, seed=74)), c.leaf(rz.uni(2, 35, 2, seed=75) * 2.5)
    return ops.subcell_warp(img, c.data(_rz_table(76)), off, (5, 7), (3, 6), 2)


RZ_CASES = {"soft_match_offset-2x5x7-3x6-r2-dq": (_rz_soft_match_offset(False), "cocos_match_refine_bwd_query_f16x3"),
            "soft_match_offset-2x5x7-3x6-r2-dq-dk": (_rz_soft_match_offset(True), "cocos_match_refine_bwd_key_f16x3"),
            "subcell_warp-2x3x5x7-d2": (_rz_subcell_warp, "cocos_gather_patches_subcell_bwd_off")}
for _name, (_body, _) in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_inside_red_zones(name, monkeypatch):
    """forward + backward on odd sizes with out-of-range centres under tests/guarded_alloc.guarded: no guard byte changes, every
    returned value and gradient is finite (a read outside a buffer, or of one nobody wrote, carries the guard's NaN), every leaf
    gets its gradient"""
    rz.test_red_zones(name, monkeypatch)
    assert RZ_CASES[name][1] in set(rz.COVERAGE[name][0])
