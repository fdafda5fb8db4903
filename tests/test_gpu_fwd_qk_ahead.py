"""The two schedules of the split-precision forward's key-tile loop (corr_fused_fwd_f16x3.hip, QKA): QK(t+1) issued under the
softmax of tile t, against QK / softmax / P.V in turn.  The arithmetic is the same in the same order, so `out`, `lse` and the saved
logits must be EQUAL BIT FOR BIT — on the same operand planes, with the process-wide selection (cocos_corr_fwd_f16x3_qk_ahead)
switched between the two launches.

Shapes: B = 2, Nq = 128 / 256 (one / two query blocks per sample), Nk = 32 (one tile: no next tile at all), 64 (two tiles), 96 (odd
tile count: buffer parity), 160 (five tiles: steady state and the last-tile look-ahead clamp); Cv = 3 (one value block) / 154 (five);
V all float / one-hot label channels from channel 32 on (the lo-plane mask flavour runs when Cv > 32); keys per sample / ONE shared key
set; logits stored / not stored.  The shared-key entry point is inference only (it refuses saved_logits), so that combination runs
without logits only: three pairs of launches per shape.

Every launch runs between red zones (tests/guarded_alloc.py: planes, outputs and the logits buffer are carved out of guarded
buffers, outputs pre-filled with NaN) and with every pointer argument checked against the allocator's live blocks
(tests/test_gpu_live_buffers.py).  One further case runs the ahead schedule through ops.corr_softmax_warp against the fp64 oracle
at tests/test_gpu_parity.py's tolerance: bit-identity alone would not notice two equally wrong kernels."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded_alloc import guarded  # noqa: E402
from test_gpu_live_buffers import _Guard  # noqa: E402

from oracle import corr_oracle as co  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OUT_TOL = 2e-4          # tests/test_gpu_parity.py: max|x - ref| / max|ref| of the forward against the fp64 oracle
B, K = 2, 256
DENSE, SHARED = "cocos_corr_softmax_warp_fwd_f16x3_ex", "cocos_corr_softmax_warp_fwd_f16x3_shared"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


@pytest.fixture()
def schedule(hip_lib):
    """select(mode) -> the library's process-wide selection; the one ops.FWD_QK_AHEAD stands for is put back afterwards"""
    from cocosnet_amd import ops
    yield lambda mode: hip_lib.cocos_corr_fwd_f16x3_qk_ahead(int(mode))
    hip_lib.cocos_corr_fwd_f16x3_qk_ahead(1 if ops.FWD_QK_AHEAD else 0)


def _clear_pools():
    from cocosnet_amd import ops
    ops._tls.zero_pool.clear()
    ops._tls.known_amax.clear()


def _planes(g, Nq, Nk, Cv, onehot, seed):
    """operand planes inside guarded buffers: unit-norm q [B], keys / values per sample (index 0) and of sample 0 alone (index 1)"""
    from cocosnet_amd import ops
    gen = torch.Generator().manual_seed(seed)
    unit = lambda n, N: torch.nn.functional.normalize(torch.randn(n, K, N, generator=gen), dim=1)
    q, k = unit(B, Nq), unit(B, Nk)
    k[:, :, :min(Nq, Nk):3] = q[:, :, :min(Nq, Nk):3]          # some rows peaked: the lazy rescale of O is taken in later tiles too
    v = torch.rand(B, Cv, Nk, generator=gen) * 2 - 1
    if onehot:        # label channels: exact in f16, their lo plane is all zero
        first = min(32, Cv - 1)
        lab = torch.randint(0, Cv - first, (B, 1, Nk), generator=gen)
        v[:, first:] = torch.zeros(B, Cv - first, Nk).scatter_(1, lab, 1.0)
    q, k, v = g.place(q), g.place(k), g.place(v)
    qh, ql = ops.split_f16(q, True, ops.SPLIT_OPERAND_SCALE)
    sets = []
    for kk, vv in ((k, v), (k[:1].contiguous(), v[:1].contiguous())):
        kk, vv = g.place(kk), g.place(vv)
        kh, kl = ops.split_f16(kk, True, ops.SPLIT_OPERAND_SCALE)
        vh, vl, vs, mask = ops.split_f16_chan_mask(vv, ops.absmax(vv), ops.VALUE_LO_SKIP and Cv > 32)
        sets.append(((kh, kl, vh, vl), vs, mask))
    if onehot and Cv > 32:
        assert all(int(m.view(torch.int32).item()) & ~1 == 0 for _, _, m in sets)       # the masked flavour is what runs
    return (qh, ql), sets


def _launch(name, q, kv, vs, mask, Nq, Nk, Cv, stored):
    from cocosnet_amd import _lib, ops
    nan = float("nan")
    out, lse = torch.full((B, Cv, Nq), nan, device=DEV), torch.full((B, Nq), nan, device=DEV)
    lg = torch.full((_lib.load().cocos_corr_softmax_warp_saved_logits_bytes(B, Nq, Nk) // 4,), nan, device=DEV) if stored else None
    head = (q[0].data_ptr(), q[1].data_ptr(), *[t.data_ptr() for t in kv], out.data_ptr(), lse.data_ptr(),
            None if lg is None else lg.data_ptr(), vs.data_ptr(), None if mask is None else mask.data_ptr(), B, K, Nq, Nk, Cv, 100.0,
            ops.SPLIT_OPERAND_SCALE)
    tail = (None, None, None, None, 0) if name == DENSE else (0, 0)
    _lib.call(name, *head, *tail, torch.cuda.current_stream().cuda_stream)
    return out, lse, lg


@pytest.mark.parametrize("onehot", [False, True], ids=["vfloat", "vonehot"])
@pytest.mark.parametrize("Cv", [3, 154])
@pytest.mark.parametrize("Nk", [32, 64, 96, 160])
@pytest.mark.parametrize("Nq", [128, 256])
def test_ahead_schedule_is_bit_identical(Nq, Nk, Cv, onehot, schedule, monkeypatch):
    live = _Guard(monkeypatch)
    with guarded() as g:
        _clear_pools()
        q, sets = _planes(g, Nq, Nk, Cv, onehot, seed=Nq + 7 * Nk + Cv)
        calls = 0
        for name, (kv, vs, mask), stored in ((DENSE, sets[0], True), (DENSE, sets[0], False), (SHARED, sets[1], False)):
            res = {}
            for mode in (0, 1):
                assert schedule(mode) in (0, 1)
                res[mode] = _launch(name, q, kv, vs, mask, Nq, Nk, Cv, stored)
                assert schedule(-1) == mode
                calls += 1
            g.check()
            what = (name, "logits stored" if stored else "no logits")
            for a, b_, part in zip(res[0], res[1], ("out", "lse", "logits")):
                if a is None:
                    assert b_ is None and not stored
                    continue
                assert torch.isfinite(a).all(), (what, part)          # NaN: a slot the kernel left unwritten, or a read outside a buffer
                assert torch.equal(a, b_), (what, part, float((a - b_).abs().max()))
        _clear_pools()
    assert not g.violations, "guard bytes changed:\n" + g.report()
    assert g.guarded_count >= 10 and {DENSE, SHARED} <= g.entries
    live.check(calls, 9 * calls)


def test_ahead_schedule_matches_the_fp64_oracle(schedule, monkeypatch):
    """On path (ops.corr_softmax_warp with FWD_QK_AHEAD; q differentiated, so the training forward that stores its logits) at five
    tiles, two query blocks, five value blocks, against the oracle the forward tests of tests/test_gpu_parity.py use."""
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    monkeypatch.setattr(ops, "FWD_QK_AHEAD", True)
    Nq, Nk, Cv = 256, 160, 154
    rs = np.random.RandomState(3)
    q = rs.standard_normal((B, K, Nq))
    k = rs.standard_normal((B, K, Nk))
    k[:, :, :40] = q[:, :, :40] + 0.05 * rs.standard_normal((B, K, 40))          # some near-one-hot rows
    qn, kn = co.center_l2norm(q, True), co.center_l2norm(k, True)
    v = rs.uniform(-1, 1, (B, Cv, Nk))
    ref = co.corr_softmax_warp(qn, kn, v, 100.0)
    host = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    schedule(0)
    live = _Guard(monkeypatch)
    with guarded() as g:
        _clear_pools()
        out = ops.corr_softmax_warp(g.place(host(qn)).requires_grad_(True), g.place(host(kn)), g.place(host(v)), 100.0)
        g.check()
        _clear_pools()
    assert schedule(-1) == 1                                     # the call selected it
    assert not g.violations, "guard bytes changed:\n" + g.report()
    assert DENSE in g.entries
    live.check(1, 9)
    assert torch.isfinite(out).all()
    err = float(np.abs(out.detach().double().cpu().numpy() - ref).max() / np.abs(ref).max())
    assert err < OUT_TOL, err
