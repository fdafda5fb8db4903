"""K42 on the GPU: ops.sparse_softmax_warp (forward and the three gradients), hot_path.correspondence_sparse and
NoVGGCorrespondence.sparse_warp.

The reference is `_ref` below, a torch fp64 restatement of the definition on the SAME idx, with autograd for the gradients:
    s[b,i,r] = inv_t <qn[b,:,i], kn[b,:,idx[b,i,r]]>,  w = softmax_r s,  out[b,:,i] = sum_r w[b,i,r] v[b,:,idx[b,i,r]].
Tolerances are tests/test_gpu_parity.py's (imported): OUT_TOL on outputs, GRAD_TOL on gradients, its `rel` measure.  No floor is needed:
with k = 1 the logit gradients are exactly zero on both sides (w = 1, ds = w (dw - w dw) = 0), everywhere else the largest reference
entry is far from zero."""
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_red_zones as rz  # noqa: E402
from test_gpu_parity import GRAD_TOL, OUT_TOL, rel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INV_T = 100.0
B = 2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _unit(x):
    x = x.double()
    return (x / x.norm(dim=1, keepdim=True)).float().contiguous()


def _gather(t, idx):
    """t [B,C,Nk], idx [B,Nq,k] -> [B,Nq,k,C]"""
    return torch.stack([t[b].t()[idx[b]] for b in range(t.shape[0])])


def _ref(qn, kn, v, idx, inv_t=INV_T, weights=False):
    """the definition in the dtype of its inputs (fp64 in every test)"""
    s = inv_t * torch.einsum("bci,birc->bir", qn, _gather(kn, idx))
    w = torch.softmax(s, dim=-1)
    out = torch.einsum("bir,birc->bci", w, _gather(v, idx))
    return (out, w) if weights else out


def _ref_grads(qn, kn, v, idx, dout):
    leaves = [t.double().clone().requires_grad_(True) for t in (qn, kn, v)]
    out = _ref(*leaves, idx.long())
    out.backward(dout.double())
    return out.detach(), [t.grad for t in leaves]


def _run(qn, kn, v, idx, dout, need=(True, True, True)):
    from cocosnet_amd import ops
    leaves = [t.clone().requires_grad_(n) for t, n in zip((qn, kn, v), need)]
    out = ops.sparse_softmax_warp(*leaves, idx, INV_T)
    out.backward(dout)
    torch.cuda.synchronize()
    return out.detach(), [t.grad for t in leaves]


_CASES = {}


def _case(Nq, Nk, Cv):
    """(qn, kn, v, dout, L fp64 logits) on the device: unit-norm random columns with a few keys planted next to chosen queries (peaked
    rows next to diffuse ones).  Made once per shape, shared, never written."""
    key = (Nq, Nk, Cv)
    if key not in _CASES:
        g = _gen(Nq * 1000 + Nk + Cv)
        q = _unit(torch.randn(B, 256, Nq, generator=g))
        k = torch.randn(B, 256, Nk, generator=g)
        for n, (i, j) in enumerate([(0, 3), (5, Nk - 1), (Nq - 1, 0), (7, 3)]):      # (key 3 is planted twice: the last one stays)
            k[:, :, j] = q[:, :, i] * 4.0 + 0.2 * (n + 1) * torch.randn(B, 256, generator=g)
        k = _unit(k)
        v = torch.randn(B, Cv, Nk, generator=g)
        dout = torch.randn(B, Cv, Nq, generator=g)
        q, k, v, dout = (t.to(DEV) for t in (q, k, v, dout))
        L = INV_T * torch.einsum("bci,bcj->bij", q.double(), k.double())
        _CASES[key] = (q, k, v, dout, L)
    return _CASES[key]


def _judge(tag, got, want):
    (out, grads), (out_r, grads_r) = got, want
    errs = [rel(out, out_r.cpu().numpy())] + [rel(g, r.cpu().numpy()) for g, r in zip(grads, grads_r)]
    print(f"[sparse_warp] {tag}: rel out {errs[0]:.3e}  dqn {errs[1]:.3e}  dkn {errs[2]:.3e}  dv {errs[3]:.3e}")
    assert all(bool(torch.isfinite(t).all()) for t in [out] + grads), tag
    assert errs[0] < OUT_TOL, (tag, errs)
    assert max(errs[1:]) < GRAD_TOL, (tag, errs)


# ---------------------------------------------------------------------------------------------------------------- the op against fp64
@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("Cv", [3, 5, 154])
@pytest.mark.parametrize("Nq,Nk", [(64, 64), (96, 160)])
def test_op_against_fp64(Nq, Nk, Cv, k):
    qn, kn, v, dout, L = _case(Nq, Nk, Cv)
    idx = L.topk(k, dim=-1).indices
    _judge(f"({Nq},{Nk}) Cv={Cv} k={k}", _run(qn, kn, v, idx, dout), _ref_grads(qn, kn, v, idx, dout))


def test_int32_and_int64_tables_agree_bitwise():
    qn, kn, v, dout, L = _case(64, 64, 5)
    idx = L.topk(4, dim=-1).indices
    a, b = _run(qn, kn, v, idx, dout), _run(qn, kn, v, idx.to(torch.int32), dout)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


# ---------------------------------------------------------------------------------------------------------------- adversarial tables
def _table(kind):
    """idx [B,64,4] for Nq = Nk = 64"""
    _, _, _, _, L = _case(64, 64, 5)
    idx = L.topk(4, dim=-1).indices.clone()
    if kind == "hub":                        # every query names key 0 in rank 0 (a row may then hold 0 twice: legal)
        idx[:, :, 0] = 0
    elif kind == "half":                     # only even keys are named
        idx = 2 * torch.randint(0, 32, (B, 64, 4), generator=_gen(7)).to(DEV)
    elif kind == "repeat":                   # rows with one key two and four times
        idx[:, 3, 1] = idx[:, 3, 0]
        idx[:, 9, :] = idx[:, 9, :1]
    elif kind == "range":                    # values outside [0, Nk): clamped
        idx[:, 1, 0], idx[:, 2, 3], idx[:, 4, 2], idx[0, 5, 1] = -1, 64, 10 ** 9, -(2 ** 40)
    return idx


@pytest.mark.parametrize("kind", ["hub", "half", "repeat", "range"])
def test_adversarial_index_tables(kind):
    qn, kn, v, dout, _ = _case(64, 64, 5)
    idx = _table(kind)
    if kind == "half":
        # allocator history: the blocks the op's torch.empty calls are about to reuse hold NaN — a key nobody names must get its zeros
        # from the kernel, not from a fill that happened to be there
        junk = [torch.full((n,), float("nan"), device=DEV) for n in (B * 64 * 256, B * 64 * 256, B * 64 * 5, B * 64 * 5, B * 64 * 4)]
        del junk
    got = _run(qn, kn, v, idx, dout)
    _judge(kind, got, _ref_grads(qn, kn, v, idx.clamp(0, 63), dout))
    if kind == "half":
        _, (_, dkn, dv) = got
        assert bool((dkn[:, :, 1::2] == 0).all()) and bool((dv[:, :, 1::2] == 0).all())
        assert bool((dkn[:, :, 0::2] != 0).any()) and bool((dv[:, :, 0::2] != 0).any())
        _, (_, dkn2, dv2) = _run(qn, kn, v, idx, dout)       # a second history: the same bits
        assert torch.equal(dkn, dkn2) and torch.equal(dv, dv2)


# ---------------------------------------------------------------------------------------------------------------- dense limit
def test_full_support_is_the_dense_op():
    """Nq = Nk = 8, k = 8, idx = arange: the sparse op at full support against ops.corr_softmax_warp on the same inputs"""
    from cocosnet_amd import ops
    g = _gen(88)
    qn, kn = _unit(torch.randn(B, 256, 8, generator=g)).to(DEV), _unit(torch.randn(B, 256, 8, generator=g)).to(DEV)
    v, dout = torch.randn(B, 5, 8, generator=g).to(DEV), torch.randn(B, 5, 8, generator=g).to(DEV)
    idx = torch.arange(8, device=DEV).expand(B, 8, 8).contiguous()
    out, grads = _run(qn, kn, v, idx, dout)
    leaves = [t.clone().requires_grad_(True) for t in (qn, kn, v)]
    dense = ops.corr_softmax_warp(*leaves, INV_T)
    dense.backward(dout)
    errs = [rel(out, dense.detach().cpu().numpy())] + [rel(a, b.grad.cpu().numpy()) for a, b in zip(grads, leaves)]
    print(f"[sparse_warp] dense limit: rel out {errs[0]:.3e}  dqn {errs[1]:.3e}  dkn {errs[2]:.3e}  dv {errs[3]:.3e}")
    assert max(errs) < OUT_TOL, errs


# ---------------------------------------------------------------------------------------------------------------- determinism, subsets
def test_same_call_twice_same_bits():
    qn, kn, v, dout, L = _case(96, 160, 154)
    idx = L.topk(8, dim=-1).indices
    idx[:, ::2, 0] = 7                       # a long list for one key
    a, b = _run(qn, kn, v, idx, dout), _run(qn, kn, v, idx, dout)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("need", [s for s in itertools.product([False, True], repeat=3) if any(s)],
                         ids=lambda s: "".join(n for n, on in zip("qkv", s) if on))
def test_gradient_subsets(need):
    """each non-empty subset of {qn, kn, v}: None outside it, and inside it the all-three run's gradients (every gradient is computed by
    the same launches whichever others are asked for: the same bits)"""
    qn, kn, v, dout, L = _case(96, 160, 5)
    idx = L.topk(3, dim=-1).indices
    out_all, grads_all = _run(qn, kn, v, idx, dout)
    out, grads = _run(qn, kn, v, idx, dout, need)
    assert torch.equal(out, out_all)
    for g, g_all, on in zip(grads, grads_all, need):
        assert (g is None) if not on else torch.equal(g, g_all)
    _judge(f"subset {need}", (out_all, grads_all), _ref_grads(qn, kn, v, idx, dout))


def test_no_grad_forward_and_weights():
    from cocosnet_amd import ops
    qn, kn, v, _, L = _case(64, 64, 5)
    idx = L.topk(4, dim=-1).indices
    with torch.no_grad():
        out, w = ops.sparse_softmax_warp(qn, kn, v, idx, INV_T, return_weights=True)
    out_r, w_r = _ref(qn.double(), kn.double(), v.double(), idx, weights=True)
    assert not out.requires_grad and w.shape == (B, 64, 4)
    assert rel(out, out_r.cpu().numpy()) < OUT_TOL and rel(w, w_r.cpu().numpy()) < OUT_TOL


# ---------------------------------------------------------------------------------------------------------------- memory
def test_nothing_hw_by_hw_is_allocated():
    """B = 2, a 64 x 64 grid, Cv = 3, k = 8, forward + backward with all three gradients: the peak above what is allocated when the op is
    called stays below a QUARTER of one fp32 logits matrix (B N N 4 / 4 bytes = 33.5 MB) — a condition, not a measurement.
    The candidates come from ops.corr_topk on a shared OperandPlanes, as in correspondence_sparse, so the four operand planes
    (4 x B N 256 x 2 bytes = 16.8 MB) exist when the op is called: they are the selection's, the op adds none.  What the op must add is
    its two operand gradients (2 x B 256 N x 4 bytes = 16.8 MB: half of the bound before anything else) plus its [B,N,k] state."""
    from cocosnet_amd import ops
    N, Cv, k = 4096, 3, 8
    g = _gen(4096)
    qn, kn = (_unit(torch.randn(B, 256, N, generator=g)).to(DEV).requires_grad_(True) for _ in range(2))
    v = torch.randn(B, Cv, N, generator=g).to(DEV).requires_grad_(True)
    dout = torch.randn(B, Cv, N, generator=g).to(DEV)
    planes = ops.OperandPlanes()
    with torch.no_grad():
        for t in (qn, kn):
            planes.get(t, True, ops.SPLIT_OPERAND_SCALE)
    idx, _, _ = ops.corr_topk(qn, kn, INV_T, k, planes)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.sparse_softmax_warp(qn, kn, v, idx, INV_T, planes)
    out.backward(dout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"[sparse_warp] peak above the inputs and the selection's planes: {peak / 2 ** 20:.1f} MiB (bound {B * N * N / 2 ** 20:.1f} MiB)")
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in (qn, kn, v))
    assert peak < B * N * N * 4 // 4, peak


# ---------------------------------------------------------------------------------------------------------------- hot path and module
def _hot_ref(theta, phi, ref_img, ref_seg, idx, down, direct, inv_t):
    """fp64: centre over channels + L2 norm as oracle/torch_ref.py states them, then gather, softmax and blend on `idx`, then nearest
    up-sampling of the image channels"""
    import torch.nn.functional as F
    from oracle.torch_ref import _unit_columns
    Bq, C, fh, fw = theta.shape
    qn, kn = _unit_columns(theta.reshape(Bq, C, -1), True), _unit_columns(phi.reshape(Bq, C, -1), True)
    vals = [F.avg_pool2d(ref_img.double(), down).reshape(Bq, 3, -1)]
    if direct:
        vals.append(F.interpolate(ref_seg.double(), scale_factor=1 / down, mode="nearest").reshape(Bq, ref_seg.shape[1], -1))
    o = _ref(qn, kn, torch.cat(vals, 1), idx, inv_t)
    warp = F.interpolate(o[:, :3].reshape(Bq, 3, fh, fw), scale_factor=down, mode="nearest")
    return warp, (o[:, 3:].reshape(Bq, -1, fh, fw) if direct else None)


@pytest.mark.parametrize("topk", [1, 4])
@pytest.mark.parametrize("losstype", ["direct", "none"])
def test_correspondence_sparse_against_fp64(losstype, topk):
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match, correspondence_sparse
    g = _gen(31 + topk)
    theta0, phi0 = torch.randn(2, 256, 8, 8, generator=g).to(DEV), torch.randn(2, 256, 8, 8, generator=g).to(DEV)
    ref_img = (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).to(DEV)
    onehot = lambda: torch.zeros(2, 5, 32, 32).scatter_(1, torch.randint(0, 5, (2, 1, 32, 32), generator=g), 1.0).to(DEV)
    seg, ref_seg = onehot(), onehot()
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4, warp_mask_losstype=losstype)
    direct = losstype == "direct"
    theta, phi = theta0.clone().requires_grad_(True), phi0.clone().requires_grad_(True)
    out = correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, 0.01, topk)
    assert set(out) == {"warp_out", "match_index", "match_weight"} | ({"warp_mask"} if direct else set())
    assert out["warp_out"].shape == (2, 3, 32, 32) and out["match_index"].shape == out["match_weight"].shape == (2, topk, 8, 8)
    assert out["match_index"].dtype == torch.int64 and not out["match_weight"].requires_grad
    m = correspondence_match(theta0, phi0, cfg, 0.01, topk=topk)
    assert torch.equal(out["match_index"], m.index if topk > 1 else m.index.unsqueeze(1))
    g_out, g_mask = torch.randn(2, 3, 32, 32, generator=g).to(DEV), torch.randn(2, 5, 8, 8, generator=g).to(DEV)
    loss = (out["warp_out"] * g_out).sum() + ((out["warp_mask"] * g_mask).sum() if direct else 0.0)
    loss.backward()
    # the fp64 restatement on the returned candidates
    idx = out["match_index"].permute(0, 2, 3, 1).reshape(2, 64, topk)
    th64, ph64 = theta0.double().requires_grad_(True), phi0.double().requires_grad_(True)
    warp_r, mask_r = _hot_ref(th64, ph64, ref_img, ref_seg, idx, 4, direct, 100.0)
    loss_r = (warp_r * g_out.double()).sum() + ((mask_r * g_mask.double()).sum() if direct else 0.0)
    errs = {"warp_out": rel(out["warp_out"], warp_r.detach().cpu().numpy())}
    if direct:
        assert out["warp_mask"].shape == (2, 5, 8, 8)
        errs["warp_mask"] = rel(out["warp_mask"], mask_r.detach().cpu().numpy())
    if topk > 1:     # (k = 1: w = 1, the logits carry no gradient and the loss does not depend on theta / phi at all)
        loss_r.backward()
        errs["d theta"], errs["d phi"] = rel(theta.grad, th64.grad.cpu().numpy()), rel(phi.grad, ph64.grad.cpu().numpy())
    print(f"[sparse_warp] correspondence_sparse {losstype} k={topk}: " + "  ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    assert all(e < (GRAD_TOL if n.startswith("d ") else OUT_TOL) for n, e in errs.items()), errs
    if topk == 1:
        assert float(theta.grad.abs().max()) == 0.0 and float(phi.grad.abs().max()) == 0.0
    assert float(out["match_weight"].sum(1).sub(1).abs().max()) < 1e-5


def test_module_sparse_warp():
    """NoVGGCorrespondence.sparse_warp on ade20k_options(match_kernel=1) at the module tests' smallest crop: keys, shapes, finite
    values, gradients at theta.weight and phi.weight"""
    from test_gpu_exemplar import _module_case
    net, ref_img, real, seg, ref_seg = _module_case("ade20k_options", 64, 2, 2, match_kernel=1)
    out = net.sparse_warp(ref_img, real, seg, ref_seg, topk=4)
    assert {"warp_out", "warp_mask", "match_index", "match_weight"} <= set(out)
    assert out["warp_out"].shape == (2, 3, 64, 64) and out["warp_mask"].shape == (2, 7, 16, 16)
    assert out["match_index"].shape == out["match_weight"].shape == (2, 4, 16, 16)
    assert all(bool(torch.isfinite(out[n]).all()) for n in ("warp_out", "warp_mask", "match_weight"))
    with torch.no_grad():
        assert torch.equal(out["match_index"], net.match(ref_img, seg, ref_seg, topk=4)["match_index"])
    (out["warp_out"].square().sum() + out["warp_mask"].square().sum()).backward()
    for p in (net.theta.weight, net.phi.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- red zones
# The case joins tests/test_gpu_red_zones.py's table at import time, as the K36 - K41 files' cases do; tests/test_gpu_match_sparse_warp.py
# runs it before that file's "every entry point was reached" audit is collected, this file runs it with the rest of K42's tests.
def _rz_sparse_warp(c):
    from cocosnet_amd import ops
    q, k = c.leaf(rz.unit(2, 256, 37, 41)), c.leaf(rz.unit(2, 256, 22, 42))
    v = c.leaf(rz.rnd(2, 5, 22, seed=43))
    idx = torch.randint(-2, 25, (2, 37, 3), generator=torch.Generator().manual_seed(44))      # odd sizes, out-of-range entries
    idx[:, :, 0] = 21                                                                         # the last key, named by every query
    return [ops.sparse_softmax_warp(q, k, v, c.data(idx), 100.0)]


RZ_CASES = {"sparse_softmax_warp-2x37x22-Cv5-k3": _rz_sparse_warp}
for _name, _body in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_op_inside_red_zones(name, monkeypatch):
    """forward + backward under tests/guarded_alloc.guarded: no guard byte changes, every returned tensor and gradient is finite (a read
    outside a buffer, or of one nobody wrote, carries the guard's NaN), every leaf gets its gradient"""
    rz.test_red_zones(name, monkeypatch)
    assert {"cocos_sparse_softmax_warp_fwd_f16x3", "cocos_sparse_softmax_warp_bwd_query_f16x3", "cocos_sparse_softmax_warp_bwd_key_f16x3",
            "cocos_transpose_f32"} <= set(rz.COVERAGE[name][0])
