"""K54 on the GPU: the BIAS instantiations of the box readout (cocos_box3_topk_bias_f16x3), ops.box3_topk_biased, ops.box3_sinkhorn and
the two _BoxedCorr methods on top of them.

Arbiter, bounds and inputs: tests/transport_box3_case.py — the fp64 box logit matrix of tests/test_gpu_match_box3.py under
tests/transport_case.py's biased_topk / sinkhorn / masses / decided; one launch is held to
    lse_bound(bias) = TOL * (INV_T + max |finite bias|) / INV_T          (TOL = 4 E_BOX of tests/test_gpu_match_box3.py, imported)
a potential after n half-steps to n * lse_bound, and an index to the arbiter's wherever the arbiter decides it; at most 1 % of the
ranks may be undecided (tests/test_match_box3_transport_cpu.py checks that on the arbiter alone).  The fp32-torch arm's errors are
printed beside the kernel's; they are not part of any bound.
The file name sorts before test_gpu_red_zones.py: its red-zone case has run when that file's audit is collected."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy_case as ac  # noqa: E402
import test_gpu_red_zones as rz  # noqa: E402
import transport_box3_case as bc  # noqa: E402
import transport_case as tc  # noqa: E402
from test_gpu_match_box3 import DEV, INV_T, KC, _case  # noqa: E402

pytestmark = pytest.mark.gpu
ENTRY = "cocos_box3_topk_bias_f16x3"
NEG_INF = float("-inf")
DIRS = dict(argnames="transposed", argvalues=[False, True], ids=["rows", "transposed"])
GRID = dict(argnames="h,w,B", argvalues=bc.GRIDS, ids=bc.GRID_IDS)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def _biased(opnd, bias, h, w, k, transposed):
    from cocosnet_amd import ops
    t, mu, a, nu, b = opnd
    if transposed:
        mu, a, nu, b = nu, b, mu, a
    return ops.box3_topk_biased(t, mu, a, nu, b, bias.to(DEV), h, w, KC, INV_T, k, transposed=transposed)


def _plain(opnd, h, w, k, transposed):
    from cocosnet_amd import ops
    t, mu, a, nu, b = opnd
    if transposed:
        mu, a, nu, b = nu, b, mu, a
    return ops.box3_topk(t, mu, a, nu, b, h, w, KC, INV_T, k, transposed=transposed)


_FP32 = {}


def _fp32_logits(h, w, B):
    """the arbiter's chain in plain fp32 torch (printed beside the kernel's error, never asserted)"""
    if (h, w) not in _FP32:
        theta, phi = _case(h, w, B)[:2]
        with ac.plain_fp32():
            def unit(x):
                u = F.unfold(x, kernel_size=3, padding=1)
                u = u - u.mean(dim=1, keepdim=True)
                return u / (torch.norm(u, 2, 1, keepdim=True) + torch.finfo(torch.float32).eps)
            _FP32[(h, w)] = INV_T * torch.matmul(unit(theta).transpose(1, 2), unit(phi))
    return _FP32[(h, w)]


def _judge(tag, idx, val, lse, L, bias, L32=None, check_idx=True):
    """idx against the arbiter where the arbiter decides, val and lse inside lse_bound(bias) -> the figures"""
    kk = idx.shape[-1]
    bias = bias.to(DEV)
    a_idx, a_val, a_lse, z = tc.biased_topk(L, bias, kk)
    bound = bc.lse_bound(bias)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and tuple(idx.shape) == tuple(a_idx.shape), tag
    assert not bool(torch.isnan(val).any()) and not bool(torch.isnan(lse).any()), f"{tag}: NaN"
    assert int(idx.min()) >= 0 and int(idx.max()) < z.shape[-1], tag
    dec = tc.decided(z, kk, bound)
    excused = 1.0 - dec.double().mean().item()
    picked = z.gather(-1, idx.long())
    fin = torch.isfinite(picked)
    rows = torch.isfinite(a_lse)
    e_val = (val.double() - picked)[fin].abs().max().item() if bool(fin.any()) else 0.0
    e_lse = (lse.double() - a_lse)[rows].abs().max().item() if bool(rows.any()) else 0.0
    arm = ""
    if L32 is not None:
        z32 = L32 + bias.unsqueeze(1)
        e_val32 = (z32.gather(-1, a_idx).double() - a_val)[torch.isfinite(a_val)].abs().max().item()
        e_lse32 = (torch.logsumexp(z32, -1).double() - a_lse)[rows].abs().max().item()
        arm = f"  (fp32 torch arm: val {e_val32:.3e}, lse {e_lse32:.3e})"
    print(f"[transport-box3] {tag}: |val - z[idx]| = {e_val:.3e}  |lse - logsumexp z| = {e_lse:.3e}  bound {bound:.3e}  "
          f"excused {excused:.5f}{arm}")
    if check_idx:
        assert excused <= bc.EXCUSED_MAX, (tag, excused)
        assert torch.equal(idx.long()[dec], a_idx[dec]), f"{tag}: idx differs from the arbiter at {int((idx.long() != a_idx)[dec].sum())} decided positions"
    assert torch.equal(torch.isfinite(val), fin), f"{tag}: val is not finite exactly where the picked element is"
    assert torch.equal(torch.isfinite(lse), rows), f"{tag}: lse is not finite exactly on the rows with a key"
    assert e_val <= bound, (tag, e_val, bound)
    assert e_lse <= bound, (tag, e_lse, bound)
    return e_val, e_lse


# ---------------------------------------------------------------------------------------------------------------- the readout
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize(**DIRS)
@pytest.mark.parametrize(**GRID)
def test_zero_bias_is_the_unbiased_entry_bitwise(h, w, B, transposed, k):
    """tt + 0 / a_n is tt in every register, so all three outputs are cocos_box3_topk_f16x3's bits"""
    opnd = _case(h, w, B)[2]
    want = _plain(opnd, h, w, k, transposed)
    got = _biased(opnd, torch.zeros(B, h * w), h, w, k, transposed)
    for a, b_, what in zip(got, want, ("idx", "val", "lse")):
        assert torch.equal(a, b_), f"{what} differs from cocos_box3_topk_f16x3"


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize(**DIRS)
@pytest.mark.parametrize(**GRID)
def test_biased_readout_against_the_arbiter(h, w, B, transposed, k):
    _, _, opnd, L = _case(h, w, B)
    bias = bc.bias_for(h, w, B, transposed)
    got = _biased(opnd, bias, h, w, k, transposed)
    L32 = _fp32_logits(h, w, B)
    _judge(f"random bias ({h},{w}) {'transposed' if transposed else 'rows'} k={k}", *got, bc.directed(L, transposed), bias,
           L32=bc.directed(L32, transposed))
    again = _biased(opnd, bias, h, w, k, transposed)
    assert all(torch.equal(a, b_) for a, b_ in zip(got, again)), "two runs on the same inputs differ"


@pytest.mark.parametrize(**DIRS)
def test_a_low_logit_with_a_high_bias_wins(transposed):
    h, w, B = 4, 64, 2
    _, _, opnd, L = _case(h, w, B)
    Ld = bc.directed(L, transposed)
    j = Ld.sum(1).argmin(-1)                                 # per sample the key the queries like least
    bias = torch.zeros(B, h * w)
    bias[torch.arange(B), j.cpu()] = 2.5 * INV_T             # more than the logits' whole range
    idx, val, lse = _biased(opnd, bias, h, w, 4, transposed)
    _judge(f"high bias {'transposed' if transposed else 'rows'}", idx, val, lse, Ld, bias)
    assert torch.equal(idx[..., 0].long(), j.view(B, 1).expand(-1, h * w))
    assert bool((idx[..., 1:].long() != j.view(B, 1, 1)).all())


@pytest.mark.parametrize(**DIRS)
@pytest.mark.parametrize("h,w", [(4, 64), (40, 128)], ids=["4x64", "40x128"])
def test_equal_logits_with_equal_bias_resolve_to_the_lower_index(h, w, transposed):
    """T = 0, mu = nu = 0, a = b = 1: every logit is 0, so z' is the bias.  Six keys carry the same bias above all others — two in one
    half-wave's registers of a tile, one in the other half's, one in the next tile, two far away (past the first chunk at 5120 keys):
    the k best come in ascending key order through the register scan, the tile loop and the half-wave merge; val = the bias, and
    the lse is log(6 e^3 + (N - 6))"""
    from cocosnet_amd import ops
    B, N = 1, h * w
    z, one = torch.zeros(B, N, device=DEV), torch.ones(B, N, device=DEV)
    keys = [33, 35, 38, 70, N - 100, N - 5]
    bias = torch.zeros(B, N)
    bias[:, keys] = 3.0
    t = torch.zeros(B * N * N, device=DEV)
    for k in (1, 2, 4):
        # (scale 64: the query factor a_n and 1 / a_n are powers of two, so val = (3 / 64) * 64 is the bias exactly)
        idx, val, lse = ops.box3_topk_biased(t, z, one, z, one, bias.to(DEV), h, w, KC, 64.0, k, transposed=transposed)
        assert idx[0].tolist() == [keys[:k]] * N, idx[0, :3].tolist()
        assert bool((val == 3.0).all())
        assert (lse.double() - math.log(6 * math.exp(3.0) + N - 6)).abs().max().item() <= bc.lse_bound(bias, inv_t=64.0)


@pytest.mark.parametrize(**DIRS)
def test_a_row_with_every_key_excluded(transposed):
    h, w, B = 4, 64, 2
    opnd = _case(h, w, B)[2]
    bias = bc.bias_for(h, w, B, transposed).clone()
    bias[1] = NEG_INF
    for k in (1, 4):
        idx, val, lse = _biased(opnd, bias, h, w, k, transposed)
        assert not bool(torch.isnan(val).any()) and not bool(torch.isnan(lse).any())
        assert int(idx.min()) >= 0 and int(idx.max()) < h * w
        assert bool((lse[1] == NEG_INF).all()) and bool((val[1] == NEG_INF).all())
        assert bool(torch.isfinite(lse[0]).all()) and bool(torch.isfinite(val[0]).all())


@pytest.mark.parametrize(**DIRS)
def test_half_of_every_tile_excluded_and_a_deep_potential(transposed):
    """keys 8g + 4..7 of every tile excluded: the upper half-wave sees nothing and merges with l = 0; the finite bias sits at -300, so
    the first finite maximum is far below -128 in log2 units — the rescale of the empty state must not make 0 * inf"""
    h, w, B = 4, 64, 2
    _, _, opnd, L = _case(h, w, B)
    bias = torch.full((B, h * w), -300.0)
    bias[:, (torch.arange(h * w) % 8) >= 4] = NEG_INF
    for k in (1, 4):
        idx, val, lse = _biased(opnd, bias, h, w, k, transposed)
        _judge(f"half excluded, deep {'transposed' if transposed else 'rows'} k={k}", idx, val, lse, bc.directed(L, transposed), bias,
               check_idx=False)
        assert bool((idx % 8 < 4).all())


@pytest.mark.parametrize(**DIRS)
def test_a_bias_run_that_straddles_a_chunk_boundary(transposed):
    """5120 keys: everything excluded but six keys around 2048 and six around 4096, where the ring's buffers change"""
    h, w, B = 40, 128, 1
    _, _, opnd, L = _case(h, w, B)
    bias = torch.full((B, h * w), NEG_INF)
    run = torch.tensor([1.0, -2.0, 4.0, 0.5, -7.0, 3.0])
    bias[:, 2045:2051] = run
    bias[:, 4093:4099] = run + 0.25
    allowed = set(range(2045, 2051)) | set(range(4093, 4099))
    for k in (1, 4, 8):
        idx, val, lse = _biased(opnd, bias, h, w, k, transposed)
        _judge(f"chunk run {'transposed' if transposed else 'rows'} k={k}", idx, val, lse, bc.directed(L, transposed), bias, check_idx=False)
        assert set(idx.unique().tolist()) <= allowed and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(val).all())


def test_public_op_detaches_and_refuses():
    from cocosnet_amd import ops
    h, w, B = 4, 64, 2
    t, mu, a, nu, b = _case(h, w, B)[2]
    bias = bc.bias_for(h, w, B, False).to(DEV)
    got = ops.box3_topk_biased(t, mu.clone().requires_grad_(True), a, nu, b, bias, h, w, KC, INV_T, 3)
    want = ops.box3_topk_biased(t, mu, a, nu, b, bias, h, w, KC, INV_T, 3)
    assert all(torch.equal(x, y) for x, y in zip(got, want)) and not any(x.requires_grad for x in got)
    assert got[0].shape == (B, h * w, 3) and got[2].shape == (B, h * w)
    with pytest.raises(ops._lib.CocosHipError, match="no CPU fallback"):
        ops.box3_topk_biased(t, mu, a, nu, b, bias.cpu(), h, w, KC, INV_T, 3)
    with pytest.raises(ValueError, match="not differentiable"):
        ops.box3_topk_biased(t, mu, a, nu, b, bias.clone().requires_grad_(True), h, w, KC, INV_T, 3)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.box3_topk_biased(t, mu, a, nu, b, bias, h, 2 * w, KC, INV_T, 3)


# ---------------------------------------------------------------------------------------------------------------- Sinkhorn
_SINK = {}


def _sink_ref(h, w, B, iters, tau):
    key = (h, w, iters, tau)
    if key not in _SINK:
        _SINK[key] = tc.sinkhorn(_case(h, w, B)[3], iters, tau)
    return _SINK[key]


@pytest.mark.parametrize("tau", [1.0, 0.5])
@pytest.mark.parametrize("iters", [1, 3, 5])
@pytest.mark.parametrize("h,w,B", bc.GRIDS[:2], ids=bc.GRID_IDS[:2])
def test_sinkhorn_potentials_against_the_restatement(h, w, B, iters, tau):
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import _BoxedCorr
    theta, phi, opnd, L = _case(h, w, B)
    t, mu, a, nu, b = opnd
    f, g, row_lse = ops.box3_sinkhorn(t, mu, a, nu, b, h, w, KC, INV_T, iters, tau)
    rf, rg, rl = _sink_ref(h, w, B, iters, tau)
    per = bc.lse_bound(torch.cat((rf.reshape(-1), rg.reshape(-1))))
    bound = 2 * iters * per
    e_f, e_g, e_l = ((x.double() - y).abs().max().item() for x, y in ((f, rf), (g, rg), (row_lse, rl)))
    print(f"[transport-box3] sinkhorn ({h},{w}) iters={iters} tau={tau}: |f - ref| = {e_f:.3e}  |g - ref| = {e_g:.3e}  "
          f"|row_lse - ref| = {e_l:.3e}  per-lse bound {per:.3e} x {2 * iters} half-steps = {bound:.3e}")
    N = h * w
    assert f.shape == (B, N) and g.shape == (B, N) and row_lse.shape == (B, N) and not any(x.requires_grad for x in (f, g, row_lse))
    assert e_f <= bound and e_g <= bound and e_l <= bound + per, (e_f, e_g, e_l, bound)
    if tau == 1.0:      # balanced: the column marginals are exact after every full iteration
        col_lse = ops.box3_topk_biased(t, nu, b, mu, a, f, h, w, KC, INV_T, 1, transposed=True)[2]
        key_mass = torch.exp(g + col_lse + math.log(N))
        e_m = (key_mass.double() - 1).abs().max().item()
        print(f"[transport-box3] sinkhorn ({h},{w}) iters={iters}: |key_mass - 1| = {e_m:.3e}")
        assert e_m <= bound, (e_m, bound)
    again = _BoxedCorr(theta, phi, INV_T).sinkhorn(iters, tau)
    assert all(torch.equal(x, y) for x, y in zip((f, g, row_lse), again)), "_BoxedCorr.sinkhorn differs from ops.box3_sinkhorn"


def test_sinkhorn_through_the_chunk_ring():
    """5120 keys, one iteration: both half-steps restage the potential chunk by chunk"""
    from cocosnet_amd import ops
    h, w, B = bc.GRIDS[2]
    t, mu, a, nu, b = _case(h, w, B)[2]
    f, g, row_lse = ops.box3_sinkhorn(t, mu, a, nu, b, h, w, KC, INV_T, 1, 1.0)
    rf, rg, rl = _sink_ref(h, w, B, 1, 1.0)
    per = bc.lse_bound(torch.cat((rf.reshape(-1), rg.reshape(-1))))
    e_f, e_g, e_l = ((x.double() - y).abs().max().item() for x, y in ((f, rf), (g, rg), (row_lse, rl)))
    print(f"[transport-box3] sinkhorn ({h},{w}) iters=1: |f - ref| = {e_f:.3e}  |g - ref| = {e_g:.3e}  |row_lse - ref| = {e_l:.3e}  "
          f"per-lse bound {per:.3e}")
    assert e_f <= 2 * per and e_g <= 2 * per and e_l <= 3 * per, (e_f, e_g, e_l, per)


def test_boxed_corr_match_biased_is_the_op():
    from cocosnet_amd.hot_path import _BoxedCorr
    h, w, B = 4, 64, 2
    theta, phi, opnd, _ = _case(h, w, B)
    corr = _BoxedCorr(theta, phi, INV_T)
    for transposed in (False, True):
        bias = bc.bias_for(h, w, B, transposed)
        got = corr.match_biased(not transposed, bias.to(DEV), 4)
        want = _biased(opnd, bias, h, w, 4, transposed)
        assert all(torch.equal(x, y) for x, y in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------- guards
def test_sinkhorn_hands_over_live_buffers_only(monkeypatch):
    import test_gpu_live_buffers as lb
    from cocosnet_amd import ops
    h, w, B = 4, 64, 2
    t, mu, a, nu, b = _case(h, w, B)[2]
    guard = lb._Guard(monkeypatch)
    f, g, _ = ops.box3_sinkhorn(t, mu, a, nu, b, h, w, KC, INV_T, 3, 0.5)
    ops.box3_topk_biased(t, mu, a, nu, b, g, h, w, KC, INV_T, 4)
    guard.check(8, 8 * 9)      # 2 * 3 + 1 + 1 launches, nine device pointers each


def _rz_box3_transport(c):
    """both directions of the biased readout at k = 4 and a two-iteration Sinkhorn, bias and outputs between red zones"""
    from cocosnet_amd import ops
    B, h, w = 2, 4, 64
    th = c.data(rz.rnd(B, 256, h, w, seed=71) + 0.15)
    ph = c.data(0.05 * rz.rnd(B, 256, h, w, seed=71).roll((1, 5), (2, 3)) + rz.rnd(B, 256, h, w, seed=72) - 0.1)
    bias = c.data(tc.make_bias(B, h * w, 54).to(DEV))
    with torch.no_grad():
        (mu, a), (nu, b) = ops.unfold3_stats(th, KC), ops.unfold3_stats(ph, KC)
        t = ops.box3_corr_xbox(th, ph)
    idx4 = ops.box3_topk_biased(t, mu, a, nu, b, bias, h, w, KC, 100.0, 4)[0]
    v = c.data(rz.rnd(B, 5, h * w, seed=73))
    finite = c.data(torch.nan_to_num(bias, neginf=0.0))
    warp = ops.box3_sparse_softmax_warp(th, ph, mu, a, nu, b, v, idx4, 100.0, return_weights=True, k_bias=finite)
    return (list(warp) + list(ops.box3_topk_biased(t, mu, a, nu, b, bias, h, w, KC, 100.0, 4))
            + list(ops.box3_topk_biased(t, nu, b, mu, a, bias, h, w, KC, 100.0, 4, transposed=True))
            + list(ops.box3_sinkhorn(t, mu, a, nu, b, h, w, KC, 100.0, 2, 1.0)))


RZ_CASES = {"box3_topk_biased+sinkhorn-2x4x64": _rz_box3_transport}
for _name, _body in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_the_new_op_inside_red_zones(name, monkeypatch):
    rz.test_red_zones(name, monkeypatch)
    assert {ENTRY, "cocos_box3_sparse_softmax_warp_bias_fwd"} <= set(rz.COVERAGE[name][0])


# ---------------------------------------------------------------------------------------------------------------- deep bias, no exclusions
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize(**DIRS)
def test_a_deep_finite_bias_without_exclusions(transposed, k):
    """every key at -300 +- 5: nothing is excluded, so both half-waves see keys and only the FIRST move of the maximum meets an empty
    state with a reference below -128 log2 units — the first-move select on its own"""
    h, w, B = 4, 64, 2
    _, _, opnd, L = _case(h, w, B)
    bias = -300.0 + 5.0 * torch.randn(B, h * w, generator=torch.Generator().manual_seed(11))
    idx, val, lse = _biased(opnd, bias, h, w, k, transposed)
    _judge(f"deep bias {'transposed' if transposed else 'rows'} k={k}", idx, val, lse, bc.directed(L, transposed), bias, check_idx=False)
    assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(val).all())


# ---------------------------------------------------------------------------------------------------------------- planted collapse
def test_planted_collapse_is_undone_by_five_balanced_iterations():
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match, correspondence_transport_box3
    theta, phi, hub = (x.to(DEV) if torch.is_tensor(x) else x for x in bc.planted())
    B, _, h, w = theta.shape
    N = h * w
    L = bc._arbiter(theta, phi)
    share = bc.hub_share(L, hub)
    assert float(share.min()) >= bc.PLANT_MIN_SHARE                     # the collapse, on the arbiter first
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    plain = correspondence_match(theta, phi, cfg, 1.0 / INV_T)
    k_share = (plain.index.reshape(B, N) == hub).double().mean(-1)
    assert float(k_share.min()) >= float(share.min())                    # ... and on the kernels
    rf, rg, _ = tc.sinkhorn(L, 5, 1.0)
    a_idx, _, _, z = tc.biased_topk(L, rg, 1)
    a_load = bc.loads(a_idx[..., 0], N)
    res = correspondence_transport_box3(theta, phi, cfg, 1.0 / INV_T, iters=5, tau=1.0)
    idx = res["readout"].index.reshape(B, N)
    k_load = bc.loads(idx, N)
    print(f"[transport-box3] planted: hub share {float(share.min()):.3f} (kernels {float(k_share.min()):.3f}); max load after 5 iterations: "
          f"arbiter {int(a_load.max())}, kernels {int(k_load.max())}")
    assert int(a_load.max()) <= bc.PLANT_MAX_LOAD and int(k_load.max()) <= bc.PLANT_MAX_LOAD
    dec = tc.decided(z, 1, 10 * bc.lse_bound(torch.cat((rf.reshape(-1), rg.reshape(-1)))))[..., 0]
    assert torch.equal(idx[dec], a_idx[..., 0][dec])
    assert float((res["key_mass"].double() - 1).abs().max()) <= 10 * bc.lse_bound(rg)


# ---------------------------------------------------------------------------------------------------------------- the route
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("tau", [1.0, 0.5])
def test_correspondence_transport_box3_against_the_arbiter(tau, k):
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_transport_box3
    h, w, B = 4, 64, 2
    theta, phi, _, L = _case(h, w, B)
    N, iters = h * w, 5
    res = correspondence_transport_box3(theta, phi, HotPathConfig(match_kernel=3, PONO_C=True, down=4), 1.0 / INV_T, iters=iters, tau=tau, topk=k)
    assert set(res) == {"readout", "potential_q", "potential_k", "match_mass", "key_mass"}
    rf, rg, rl = _sink_ref(h, w, B, iters, tau)
    per = bc.lse_bound(torch.cat((rf.reshape(-1), rg.reshape(-1))))
    bound = 2 * iters * per
    m = res["readout"]
    a_idx, a_val, a_lse, z = tc.biased_topk(L, rg, k)
    mm, km = tc.masses(L, rf, rg)
    e = {"f": (res["potential_q"].reshape(B, N).double() - rf).abs().max().item(), "g": (res["potential_k"].reshape(B, N).double() - rg).abs().max().item(),
         "lse": (m.lse.reshape(B, N).double() - a_lse).abs().max().item(),
         "match_mass": (res["match_mass"].reshape(B, N).double() - mm).abs().max().item() / float(mm.max()),
         "key_mass": (res["key_mass"].reshape(B, N).double() - km).abs().max().item() / float(km.max())}
    print(f"[transport-box3] correspondence_transport_box3 tau={tau} k={k}: " + "  ".join(f"{n} {v:.3e}" for n, v in e.items()) + f"  bound {bound:.3e}")
    assert e["f"] <= bound and e["g"] <= bound and e["lse"] <= bound + per
    assert e["match_mass"] <= 2 * bound + per and e["key_mass"] <= 2 * bound + per      # exp of a sum of two bounded quantities, relative
    if tau == 1.0:
        assert float((res["key_mass"].double() - 1).abs().max()) <= bound
    got = (m.index.reshape(B, N, 1) if k == 1 else m.index.permute(0, 2, 3, 1).reshape(B, N, k))
    dec = tc.decided(z, k, bound + per)
    assert 1 - dec.double().mean().item() <= bc.EXCUSED_MAX
    assert torch.equal(got[dec], a_idx[dec])
    val = (m.max_logit.reshape(B, N, 1) if k == 1 else m.logit.permute(0, 2, 3, 1).reshape(B, N, k))
    assert (val.double() - z.gather(-1, got)).abs().max().item() <= bound + per


def _sparse_inputs(h, w, B, seed, nc=5, down=4):
    g = torch.Generator().manual_seed(seed)
    H, W = h * down, w * down
    onehot = lambda: torch.zeros(B, nc, H, W).scatter_(1, torch.randint(0, nc, (B, 1, H, W), generator=g), 1.0)
    return tuple(t.to(DEV) for t in (torch.rand(B, 3, H, W, generator=g) * 2 - 1, onehot(), onehot()))


def _record_calls(monkeypatch):
    from cocosnet_amd import _lib
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


@pytest.mark.parametrize("h,w", [(4, 64), (2, 128)], ids=["4x64", "2x128"])
def test_sparse_box3_with_transport_against_fp64(h, w, monkeypatch):
    """selection = the transport plan's top-4, blend = softmax(pair logit + g) with g detached: outputs, w and the gradients to theta
    and phi against the fp64 restatement on the route's own idx and potential, under K51's bounds; zero bias is the unbiased forward
    bitwise; transport=None is the route as it was, outputs and launch sequence"""
    import box3_sparse_case as sc
    import torch.nn.functional as Fn
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse_box3, correspondence_transport_box3
    from test_gpu_parity import GRAD_TOL, OUT_TOL, rel
    B, k = 2, 4
    theta0, phi0, _, L = _case(h, w, B)
    ref_img, seg, ref_seg = _sparse_inputs(h, w, B, 61 + h)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4, warp_mask_losstype="direct")
    tr = dict(iters=5, tau=1.0)
    theta, phi = theta0.clone().requires_grad_(True), phi0.clone().requires_grad_(True)
    out = correspondence_sparse_box3(theta, phi, ref_img, seg, ref_seg, cfg, 1.0 / INV_T, k, transport=tr)
    assert set(out) == {"warp_out", "warp_mask", "match_index", "match_weight", "potential_k", "match_mass"}
    assert not out["potential_k"].requires_grad and not out["match_weight"].requires_grad
    t_res = correspondence_transport_box3(theta0, phi0, cfg, 1.0 / INV_T, topk=k, **tr)
    assert torch.equal(out["match_index"], t_res["readout"].index) and torch.equal(out["potential_k"], t_res["potential_k"])
    N = h * w
    idx = out["match_index"].permute(0, 2, 3, 1).reshape(B, N, k)
    g = out["potential_k"].reshape(B, N)
    gen = torch.Generator().manual_seed(5)
    g_out, g_mask = torch.randn(out["warp_out"].shape, generator=gen).to(DEV), torch.randn(out["warp_mask"].shape, generator=gen).to(DEV)
    ((out["warp_out"] * g_out).sum() + (out["warp_mask"] * g_mask).sum()).backward()
    # fp64: the box logit of the k pairs through the arbiter's chain (differentiable), plus the detached potential
    th64, ph64 = theta0.double().requires_grad_(True), phi0.double().requires_grad_(True)
    vals = torch.cat([Fn.avg_pool2d(ref_img.double(), 4).reshape(B, 3, -1),
                      Fn.interpolate(ref_seg.double(), scale_factor=0.25, mode="nearest").reshape(B, ref_seg.shape[1], -1)], 1)
    s = bc._arbiter(th64, ph64).gather(2, idx) + g.double().unsqueeze(1).expand(-1, N, -1).gather(2, idx)
    w64 = torch.softmax(s, -1)
    picked = vals.gather(2, idx.reshape(B, 1, N * k).expand(-1, vals.shape[1], -1)).reshape(B, vals.shape[1], N, k)
    o = (picked * w64.unsqueeze(1)).sum(-1)
    warp_r = Fn.interpolate(o[:, :3].reshape(B, 3, h, w), scale_factor=4, mode="nearest")
    mask_r = o[:, 3:].reshape(B, -1, h, w)
    ((warp_r * g_out.double()).sum() + (mask_r * g_mask.double()).sum()).backward()
    e_w = (out["match_weight"].permute(0, 2, 3, 1).reshape(B, N, k).double() - w64.detach()).abs().max().item()
    errs = {"warp_out": rel(out["warp_out"], warp_r.detach().cpu().numpy()), "warp_mask": rel(out["warp_mask"], mask_r.detach().cpu().numpy()),
            "d theta": rel(theta.grad, th64.grad.cpu().numpy()), "d phi": rel(phi.grad, ph64.grad.cpu().numpy())}
    print(f"[transport-box3] sparse_box3(transport) ({h},{w}): |w - softmax64| = {e_w:.3e}  " + "  ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    assert e_w <= 4 * bc.lse_bound(g)      # a weight is exp of a difference of two logits, each inside the per-launch bound, times <= 1
    assert all(e < (GRAD_TOL if n.startswith("d ") else OUT_TOL) for n, e in errs.items()), errs
    # the op: zero bias is the unbiased forward bit for bit
    with torch.no_grad():
        (mu, a), (nu, b) = ops.unfold3_stats(theta0, KC), ops.unfold3_stats(phi0, KC)
        v32 = vals.float().contiguous()
        plain = ops.box3_sparse_softmax_warp(theta0, phi0, mu, a, nu, b, v32, idx, INV_T, return_weights=True)
        zero = ops.box3_sparse_softmax_warp(theta0, phi0, mu, a, nu, b, v32, idx, INV_T, return_weights=True, k_bias=torch.zeros(B, N, device=DEV))
    assert torch.equal(plain[0], zero[0]) and torch.equal(plain[1], zero[1])
    # transport=None: today's outputs and today's launch sequence
    names = _record_calls(monkeypatch)
    x = correspondence_sparse_box3(theta0, phi0, ref_img, seg, ref_seg, cfg, 1.0 / INV_T, k)
    first, n0 = list(names), len(names)
    y = correspondence_sparse_box3(theta0, phi0, ref_img, seg, ref_seg, cfg, 1.0 / INV_T, k, transport=None)
    assert names[n0:] == first and "cocos_box3_sparse_softmax_warp_bias_fwd" not in first and "cocos_box3_topk_bias_f16x3" not in first
    assert set(x) == set(y) and all(torch.equal(x[n], y[n]) for n in x)


def test_transport_route_launch_sequence(monkeypatch):
    """one x-box GEMM, 2 iters + 1 biased launches (+ one top-k launch for topk > 1), one column launch"""
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_transport_box3
    h, w, B = 4, 64, 2
    theta, phi = _case(h, w, B)[:2]
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    for k, want in ((1, 2 * 3 + 1 + 1), (4, 2 * 3 + 1 + 1 + 1)):
        names = _record_calls(monkeypatch)
        correspondence_transport_box3(theta, phi, cfg, 1.0 / INV_T, iters=3, topk=k)
        assert names.count(ENTRY) == want and names.count("cocos_box3_corr_xbox_f16x3") == 1, names
        monkeypatch.undo()


def test_module_transport_on_the_box_route():
    """crop 256, B = 2: a 64 x 64 grid.  transport_match_box3 and sparse_warp_box3(transport=) against the arbiter built from the
    module's own projections (materialised fp64 box logits)"""
    from cocosnet_amd import correspondence as cc
    from test_gpu_exemplar import _module_case
    net, ref_img, real, seg, ref_seg = _module_case("ade20k_options", 256, 2, 2, match_kernel=3)
    B, iters = 2, 3
    out = net.transport_match_box3(ref_img, seg, ref_seg, iters=iters, tau=1.0, topk=1, hard_warp=True)
    assert {"match_index", "match_xy", "match_prob", "match_lse", "potential_q", "potential_k", "match_mass", "key_mass", "warp_hard"} <= set(out)
    with torch.no_grad():
        th, ph = (x.raw() if hasattr(x, "raw") else x for x in net.project(ref_img, None, seg, ref_seg, None, lazy=True))
        Lm = bc._arbiter(th, ph)
    N = Lm.shape[1]
    rf, rg, rl = tc.sinkhorn(Lm, iters, 1.0)
    per = bc.lse_bound(torch.cat((rf.reshape(-1), rg.reshape(-1))))
    bound = 2 * iters * per
    e_g = (out["potential_k"].reshape(B, N).double() - rg).abs().max().item()
    e_l = (out["match_lse"].reshape(B, N).double() - rl).abs().max().item()
    e_m = (out["key_mass"].double() - 1).abs().max().item()
    print(f"[transport-box3] module: |g - ref| = {e_g:.3e}  |lse - ref| = {e_l:.3e}  |key_mass - 1| = {e_m:.3e}  bound {bound:.3e}  (max |L| {float(Lm.abs().max()):.1f})")
    assert e_g <= bound and e_l <= bound + per and e_m <= bound
    a_idx, _, _, z = tc.biased_topk(Lm, rg, 1)
    dec = tc.decided(z, 1, bound + per)[..., 0]
    assert torch.equal(out["match_index"].reshape(B, N)[dec], a_idx[..., 0][dec])
    del Lm, z
    sp = net.sparse_warp_box3(ref_img, real, seg, ref_seg, topk=4, transport=dict(iters=iters, tau=1.0))
    assert {"warp_out", "match_index", "match_weight", "potential_k", "match_mass"} <= set(sp)
    assert (sp["potential_k"].reshape(B, N).double() - rg).abs().max().item() <= bound
    assert float(sp["match_weight"].sum(1).sub(1).abs().max()) < 1e-5 and bool(torch.isfinite(sp["warp_out"]).all())
    sp["warp_out"].square().sum().backward()
    for p in (net.theta.weight, net.phi.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    for over in (dict(match_kernel=1), dict(match_kernel=3, PONO_C=False)):
        bad = cc.NoVGGCorrespondence(cc.ade20k_options(crop_size=64, semantic_nc=7, **over)).to(DEV)
        with pytest.raises(ValueError, match="match_kernel 3 route"):
            bad.transport_match_box3(ref_img, seg, ref_seg)


def test_transport_route_keeps_one_hw_by_hw_tensor():
    """B = 1, 64 x 64: the peak above the live bytes is under twice one T (64 MiB), and nothing HW x HW stays after return"""
    import gc
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_transport_box3
    g = torch.Generator().manual_seed(9)
    theta = (torch.randn(1, 256, 64, 64, generator=g) + 0.1).to(DEV)
    phi = (0.3 * theta.cpu().roll((1, 7), (2, 3)) + torch.randn(1, 256, 64, 64, generator=g)).to(DEV)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    one_t = 4096 * 4096 * 4
    correspondence_transport_box3(theta, phi, cfg, 0.01, iters=2)      # (warm: the library's own lazily made buffers)
    rz._clear_pools()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = correspondence_transport_box3(theta, phi, cfg, 0.01, iters=5, topk=4)
    torch.cuda.synchronize()
    held, peak = torch.cuda.memory_allocated() - before, torch.cuda.max_memory_allocated() - before
    print(f"[transport-box3] memory: peak above live {peak / 2**20:.1f} MiB (one T = {one_t / 2**20:.0f} MiB), held after return {held / 2**20:.2f} MiB")
    assert peak < 2 * one_t, peak
    assert held < one_t // 8, held
    assert bool(torch.isfinite(res["key_mass"]).all())
