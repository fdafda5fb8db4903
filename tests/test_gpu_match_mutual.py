"""K48 mutual match on the GPU: the fused sweep (cocos_corr_match_mutual_f16x3: row outputs bitwise the existing readout's, column
outputs against torch fp64), the round-trip kernel against the restatement (tests/match_mutual_case.py), and the module-level
`NoVGGCorrespondence.mutual_match` on every route.

Inputs are tests/test_gpu_match.py's `_case` (B = 3, inv_t = 100, the same seeds), so that file's recorded E_FWD = 9.70e-6 and
TOL = 4 * E_FWD apply: the logits are the same bits, only the order in which a column's exponentials are summed is new.  Every key is
judged, none excluded.  The existing readout's errors with the operands exchanged are printed next to the fused kernel's.

`test_padded_queries_never_reach_the_column_state` — the key is the negated, normalised sum of all queries.  With `_case`'s queries
alone that key's logits are NOT all negative at Nq = 132 and 388 (a query's cosine with the sum of N random unit vectors of 256
dimensions is (1 + N(0, N / 256)) / |sum|: 36 resp. 227 of the 3 x Nq logits are >= 0, the largest +8.2 resp. +17.4), so the
assertion on the fp64 L that has to hold before the kernel runs would fail for the inputs, not for the kernel.  The queries of that one
test therefore carry a shared component (0.5 e_0 added before the normalisation): every logit of the key is then below -30."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_mutual_case as mc  # noqa: E402
import test_gpu_match as tm  # noqa: E402
from guarded_alloc import guarded  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = tm.DEV
TOL, INV_T, B = tm.TOL, tm.INV_T, tm.B
#: partial query and key tiles, several key stages, a last tile of 4 keys, two and four query blocks with a last block of 4 queries
SHAPES = [(64, 64), (256, 128), (132, 68), (36, 260), (388, 132)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def _mutual(q, k):
    from cocosnet_amd import ops
    return ops._corr_match_mutual_planes(*tm._planes(q), *tm._planes(k), INV_T)


def _case(Nq, Nk):
    q, k, L, _ = tm._case(Nq, Nk)
    return q, k, L


def _col_errors(idx, mx, lse, LT):
    """the three errors of a column readout against LT = L^T [B,Nk,Nq] fp64, over every key"""
    Lmax = LT.max(dim=2).values
    picked = LT.gather(2, idx.long().unsqueeze(2)).squeeze(2)
    return ((Lmax - picked).max().item(), (mx.double() - Lmax).abs().max().item(),
            (lse.double() - torch.logsumexp(LT, dim=2)).abs().max().item())


@pytest.mark.parametrize("Nq,Nk", SHAPES)
def test_rows_are_the_existing_readout_bitwise(Nq, Nk):
    from cocosnet_amd import ops
    q, k, _ = _case(Nq, Nk)
    rows, _ = _mutual(q, k)
    want = ops._corr_match_planes(*tm._planes(q), *tm._planes(k), INV_T)
    for got, ref, name in zip(rows, want, ("row_idx", "row_max", "row_lse")):
        assert got.dtype == ref.dtype and torch.equal(got, ref), name


@pytest.mark.parametrize("Nq,Nk", SHAPES)
def test_columns_against_fp64_every_key(Nq, Nk):
    from cocosnet_amd import ops
    q, k, L = _case(Nq, Nk)
    LT = L.transpose(1, 2)
    _, (ci, cm, cl) = _mutual(q, k)
    assert ci.dtype == torch.int32 and ci.shape == (B, Nk) and int(ci.min()) >= 0 and int(ci.max()) < Nq
    e = _col_errors(ci, cm, cl, LT)
    x = _col_errors(*ops._corr_match_planes(*tm._planes(k), *tm._planes(q), INV_T), LT)
    for tag, v in (("fused columns    ", e), ("exchanged readout", x)):
        print(f"[mutual] ({Nq},{Nk}) {tag}: max L^T - L^T[idx] = {v[0]:.3e}  |max - max L^T| = {v[1]:.3e}  |lse - logsumexp L^T| = {v[2]:.3e}"
              f"  (tol {TOL:.1e})")
    assert e[0] <= TOL and e[1] <= TOL and e[2] <= TOL, e


@pytest.mark.parametrize("Nq,Nk", SHAPES)
def test_mutual_pairs_share_the_tile_element_and_calls_repeat_bitwise(Nq, Nk):
    q, k, _ = _case(Nq, Nk)
    (ri, rm, rl), (ci, cm, cl) = first = _mutual(q, k)
    pair = ci.long().gather(1, ri.long()) == torch.arange(Nq, device=DEV).unsqueeze(0)      # col_idx[row_idx[i]] == i
    assert int(pair.sum()) > 0
    assert torch.equal(rm[pair], cm.gather(1, ri.long())[pair])
    again = _mutual(q, k)
    for a, b in zip(first[0] + first[1], again[0] + again[1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("N", [64, 260, 388])
def test_planted_permutation_is_recovered_exactly(N):
    from cocosnet_amd import ops
    q = tm._unit(tm._randn(B, 256, N, seed=N))                                   # _case's queries of this size
    perm = torch.stack([torch.randperm(N, generator=torch.Generator().manual_seed(17 * N + b)) for b in range(B)]).to(DEV)
    k = q.gather(2, perm.unsqueeze(1).expand(-1, 256, -1)).contiguous()          # key j is query perm[j]
    (ri, _, _), (ci, _, _) = _mutual(q, k)
    assert torch.equal(ci.long(), perm)
    assert torch.equal(ri.long().gather(1, perm), torch.arange(N, device=DEV).unsqueeze(0).expand(B, -1))
    grid = (N // 4, 4)
    q_back, q_dist, k_back, k_dist = ops.match_round_trip(ri, ci, grid, grid)
    assert int(q_dist.max()) == 0 and int(k_dist.max()) == 0
    ar = torch.arange(N, device=DEV, dtype=torch.int32).unsqueeze(0).expand(B, -1)
    assert torch.equal(q_back, ar) and torch.equal(k_back, ar)


def test_planted_subset_pairs_are_mutual():
    """(132, 68): the keys are 68 of the 132 queries"""
    Nq, Nk = 132, 68
    q = _case(Nq, Nk)[0]
    sel = torch.stack([torch.randperm(Nq, generator=torch.Generator().manual_seed(5 + b))[:Nk] for b in range(B)]).to(DEV)
    k = q.gather(2, sel.unsqueeze(1).expand(-1, 256, -1)).contiguous()
    (ri, _, _), (ci, _, _) = _mutual(q, k)
    assert torch.equal(ci.long(), sel)
    assert torch.equal(ri.long().gather(1, sel), torch.arange(Nk, device=DEV).unsqueeze(0).expand(B, -1))


@pytest.mark.parametrize("lo,hi", [(5, 21), (5, 37), (5, 165)], ids=["same-wave", "same-workgroup", "other-workgroup"])
def test_equal_logits_return_the_lower_query(lo, hi):
    """query columns lo and hi are identical (their logits are the same bits in every column); keys 7 (first stage, group 0), 100
    (second stage, group 1) and 131 (the last tile of 4) are copies of them: col_idx is lo every time"""
    Nq, Nk = 388, 132
    q, k, _ = _case(Nq, Nk)
    q, k = q.clone(), k.clone()
    q[:, :, hi] = q[:, :, lo]
    for j in (7, 100, 131):
        k[:, :, j] = q[:, :, lo]
    (ri, rm, _), (ci, cm, _) = _mutual(q, k)
    for j in (7, 100, 131):
        assert ci[:, j].tolist() == [lo] * B, (j, ci[:, j].tolist())
    assert torch.equal(rm[:, lo], rm[:, hi]) and torch.equal(cm[:, 7], rm[:, lo])
    assert ri[:, lo].tolist() == [7] * B and ri[:, hi].tolist() == [7] * B


@pytest.mark.parametrize("Nq,Nk", [(36, 260), (132, 68), (388, 132)])
def test_padded_queries_never_reach_the_column_state(Nq, Nk):
    """one key is the negated, normalised sum of all queries: every logit of it is negative (asserted on the fp64 L first), so a
    zero-padded query of the last block (logit 0) would be its maximum and would add 1 to its sum.  Queries: see the module docstring."""
    q, k, _ = _case(Nq, Nk)
    e0 = torch.zeros(1, 256, 1, device=DEV)
    e0[0, 0, 0] = 0.5
    q = tm._unit(q + e0)
    s = q.double().sum(dim=2)
    k = k.clone()
    j = Nk - 3                                                     # in the last key tile
    k[:, :, j] = (-(s / s.norm(dim=1, keepdim=True))).float()
    L = mc.logits(q, k, INV_T)
    assert float(L[:, :, j].max()) < 0.0
    LT = L.transpose(1, 2)
    _, (ci, cm, cl) = _mutual(q, k)
    assert bool((cm[:, j] < 0).all()), cm[:, j].tolist()
    e = _col_errors(ci, cm, cl, LT)
    print(f"[mutual] padded ({Nq},{Nk}): col_max of the key {cm[:, j].tolist()}  errors {e[0]:.3e} {e[1]:.3e} {e[2]:.3e}")
    assert (cm[:, j].double() - LT[:, j].max(dim=1).values).abs().max().item() <= TOL
    assert e[0] <= TOL and e[1] <= TOL and e[2] <= TOL, e


@pytest.mark.parametrize("Nq,Nk", [(132, 68), (388, 132)])
def test_nothing_is_written_outside_outputs_and_workspace(Nq, Nk, hip_lib):
    """outputs and a workspace of exactly cocos_corr_match_mutual_workspace_bytes bytes between red zones"""
    from cocosnet_amd import _lib, ops
    q, k, _ = _case(Nq, Nk)
    want = _mutual(q, k)
    nbytes = hip_lib.cocos_corr_match_mutual_workspace_bytes(B, Nq, Nk)
    assert nbytes == 12 * B * ((Nq + 127) // 128) * Nk
    raw = tuple(tm._planes(q)) + tuple(tm._planes(k))
    with guarded() as g:
        planes = [g.place(t) for t in raw]
        outs = [torch.empty((B, n), device=DEV, dtype=dt) for n in (Nq, Nk) for dt in (torch.int32, torch.float32, torch.float32)]
        ws = torch.empty(nbytes // 4, device=DEV, dtype=torch.float32)
        _lib.call("cocos_corr_match_mutual_f16x3", *(t.data_ptr() for t in planes), *(t.data_ptr() for t in outs), ws.data_ptr(), nbytes,
                  B, 256, Nq, Nk, INV_T, ops.SPLIT_OPERAND_SCALE, torch.cuda.current_stream().cuda_stream)
        assert g.check() == [] and not g.violations, g.report()
        assert g.guarded_count == 4 + 6 + 1
        for got, ref in zip(outs, want[0] + want[1]):
            assert torch.equal(got, ref)
    with guarded() as g:                    # and through the op: every buffer it allocates is carved
        got = ops._corr_match_mutual_planes(*(g.place(t) for t in raw), INV_T)
        assert not g.violations and g.check() == [], g.report()
        assert "cocos_corr_match_mutual_f16x3" in g.entries
        assert any(a.nbytes == nbytes for a in g.allocations), "the op's workspace is not sized by the ABI function"
        for a, b in zip(got[0] + got[1], want[0] + want[1]):
            assert torch.equal(a, b)


def test_round_trip_equals_the_restatement():
    """6 x 6 -> 13 x 20 grids, random indices, some outside their range (clamped), int32 and int64"""
    from cocosnet_amd import ops
    qgrid, kgrid = (6, 6), (13, 20)
    g = torch.Generator().manual_seed(48)
    row = torch.randint(-5, 13 * 20 + 5, (B, 36), generator=g).to(DEV)
    col = torch.randint(-5, 36 + 5, (B, 260), generator=g).to(DEV)
    want = mc.round_trip(row, col, qgrid, kgrid)
    for cast in (lambda t: t, lambda t: t.to(torch.int32)):
        with guarded() as gd:
            got = ops.match_round_trip(gd.place(cast(row)), gd.place(cast(col)), qgrid, kgrid)
            assert gd.check() == [] and "cocos_match_round_trip" in gd.entries, gd.report()
        for a, b in zip(got, want):
            assert a.dtype == torch.int32 and torch.equal(a.long(), b)
    assert int(want[1].max()) > 1 and int(want[3].max()) > 1      # the case is not trivially all-zero
    # and the other way round (the wide grid asks)
    got = ops.match_round_trip(col.clamp(0, 35), row.clamp(0, 259), kgrid, qgrid)
    for a, b in zip(got, mc.round_trip(col, row, kgrid, qgrid)):
        assert torch.equal(a.long(), b)


# ---------------------------------------------------------------------------------------------------------------- the module
class _Entries:
    """the C entry points a block reaches"""

    def __init__(self, monkeypatch):
        from cocosnet_amd import _lib
        self.names = []
        real = _lib.call
        monkeypatch.setattr(_lib, "call", lambda name, *a: (self.names.append(name), real(name, *a))[1])


def _net(mk):
    """a tiny network on the plain PONO_C flag set: crop 32, down 4 -> 8 x 8 feature grids, B = 2"""
    from test_gpu_exemplar import _module_case
    return _module_case("ade20k_options", 32, 2, 2, match_kernel=mk)


def _check_round_trip_keys(out, max_dist, down):
    Bm, h, w = out["match_index"].shape
    gh, gw = out["back_index"].shape[1:]
    q_back, q_dist, k_back, k_dist = mc.round_trip(out["match_index"].reshape(Bm, -1), out["back_index"].reshape(Bm, -1), (h, w), (gh, gw))
    assert out["match_round_trip"].dtype == torch.int64 and torch.equal(out["match_round_trip"], q_back.reshape(Bm, h, w))
    assert out["match_cycle_dist"].dtype == torch.int32 and torch.equal(out["match_cycle_dist"].long(), q_dist.reshape(Bm, h, w))
    assert torch.equal(out["back_cycle_dist"].long(), k_dist.reshape(Bm, gh, gw))
    assert out["match_mutual"].dtype == torch.bool and torch.equal(out["match_mutual"], q_dist.reshape(Bm, h, w) <= max_dist)
    assert torch.equal(out["back_mutual"], k_dist.reshape(Bm, gh, gw) <= max_dist)
    if "warp_valid" in out:
        want = out["match_mutual"].float().repeat_interleave(down, 1).repeat_interleave(down, 2).unsqueeze(1)
        assert out["warp_valid"].dtype == torch.float32 and torch.equal(out["warp_valid"], want)
    for key in ("match", "back"):
        xy, gw_ = out[f"{key}_xy"], (gw if key == "match" else w)
        assert torch.equal(xy[:, 1] * gw_ + xy[:, 0], out[f"{key}_index"])


def test_module_fused_route(monkeypatch):
    net, ref_img, real, seg, ref_seg = _net(1)
    rows = net.match(ref_img, seg, ref_seg, hard_warp=True)
    cols = net.match(ref_img, seg, ref_seg, direction="cols")
    cols2 = net.match(ref_img, seg, ref_seg, direction="cols", topk=2)
    spy = _Entries(monkeypatch)
    outs = {d: net.mutual_match(ref_img, seg, ref_seg, max_dist=d, hard_warp=True) for d in (0, 1)}
    assert spy.names.count("cocos_corr_match_mutual_f16x3") == 2 and spy.names.count("cocos_match_round_trip") == 2
    assert "cocos_corr_match_f16x3" not in spy.names
    for d, out in outs.items():
        assert not any(v.requires_grad for v in out.values())
        for key in ("match_index", "match_xy", "match_prob", "match_lse", "warp_hard"):
            assert torch.equal(out[key], rows[key]), key
        e_p = (out["back_prob"].double() - cols["match_prob"].double()).abs().max().item()
        e_l = (out["back_lse"].double() - cols["match_lse"].double()).abs().max().item()
        differ = out["back_index"] != cols["match_index"]
        print(f"[mutual] module fused max_dist={d}: |back_prob - cols prob| = {e_p:.3e}  |back_lse - cols lse| = {e_l:.3e}  "
              f"indices that differ: {int(differ.sum())} of {differ.numel()}  mutual: {int(out['match_mutual'].sum())} of {out['match_mutual'].numel()}")
        assert e_p <= TOL and e_l <= TOL
        if bool(differ.any()):      # only a runner-up within the rounding of the logits may take the place of the cols readout's match
            assert torch.equal(out["back_index"][differ], cols2["match_index"][:, 1][differ])
            gap = torch.log(cols2["match_prob"][:, 0].double() / cols2["match_prob"][:, 1].double())[differ].max().item()
            assert gap <= 2 * TOL, gap
        _check_round_trip_keys(out, d, net.opt.down)
    assert bool((outs[1]["match_mutual"] | ~outs[0]["match_mutual"]).all())      # max_dist = 1 confirms at least what 0 confirms


@pytest.mark.parametrize("mk,switch", [(1, False), (3, True)], ids=["mk1-MATCH_MUTUAL_FUSED_off", "mk3"])
def test_module_two_readout_routes(mk, switch, monkeypatch):
    from cocosnet_amd import ops
    monkeypatch.setattr(ops, "MATCH_MUTUAL_FUSED", switch)
    net, ref_img, real, seg, ref_seg = _net(mk)
    rows = net.match(ref_img, seg, ref_seg, hard_warp=True)
    cols = net.match(ref_img, seg, ref_seg, direction="cols")
    spy = _Entries(monkeypatch)
    out = net.mutual_match(ref_img, seg, ref_seg, max_dist=1, hard_warp=True)
    assert "cocos_corr_match_mutual_f16x3" not in spy.names and spy.names.count("cocos_match_round_trip") == 1
    for key in ("match_index", "match_xy", "match_prob", "match_lse", "warp_hard"):
        assert torch.equal(out[key], rows[key]), key
    for key in ("index", "xy", "prob", "lse"):
        assert torch.equal(out[f"back_{key}"], cols[f"match_{key}"]), key
    _check_round_trip_keys(out, 1, net.opt.down)


@pytest.mark.parametrize("mk", [1, 3])
def test_module_with_a_prepared_exemplar(mk):
    """a record runs (the two-readout route) and agrees with the unprepared call: the indices of either pick logits of
    forward(return_corr=True)'s matrix within TOL of each other, as tests/test_gpu_match.py asks of match() with a record"""
    from cocosnet_amd import inference
    net, ref_img, real, seg, ref_seg = _net(mk)
    with torch.no_grad():
        corr = net(ref_img, real, seg, ref_seg, return_corr=True)
    plain = net.mutual_match(ref_img, seg, ref_seg)
    rec = inference.prepare_exemplar(net, ref_img, ref_seg)
    got = net.mutual_match(None, seg, None, exemplar=rec, hard_warp=True)
    for key, c in (("match_index", corr), ("back_index", corr.transpose(1, 2))):
        pick = lambda o: c.gather(2, o[key].reshape(2, -1).unsqueeze(2)).squeeze(2)
        d = (pick(plain) - pick(got)).abs().max().item()
        same = (plain[key] == got[key]).float().mean().item()
        print(f"[mutual] record mk{mk} {key}: |corr[idx_plain] - corr[idx_record]| = {d:.3e}  (equal indices: {same:.4f})")
        assert d <= TOL, (key, d)
    _check_round_trip_keys(got, 0, net.opt.down)
    assert got["warp_hard"].shape == ref_img.shape and got["warp_valid"].shape == (2, 1) + tuple(ref_img.shape[2:])


# ---- red zones: the cases join tests/test_gpu_red_zones.py's table at import time, so its coverage report and its "every entry point was
# ---- reached" audit count the two K48 entry points (as tests/test_gpu_match_labels.py does for K47).  Four query blocks with a last block of
# ---- 4 queries, a last key tile of 4: a write past an output or the workspace lands in a guard, a read past a plane meets NaN bits
import test_gpu_red_zones as rz  # noqa: E402


def _rz_corr_match_mutual(c):
    from cocosnet_amd import ops
    q, k = c.data(rz.unit(2, 256, 388, 41)), c.data(rz.unit(2, 256, 132, 42))
    rows, cols = ops.corr_match_mutual(q, k, 100.0)
    assert int(cols[0].min()) >= 0 and int(cols[0].max()) < 388 and int(rows[0].max()) < 132
    return list(rows) + list(cols)


def _rz_match_round_trip(c):
    from cocosnet_amd import ops
    g = torch.Generator().manual_seed(46)
    row = c.data(torch.randint(-3, 263, (2, 36), generator=g).to(torch.int32))
    col = c.data(torch.randint(-3, 39, (2, 260), generator=g))
    return list(ops.match_round_trip(row, col, (6, 6), (13, 20)))


RZ_CASES = {"corr_match_mutual-2x388x132": _rz_corr_match_mutual, "match_round_trip-2x6x6-13x20": _rz_match_round_trip}
for _name, _body in RZ_CASES.items():
    if _name not in rz.CASES:
        rz.case(_name, dict(PRECISION="f16x3"))(_body)


@pytest.mark.parametrize("name", list(RZ_CASES))
def test_op_inside_red_zones(name, monkeypatch):
    rz.test_red_zones(name, monkeypatch)
    assert {"corr_match_mutual-2x388x132": "cocos_corr_match_mutual_f16x3", "match_round_trip-2x6x6-13x20": "cocos_match_round_trip"}[name] \
        in set(rz.COVERAGE[name][0])
