"""The launch trace of the match family: which C-ABI entry points every correspondence_* entry point calls, in order, per route.

`cocosnet_amd._lib.call` is wrapped with a recorder that appends the entry-point name and calls the original; one call of the entry
point (forward, and backward where the route has one) is compared with a list written out below.  The lists were recorded at the commit
before the host-side helpers of the family were folded (K49's), so a refactor of the Python above the kernels that drops, adds or
reorders a launch — the K23 / K1 choice of the plane producer, a second split of the operands, a lost transpose — fails here by name.
Names only: no kernel, code object or timing is looked at.

Shapes: the smallest the routes accept — B = 1, 256 channels, content grid 4 x 8, exemplar grid 4 x 4, down = 4 (ref_img 1 x 3 x 16 x 16),
temperature 0.01, match_kernel 1 with PONO_C; the fused match_kernel-3 case needs equal 64 x 64 grids (ops.box3_fused_ok).  A
LazyProj1x1 pair takes K23 only on equal grids of whole 128-position tiles (ops.proj_norm_fused_ok), so at 4 x 8 / 4 x 4 the lazy cases
pin "project, then K1 twice", and the `k23` cases repeat the producer's four callers on equal 8 x 16 grids, where the pair is taken."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
B, C, CIN, DOWN, NC, T = 1, 256, 64, 4, 5, 0.01
SMALL = ((4, 8), (4, 4))
TILE = ((8, 16), (8, 16))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def _operands(grids, lazy, grad=False, seed=0):
    """(theta, phi) for the two grids: fp32 tensors [B,256,h,w], or a LazyProj1x1 pair over CIN input channels"""
    from cocosnet_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    out = []
    for h, w in grids:
        if lazy:
            leaves = [rnd(B, CIN, h, w), rnd(C, CIN, 1, 1) / CIN ** 0.5, rnd(C) * 0.1]
            out.append(ops.LazyProj1x1(*(t.requires_grad_(grad) for t in leaves)))
        else:
            out.append(rnd(B, C, h, w).requires_grad_(grad))
    return out


def _images(grids, seed=1):
    """(ref_img [B,3,gh*down,gw*down], seg_map one-hot on the content grid's image, ref_seg_map on the exemplar's)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    (fh, fw), (gh, gw) = grids
    ref_img = torch.rand(B, 3, gh * DOWN, gw * DOWN, device=DEV, generator=g) * 2 - 1
    segs = []
    for h, w in grids:
        lab = torch.randint(0, NC, (B, 1, h * DOWN, w * DOWN), device=DEV, generator=g)
        segs.append(torch.zeros(B, NC, h * DOWN, w * DOWN, device=DEV).scatter_(1, lab, 1.0))
    return ref_img, segs[0], segs[1]


def _label_pair(grids):
    """two labels in halves of each grid: every content label has 8 exemplar positions, so no position falls back"""
    (fh, fw), (gh, gw) = grids
    q = (torch.arange(fw, device=DEV) * 2 // fw).view(1, 1, fw).expand(B, fh, fw).contiguous()
    k = (torch.arange(gw, device=DEV) * 2 // gw).view(1, 1, gw).expand(B, gh, gw).contiguous()
    return q, k


def _cfg(mk=1):
    from cocosnet_amd.hot_path import HotPathConfig
    return HotPathConfig(match_kernel=mk, PONO_C=True, down=DOWN)


def _match(grids, lazy, mk=1, **kw):
    from cocosnet_amd.hot_path import correspondence_match
    th, ph = _operands(grids, lazy)
    if kw.get("restrict") == "pair":
        kw["restrict"] = _label_pair(grids)
    return lambda: correspondence_match(th, ph, _cfg(mk), T, **kw)


def _mutual(grids, lazy):
    from cocosnet_amd.hot_path import correspondence_mutual
    th, ph = _operands(grids, lazy)
    return lambda: correspondence_mutual(th, ph, _cfg(), T)


def _sparse(grids, lazy, **kw):
    from cocosnet_amd.hot_path import correspondence_sparse
    th, ph = _operands(grids, lazy)
    ref_img, seg, ref_seg = _images(grids)
    if kw.get("restrict") == "pair":
        kw["restrict"] = _label_pair(grids)
    return lambda: correspondence_sparse(th, ph, ref_img, seg, ref_seg, _cfg(), T, 2, **kw)


def _flow(grids, lazy):
    from cocosnet_amd.hot_path import correspondence_flow
    th, ph = _operands(grids, lazy, grad=True)
    ref_img = _images(grids)[0]
    return lambda: correspondence_flow(th, ph, ref_img, _cfg(), T, radius=1)["warp_out"].sum().backward()


def _nll(grids, lazy):
    from cocosnet_amd.hot_path import correspondence_nll
    th, ph = _operands(grids, lazy, grad=True)
    (fh, fw), (gh, gw) = grids
    target = (torch.arange(fh * fw, device=DEV) % (gh * gw)).view(1, fh, fw).expand(B, fh, fw).contiguous()
    target[:, 0, 0] = -1
    return lambda: correspondence_nll(th, ph, target, _cfg(), T)["loss_match"].backward()


#: case -> (what builds the call, the switches to set on ops for it)
CASES = {}


def _case(name, make, **switches):
    CASES[name] = (make, switches)


for _lazy in (False, True):
    _kind = "lazy" if _lazy else "tensor"
    _case(f"match-rows-{_kind}", lambda l=_lazy: _match(SMALL, l))
    _case(f"match-cols-{_kind}", lambda l=_lazy: _match(SMALL, l, direction="cols"))
    _case(f"match-topk2-{_kind}", lambda l=_lazy: _match(SMALL, l, topk=2))
    _case(f"match-refine1-{_kind}", lambda l=_lazy: _match(SMALL, l, refine=1))
    _case(f"match-restrict-{_kind}", lambda l=_lazy: _match(SMALL, l, restrict="pair"))
    _case(f"sparse-dense-{_kind}", lambda l=_lazy: _sparse(SMALL, l, search="dense"))
    _case(f"sparse-patchmatch-{_kind}", lambda l=_lazy: _sparse(SMALL, l, search="patchmatch"))
    _case(f"sparse-restrict-{_kind}", lambda l=_lazy: _sparse(SMALL, l, restrict="pair"))
    _case(f"flow-{_kind}", lambda l=_lazy: _flow(SMALL, l))
    _case(f"nll-{_kind}", lambda l=_lazy: _nll(SMALL, l))
    _case(f"mutual-fused-{_kind}", lambda l=_lazy: _mutual(SMALL, l))
    _case(f"mutual-two-calls-{_kind}", lambda l=_lazy: _mutual(SMALL, l), MATCH_MUTUAL_FUSED=False)
_case("match-materialised-top1", lambda: _match(SMALL, False), MATCH_FUSED=False)
_case("match-materialised-topk2", lambda: _match(SMALL, False, topk=2), MATCH_FUSED=False)
_case("match-box3-64x64", lambda: _match(((64, 64), (64, 64)), False, mk=3))
_case("match-rows-k23", lambda: _match(TILE, True))
_case("mutual-fused-k23", lambda: _mutual(TILE, True))
_case("flow-k23", lambda: _flow(TILE, True))
_case("nll-k23", lambda: _nll(TILE, True))

#: what the recorder printed for every case at the commit before the fold (see the module docstring) — pasted, not regenerated
EXPECTED = {
    'flow-k23': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_center_l2norm_planes_f16x3', 'cocos_corr_topk_f16x3',
        'cocos_match_refine_f16x3', 'cocos_gather_patches_subcell', 'cocos_gather_patches_subcell_bwd_off',
        'cocos_match_refine_bwd_query_f16x3', 'cocos_transpose_f32', 'cocos_match_refine_bwd_key_f16x3',
        'cocos_transpose_f32', 'cocos_proj_bwd_input_f16x3', 'cocos_proj1x1_dw_affine_pair_f16x3'
    ],
    'flow-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_absmax_accumulate',
        'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_center_l2norm_fwd_planes', 'cocos_corr_topk_f16x3', 'cocos_match_refine_f16x3', 'cocos_gather_patches_subcell',
        'cocos_gather_patches_subcell_bwd_off', 'cocos_match_refine_bwd_query_f16x3', 'cocos_transpose_f32',
        'cocos_match_refine_bwd_key_f16x3', 'cocos_transpose_f32', 'cocos_center_l2norm_bwd_planes',
        'cocos_center_l2norm_bwd_planes', 'cocos_proj1x1_dw_f16x3', 'cocos_proj1x1_bwd_f16x3', 'cocos_proj1x1_dw_f16x3',
        'cocos_proj1x1_bwd_f16x3'
    ],
    'flow-tensor': [
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_corr_topk_f16x3',
        'cocos_match_refine_f16x3', 'cocos_gather_patches_subcell', 'cocos_gather_patches_subcell_bwd_off',
        'cocos_match_refine_bwd_query_f16x3', 'cocos_transpose_f32', 'cocos_match_refine_bwd_key_f16x3',
        'cocos_transpose_f32', 'cocos_center_l2norm_bwd_planes', 'cocos_center_l2norm_bwd_planes'
    ],
    'match-box3-64x64': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_match_f16x3'
    ],
    'match-cols-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_corr_match_f16x3'
    ],
    'match-cols-tensor': [
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_corr_match_f16x3'
    ],
    'match-materialised-top1': [
        'cocos_center_l2norm_fwd', 'cocos_center_l2norm_fwd', 'cocos_absmax_accumulate', 'cocos_absmax_accumulate',
        'cocos_split_f16_ex', 'cocos_split_f16_ex', 'cocos_hgemm_f16x3', 'cocos_row_argmax_lse'
    ],
    'match-materialised-topk2': [
        'cocos_center_l2norm_fwd', 'cocos_center_l2norm_fwd', 'cocos_absmax_accumulate', 'cocos_absmax_accumulate',
        'cocos_split_f16_ex', 'cocos_split_f16_ex', 'cocos_hgemm_f16x3', 'cocos_row_topk_lse'
    ],
    'match-refine1-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_corr_match_f16x3', 'cocos_match_refine_f16x3'
    ],
    'match-refine1-tensor': [
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_corr_match_f16x3',
        'cocos_match_refine_f16x3'
    ],
    'match-restrict-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_corr_topk_labels_f16x3'
    ],
    'match-restrict-tensor': [
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_corr_topk_labels_f16x3'
    ],
    'match-rows-k23': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_center_l2norm_planes_f16x3', 'cocos_corr_match_f16x3'
    ],
    'match-rows-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_corr_match_f16x3'
    ],
    'match-rows-tensor': [
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_corr_match_f16x3'
    ],
    'match-topk2-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_corr_topk_f16x3'
    ],
    'match-topk2-tensor': [
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_corr_topk_f16x3'
    ],
    'mutual-fused-k23': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_center_l2norm_planes_f16x3',
        'cocos_corr_match_mutual_f16x3', 'cocos_match_round_trip'
    ],
    'mutual-fused-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_corr_match_mutual_f16x3', 'cocos_match_round_trip'
    ],
    'mutual-fused-tensor': [
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_corr_match_mutual_f16x3',
        'cocos_match_round_trip'
    ],
    'mutual-two-calls-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_corr_match_f16x3', 'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes',
        'cocos_corr_match_f16x3', 'cocos_match_round_trip'
    ],
    'mutual-two-calls-tensor': [
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_corr_match_f16x3',
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_corr_match_f16x3', 'cocos_match_round_trip'
    ],
    'nll-k23': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_center_l2norm_planes_f16x3',
        'cocos_corr_match_mutual_f16x3', 'cocos_pair_logits_f16x3', 'cocos_sparse_softmax_warp_bwd_key_f16x3',
        'cocos_corr_lse_bwd_f16x3', 'cocos_corr_lse_bwd_f16x3', 'cocos_pair_logits_bwd_query_f16x3', 'cocos_transpose_f32',
        'cocos_transpose_f32', 'cocos_proj_bwd_input_f16x3', 'cocos_proj1x1_dw_affine_pair_f16x3'
    ],
    'nll-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_absmax_accumulate',
        'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_center_l2norm_fwd_planes', 'cocos_corr_match_mutual_f16x3', 'cocos_pair_logits_f16x3',
        'cocos_sparse_softmax_warp_bwd_key_f16x3', 'cocos_corr_lse_bwd_f16x3', 'cocos_corr_lse_bwd_f16x3',
        'cocos_pair_logits_bwd_query_f16x3', 'cocos_transpose_f32', 'cocos_transpose_f32', 'cocos_center_l2norm_bwd_planes',
        'cocos_center_l2norm_bwd_planes', 'cocos_proj1x1_dw_f16x3', 'cocos_proj1x1_bwd_f16x3', 'cocos_proj1x1_dw_f16x3',
        'cocos_proj1x1_bwd_f16x3'
    ],
    'nll-tensor': [
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_corr_match_mutual_f16x3',
        'cocos_pair_logits_f16x3', 'cocos_sparse_softmax_warp_bwd_key_f16x3', 'cocos_corr_lse_bwd_f16x3',
        'cocos_corr_lse_bwd_f16x3', 'cocos_pair_logits_bwd_query_f16x3', 'cocos_transpose_f32', 'cocos_transpose_f32',
        'cocos_center_l2norm_bwd_planes', 'cocos_center_l2norm_bwd_planes'
    ],
    'sparse-dense-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_absmax_accumulate',
        'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_center_l2norm_fwd_planes', 'cocos_corr_topk_f16x3', 'cocos_warp_values_amax', 'cocos_transpose_f32',
        'cocos_sparse_softmax_warp_fwd_f16x3', 'cocos_transpose_f32', 'cocos_upsample_nearest_fwd'
    ],
    'sparse-dense-tensor': [
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_corr_topk_f16x3', 'cocos_warp_values_amax',
        'cocos_transpose_f32', 'cocos_sparse_softmax_warp_fwd_f16x3', 'cocos_transpose_f32', 'cocos_upsample_nearest_fwd'
    ],
    'sparse-patchmatch-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_absmax_accumulate',
        'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes',
        'cocos_corr_topk_f16x3', 'cocos_patchmatch_step_f16x3', 'cocos_patchmatch_step_f16x3', 'cocos_patchmatch_step_f16x3',
        'cocos_patchmatch_step_f16x3', 'cocos_warp_values_amax', 'cocos_transpose_f32', 'cocos_sparse_softmax_warp_fwd_f16x3',
        'cocos_transpose_f32', 'cocos_upsample_nearest_fwd'
    ],
    'sparse-patchmatch-tensor': [
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes',
        'cocos_center_l2norm_fwd_planes', 'cocos_corr_topk_f16x3', 'cocos_patchmatch_step_f16x3',
        'cocos_patchmatch_step_f16x3', 'cocos_patchmatch_step_f16x3', 'cocos_patchmatch_step_f16x3', 'cocos_warp_values_amax',
        'cocos_transpose_f32', 'cocos_sparse_softmax_warp_fwd_f16x3', 'cocos_transpose_f32', 'cocos_upsample_nearest_fwd'
    ],
    'sparse-restrict-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_absmax_accumulate',
        'cocos_absmax_accumulate', 'cocos_proj1x1_fwd_f16x3', 'cocos_center_l2norm_fwd_planes',
        'cocos_center_l2norm_fwd_planes', 'cocos_corr_topk_labels_f16x3', 'cocos_warp_values_amax', 'cocos_transpose_f32',
        'cocos_sparse_softmax_warp_fwd_f16x3', 'cocos_transpose_f32', 'cocos_upsample_nearest_fwd'
    ],
    'sparse-restrict-tensor': [
        'cocos_center_l2norm_fwd_planes', 'cocos_center_l2norm_fwd_planes', 'cocos_corr_topk_labels_f16x3',
        'cocos_warp_values_amax', 'cocos_transpose_f32', 'cocos_sparse_softmax_warp_fwd_f16x3', 'cocos_transpose_f32',
        'cocos_upsample_nearest_fwd'
    ],
}


def test_every_case_has_its_list():
    assert set(CASES) == set(EXPECTED)


@pytest.mark.parametrize("name", list(CASES))
def test_entry_points_called_in_order(name, monkeypatch):
    from cocosnet_amd import _lib, ops
    make, switches = CASES[name]
    for k, v in switches.items():
        monkeypatch.setattr(ops, k, v)
    run = make()
    trace, call = [], _lib.call

    def recorder(entry, *args):
        trace.append(entry)
        return call(entry, *args)

    monkeypatch.setattr(_lib, "call", recorder)
    run()
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "call", call)
    print(f"[trace] {name!r}: {trace!r}")
    assert trace == EXPECTED[name]
