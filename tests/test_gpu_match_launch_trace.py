"""The launch trace of the match family: which C-ABI entry points every correspondence_* entry point calls, in order, per route.

`cocosnet_amd._lib.call` is wrapped with a recorder that appends the entry-point name and calls the original; one call of the entry
point (forward, and backward where the route has one) is compared with a list written out below.  The lists were recorded at the commit
before the host-side helpers of the family were folded (K49's), so a refactor of the Python above the kernels that drops, adds or
reorders a launch — the K23 / K1 choice of the plane producer, a second split of the operands, a lost transpose — fails here by name.
Names only: no kernel, code object or timing is looked at.

Shapes: the smallest the routes accept — B = 1, 256 channels, content grid 4 x 8, exemplar grid 4 x 4, down = 4 (ref_img 1 x 3 x 16 x 16),
temperature 0.01, match_kernel 1 with PONO_C; the fused match_kernel-3 case needs equal 64 x 64 grids (ops.box3_fused_ok).  A
LazyProj1x1 pair takes K23 only on equal grids of whole 128-position tiles (ops.proj_norm_fused_ok), so at 4 x 8 / 4 x 4 the lazy cases
pin "project, then K1 twice", and the `k23` cases repeat the producer's four callers on equal 8 x 16 grids, where the pair is taken.

The `box3-` cases pin the match_kernel-3 routes (K37, K41, K51 - K55) the same way.  Their lists were recorded at 65b2e86, the commit
before the host side of that family was folded.  Shapes: equal 4 x 64 grids (N = 256, T is 256 x 256, ref_img 1 x 3 x 16 x 256), the
smallest cocos_box3_fused_supported takes; no member needed a larger one.  The labels are _label_pair's halves: 128 allowed positions
per label, so nothing falls back.  A lazy pair requires a gradient on every leaf where the route differentiates and on none where it
is forward-only, so ops.proj_raw_fused_ok takes it and the K25 choice is pinned; `box3-match-rows-lazy-unfused-proj` pins the other
arm of the forward-only prologue ("project, then detach").  The `box3-hot-path-cycle` cases run correspondence_hot_path with the
cycle terms, where _BoxedCorr.rows, .cols and .rows again share one T and one gradient sink."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
B, C, CIN, DOWN, NC, T = 1, 256, 64, 4, 5, 0.01
SMALL = ((4, 8), (4, 4))
TILE = ((8, 16), (8, 16))
BOX = ((4, 64), (4, 64))


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


def _match_box3(lazy, **kw):
    from cocosnet_amd.hot_path import correspondence_match_box3
    th, ph = _operands(BOX, lazy)
    return lambda: correspondence_match_box3(th, ph, _cfg(3), T, restrict=_label_pair(BOX), **kw)


def _transport_box3(lazy, topk):
    from cocosnet_amd.hot_path import correspondence_transport_box3
    th, ph = _operands(BOX, lazy)
    return lambda: correspondence_transport_box3(th, ph, _cfg(3), T, iters=2, topk=topk)


def _sparse_box3(lazy, **kw):
    from cocosnet_amd.hot_path import correspondence_sparse_box3
    th, ph = _operands(BOX, lazy, grad=True)
    ref_img, seg, ref_seg = _images(BOX)
    if kw.get("restrict") == "pair":
        kw["restrict"] = _label_pair(BOX)
    return lambda: correspondence_sparse_box3(th, ph, ref_img, seg, ref_seg, _cfg(3), T, 2, **kw)["warp_out"].sum().backward()


def _flow_box3(lazy):
    from cocosnet_amd.hot_path import correspondence_flow_box3
    th, ph = _operands(BOX, lazy, grad=True)
    ref_img = _images(BOX)[0]
    return lambda: correspondence_flow_box3(th, ph, ref_img, _cfg(3), T, radius=1)["warp_out"].sum().backward()


def _nll_box3(lazy, symmetric):
    from cocosnet_amd.hot_path import correspondence_nll_box3
    th, ph = _operands(BOX, lazy, grad=True)
    (fh, fw), (gh, gw) = BOX
    target = ((torch.arange(fh * fw, device=DEV) * 7 + 3) % (gh * gw)).view(1, fh, fw).expand(B, fh, fw).contiguous()
    target[:, 0, 0] = -1
    return lambda: correspondence_nll_box3(th, ph, target, _cfg(3), T, symmetric=symmetric)["loss_match"].backward()


def _hot_path_cycle(lazy):
    """correspondence_hot_path on match_kernel 3 with the cycle terms (test_gpu_mk3_sizes' cfg3 flags): a row pass, a column pass and a
    second row pass over one T, forward and backward"""
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_hot_path
    th, ph = _operands(BOX, lazy, grad=True)
    ref_img, seg, ref_seg = _images(BOX)
    real_img = _images(BOX, seed=2)[0]
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=DOWN, warp_bilinear=True, isTrain=True, warp_mask_losstype="none",
                        warp_cycle_w=1.0, two_cycle=True)

    def run():
        out = correspondence_hot_path(th, ph, ref_img, real_img, seg, ref_seg, cfg)
        sum(out[k].sum() for k in sorted(out)).backward()
    return run


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
for _lazy in (False, True):
    _kind = "lazy" if _lazy else "tensor"
    _case(f"box3-match-rows-{_kind}", lambda l=_lazy: _match(BOX, l, mk=3))
    _case(f"box3-match-cols-{_kind}", lambda l=_lazy: _match(BOX, l, mk=3, direction="cols"))
    _case(f"box3-match-rows-topk2-{_kind}", lambda l=_lazy: _match(BOX, l, mk=3, topk=2))
    _case(f"box3-match-cols-topk2-{_kind}", lambda l=_lazy: _match(BOX, l, mk=3, direction="cols", topk=2))
    _case(f"box3-restrict-rows-{_kind}", lambda l=_lazy: _match_box3(l))
    _case(f"box3-restrict-cols-{_kind}", lambda l=_lazy: _match_box3(l, direction="cols"))
    _case(f"box3-restrict-rows-topk2-{_kind}", lambda l=_lazy: _match_box3(l, topk=2))
    _case(f"box3-transport-top1-{_kind}", lambda l=_lazy: _transport_box3(l, 1))
    _case(f"box3-transport-topk2-{_kind}", lambda l=_lazy: _transport_box3(l, 2))
    _case(f"box3-sparse-{_kind}", lambda l=_lazy: _sparse_box3(l))
    _case(f"box3-sparse-transport-{_kind}", lambda l=_lazy: _sparse_box3(l, transport=dict(iters=2, tau=1.0)))
    _case(f"box3-sparse-restrict-{_kind}", lambda l=_lazy: _sparse_box3(l, restrict="pair"))
    _case(f"box3-flow-{_kind}", lambda l=_lazy: _flow_box3(l))
    _case(f"box3-nll-symmetric-{_kind}", lambda l=_lazy: _nll_box3(l, True))
    _case(f"box3-nll-rows-only-{_kind}", lambda l=_lazy: _nll_box3(l, False))
    _case(f"box3-hot-path-cycle-{_kind}", lambda l=_lazy: _hot_path_cycle(l))
_case("box3-match-rows-lazy-unfused-proj", lambda: _match(BOX, True, mk=3), PROJ_BWD_FUSED=False)

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
    # ---- the match_kernel-3 routes, recorded at 65b2e86 (see the module docstring) ----
    'box3-flow-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3', 'cocos_absmax4',
        'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_match_f16x3', 'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax',
        'cocos_transpose_f32', 'cocos_transpose_f32', 'cocos_box3_match_refine_fwd', 'cocos_gather_patches_subcell',
        'cocos_gather_patches_subcell_bwd_off', 'cocos_box3_match_refine_bwd_pair', 'cocos_box3_match_refine_bwd_theta',
        'cocos_transpose_f32', 'cocos_box3_match_refine_bwd_key', 'cocos_transpose_f32', 'cocos_unfold3_stats_bwd',
        'cocos_unfold3_stats_bwd', 'cocos_absmax_accumulate', 'cocos_proj1x1_stream_f16x3', 'cocos_proj1x1_dw_f16x3',
        'cocos_absmax_accumulate', 'cocos_proj1x1_stream_f16x3', 'cocos_proj1x1_dw_f16x3'
    ],
    'box3-flow-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_match_f16x3', 'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax',
        'cocos_transpose_f32', 'cocos_transpose_f32', 'cocos_box3_match_refine_fwd', 'cocos_gather_patches_subcell',
        'cocos_gather_patches_subcell_bwd_off', 'cocos_box3_match_refine_bwd_pair', 'cocos_box3_match_refine_bwd_theta',
        'cocos_transpose_f32', 'cocos_box3_match_refine_bwd_key', 'cocos_transpose_f32', 'cocos_unfold3_stats_bwd',
        'cocos_unfold3_stats_bwd'
    ],
    'box3-hot-path-cycle-lazy': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_warp_values_amax', 'cocos_box3_corr_xbox_f16x3', 'cocos_split_f16_chan_mask', 'cocos_box3_softmax_warp_fwd_f16x3',
        'cocos_warp_head_fwd_ex', 'cocos_warp_values_amax', 'cocos_absmax_accumulate', 'cocos_split_f16_chan_mask',
        'cocos_box3_softmax_warp_fwd_f16x3', 'cocos_absmax_accumulate', 'cocos_split_f16_chan_mask',
        'cocos_box3_softmax_warp_fwd_f16x3', 'cocos_absmax_accumulate', 'cocos_rowdot_f64', 'cocos_split_f16_transpose_pair',
        'cocos_box3_softmax_warp_bwd_f16x3', 'cocos_split_f16_ex', 'cocos_hgemm_f16x3', 'cocos_absmax_accumulate', 'cocos_rowdot_f64',
        'cocos_split_f16_transpose_pair', 'cocos_box3_softmax_warp_bwd_f16x3', 'cocos_split_f16_ex', 'cocos_hgemm_f16x3',
        'cocos_warp_head_bwd_ex', 'cocos_split_f16_transpose_pair', 'cocos_box3_softmax_warp_bwd_f16x3',
        'cocos_box3_adjoint_planes_f16x3', 'cocos_hgemm_f16x3', 'cocos_hgemm_f16x3', 'cocos_unfold3_stats_bwd_maps_pair',
        'cocos_proj_bwd_input_planes_f16x3', 'cocos_proj1x1_dw_affine_pair_f16x3'
    ],
    'box3-hot-path-cycle-tensor': [
        'cocos_warp_values_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex',
        'cocos_split_f16_ex', 'cocos_box3_corr_xbox_f16x3', 'cocos_split_f16_chan_mask', 'cocos_box3_softmax_warp_fwd_f16x3',
        'cocos_warp_head_fwd_ex', 'cocos_warp_values_amax', 'cocos_absmax_accumulate', 'cocos_split_f16_chan_mask',
        'cocos_box3_softmax_warp_fwd_f16x3', 'cocos_absmax_accumulate', 'cocos_split_f16_chan_mask',
        'cocos_box3_softmax_warp_fwd_f16x3', 'cocos_absmax_accumulate', 'cocos_rowdot_f64', 'cocos_split_f16_transpose_pair',
        'cocos_box3_softmax_warp_bwd_f16x3', 'cocos_split_f16_ex', 'cocos_hgemm_f16x3', 'cocos_absmax_accumulate', 'cocos_rowdot_f64',
        'cocos_split_f16_transpose_pair', 'cocos_box3_softmax_warp_bwd_f16x3', 'cocos_split_f16_ex', 'cocos_hgemm_f16x3',
        'cocos_warp_head_bwd_ex', 'cocos_split_f16_transpose_pair', 'cocos_box3_softmax_warp_bwd_f16x3',
        'cocos_box3_adjoint_planes_f16x3', 'cocos_split_f16_ex', 'cocos_hgemm_f16x3', 'cocos_split_f16_ex', 'cocos_hgemm_f16x3',
        'cocos_unfold3_stats_bwd', 'cocos_unfold3_stats_bwd'
    ],
    'box3-match-cols-lazy': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_match_f16x3'
    ],
    'box3-match-cols-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_match_f16x3'
    ],
    'box3-match-cols-topk2-lazy': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_f16x3'
    ],
    'box3-match-cols-topk2-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_f16x3'
    ],
    'box3-match-rows-lazy': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_match_f16x3'
    ],
    'box3-match-rows-lazy-unfused-proj': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3',
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_match_f16x3'
    ],
    'box3-match-rows-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_match_f16x3'
    ],
    'box3-match-rows-topk2-lazy': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_f16x3'
    ],
    'box3-match-rows-topk2-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_f16x3'
    ],
    'box3-nll-rows-only-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3', 'cocos_absmax4',
        'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_match_f16x3', 'cocos_transpose_f32', 'cocos_transpose_f32',
        'cocos_box3_pair_logit_fwd', 'cocos_box3_match_f16x3', 'cocos_box3_pair_logit_bwd_pair',
        'cocos_box3_sparse_softmax_warp_bwd_theta', 'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_key',
        'cocos_transpose_f32', 'cocos_box3_lse_bwd_f16x3', 'cocos_box3_adjoint_planes_f16x3', 'cocos_hgemm_f16x3', 'cocos_hgemm_f16x3',
        'cocos_unfold3_stats_bwd_maps_pair', 'cocos_proj_bwd_input_planes_f16x3', 'cocos_proj1x1_dw_affine_pair_f16x3',
        'cocos_absmax_accumulate', 'cocos_proj1x1_stream_f16x3', 'cocos_proj1x1_dw_f16x3', 'cocos_absmax_accumulate',
        'cocos_proj1x1_stream_f16x3', 'cocos_proj1x1_dw_f16x3'
    ],
    'box3-nll-rows-only-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_match_f16x3', 'cocos_transpose_f32', 'cocos_transpose_f32',
        'cocos_box3_pair_logit_fwd', 'cocos_box3_match_f16x3', 'cocos_box3_pair_logit_bwd_pair',
        'cocos_box3_sparse_softmax_warp_bwd_theta', 'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_key',
        'cocos_transpose_f32', 'cocos_box3_lse_bwd_f16x3', 'cocos_box3_adjoint_planes_f16x3', 'cocos_split_f16_ex', 'cocos_hgemm_f16x3',
        'cocos_split_f16_ex', 'cocos_hgemm_f16x3', 'cocos_unfold3_stats_bwd', 'cocos_unfold3_stats_bwd'
    ],
    'box3-nll-symmetric-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3', 'cocos_absmax4',
        'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_match_f16x3', 'cocos_box3_match_f16x3', 'cocos_transpose_f32', 'cocos_transpose_f32',
        'cocos_box3_pair_logit_fwd', 'cocos_box3_sparse_softmax_warp_bwd_key', 'cocos_box3_pair_logit_bwd_pair',
        'cocos_box3_sparse_softmax_warp_bwd_theta', 'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_key',
        'cocos_transpose_f32', 'cocos_box3_lse_bwd_f16x3', 'cocos_box3_lse_bwd_f16x3', 'cocos_box3_adjoint_planes_f16x3',
        'cocos_hgemm_f16x3', 'cocos_hgemm_f16x3', 'cocos_unfold3_stats_bwd_maps_pair', 'cocos_proj_bwd_input_planes_f16x3',
        'cocos_proj1x1_dw_affine_pair_f16x3', 'cocos_absmax_accumulate', 'cocos_proj1x1_stream_f16x3', 'cocos_proj1x1_dw_f16x3',
        'cocos_absmax_accumulate', 'cocos_proj1x1_stream_f16x3', 'cocos_proj1x1_dw_f16x3'
    ],
    'box3-nll-symmetric-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_match_f16x3', 'cocos_box3_match_f16x3', 'cocos_transpose_f32', 'cocos_transpose_f32',
        'cocos_box3_pair_logit_fwd', 'cocos_box3_sparse_softmax_warp_bwd_key', 'cocos_box3_pair_logit_bwd_pair',
        'cocos_box3_sparse_softmax_warp_bwd_theta', 'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_key',
        'cocos_transpose_f32', 'cocos_box3_lse_bwd_f16x3', 'cocos_box3_lse_bwd_f16x3', 'cocos_box3_adjoint_planes_f16x3',
        'cocos_split_f16_ex', 'cocos_hgemm_f16x3', 'cocos_split_f16_ex', 'cocos_hgemm_f16x3', 'cocos_unfold3_stats_bwd',
        'cocos_unfold3_stats_bwd'
    ],
    'box3-restrict-cols-lazy': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_labels_f16x3'
    ],
    'box3-restrict-cols-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_labels_f16x3'
    ],
    'box3-restrict-rows-lazy': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_labels_f16x3'
    ],
    'box3-restrict-rows-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_labels_f16x3'
    ],
    'box3-restrict-rows-topk2-lazy': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_labels_f16x3'
    ],
    'box3-restrict-rows-topk2-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_labels_f16x3'
    ],
    'box3-sparse-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3', 'cocos_absmax4',
        'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_f16x3', 'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax',
        'cocos_warp_values_amax', 'cocos_transpose_f32', 'cocos_transpose_f32', 'cocos_transpose_f32',
        'cocos_box3_sparse_softmax_warp_fwd', 'cocos_transpose_f32', 'cocos_upsample_nearest_fwd', 'cocos_upsample_nearest_bwd',
        'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_pair', 'cocos_box3_sparse_softmax_warp_bwd_theta',
        'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_key', 'cocos_transpose_f32', 'cocos_unfold3_stats_bwd',
        'cocos_unfold3_stats_bwd', 'cocos_absmax_accumulate', 'cocos_proj1x1_stream_f16x3', 'cocos_proj1x1_dw_f16x3',
        'cocos_absmax_accumulate', 'cocos_proj1x1_stream_f16x3', 'cocos_proj1x1_dw_f16x3'
    ],
    'box3-sparse-restrict-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3', 'cocos_absmax4',
        'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_labels_f16x3', 'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax',
        'cocos_warp_values_amax', 'cocos_transpose_f32', 'cocos_transpose_f32', 'cocos_transpose_f32',
        'cocos_box3_sparse_softmax_warp_fwd', 'cocos_transpose_f32', 'cocos_upsample_nearest_fwd', 'cocos_upsample_nearest_bwd',
        'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_pair', 'cocos_box3_sparse_softmax_warp_bwd_theta',
        'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_key', 'cocos_transpose_f32', 'cocos_unfold3_stats_bwd',
        'cocos_unfold3_stats_bwd', 'cocos_absmax_accumulate', 'cocos_proj1x1_stream_f16x3', 'cocos_proj1x1_dw_f16x3',
        'cocos_absmax_accumulate', 'cocos_proj1x1_stream_f16x3', 'cocos_proj1x1_dw_f16x3'
    ],
    'box3-sparse-restrict-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_labels_f16x3', 'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax',
        'cocos_warp_values_amax', 'cocos_transpose_f32', 'cocos_transpose_f32', 'cocos_transpose_f32',
        'cocos_box3_sparse_softmax_warp_fwd', 'cocos_transpose_f32', 'cocos_upsample_nearest_fwd', 'cocos_upsample_nearest_bwd',
        'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_pair', 'cocos_box3_sparse_softmax_warp_bwd_theta',
        'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_key', 'cocos_transpose_f32', 'cocos_unfold3_stats_bwd',
        'cocos_unfold3_stats_bwd'
    ],
    'box3-sparse-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_f16x3', 'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax',
        'cocos_warp_values_amax', 'cocos_transpose_f32', 'cocos_transpose_f32', 'cocos_transpose_f32',
        'cocos_box3_sparse_softmax_warp_fwd', 'cocos_transpose_f32', 'cocos_upsample_nearest_fwd', 'cocos_upsample_nearest_bwd',
        'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_pair', 'cocos_box3_sparse_softmax_warp_bwd_theta',
        'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_key', 'cocos_transpose_f32', 'cocos_unfold3_stats_bwd',
        'cocos_unfold3_stats_bwd'
    ],
    'box3-sparse-transport-lazy': [
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3',
        'cocos_absmax_accumulate', 'cocos_absmax_accumulate', 'cocos_proj_weight_planes', 'cocos_proj1x1_stream_f16x3', 'cocos_absmax4',
        'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3',
        'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_unfold3_stats_fwd_amax',
        'cocos_unfold3_stats_fwd_amax', 'cocos_warp_values_amax', 'cocos_transpose_f32', 'cocos_transpose_f32', 'cocos_transpose_f32',
        'cocos_box3_sparse_softmax_warp_bias_fwd', 'cocos_transpose_f32', 'cocos_upsample_nearest_fwd', 'cocos_upsample_nearest_bwd',
        'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_pair', 'cocos_box3_sparse_softmax_warp_bwd_theta',
        'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_key', 'cocos_transpose_f32', 'cocos_unfold3_stats_bwd',
        'cocos_unfold3_stats_bwd', 'cocos_absmax_accumulate', 'cocos_proj1x1_stream_f16x3', 'cocos_proj1x1_dw_f16x3',
        'cocos_absmax_accumulate', 'cocos_proj1x1_stream_f16x3', 'cocos_proj1x1_dw_f16x3'
    ],
    'box3-sparse-transport-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3',
        'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_unfold3_stats_fwd_amax',
        'cocos_unfold3_stats_fwd_amax', 'cocos_warp_values_amax', 'cocos_transpose_f32', 'cocos_transpose_f32', 'cocos_transpose_f32',
        'cocos_box3_sparse_softmax_warp_bias_fwd', 'cocos_transpose_f32', 'cocos_upsample_nearest_fwd', 'cocos_upsample_nearest_bwd',
        'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_pair', 'cocos_box3_sparse_softmax_warp_bwd_theta',
        'cocos_transpose_f32', 'cocos_box3_sparse_softmax_warp_bwd_key', 'cocos_transpose_f32', 'cocos_unfold3_stats_bwd',
        'cocos_unfold3_stats_bwd'
    ],
    'box3-transport-top1-lazy': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3',
        'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3'
    ],
    'box3-transport-top1-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3',
        'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3'
    ],
    'box3-transport-topk2-lazy': [
        'cocos_absmax4', 'cocos_proj_weight_prep_pair', 'cocos_proj_raw_planes_stats_f16x3', 'cocos_unfold3_stats_finish_pair',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3',
        'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3'
    ],
    'box3-transport-topk2-tensor': [
        'cocos_unfold3_stats_fwd_amax', 'cocos_unfold3_stats_fwd_amax', 'cocos_split_f16_ex', 'cocos_split_f16_ex',
        'cocos_box3_corr_xbox_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3',
        'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3', 'cocos_box3_topk_bias_f16x3'
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
