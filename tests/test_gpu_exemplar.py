"""Prepared exemplars on the GPU: the shared-exemplar K2 entry point against the existing one (bitwise), and `NoVGGCorrespondence`
with a record against the ordinary route (OUT_TOL, the bound tests/test_gpu_parity.py puts on the path's outputs)."""
import pytest
import torch

from cocosnet_amd._lib import CONSTANTS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OUT_TOL = 2e-4
COCOS_ERR_INVALID, COCOS_ERR_UNSUPPORTED = CONSTANTS["COCOS_ERR_INVALID"], CONSTANTS["COCOS_ERR_UNSUPPORTED"]


# ---- kernel level -----------------------------------------------------------------------------------------------------------------
def _planes_case(Nq, Nk, Cv, B=3, K=256, seed=0, zero_lo=False):
    """operand planes of unit-norm q [B], ONE key / value set, and that set replicated B times"""
    from cocosnet_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    unit = lambda n, N: torch.nn.functional.normalize(torch.randn(n, K, N, device=DEV, generator=g), dim=1)
    q, k1 = unit(B, Nq), unit(1, Nk)
    v1 = torch.randn(1, Cv, Nk, device=DEV, generator=g)
    if zero_lo:      # channels >= 32 exact in f16 (labels): their lo plane is all zero and the masked flavour runs
        v1[:, 32:] = (v1[:, 32:] > 0).float()
    qh, ql = ops.split_f16(q, True, ops.SPLIT_OPERAND_SCALE)
    kh1, kl1 = ops.split_f16(k1, True, ops.SPLIT_OPERAND_SCALE)
    vh1, vl1, vs, mask = ops.split_f16_chan_mask(v1, ops.absmax(v1), Cv > 32)
    rep = lambda t: t.expand(B, *t.shape[1:]).contiguous()
    return (qh, ql), (kh1, kl1, vh1, vl1), (rep(kh1), rep(kl1), rep(vh1), rep(vl1)), vs, mask


def _fwd(name, q, kv, vs, mask, B, Nq, Nk, Cv, extra, K=256, saved=None):
    from cocosnet_amd import _lib, ops
    out = torch.full((B, Cv, Nq), float("nan"), device=DEV)
    lse = torch.full((B, Nq), float("nan"), device=DEV)
    _lib.call(name, q[0].data_ptr(), q[1].data_ptr(), *[t.data_ptr() for t in kv], out.data_ptr(), lse.data_ptr(), saved,
              vs.data_ptr(), None if mask is None else mask.data_ptr(), B, K, Nq, Nk, Cv, 100.0, ops.SPLIT_OPERAND_SCALE, *extra,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out, lse


@pytest.mark.parametrize("Cv", [3, 35, 159])
@pytest.mark.parametrize("Nq,Nk", [(64, 64), (256, 128), (132, 68)])
def test_shared_entry_point_equals_the_existing_one_bitwise(Nq, Nk, Cv, hip_lib):
    B = 3
    q, one, rep, vs, mask = _planes_case(Nq, Nk, Cv, B, seed=Nq + Cv, zero_lo=(Cv == 35))
    if Cv == 35:
        assert int(mask.view(torch.int32).item()) & ~1 == 0      # the masked flavour is what runs
    ref, ref_lse = _fwd("cocos_corr_softmax_warp_fwd_f16x3", q, rep, vs, mask, B, Nq, Nk, Cv, (None, None))
    assert torch.isfinite(ref).all()
    shared, shared_lse = _fwd("cocos_corr_softmax_warp_fwd_f16x3_shared", q, one, vs, mask, B, Nq, Nk, Cv, (0, 0))
    assert torch.equal(shared, ref) and torch.equal(shared_lse, ref_lse)
    dense, dense_lse = _fwd("cocos_corr_softmax_warp_fwd_f16x3_shared", q, rep, vs, mask, B, Nq, Nk, Cv, (Nk * 256, Cv * Nk))
    assert torch.equal(dense, ref) and torch.equal(dense_lse, ref_lse)


def test_shared_entry_point_rejects_what_it_does_not_take(hip_lib):
    from cocosnet_amd import _lib
    B, Nq, Nk, Cv = 2, 64, 64, 3
    q, one, rep, vs, mask = _planes_case(Nq, Nk, Cv, B)
    name = "cocos_corr_softmax_warp_fwd_f16x3_shared"

    def code(**kw):
        a = dict(q=q, kv=one, vs=vs, mask=mask, B=B, Nq=Nq, Nk=Nk, Cv=Cv, extra=(0, 0))
        a.update(kw)
        with pytest.raises(_lib.CocosHipError) as e:
            out, _ = _fwd(name, **a)
        return e.value.code

    saved = torch.empty(_lib.load().cocos_corr_softmax_warp_saved_logits_bytes(B, Nq, Nk) // 4, device=DEV)
    assert code(saved=saved.data_ptr()) == COCOS_ERR_INVALID          # inference only
    assert code(K=128) == COCOS_ERR_UNSUPPORTED
    assert code(Cv=160) == COCOS_ERR_UNSUPPORTED                      # (rejected before anything is read: the planes hold 3 channels)
    assert code(extra=(Nk * 256, 0)) == COCOS_ERR_INVALID             # keys dense, values shared
    assert code(extra=(7, 7)) == COCOS_ERR_INVALID


# ---- module level -----------------------------------------------------------------------------------------------------------------
def _module_case(options, crop, B, Be, seed=0, freeze=False, **over):
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd import inference
    opt = getattr(cc, options)(crop_size=crop, semantic_nc=7, **over)
    torch.manual_seed(seed)
    net = cc.NoVGGCorrespondence(opt).to(DEV)
    net.init_weights(opt.init_type, opt.init_variance)
    net.eval()
    if freeze:
        inference.freeze(net)
    g = torch.Generator(device=DEV).manual_seed(seed + 4)
    onehot = lambda n: torch.zeros(n, 7, crop, crop, device=DEV).scatter_(
        1, torch.randint(0, 7, (n, 1, crop, crop), device=DEV, generator=g), 1.0)
    ref_img = torch.rand(Be, 3, crop, crop, device=DEV, generator=g) * 2 - 1
    real = torch.rand(B, 3, crop, crop, device=DEV, generator=g) * 2 - 1
    return net, ref_img, real, onehot(B), onehot(Be)


def _rep(t, B):
    return t if t.shape[0] == B else t.expand(B, -1, -1, -1).contiguous()


def _compare(net, ref_img, real, seg, ref_seg, **kw):
    from cocosnet_amd import inference
    B = real.shape[0]
    with torch.no_grad():
        want = net(_rep(ref_img, B), real, seg, _rep(ref_seg, B), **kw)
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
        got = net(None, real, seg, None, exemplar=rec, **kw)
    torch.cuda.synchronize()
    if isinstance(want, torch.Tensor):
        want, got = {"corr": want}, {"corr": got}
    assert sorted(got) == sorted(want)
    worst = 0.0
    for k in want:
        assert got[k].shape == want[k].shape, k
        assert torch.isfinite(got[k]).all(), k
        err = (got[k] - want[k]).abs().max().item()
        print(f"[exemplar] {k}: max |recorded - ordinary| = {err:.3e}")
        worst = max(worst, err)
        assert err <= OUT_TOL, (k, err)
    return rec, worst


_CONFIGS = {
    "ade20k_mk1": ("ade20k_options", dict(match_kernel=1)),
    "ade20k_mk3": ("ade20k_options", dict(match_kernel=3)),
    "celebahq": ("celebahq_edge_options", dict(match_kernel=1, show_corr=True)),
    "deepfashion": ("deepfashion_options", dict(match_kernel=1)),
    # cycle mask: the column pass and a second row pass over per-call values (the record's key planes through the ordinary kernels)
    "ade20k_cycle": ("ade20k_options", dict(match_kernel=1, warp_mask_losstype="cycle")),
}


@pytest.mark.parametrize("Be", ["B", 1])
@pytest.mark.parametrize("freeze", [False, True])
@pytest.mark.parametrize("crop", [64, 32])
@pytest.mark.parametrize("config", ["ade20k_mk1", "celebahq", "deepfashion", "ade20k_mk3", "ade20k_cycle"])
def test_module_with_a_record_matches_the_ordinary_route(config, crop, freeze, Be, hip_lib):
    options, over = _CONFIGS[config]
    B = 2
    case = _module_case(options, crop, B, B if Be == "B" else 1, freeze=freeze, **over)
    rec, _ = _compare(*case)
    assert rec.repreparations == 0


@pytest.mark.parametrize("Be", ["B", 1])
@pytest.mark.parametrize("freeze", [False, True])
def test_fused_match_kernel_3_with_a_record(freeze, Be, hip_lib):
    """the fused box family needs a 64-wide grid: crop 256"""
    from cocosnet_amd import ops
    B = 2
    case = _module_case("ade20k_options", 256, B, B if Be == "B" else 1, freeze=freeze, match_kernel=3)
    assert ops.box3_fused_ok(B, 256, 64, 64)
    _compare(*case)


@pytest.mark.parametrize("Be", ["B", 1])
def test_generic_back_end_with_a_record(Be, hip_lib):
    B = 2
    case = _module_case("ade20k_options", 64, B, B if Be == "B" else 1, match_kernel=1)
    _compare(*case, return_corr=True)
    _compare(*case, WTA_scale_weight=0.5)


def test_two_calls_with_one_record_are_bitwise_equal(hip_lib):
    from cocosnet_amd import inference
    net, ref_img, real, seg, ref_seg = _module_case("ade20k_options", 64, 2, 1, match_kernel=1)
    with torch.no_grad():
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
        a = net(None, real, seg, None, exemplar=rec)
        b = net(None, real, seg, None, exemplar=rec)
    for k in a:
        assert torch.equal(a[k], b[k]), k


class _Counter:
    """(name, arguments) of the C-ABI calls, through the hook ops._call offers its timer"""

    def __init__(self, monkeypatch):
        from cocosnet_amd import _lib
        self.calls = []
        real_call = _lib.call

        def counting(name, *args):
            self.calls.append((name, args))
            return real_call(name, *args)
        monkeypatch.setattr(_lib, "call", counting)

    def take(self):
        out, self.calls = self.calls, []
        return out


def _conv_batches(calls):
    """batch argument (the first `int` of the signature) of every convolution launch"""
    import ctypes
    from cocosnet_amd import _lib
    out = []
    for name, args in calls:
        if name.startswith("cocos_conv2d") and "weight_planes" not in name:
            out.append(args[_lib._SIGNATURES[name][1].index(ctypes.c_int)])
    return out


@pytest.mark.parametrize("crop", [64, 32])
def test_no_exemplar_side_work_with_a_record(crop, hip_lib, monkeypatch):
    """B = 2 inputs, ONE exemplar: the ordinary route (fed the exemplar twice) runs both adaptors at batch 2 and the shared blocks at
    batch 4; with a record every convolution left is the content stream's, at batch 2."""
    from cocosnet_amd import inference
    B = 2
    net, ref_img, real, seg, ref_seg = _module_case("ade20k_options", crop, B, 1, freeze=True, match_kernel=1)
    ref2, ref_seg2 = _rep(ref_img, B), _rep(ref_seg, B)
    with torch.no_grad():
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
        net(None, real, seg, None, exemplar=rec)          # (the route's lazy products are made by the first call)
        net(ref2, real, seg, ref_seg2)
        counter = _Counter(monkeypatch)
        net(ref2, real, seg, ref_seg2)
        ordinary = counter.take()
        net(None, real, seg, None, exemplar=rec)
        recorded = counter.take()
    n = lambda calls, pre: sum(1 for name, _ in calls if name.startswith(pre))
    # convolutions: none on a tensor of the exemplar's batch (1) or of both streams (4); what is gone is exactly the image adaptor
    # (the two adaptors are one architecture: half of the ordinary route's batch-2 launches)
    conv_o, conv_r = _conv_batches(ordinary), _conv_batches(recorded)
    assert conv_o and set(conv_o) == {B, 2 * B}, sorted(set(conv_o))
    assert set(conv_r) == {B}, sorted(set(conv_r))
    assert len(conv_r) == conv_o.count(B) // 2 + conv_o.count(2 * B)
    # the value side is the record's
    assert n(ordinary, "cocos_warp_values") >= 1 and n(recorded, "cocos_warp_values") == 0
    assert n(ordinary, "cocos_split_f16_chan_mask") >= 1 and n(recorded, "cocos_split_f16") == 0
    # the key side is the record's: the projection + normalisation runs for ONE problem (theta), not for the pair
    if crop == 64:      # K23
        k23 = lambda calls: [args[0] for name, args in calls if name == "cocos_proj_center_l2norm_planes_f16x3"]
        assert k23(ordinary) == [2] and k23(recorded) == [1]
    else:               # K0 + K1's planes flavour, per tensor
        assert n(ordinary, "cocos_center_l2norm_fwd_planes") == 2 and n(recorded, "cocos_center_l2norm_fwd_planes") == 1
        assert n(ordinary, "cocos_proj1x1") == 2 * n(recorded, "cocos_proj1x1") > 0
    assert n(recorded, "cocos_corr_softmax_warp_fwd_f16x3_shared") == 1 and n(ordinary, "cocos_corr_softmax_warp_fwd_f16x3_shared") == 0
    assert n(recorded, "cocos_corr_softmax_warp_fwd_f16x3_ex") == 0
    assert len(recorded) < len(ordinary)


def test_a_recorded_forward_hands_over_live_buffers_only(hip_lib, monkeypatch):
    from test_gpu_live_buffers import _Guard
    from cocosnet_amd import inference
    net, ref_img, real, seg, ref_seg = _module_case("ade20k_options", 64, 2, 1, freeze=True, match_kernel=1)
    guard = _Guard(monkeypatch)
    with torch.no_grad():
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
        for _ in range(2):
            net(None, real, seg, None, exemplar=rec)
    guard.check(50, 200)


def test_a_recorded_forward_with_poisoned_empty(hip_lib):
    """every torch.empty filled with NaN (what COCOS_POISON_EMPTY=1 switches on for the whole suite, tests/conftest.py): a buffer the
    recorded route reads before a kernel wrote it shows up as a NaN in the outputs"""
    net, ref_img, real, seg, ref_seg = _module_case("ade20k_options", 64, 2, 1, match_kernel=1)
    det, fill = torch.are_deterministic_algorithms_enabled(), torch.utils.deterministic.fill_uninitialized_memory
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.utils.deterministic.fill_uninitialized_memory = True
    try:
        _compare(net, ref_img, real, seg, ref_seg)
    finally:
        torch.use_deterministic_algorithms(det, warn_only=warn)
        torch.utils.deterministic.fill_uninitialized_memory = fill


def test_a_write_to_the_exemplar_prepares_again(hip_lib):
    from cocosnet_amd import inference
    net, ref_img, real, seg, ref_seg = _module_case("ade20k_options", 64, 2, 2, match_kernel=1)
    with torch.no_grad():
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
        a = net(None, real, seg, None, exemplar=rec)
        ref_img.mul_(-1.0)
        b = net(None, real, seg, None, exemplar=rec)
        want = net(ref_img, real, seg, ref_seg)
    assert rec.repreparations == 1
    assert not torch.equal(a["warp_out"], b["warp_out"])
    for k in want:
        assert (b[k] - want[k]).abs().max().item() <= OUT_TOL, k
