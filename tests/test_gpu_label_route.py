"""The label route at module level: a one-hot map that carries a label record (cocosnet_amd.labels) takes K35 in the seg adaptor's
layer1 and in the seven SPADE.mlp_shared convolutions of its three SPADEResnetBlocks; the same tensor without the record (clone), a
tensor written after the record was attached, and COCOS_LABEL_CONV=0 take the dense route — and all of them compute the module."""
import contextlib
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NC, B, SIZE = 151, 2, 32
LABEL_FWD = "cocos_label_conv3x3_fwd"


def _adaptor(seed=0):
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd import producers
    opt = cc.ade20k_options(semantic_nc=NC, ngf=64)
    opt.spade_ic = NC
    torch.manual_seed(seed)
    net = producers.AdaptiveFeatureGenerator(opt).to(DEV)
    return net.eval()                           # eval: the spectral-norm power iteration stands still, every arm sees the same W / sigma


def _label_map(seed=1, size=SIZE):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, NC, (B, 1, size // 4, size // 4), device=DEV, generator=g).repeat_interleave(4, 2).repeat_interleave(4, 3)


class _Spy:
    """C-ABI calls by name (the `_lib.call` interception of tests/test_gpu_live_buffers.py), dense convolutions by input channels,
    nearest resizes by input channels"""

    def __init__(self, monkeypatch):
        from cocosnet_amd import _lib, ops
        self.names, self.conv_cin, self.resize_cin = [], [], []
        real_call, real_conv, real_interp = _lib.call, ops.conv2d, F.interpolate
        monkeypatch.setattr(_lib, "call", lambda name, *a: (self.names.append(name), real_call(name, *a))[1])
        monkeypatch.setattr(ops, "conv2d", lambda x, *a, **k: (self.conv_cin.append(x.shape[1]), real_conv(x, *a, **k))[1])
        monkeypatch.setattr(F, "interpolate", lambda x, *a, **k: (self.resize_cin.append(x.shape[1]), real_interp(x, *a, **k))[1])

    def reset(self):
        del self.names[:], self.conv_cin[:], self.resize_cin[:]

    def count(self, name):
        return sum(1 for n in self.names if n == name)


def _rel(a, r):
    return float((a.double() - r).abs().max() / (r.abs().max() + 1e-300))


def test_the_record_moves_eight_convolutions_to_the_label_kernel(hip_lib, monkeypatch):
    from cocosnet_amd import labels
    net = _adaptor()
    seg = labels.one_hot(_label_map(), NC)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        y = net(seg, seg)
        assert spy.count(LABEL_FWD) == 1 + 7, spy.count(LABEL_FWD)
        assert NC not in spy.conv_cin and NC not in spy.resize_cin, (spy.conv_cin, spy.resize_cin)
        spy.reset()
        dense = seg.clone()
        y_dense = net(dense, dense)                      # no record: the dense route, as before
        assert spy.count(LABEL_FWD) == 0 and spy.conv_cin.count(NC) == 8 and spy.resize_cin.count(NC) == 3
        spy.reset()
        monkeypatch.setattr(labels, "LABEL_CONV", "0")   # the A/B switch hides the record
        y_off = net(seg, seg)
        assert spy.count(LABEL_FWD) == 0 and spy.conv_cin.count(NC) == 8
    assert torch.equal(y_off, y_dense)
    assert _rel(y, y_dense.double()) < 1e-3              # (both are held to fp64 below)


@contextlib.contextmanager
def _forced(tape):
    """tests/kink_tape.py's sites, plus the one this route adds: SPADE's ReLU inside the label call — the kernel runs WITHOUT its fused
    ReLU (its linear part) and the recorded pattern is applied on top, exactly as the helper treats the dense mlp_shared."""
    import kink_tape
    from cocosnet_amd import spade as sp
    with kink_tape.install(tape):
        taped = sp.shared_activation

        def shared_activation(self, segmap, labels=None, sample=1):
            if labels is None:
                return taped(self, segmap)
            return tape.act(self.mlp_shared[1](segmap, reflect=1, labels=labels, sample=sample, relu=False), 0.0)
        sp.shared_activation = shared_activation
        try:
            yield tape
        finally:
            sp.shared_activation = taped


def test_label_and_dense_arms_against_an_fp64_copy_on_its_branch_pattern(hip_lib, monkeypatch):
    """Forward and EVERY parameter gradient of the adaptor, three times: seg with its record (label route), seg.clone() (dense route)
    and a torch-fp64 copy of the module.  The bound is the one tests/test_gpu_conv.py applies to the producers' dense arm on the forced
    branch pattern (test_module_end_to_end_every_gradient_on_the_fp64_branch_pattern): 1e-3 of each tensor's range."""
    import kink_tape
    from cocosnet_amd import labels
    net = _adaptor()
    seg = labels.one_hot(_label_map(), NC)
    tape = kink_tape.KinkTape()
    spy = _Spy(monkeypatch)
    with _forced(tape):
        net64 = copy.deepcopy(net).double()
        seg64 = seg.double()
        y64 = net64(seg64, seg64)
        G = torch.randn(y64.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
        y64.backward(G.double())
        want = {"y": y64.detach(), **{"d " + n: p.grad.clone() for n, p in net64.named_parameters()}}
        errs = {}
        for arm, inp in (("label", seg), ("dense", seg.clone())):
            net.zero_grad()
            tape.rewind("replay")
            spy.reset()
            y = net(inp, inp)
            y.backward(G)
            assert tape.pos == len(tape.masks)
            assert spy.count(LABEL_FWD) == (8 if arm == "label" else 0)
            assert spy.count("cocos_label_conv3x3_bwd") == (8 if arm == "label" else 0)
            got = {"y": y.detach(), **{"d " + n: p.grad.clone() for n, p in net.named_parameters()}}
            assert sorted(got) == sorted(want)
            errs[arm] = {k: _rel(got[k], want[k]) for k in want}
    worst = {arm: max(e.items(), key=lambda kv: kv[1]) for arm, e in errs.items()}
    print("LABEL_ROUTE_FP64", worst)
    bad = {arm: {k: v for k, v in e.items() if not v < 1e-3} for arm, e in errs.items()}
    assert not bad["label"] and not bad["dense"], bad


def test_a_write_after_the_record_takes_the_dense_route(hip_lib, monkeypatch):
    """The CelebA-HQ glasses write (pix2pix_model.py:191) bumps the tensor's version: the record is stale and is not read."""
    from cocosnet_amd import labels
    net = _adaptor()
    seg = labels.one_hot(_label_map(), NC)
    seg[:, -3:-2] = (torch.rand(B, 1, SIZE, SIZE, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)) > 0.5).float()
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        y = net(seg, seg)
        assert spy.count(LABEL_FWD) == 0 and spy.conv_cin.count(NC) == 8
        net64 = copy.deepcopy(net).double()
        y64 = net64(seg.double(), seg.double())
    assert _rel(y, y64) < 1e-3


def _corr(**flags):
    from cocosnet_amd import correspondence as cc
    opt = cc.ade20k_options(semantic_nc=NC, match_kernel=1, **flags)
    torch.manual_seed(0)
    net = cc.NoVGGCorrespondence(opt).to(DEV)
    net.init_weights(opt.init_type, opt.init_variance)
    g = torch.Generator(device=DEV).manual_seed(5)
    img, real = (torch.rand(B, 3, SIZE, SIZE, device=DEV, generator=g) * 2 - 1 for _ in range(2))
    return opt, net.eval(), img, real


def test_whole_module_with_recorded_maps(hip_lib, monkeypatch):
    """NoVGGCorrespondence.forward with recorded seg_map / ref_seg_map: outputs equal the oracle applied to the module's own
    projections within tests/test_gpu_parity.py's OUT_TOL, the content stream runs the label kernel; with opt.mask_noise the
    content stream's input is seg_map + noise — a new tensor without a record — and takes the dense route."""
    from test_gpu_parity import OUT_TOL, rel
    from cocosnet_amd import labels
    from oracle import corr_oracle as co
    opt, net, img, real = _corr()
    seg, ref_seg = labels.one_hot(_label_map(1), NC), labels.one_hot(_label_map(2), NC)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        out = net(img, real, seg, ref_seg)
        assert spy.count(LABEL_FWD) == 8
        th, ph = net.project(img, real, seg, ref_seg)
    oflags = dict(match_kernel=opt.match_kernel, PONO_C=opt.PONO_C, down=opt.down, warp_bilinear=opt.warp_bilinear, isTrain=opt.isTrain,
                  warp_mask_losstype=opt.warp_mask_losstype, warp_cycle_w=opt.warp_cycle_w, two_cycle=opt.two_cycle)
    n = lambda t: t.cpu().numpy()
    ref = co.hot_path_forward(n(th), n(ph), n(img), n(real), n(seg), n(ref_seg), co.default_opt(**oflags))
    for k, r in ref.items():
        assert rel(out[k], r) < OUT_TOL, k
    with torch.no_grad():
        th_dense, _ = net.project(img, real, seg.clone(), ref_seg.clone())
    assert _rel(th, th_dense.double()) < 1e-3
    opt.mask_noise = True
    spy.reset()
    with torch.no_grad():
        net(img, real, seg, ref_seg)
    assert spy.count(LABEL_FWD) == 0 and spy.conv_cin.count(NC) == 8


def test_frozen_layers_build_their_tap_table_once(hip_lib, monkeypatch):
    from cocosnet_amd import inference, labels
    net = _adaptor()
    seg = labels.one_hot(_label_map(), NC)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        y0 = net(seg, seg)
        assert spy.count("cocos_label_conv_table") == 8            # unfrozen: a table per call
        inference.freeze(net)
        spy.reset()
        y1, y2 = net(seg, seg), net(seg, seg)
        assert spy.count(LABEL_FWD) == 16 and spy.count("cocos_label_conv_table") == 8, spy.count("cocos_label_conv_table")
        assert torch.equal(y1, y0) and torch.equal(y2, y0)
        net.load_state_dict(copy.deepcopy(net.state_dict()))       # in-place copies: every record is stale
        spy.reset()
        y3 = net(seg, seg)
        assert spy.count("cocos_label_conv_table") == 8 and torch.equal(y3, y0)


def test_the_cells_the_label_kernel_leaves_are_exact(hip_lib, monkeypatch):
    """tests/cache_audit.py over the label route: each of the eight max|y| cells K35 leaves holds exactly max|y| when it is remembered
    (the audit's wrapper asserts it at the call), under the table's own key.  Nothing downstream recalls them today — layer1's output
    goes to K13 / K34 and SPADE's shared activation to a ReflectionPad2d, neither of which reads a maximum — so no consumer is
    asserted; tests/test_gpu_label_conv.py checks that `_recall_amax(y)` finds the cell."""
    import cache_audit
    from cocosnet_amd import labels, ops
    monkeypatch.setattr(ops, "CONV_PRECISION", "f16x3")
    net = _adaptor()
    seg = labels.one_hot(_label_map(), NC)
    cache_audit.clear_caches()
    left = []
    real = ops._glue_remember
    monkeypatch.setattr(ops, "_glue_remember", lambda t, cell: (left.append((t, cell)), real(t, cell))[1])
    a = cache_audit.audit(monkeypatch)
    with torch.no_grad():
        net(seg, seg)
    assert len(left) == 8 and all(c is not None for _, c in left)
    mine = {id(c) for _, c in left}
    assert sum(1 for cell, _ in a._made_by.values() if id(cell) in mine) == 8      # each went through the audited _remember_amax
    for t, c in left:
        assert float(c) == float(t.abs().max())
