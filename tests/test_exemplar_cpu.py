"""Prepared exemplars (inference.prepare_exemplar) on the CPU: the record stands in for the exemplar stream of project() exactly.

On the CPU the two streams go through `self.layer` separately, so everything here is bitwise: theta_raw with a record equals the
ordinary project()'s, phi_raw is the record's, a stale record prepares again, and a record is refused wherever a gradient could be
wanted through the exemplar side."""
import pytest
import torch

from cocosnet_amd import correspondence as cc
from cocosnet_amd import inference


def _case(options=cc.ade20k_options, B=2, Be=None, seed=0, **over):
    opt = options(crop_size=32, semantic_nc=5, **over)
    torch.manual_seed(seed)
    net = cc.NoVGGCorrespondence(opt)
    net.init_weights(opt.init_type, opt.init_variance)
    net.eval()
    g = torch.Generator().manual_seed(seed + 1)
    S, nc = 32, opt.semantic_nc
    onehot = lambda n: torch.zeros(n, nc, S, S).scatter_(1, torch.randint(0, nc, (n, 1, S, S), generator=g), 1.0)
    Be = B if Be is None else Be
    ref_img = torch.rand(Be, 3, S, S, generator=g) * 2 - 1
    real = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    return net, ref_img, real, onehot(B), onehot(Be)


@pytest.mark.parametrize("options", [cc.ade20k_options, cc.deepfashion_options])
def test_project_with_a_record_is_bitwise_the_ordinary_project(options):
    net, ref_img, real, seg, ref_seg = _case(options)
    with torch.no_grad():
        theta0, phi0 = net.project(ref_img, real, seg, ref_seg)
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
        theta1, phi1 = net.project(None, real, seg, None, exemplar=rec)
    assert torch.equal(theta1, theta0)
    assert torch.equal(phi1, phi0) and torch.equal(phi1, rec.phi_raw())
    assert rec.repreparations == 0


def test_one_exemplar_for_all_inputs():
    net, ref_img, real, seg, ref_seg = _case(B=3, Be=1)
    with torch.no_grad():
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
        theta1, phi1 = net.project(None, real, seg, None, exemplar=rec)
        theta0, phi0 = net.project(ref_img.expand(3, -1, -1, -1), real, seg, ref_seg.expand(3, -1, -1, -1))
    assert rec.batch == 1 and phi1.shape[0] == 1
    assert torch.equal(theta1, theta0)
    # (the CPU convolutions pick their blocking by batch size: a batch of 1 and row 0 of a batch of 3 differ in the order of the fp32 sums)
    torch.testing.assert_close(phi1, phi0[:1], rtol=1e-5, atol=1e-6)


def test_the_exemplar_stream_does_not_run_with_a_record(monkeypatch):
    net, ref_img, real, seg, ref_seg = _case()
    with torch.no_grad():
        theta0, _ = net.project(ref_img, real, seg, ref_seg)
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)

        def boom(*a, **k):
            raise AssertionError("the exemplar stream ran")
        monkeypatch.setattr(net.adaptive_model_img, "forward", boom)
        monkeypatch.setattr(net.phi, "forward", boom)
        theta1, _ = net.project(None, real, seg, None, exemplar=rec)
    assert torch.equal(theta1, theta0)


def _edit_ref_img(net, rec):
    rec.ref_img.mul_(0.5)


def _load_state_dict(net, rec):
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    for k in sd:
        if k.startswith("phi.") or k.startswith("adaptive_model_img."):
            sd[k] = sd[k] * 1.25
    net.load_state_dict(sd)


def _edit_layer_weight(net, rec):
    with torch.no_grad():
        next(net.layer.parameters()).add_(0.01)


@pytest.mark.parametrize("edit", [_edit_ref_img, _load_state_dict, _edit_layer_weight])
def test_a_stale_record_prepares_again(edit):
    net, ref_img, real, seg, ref_seg = _case()
    with torch.no_grad():
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
        before = rec.phi_raw().clone()
        edit(net, rec)
        assert rec.stale()
        _, phi1 = net.project(None, real, seg, None, exemplar=rec)
        assert rec.repreparations == 1 and not rec.stale()
        fresh = inference.prepare_exemplar(net, ref_img, ref_seg)
        theta0, phi0 = net.project(ref_img, real, seg, ref_seg)
        net.project(None, real, seg, None, exemplar=rec)
    assert rec.repreparations == 1                      # (nothing changed since: no third preparation)
    assert torch.equal(phi1, fresh.phi_raw()) and torch.equal(phi1, phi0)
    assert not torch.equal(phi1, before)


def test_refusals():
    net, ref_img, real, seg, ref_seg = _case()
    with torch.no_grad():
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
    net.train()
    with pytest.raises(ValueError):
        inference.prepare_exemplar(net, ref_img, ref_seg)
    with pytest.raises(ValueError), torch.no_grad():
        net.project(None, real, seg, None, exemplar=rec)
    net.eval()
    net.opt.isTrain = True
    with pytest.raises(ValueError):                     # grad mode with isTrain
        net.project(None, real, seg, None, exemplar=rec)
    net.opt.warp_cycle_w = 1.0
    with pytest.raises(ValueError), torch.no_grad():   # a training term, even without grad mode
        net.project(None, real, seg, None, exemplar=rec)
    with pytest.raises(ValueError), torch.no_grad():
        net.forward(None, real, seg, None, exemplar=rec)
    net.opt.isTrain = False
    with pytest.raises(ValueError), torch.no_grad():   # the path computes the cycle terms whenever warp_cycle_w > 0
        net.project(None, real, seg, None, exemplar=rec)
    net.opt.warp_cycle_w = 0.0
    with pytest.raises(ValueError), torch.no_grad():   # Be = 2 against B = 3
        net.project(None, torch.cat((real, real[:1])), torch.cat((seg, seg[:1])), None, exemplar=rec)
    with pytest.raises(ValueError), torch.no_grad():   # no exemplar at all
        net.project(None, real, seg, None)
    with pytest.raises(ValueError), torch.no_grad():
        net.forward(None, real, seg, None)
    other = _case(seed=3)[0]
    with pytest.raises(ValueError), torch.no_grad():   # a record of another network
        other.project(None, real, seg, None, exemplar=rec)


def test_frozen_off_ignores_the_record(monkeypatch):
    net, ref_img, real, seg, ref_seg = _case(B=2, Be=1)
    with torch.no_grad():
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
        theta0, phi0 = net.project(ref_img.expand(2, -1, -1, -1), real, seg, ref_seg.expand(2, -1, -1, -1))
        monkeypatch.setattr(inference, "FROZEN", False)
        calls = []
        real_fwd = net.adaptive_model_img.forward
        monkeypatch.setattr(net.adaptive_model_img, "forward", lambda *a, **k: calls.append(1) or real_fwd(*a, **k))
        theta1, phi1 = net.project(None, real, seg, None, exemplar=rec)
    assert calls, "the ordinary route (exemplar stream included) must run with inference.FROZEN off"
    with torch.no_grad():
        rec.ref_img.mul_(0.5)
        net.project(None, real, seg, None, exemplar=rec)
    assert rec.stale() and rec.repreparations == 0      # an ignored record is not prepared again either
    assert torch.equal(theta1, theta0) and torch.equal(phi1, phi0) and phi1.shape[0] == 2


def test_state_dict_keys_are_untouched():
    net, ref_img, real, seg, ref_seg = _case()
    keys = list(net.state_dict().keys())
    with torch.no_grad():
        rec = inference.prepare_exemplar(net, ref_img, ref_seg)
        net.project(None, real, seg, None, exemplar=rec)
    assert list(net.state_dict().keys()) == keys
    assert not any(isinstance(v, inference.PreparedExemplar) for v in vars(net).values())
