"""Frozen-weight inference (cocosnet_amd/inference.py), the host side: records are plain attributes, state_dict() is untouched, the
eligibility rule, validation against (data_ptr, _version), and the hook for the reference's facade.  No GPU: on CPU modules the records
are attached and never used; staleness is exercised with a fake `prepare` callable."""
import contextlib
import importlib

import pytest
import torch
import torch.nn as nn

from cocosnet_amd import correspondence as cc
from cocosnet_amd import inference, producers, vgg


def _fake_prepare(log):
    def prepare(rec):
        log.append(rec.name)
        rec.weight = rec.sources()[0].detach()
        rec.amax = rec.weight.abs().max().reshape(1)
    return prepare


def _small_net():
    torch.manual_seed(0)
    return nn.Sequential(producers.Conv2d(3, 8, 3, padding=1), nn.ReLU(),
                         producers.hip_spectral_norm(producers.Conv2d(8, 8, 3, padding=1)), nn.ReLU(),
                         producers.Conv2d(8, 4, 1))


def test_freeze_on_cpu_modules_leaves_outputs_and_state_dict_alone():
    net = _small_net().eval()
    x = torch.randn(2, 3, 12, 12)
    with torch.no_grad():
        want = net(x)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    names, buffers = [n for n, _ in net.named_parameters()], [n for n, _ in net.named_buffers()]
    report = inference.freeze(net)
    assert report.layers == 3 and report.spectral == 1 and report.skipped == [] and report.launches == 0
    assert all(inference.record_of(m) is not None for m in net if isinstance(m, nn.Conv2d))
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert [n for n, _ in net.named_parameters()] == names and [n for n, _ in net.named_buffers()] == buffers
    with torch.no_grad():
        got = net(x)
    assert torch.equal(got, want)
    # never used on CPU tensors: not prepared, no planes
    assert all(not r.prepared and r.use() is None and r._layouts == {} for r in report.records)
    assert inference.unfreeze(net) == 3
    assert all(inference.record_of(m) is None for m in net)
    final = net.state_dict()
    assert list(final) == list(before) and all(torch.equal(final[k], before[k]) for k in before)
    with torch.no_grad():
        assert torch.equal(net(x), want)


def test_freeze_accepts_a_dictionary_of_networks_and_the_whole_correspondence_network():
    opt = cc.ade20k_options(semantic_nc=5)
    torch.manual_seed(0)
    corr = cc.NoVGGCorrespondence(opt).eval()
    v = vgg.VGG19_feature_color_torchversion().eval()
    keys = list(corr.state_dict())
    report = inference.freeze({"netCorr": corr, "vgg": v, "netD": None})
    convs = [m for m in corr.modules() if isinstance(m, producers.Conv2d)]
    assert report.layers == len(convs) + 2 + 16 and report.spectral > 0
    assert inference.record_of(corr.theta) is not None and inference.record_of(corr.phi) is not None
    assert list(corr.state_dict()) == keys
    # the input-gradient layout is kept for the fixed VGG only
    assert all(inference.record_of(m).keep_dgrad for m in v.modules() if isinstance(m, producers.Conv2d))
    assert not any(inference.record_of(m).keep_dgrad for m in convs)
    assert any(r.name.startswith("netCorr.") for r in report.records) and any(r.name.startswith("vgg.") for r in report.records)
    with pytest.raises(TypeError):
        inference.freeze(3)


def test_the_framework_spectral_hook_gets_the_record_lookup_and_an_unknown_one_is_left_alone():
    sn = producers._sn_mod.SpectralNorm
    torch.manual_seed(1)
    m = nn.Sequential(torch.nn.utils.spectral_norm(producers.Conv2d(4, 4, 3))).eval()
    x = torch.randn(1, 4, 8, 8)
    with torch.no_grad():
        want = m(x)
    hook = next(h for h in m[0]._forward_pre_hooks.values() if isinstance(h, sn))
    assert type(hook) is sn
    report = inference.freeze(m)
    assert report.layers == 1 and report.spectral == 1 and report.skipped == []
    assert type(hook) is producers._SpectralNormRecord
    with torch.no_grad():
        assert torch.equal(m(x), want)
    inference.unfreeze(m)
    assert type(hook) is sn and inference.record_of(m[0]) is None

    class Other(sn):
        pass
    hook.__class__ = Other
    report = inference.freeze(m)
    assert report.layers == 0 and report.skipped == ["0"] and inference.record_of(m[0]) is None and type(hook) is Other


def test_eligibility_rule():
    net = _small_net()
    report = inference.freeze(net, prepare=_fake_prepare([]))
    plain, spectral = report.records[0], report.records[1]
    net.eval()
    # grad enabled with requires_grad=True on the weight: today's route
    assert torch.is_grad_enabled() and not plain.eligible() and not spectral.eligible()
    with torch.no_grad():
        assert plain.eligible() and spectral.eligible()
        # train() on a spectral layer: the power iteration must run
        net.train()
        assert not spectral.eligible() and not plain.eligible()
        net.eval()
    # frozen parameters with an input that needs gradients (the fixed VGG inside a training step)
    v = vgg.VGG19_feature_color_torchversion().eval()
    for p in v.parameters():
        p.requires_grad_(False)
    vr = inference.freeze(v, prepare=_fake_prepare([]))
    assert torch.is_grad_enabled() and all(r.eligible() for r in vr.records)
    next(v.parameters()).requires_grad_(True)
    assert not vr.records[0].eligible() and vr.records[1].eligible()
    # the A/B switch bypasses attached records
    try:
        inference.FROZEN = False
        assert not any(r.eligible() for r in vr.records)
    finally:
        inference.FROZEN = True
    # CPU weights are never served from a record, eligible or not
    with torch.no_grad():
        assert plain.eligible() and plain.use() is None


def test_validation_reports_stale_after_load_state_dict_and_in_place_edits():
    net = _small_net().eval()
    log = []
    report = inference.freeze(net, prepare=_fake_prepare(log))
    plain, spectral = report.records[0], report.records[1]
    assert not plain.stale() and not plain.prepared            # nothing prepared yet: nothing to be stale
    plain.ensure(); spectral.ensure()
    assert log == ["0", "2"] and plain.prepared and report.repreparations == 0
    plain.ensure()
    assert log == ["0", "2"] and not plain.stale()             # unchanged tensors: the record stands
    w0 = plain.weight
    sd = {k: v.clone() + 0.25 for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    assert plain.stale() and spectral.stale()
    plain.ensure()
    assert report.repreparations == 1 and log[-1] == "0" and not plain.stale()
    assert plain._layouts == {} and torch.equal(plain.weight, w0) and torch.equal(plain.amax, net[0].weight.detach().abs().max().reshape(1))
    spectral.ensure()
    assert report.repreparations == 2 and not spectral.stale()
    with torch.no_grad():
        net[2].weight_orig.mul_(0.5)                            # a manual in-place edit
    assert spectral.stale() and not plain.stale()
    with torch.no_grad():
        net[2].weight_u.add_(0.1)
    spectral.ensure()
    assert report.repreparations == 3 and not spectral.stale()
    # a replaced parameter (another address) is a mismatch too
    net[0].weight = nn.Parameter(net[0].weight.detach().clone())
    assert plain.stale()


def test_the_spectral_hook_hands_out_the_record_only_when_it_may():
    """compute_weight consults the record in eval() only; on CPU tensors the record is never usable, so the values are the hook's own."""
    net = _small_net().eval()
    x = torch.randn(1, 8, 6, 6)
    with torch.no_grad():
        want = net[2](x)
    inference.freeze(net)
    with torch.no_grad():
        assert torch.equal(net[2](x), want)
    net.train()
    u = net[2].weight_u.clone()
    net[2](x)
    assert not torch.equal(net[2].weight_u, u)                  # train(): the power iteration ran


# ---- the reference's facade: built the way tests/test_facade_cpu.py builds it ---------------------------------------------------------
from oracle import ref_harness as rh      # noqa: E402

needs_reference = pytest.mark.skipif(not rh.reference_available(), reason="the reference tree is not present")


def _facade_opt():
    import argparse
    networks = rh.load_reference()
    with rh._cwd(rh.REFERENCE_ROOT):
        to = importlib.import_module("options.test_options").TestOptions()
        parser = to.initialize(argparse.ArgumentParser())
        parser = networks.modify_commandline_options(parser, False)
        opt, _ = parser.parse_known_args([])
    flags = dict(name="facade_test", dataset_mode="ade20k", gpu_ids=[], use_attention=True, maskmix=True, warp_mask_losstype="direct",
                 PONO=True, PONO_C=True, batchSize=1, isTrain=False, semantic_nc=151, label_nc=150, contain_dontcare_label=True,
                 no_instance=True, crop_size=256, load_size=256, aspect_ratio=1.0)
    for k, v in flags.items():
        setattr(opt, k, v)
    return opt


def _facade_build(opt):
    p2p = importlib.import_module("models.pix2pix_model")
    torch.manual_seed(0)
    with rh._cwd(rh.REFERENCE_ROOT), contextlib.redirect_stdout(None):
        return p2p.Pix2PixModel(opt).eval()


@needs_reference
def test_install_and_restore_round_trip_on_the_reference_facade():
    networks = rh.load_reference()
    ref_corr = importlib.import_module(networks.__name__ + ".correspondence")
    p2p = importlib.import_module("models.pix2pix_model")
    original_cls, original_init = ref_corr.NoVGGCorrespondence, p2p.Pix2PixModel.initialize_networks
    opt = _facade_opt()
    try:
        cc.install_into_reference(networks)
        replaced = inference.install_inference_into_reference(networks)
        assert replaced == {"initialize_networks": original_init}
        assert p2p.Pix2PixModel.initialize_networks is not original_init
        model = _facade_build(opt)
        report = model.frozen_report
        assert isinstance(report, inference.FrozenReport) and report.layers > 20 and report.repreparations == 0
        corr = model.net["netCorr"]
        assert inference.record_of(corr.theta) is not None and inference.record_of(corr.phi) is not None
        assert "frozen_report" not in model.state_dict() and not any("_cocos_frozen" in k for k in model.state_dict())
        inference.restore_reference_inference(networks, replaced)
        assert p2p.Pix2PixModel.initialize_networks is original_init
        again = _facade_build(opt)
        assert not hasattr(again, "frozen_report") and inference.record_of(again.net["netCorr"].theta) is None
        assert list(again.state_dict()) == list(model.state_dict())
    finally:
        p2p.Pix2PixModel.initialize_networks = original_init
        ref_corr.NoVGGCorrespondence = original_cls
