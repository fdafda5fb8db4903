"""Host logic of the label route (cocosnet_amd.labels): the one-hot drop-in, the validity rule of the record, the reference's facade.
No GPU: off the device the record is attached but never used — the networks compute exactly what they compute without it."""
import argparse
import importlib

import pytest
import torch

from oracle import ref_harness as rh


def _label_map(B=2, nc=7, H=12, W=10, seed=0):
    return torch.randint(0, nc, (B, 1, H, W), generator=torch.Generator().manual_seed(seed))


def test_one_hot_on_the_host_equals_scatter_bitwise():
    from cocosnet_amd import labels
    lab = _label_map()
    seg = labels.one_hot(lab, 7)
    assert seg.dtype == torch.float32 and torch.equal(seg, torch.zeros(2, 7, 12, 10).scatter_(1, lab, 1.0))
    rec = labels.record_of(seg)
    assert rec is not None and rec.nc == 7 and rec.index.dtype == torch.int32 and torch.equal(rec.index.long(), lab[:, 0])


def test_a_fresh_record_is_found_and_every_other_tensor_object_misses():
    from cocosnet_amd import labels
    seg = labels.one_hot(_label_map(), 7)
    assert labels.record_of(seg) is labels.record_of(seg) is not None
    for other in (seg.clone(), seg[:, :], seg + 0, torch.cat([seg, seg]), seg.detach(), seg.view(2, 7, 12, 10)):
        assert labels.record_of(other) is None
    assert labels.record_of(None) is None and labels.record_of(torch.zeros(1, 2, 3, 3)) is None


@pytest.mark.parametrize("write", ["glasses", "add_"])
def test_an_in_place_write_invalidates_the_record(write):
    from cocosnet_amd import labels
    seg = labels.one_hot(_label_map(), 7)
    assert labels.record_of(seg) is not None
    if write == "glasses":                  # the CelebA-HQ glasses channel (pix2pix_model.py:191)
        seg[:, -3:-2] = torch.ones(2, 1, 12, 10)
    else:
        seg.add_(0)
    assert labels.record_of(seg) is None
    assert labels.record_of(labels.attach(seg, _label_map())) is not None      # a new attach starts from the tensor as it is now


def test_label_conv_off_hides_every_record(monkeypatch):
    from cocosnet_amd import labels
    seg = labels.one_hot(_label_map(), 7)
    for off in (False, "0"):
        monkeypatch.setattr(labels, "LABEL_CONV", off)
        assert labels.record_of(seg) is None
    monkeypatch.setattr(labels, "LABEL_CONV", "1")
    assert labels.record_of(seg) is not None


def test_attach_verifies_one_hotness_on_request():
    from cocosnet_amd import labels
    lab = _label_map()
    seg = torch.zeros(2, 7, 12, 10).scatter_(1, lab, 1.0)
    rec = labels.record_of(labels.attach(seg, lab, verify=True))
    assert rec is not None and torch.equal(rec.index.long(), lab[:, 0])
    bad = seg.clone()
    bad[0, 3, 4, 5] += 0.5
    with pytest.raises(ValueError, match="one-hot"):
        labels.attach(bad, lab, verify=True)
    with pytest.raises(ValueError, match="one-hot"):
        labels.attach(seg.clone(), lab.flip(0), verify=True)
    with pytest.raises(ValueError):
        labels.attach(seg[:, :, :6], lab)                                      # another grid
    assert labels.record_of(labels.attach(bad, lab)) is not None               # verify=False: the caller's word is taken


def test_whole_ratio():
    from cocosnet_amd import labels
    rec = labels.record_of(labels.one_hot(_label_map(1, 3, 32, 16), 3))
    assert [labels.whole_ratio(rec, s) for s in ((32, 16), (8, 4), (16, 4), (5, 4), (64, 32))] == [1, 4, 0, 0, 0]


def test_the_predicate_takes_no_host_tensors():
    from cocosnet_amd import labels, ops
    rec = labels.record_of(labels.one_hot(_label_map(), 7))
    assert not ops.label_conv_ok(torch.zeros(16, 7, 3, 3), rec.index)


def test_a_host_forward_ignores_the_record_bitwise(monkeypatch):
    """NoVGGCorrespondence.forward on the host (the oracle's restatement behind the hot path's signature, as tests/test_facade_cpu.py
    runs it) with a recorded seg_map equals the same call on seg_map.clone(): the record is not used off the GPU, and no framework
    restatement of K35 stands in for it."""
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd import labels, ops
    from oracle import torch_ref as tr
    monkeypatch.setattr(cc, "correspondence_hot_path",
                        lambda th, ph, ri, re, sm, rs, cfg, temperature=0.01, detach_flag=False, WTA_scale_weight=1, return_corr=False, **kw:
                        tr.hot_path(th, ph, ri, re, sm, rs, cfg, temperature=temperature, detach_flag=detach_flag,
                                    WTA_scale_weight=WTA_scale_weight, return_corr=return_corr))
    called = []
    real_fn = ops.label_conv3x3
    monkeypatch.setattr(ops, "label_conv3x3", lambda *a, **k: (called.append(1), real_fn(*a, **k))[1])
    opt = cc.ade20k_options(semantic_nc=5, match_kernel=1)
    torch.manual_seed(0)
    net = cc.NoVGGCorrespondence(opt).eval()
    g = torch.Generator().manual_seed(1)
    img, real = torch.rand(1, 3, 32, 32, generator=g) * 2 - 1, torch.rand(1, 3, 32, 32, generator=g) * 2 - 1
    seg = labels.one_hot(_label_map(1, 5, 32, 32, seed=3), 5)
    ref_seg = labels.one_hot(_label_map(1, 5, 32, 32, seed=4), 5)
    assert labels.record_of(seg) is not None
    with torch.no_grad():
        a = net(img, real, seg, ref_seg)
        b = net(img, real, seg.clone(), ref_seg.clone())
    assert not called and sorted(a) == sorted(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k


# ---- the reference's facade -------------------------------------------------------------------------------------------------------
needs_reference = pytest.mark.skipif(not rh.reference_available(), reason="the reference checkout is not present")


def _bare_model(dataset_mode, nc):
    """A Pix2PixModel with what preprocess_input reads and nothing else (no networks are built)"""
    rh.load_reference()
    p2p = importlib.import_module("models.pix2pix_model")
    model = p2p.Pix2PixModel.__new__(p2p.Pix2PixModel)
    torch.nn.Module.__init__(model)
    model.opt = argparse.Namespace(dataset_mode=dataset_mode, gpu_ids=[], label_nc=nc - 1, contain_dontcare_label=True)
    model.FloatTensor = torch.FloatTensor
    return model


def _data(nc, channels=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    lab = lambda: torch.randint(0, nc, (2, channels, 16, 16), generator=g)
    return {"label": lab(), "label_ref": lab(), "image": torch.zeros(2, 3, 16, 16), "ref": torch.zeros(2, 3, 16, 16),
            "self_ref": torch.zeros(2)}


@needs_reference
def test_install_into_reference_attaches_records_in_label_modes_only():
    from cocosnet_amd import labels
    networks = rh.load_reference()
    p2p = importlib.import_module("models.pix2pix_model")
    original = p2p.Pix2PixModel.preprocess_input
    replaced = labels.install_into_reference(networks)
    try:
        assert p2p.Pix2PixModel.preprocess_input is not original and replaced["preprocess_input"] is original
        data = _data(151)
        label, sem, _, _, _, label_ref, ref_sem = _bare_model("ade20k", 151).preprocess_input(data)
        assert torch.equal(sem, torch.zeros(2, 151, 16, 16).scatter_(1, data["label"], 1.0))
        for t, lab in ((sem, data["label"]), (ref_sem, data["label_ref"])):
            rec = labels.record_of(t)
            assert rec is not None and rec.nc == 151 and torch.equal(rec.index.long(), lab[:, 0])
        # celebahq: even channels are the labels, odd ones the glasses mask written INTO the one-hot tensor afterwards
        data = _data(16, channels=2, seed=1)
        data["label"][:, 0].clamp_(max=12)
        data["label_ref"][:, 0].clamp_(max=12)
        data["label"][:, 1].clamp_(max=1)
        data["label_ref"][:, 1].clamp_(max=1)
        out = _bare_model("celebahq", 19).preprocess_input(data)
        assert out[1].shape == (2, 19, 16, 16) and labels.record_of(out[1]) is None and labels.record_of(out[6]) is None
    finally:
        labels.restore_reference(networks, replaced)
    assert p2p.Pix2PixModel.preprocess_input is original
