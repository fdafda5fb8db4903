"""The VGG19 drop-in (cocosnet_amd.vgg) without a GPU: state_dict and CPU forward against the reference's own class, key handling,
the layers a shallow key skips, the install hook, the golden files, and K27's argument checks (made before any HIP call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle.ref_harness import load_reference, reference_available

import vgg_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
needs_ref = pytest.mark.skipif(not reference_available(), reason="the reference checkout is not on this machine")
ALL_KEYS = ["r11", "r12", "p1", "r21", "r22", "p2", "r31", "r32", "r33", "r34", "p3",
            "r41", "r42", "r43", "r44", "p4", "r51", "r52", "r53", "r54", "p5"]


def _ref_class():
    return load_reference().correspondence.VGG19_feature_color_torchversion


def _pair(pool="max", nc=False, ic=3):
    from cocosnet_amd.vgg import VGG19_feature_color_torchversion
    ref = _ref_class()(pool=pool, vgg_normal_correct=nc, ic=ic)
    ours = VGG19_feature_color_torchversion(pool=pool, vgg_normal_correct=nc, ic=ic)
    ours.load_state_dict(ref.state_dict(), strict=True)
    return ref, ours


@needs_ref
@pytest.mark.parametrize("pool", ["max", "avg"])
@pytest.mark.parametrize("ic", [3, 1])
def test_state_dict_keys_and_shapes_equal_the_reference(pool, ic):
    ref, ours = _pair(pool, ic=ic)
    rs, os_ = ref.state_dict(), ours.state_dict()
    assert list(rs.keys()) == list(os_.keys())
    assert all(rs[k].shape == os_[k].shape for k in rs)
    assert [n for n, _ in ref.named_modules()] == [n for n, _ in ours.named_modules()]


@needs_ref
@pytest.mark.parametrize("pool", ["max", "avg"])
@pytest.mark.parametrize("nc", [False, True])
@pytest.mark.parametrize("preprocess", [True, False])
@pytest.mark.parametrize("size", [(32, 48), (40, 40)])
def test_cpu_forward_equals_the_reference_bitwise(pool, nc, preprocess, size):
    torch.manual_seed(1)
    ref, ours = _pair(pool, nc)
    x = torch.rand(2, 3, *size)
    if nc:
        x = x * 2 - 1
    want = ref(x, ALL_KEYS, preprocess=preprocess)
    got = ours(x, ALL_KEYS, preprocess=preprocess)
    for k, a, b in zip(ALL_KEYS, got, want):
        assert a.shape == b.shape and torch.equal(a, b), k
    # and each key on its own (the drop-in stops at the deepest requested key)
    for k in ("r12", "p1", "r22", "p3", "r52"):
        assert torch.equal(ours(x, [k], preprocess=preprocess)[0], want[ALL_KEYS.index(k)]), k


@needs_ref
def test_key_order_duplicates_and_unknown_keys_like_the_reference():
    ref, ours = _pair()
    x = torch.rand(1, 3, 32, 32)
    keys = ["r42", "r12", "r42", "p2", "r12"]
    got, want = ours(x, keys), ref(x, keys)
    assert len(got) == len(want) == 5
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert got[0] is got[2] and got[1] is got[4]
    for bad in (["r12", "r99"], ["conv1_1"], ["R12"]):
        with pytest.raises(KeyError) as e_ours:
            ours(x, bad)
        with pytest.raises(KeyError) as e_ref:
            ref(x, bad)
        assert e_ours.value.args == e_ref.value.args


def test_shallow_keys_skip_the_deeper_layers():
    from cocosnet_amd.vgg import VGG19_feature_color_torchversion
    net = VGG19_feature_color_torchversion()
    calls = {}
    for name, m in net.named_modules():
        if name.startswith(("conv", "pool")):
            m.register_forward_hook(lambda mod, i, o, name=name: calls.__setitem__(name, calls.get(name, 0) + 1))
    net(torch.rand(1, 3, 32, 32), ["r12", "r22", "r32", "r42", "r52"])
    assert calls.get("conv5_2") == 1 and calls.get("pool4") == 1
    assert "conv5_3" not in calls and "conv5_4" not in calls and "pool5" not in calls
    calls.clear()
    net(torch.rand(1, 3, 32, 32), ["r12"])
    assert set(calls) == {"conv1_1", "conv1_2"}


@needs_ref
def test_install_into_reference_and_strict_load():
    networks = load_reference()
    from cocosnet_amd.vgg import VGG19_feature_color_torchversion, install_vgg_into_reference
    old = networks.correspondence.VGG19_feature_color_torchversion
    ref = old(vgg_normal_correct=True)
    try:
        assert install_vgg_into_reference(networks) is VGG19_feature_color_torchversion
        net = networks.correspondence.VGG19_feature_color_torchversion(vgg_normal_correct=True)
        assert isinstance(net, VGG19_feature_color_torchversion) and net.vgg_normal_correct
        net.load_state_dict(ref.state_dict(), strict=True)
    finally:
        networks.correspondence.VGG19_feature_color_torchversion = old


@pytest.mark.parametrize("nc", [0, 1])
def test_cpu_module_reproduces_the_golden(nc):
    """The reference's outputs and input gradient (tools/make_vgg_golden.py) from the drop-in on the CPU: the same framework ops."""
    from cocosnet_amd.vgg import VGG19_feature_color_torchversion
    g = np.load(os.path.join(GOLDEN, f"vgg19_nc{nc}.npz"))
    net = VGG19_feature_color_torchversion(vgg_normal_correct=bool(nc))
    net.load_state_dict(vgg_case.state_dict(), strict=True)
    x = torch.from_numpy(g["x"]).requires_grad_(True)
    assert torch.equal(x.detach(), vgg_case.input_image(bool(nc)))
    outs = net(x, list(vgg_case.GOLDEN_KEYS))
    vgg_case.loss(outs).backward()
    for k, o in zip(vgg_case.GOLDEN_KEYS, outs):
        r = g[k]
        assert np.abs(o.detach().numpy() - r).max() <= 1e-5 * np.abs(r).max(), k
    assert np.abs(x.grad.numpy() - g["dx"]).max() <= 1e-5 * np.abs(g["dx"]).max()


def test_golden_files_are_small():
    assert sum(os.path.getsize(os.path.join(GOLDEN, f"vgg19_nc{nc}.npz")) for nc in (0, 1)) < 1 << 20


# ---- K27 argument checks (no HIP call is made) ---------------------------------------------------------------------------------
one = ctypes.c_void_p(16)
two = ctypes.c_void_p(32)


def test_k27_rejects_null_and_aliased_pointers(hip_lib):
    assert hip_lib.cocos_vgg_preprocess_fwd(None, one, None, 1, 4, 4, 0, None) == -1
    assert hip_lib.cocos_vgg_preprocess_fwd(one, one, None, 1, 4, 4, 0, None) == -1
    assert hip_lib.cocos_vgg_preprocess_bwd(one, None, 1, 4, 4, 1, None) == -1
    assert hip_lib.cocos_relu_fwd(one, one, None, 16, None) == -1
    assert hip_lib.cocos_relu_bwd(one, two, one, None, 16, None) == -1
    assert hip_lib.cocos_relu_pool2_fwd(one, None, None, None, 1, 4, 4, 0, None) == -1
    assert hip_lib.cocos_relu_pool2_fwd(one, two, two, None, 1, 4, 4, 0, None) == -1
    assert hip_lib.cocos_relu_pool2_bwd(one, None, None, one, None, 1, 4, 4, 0, None) == -1
    assert b"null" in hip_lib.cocos_last_error_string()


def test_k27_rejects_bad_shapes(hip_lib):
    assert hip_lib.cocos_vgg_preprocess_fwd(one, two, None, 0, 4, 4, 0, None) == -1
    assert hip_lib.cocos_relu_fwd(one, two, None, -1, None) == -1
    assert hip_lib.cocos_relu_fwd(one, two, None, 0, None) == 0          # nothing to do
    assert hip_lib.cocos_relu_pool2_fwd(one, None, two, None, 1, 4, 4, 2, None) == -1      # mode 0 | 1
    assert hip_lib.cocos_relu_pool2_bwd(one, None, None, two, None, 0, 4, 4, 0, None) == -1
    # no 2x2 window: unsupported (the module then takes the framework's route, which raises its own error)
    assert hip_lib.cocos_relu_pool2_fwd(one, None, two, None, 1, 1, 4, 0, None) == -2
    assert hip_lib.cocos_relu_pool2_bwd(one, None, None, two, None, 1, 4, 1, 1, None) == -2
    assert b"2x2" in hip_lib.cocos_last_error_string()
