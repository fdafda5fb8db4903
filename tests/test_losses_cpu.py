"""The loss block (cocosnet_amd.losses) without a GPU: on the CPU the module runs the framework's op sequence, so its functions and
classes equal the reference's own bitwise; the install hook against the reference's real compute_generator_loss /
compute_discriminator_loss on a stub `self`; the golden files; K28's argument checks (made before any HIP call)."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.ref_harness import load_reference, reference_available

import loss_case
from cocosnet_amd import losses

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
needs_ref = pytest.mark.skipif(not reference_available(), reason="the reference checkout is not on this machine")
REL = 2.0 ** -22


def _ref():
    networks = load_reference()
    p2p = importlib.import_module("models.pix2pix_model")
    return networks, p2p, p2p.util


# ---- 1. functions and classes, bitwise ------------------------------------------------------------------------------------------
@needs_ref
def test_weighted_l1_and_mse_equal_the_reference_bitwise():
    _, _, util = _ref()
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(4, 6, 5, 7, generator=g), torch.randn(4, 6, 5, 7, generator=g)
    w = torch.rand(4, 1, 1, 1, generator=g)
    assert torch.equal(losses.weighted_l1_loss(a, b, w), util.weighted_l1_loss(a, b, w))
    assert torch.equal(losses.mse_loss(a, b), util.mse_loss(a, b))
    assert torch.equal(losses.mse_loss(a), util.mse_loss(a))
    assert torch.equal(losses.L1Loss()(a, b), torch.nn.L1Loss()(a, b))


@needs_ref
@pytest.mark.parametrize("gan_mode,for_discriminator,target_is_real", [
    (m, d, r) for m in ("hinge", "ls", "original", "w") for d in (True, False) for r in (True, False)
    if (m, d, r) != ("hinge", False, False)])          # (the reference asserts that the generator's hinge loss aims for real)
def test_ganloss_equals_the_reference_bitwise(gan_mode, for_discriminator, target_is_real):
    networks, _, _ = _ref()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 1, 7, 5, generator=g)
    nested = [[torch.randn(3, 4, 9, 9, generator=g), torch.randn(3, 1, 6, 6, generator=g)], [torch.randn(3, 1, 3, 3, generator=g)]]
    ref, ours = networks.GANLoss(gan_mode), losses.GANLoss(gan_mode)
    for inp in (x, nested, [x, x * 2]):
        want, got = ref(inp, target_is_real, for_discriminator), ours(inp, target_is_real, for_discriminator)
        assert got.shape == want.shape and torch.equal(got, want)


def test_ganloss_rejects_an_unknown_mode():
    with pytest.raises(ValueError):
        losses.GANLoss("softplus")


# ---- 2. the install hook against the reference's real methods --------------------------------------------------------------------
def _close(a, b, what):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, what
    err = (a - b).abs()
    assert bool((err <= REL * b.abs()).all()), (what, float(err.max()), float(b.abs().max()))


def _run_generator(p2p, networks, name, size, **over):
    inputs = loss_case.require_grad(loss_case.make_inputs(name, size=size))
    model = loss_case.StubModel(loss_case.options(name, **over), inputs, networks.GANLoss, torch.nn.L1Loss)
    G, out = loss_case.run_generator(p2p.Pix2PixModel.compute_generator_loss, model)
    loss_case.total(G).backward()
    return G, out, {k: (t.grad.clone() if t.grad is not None else None) for k, t in loss_case.leaves(inputs)}, model


CASES_2 = [("ade20k", (256, 256), {}), ("ade20k", None, {"which_perceptual": "5_2"}), ("ade20k_odd", None, {}), ("celebahq", None, {}),
           ("celebahq", None, {"which_perceptual": "4_2"}), ("no_ganfeat", None, {})]


@needs_ref
@pytest.mark.parametrize("name,size,over", CASES_2, ids=[f"{n}-{s}-{'-'.join(o.values())}" for n, s, o in CASES_2])
def test_installed_generator_loss_equals_the_reference_inline_code(name, size, over):
    networks, p2p, util = _ref()
    own = p2p.Pix2PixModel.compute_generator_loss
    want, _, want_g, _ = _run_generator(p2p, networks, name, size, **over)
    replaced = losses.install_losses_into_reference(networks)
    try:
        assert p2p.Pix2PixModel.compute_generator_loss is losses.compute_generator_loss and networks.GANLoss is losses.GANLoss
        assert util.weighted_l1_loss is losses.weighted_l1_loss and util.mse_loss is losses.mse_loss
        got, out, got_g, model = _run_generator(p2p, networks, name, size, **over)
    finally:
        losses.restore_reference_losses(networks, replaced)
    assert model.calls == ["generate_fake", "discriminate", "vggnet_fix"] and "fake_image" in out
    assert list(got) == list(want)
    if name.startswith("ade20k"):
        assert "mask" in want and float(want["mask"]) > 0
    if name == "celebahq":
        assert "G_warp_cycle" in want and "G_warp_self" in want
    assert ("GAN_Feat" in want) == (name != "no_ganfeat")
    for k in want:
        _close(got[k], want[k], k)
    for k in want_g:
        assert (got_g[k] is None) == (want_g[k] is None), k
        if want_g[k] is not None:
            _close(got_g[k], want_g[k], "d " + k)
    # put back: the reference's own method runs as before
    assert p2p.Pix2PixModel.compute_generator_loss is own and networks.GANLoss is replaced["GANLoss"]
    again, _, _, _ = _run_generator(p2p, networks, name, size, **over)
    assert all(torch.equal(again[k], want[k]) for k in want)


@needs_ref
@pytest.mark.parametrize("name", sorted(loss_case.CASES))
def test_installed_discriminator_loss_equals_the_reference(name):
    networks, p2p, _ = _ref()
    mk = lambda: loss_case.StubModel(loss_case.options(name), loss_case.require_grad(loss_case.make_inputs(name)), networks.GANLoss, torch.nn.L1Loss)
    want = loss_case.run_discriminator(p2p.Pix2PixModel.compute_discriminator_loss, mk())
    replaced = losses.install_losses_into_reference(networks)
    try:
        got = loss_case.run_discriminator(p2p.Pix2PixModel.compute_discriminator_loss, mk())
    finally:
        losses.restore_reference_losses(networks, replaced)
    assert list(got) == list(want) == ["D_Fake", "D_real"]
    for k in want:
        _close(got[k], want[k], k)


# ---- 3. the goldens ---------------------------------------------------------------------------------------------------------------
@needs_ref
def test_committed_goldens_equal_what_the_tool_writes_now(tmp_path):
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "make_loss_golden.py"), "--out", str(tmp_path)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for name in sorted(loss_case.CASES):
        new, old = np.load(tmp_path / f"loss_block_{name}.npz"), np.load(os.path.join(GOLDEN, f"loss_block_{name}.npz"))
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            assert np.array_equal(new[k], old[k]), (name, k)


@pytest.mark.parametrize("name", sorted(loss_case.CASES))
def test_cpu_module_reproduces_the_golden(name):
    """The reference's dictionaries and gradients from cocosnet_amd.losses on the CPU (no reference needed)."""
    g = np.load(os.path.join(GOLDEN, f"loss_block_{name}.npz"))
    inputs = loss_case.require_grad(loss_case.make_inputs(name))
    assert np.array_equal(inputs["label"].numpy(), g["label"]) and np.array_equal(inputs["ref_label"].numpy(), g["ref_label"])
    assert np.array_equal(np.array([float(t.detach().double().sum()) for _, t in loss_case.leaves(inputs)]), g["checksum"])
    model = loss_case.StubModel(loss_case.options(name), inputs, losses.GANLoss, losses.L1Loss)
    G, _ = loss_case.run_generator(losses.compute_generator_loss, model)
    loss_case.total(G).backward()
    assert ["G." + k for k in G] == [k for k in g.files if k.startswith("G.")]
    for k, v in G.items():
        _close(v, torch.from_numpy(g["G." + k]), k)
    for k, t in loss_case.leaves(inputs):
        got = t.grad if t.grad is not None else torch.zeros_like(t)
        _close(got, torch.from_numpy(g["dG." + k]), "d " + k)
    loss_case.require_grad(inputs)
    D = loss_case.run_discriminator(losses.compute_discriminator_loss, model)
    last = [d[-1] for d in inputs["pred_fake"]]
    grads = torch.autograd.grad(loss_case.total(D), last)
    for k, v in D.items():
        _close(v, torch.from_numpy(g["D." + k]), k)
    for i, gr in enumerate(grads):
        _close(gr, torch.from_numpy(g[f"dD.pred_fake_last.{i}"]), f"dD pred_fake_last {i}")


def test_golden_files_are_small():
    sizes = [os.path.getsize(os.path.join(GOLDEN, f"loss_block_{n}.npz")) for n in loss_case.CASES]
    assert max(sizes) < os.path.getsize(os.path.join(GOLDEN, "vgg19_nc0.npz")) / 2


# ---- no CPU fallback below the module; K28's argument checks (no HIP call is made) -----------------------------------------------
def test_ops_refuse_cpu_and_non_fp32_tensors():
    from cocosnet_amd import _lib, ops
    x = torch.zeros(2, 3)
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.pair_loss([(x, x, None, 1.0, 0.0)])
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.gan_loss([x], "hinge_d_real")
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.mask_nll_loss(torch.zeros(1, 2, 1, 1), torch.zeros(1, 1, 4, 4, dtype=torch.int64), torch.zeros(1, 1, 4, 4, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.pair_loss([(x, x, None, 1.0, 0.0)] * 17)
    with pytest.raises(ValueError):
        ops.gan_loss([x], "softplus")


one, two, three = ctypes.c_void_p(16), ctypes.c_void_p(32), ctypes.c_void_p(48)


def _tab(ctype, *vals):
    return (ctype * len(vals))(*vals)


def test_k28_rejects_bad_arguments(hip_lib):
    n1, c1 = _tab(ctypes.c_longlong, 8), _tab(ctypes.c_float, 1.0)
    a = _tab(ctypes.c_void_p, 16)
    assert hip_lib.cocos_pair_loss_fwd(0, a, None, None, n1, None, c1, c1, two, three, None) == -1
    assert hip_lib.cocos_pair_loss_fwd(17, a, None, None, n1, None, c1, c1, two, three, None) == -1
    assert hip_lib.cocos_pair_loss_fwd(1, _tab(ctypes.c_void_p, 0), None, None, n1, None, c1, c1, two, three, None) == -1
    assert hip_lib.cocos_pair_loss_fwd(1, a, None, None, _tab(ctypes.c_longlong, 0), None, c1, c1, two, three, None) == -1
    assert hip_lib.cocos_pair_loss_fwd(1, a, None, None, n1, _tab(ctypes.c_longlong, 3), c1, c1, two, three, None) == -1
    assert b"does not divide" in hip_lib.cocos_last_error_string()
    assert hip_lib.cocos_pair_loss_fwd(1, a, None, None, n1, None, c1, c1, None, three, None) == -1
    assert hip_lib.cocos_pair_loss_bwd(1, a, None, None, a, n1, None, c1, c1, two, None) == -1                 # da aliases a
    assert hip_lib.cocos_gan_loss_fwd(9, a, n1, 0, 0.0, two, three, None) == -1
    assert hip_lib.cocos_gan_loss_fwd(1, a, n1, 6, 0.0, two, three, None) == -1
    assert hip_lib.cocos_gan_loss_bwd(1, a, None, n1, 0, 0.0, two, None) == -1
    assert hip_lib.cocos_mask_nll_fwd(one, two, three, 0, 4, 8, 8, 8, 8, one, two, three, None) == -1
    assert hip_lib.cocos_mask_nll_fwd(one, two, three, 1, 257, 8, 8, 8, 8, one, two, three, None) == -2
    assert b"class set" in hip_lib.cocos_last_error_string()
    assert hip_lib.cocos_mask_nll_fwd(one, two, three, 1, 4, 3, 8, 8, 8, one, two, three, None) == -2
    assert hip_lib.cocos_mask_nll_fwd(one, two, three, 1, 4, 8, 8, 8, 3, one, two, three, None) == -2          # the reference map too
    assert hip_lib.cocos_mask_nll_fwd(None, two, three, 1, 4, 8, 8, 8, 8, one, two, three, None) == -1
    assert hip_lib.cocos_mask_nll_bwd(one, two, three, one, two, one, 1, 4, 8, 8, None) == -1                  # dp aliases p


def test_k28_planners(hip_lib):
    parts = hip_lib.cocos_loss_partials
    assert parts(1, _tab(ctypes.c_longlong, 1)) == 1
    assert parts(2, _tab(ctypes.c_longlong, 4096, 4097)) == 3
    assert parts(1, _tab(ctypes.c_longlong, 1 << 26)) == 1024          # the cap per segment
    assert parts(0, _tab(ctypes.c_longlong, 1)) == 0 and parts(17, _tab(ctypes.c_longlong, *([1] * 17))) == 0
    assert hip_lib.cocos_mask_nll_partials(8, 256, 256) == 8 * 4 and hip_lib.cocos_mask_nll_partials(1, 3, 8) == 0
