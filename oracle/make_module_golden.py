"""Record what the REFERENCE's own modules compute for seeded parameters (oracle.golden_cases.seeded_state_dict) ->
tests/golden/producers_<case>.npz (build container only; imports the reference read-only through oracle/ref_harness.py).

  producers_<case>.npz   theta / phi (the inputs of the hot path, correspondence.py:272 / :282) of the reference's
                         NoVGGCorrespondence in eval mode, for tests/test_module_cpu.py::test_producers_match_the_reference_code
  contextual_loss.npz    ContextualLoss_forward(opt)(X, Y, h=0.1) of the reference class (ContextualLoss.py:93-137), PONO and
                         non-PONO centring, for tests/test_module_cpu.py::test_contextual_loss_module_equals_the_reference_class_on_cpu

Run: python -m oracle.make_module_golden"""
import os

import numpy as np
import torch

from . import golden_cases as gc
from . import ref_harness as rh

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

#: name -> flags of the producer cases (tests/test_module_cpu.py::PRODUCER_CASES)
PRODUCER_CASES = {
    "ade_mk1": dict(semantic_nc=6, maskmix=True, PONO=True, PONO_C=True, match_kernel=1),
    "adaptor_k4": dict(semantic_nc=4, maskmix=False, PONO=True, PONO_C=True, adaptor_kernel=4, warp_bilinear=True),
    "all_options": dict(semantic_nc=5, maskmix=True, PONO=False, use_coordconv=True, adaptor_se=True,
                        adaptor_nonlocal=True, adaptor_res_deeper=True, dilation_conv=True, warp_stride=2),
}
PRODUCER_SEED = 3


def producer_inputs(nc, size=32):
    """The seeded CPU inputs of the producer cases: batch 2, one-hot label maps, the reference map is the batch flipped."""
    g = torch.Generator().manual_seed(0)
    img = torch.rand(2, 3, size, size, generator=g) * 2 - 1
    lab = torch.randint(0, nc, (2, 1, size, size), generator=g)
    seg = torch.zeros(2, nc, size, size).scatter_(1, lab, 1.0)
    return img, seg, seg.flip(0)


def contextual_inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(2, 16, 6, 5, generator=g), torch.randn(2, 16, 6, 5, generator=g) + 0.2


def main():
    for name, flags in PRODUCER_CASES.items():
        ref = rh.build_reference_corr(rh.make_opt(**flags), seed=PRODUCER_SEED).eval()
        ref.load_state_dict(gc.seeded_state_dict(ref.state_dict(), PRODUCER_SEED), strict=True)
        img, seg, ref_seg = producer_inputs(flags["semantic_nc"])
        got = {}
        hooks = [ref.theta.register_forward_hook(lambda m, i, o: got.__setitem__("theta", o.detach())),
                 ref.phi.register_forward_hook(lambda m, i, o: got.__setitem__("phi", o.detach()))]
        with torch.no_grad():
            ref(img, img, seg, ref_seg)
        for h in hooks:
            h.remove()
        path = os.path.join(GOLDEN, f"producers_{name}.npz")
        np.savez_compressed(path, **{k: v.numpy().astype(np.float32) for k, v in got.items()})
        print(path, {k: tuple(v.shape) for k, v in got.items()}, os.path.getsize(path) // 1024, "KiB")
    import importlib
    from types import SimpleNamespace
    rh.load_reference()
    ctx = importlib.import_module("models.networks.ContextualLoss")
    X, Y = contextual_inputs()
    with torch.no_grad():
        rec = {f"pono_{int(p)}": ctx.ContextualLoss_forward(SimpleNamespace(PONO=p))(X, Y, h=0.1).numpy() for p in (True, False)}
    np.savez(os.path.join(GOLDEN, "contextual_loss.npz"), **rec)
    print("contextual_loss.npz", {k: v.shape for k, v in rec.items()})


if __name__ == "__main__":
    main()
