"""Write tests/golden/loss_block_<case>.npz: the reference's OWN Pix2PixModel.compute_generator_loss / compute_discriminator_loss
(models/pix2pix_model.py:205-296) run on the CPU as unbound functions on the stub `self` of tests/loss_case.py (canned generate_fake,
discriminate and vggnet_fix, the reference's GANLoss and nn.L1Loss, a contextual loss of zero) — the loss dictionaries, the gradient
of their sum with respect to every canned network output, the small inputs and a checksum of the large ones (they are a function
of the case's seed).  Needs the reference checkout (oracle.ref_harness).  `--out DIR` writes elsewhere (tests/test_losses_cpu.py
regenerates into a temporary directory and compares)."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import loss_case  # noqa: E402
from oracle.ref_harness import load_reference  # noqa: E402


def golden_arrays(name):
    networks = load_reference()
    p2p = importlib.import_module("models.pix2pix_model")
    inputs = loss_case.require_grad(loss_case.make_inputs(name))
    model = loss_case.StubModel(loss_case.options(name), inputs, networks.GANLoss, torch.nn.L1Loss)
    G, _ = loss_case.run_generator(p2p.Pix2PixModel.compute_generator_loss, model)
    loss_case.total(G).backward()
    arrays = {"G." + k: v.detach().numpy() for k, v in G.items()}
    arrays.update({"dG." + k: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for k, t in loss_case.leaves(inputs)})
    loss_case.require_grad(inputs)
    D = loss_case.run_discriminator(p2p.Pix2PixModel.compute_discriminator_loss, model)
    pf = [d[-1] for d in inputs["pred_fake"]]
    # compute_discriminator_loss reads only the last entry of each discriminator's list; pred_real is canned without a gradient
    grads = torch.autograd.grad(loss_case.total(D), pf, allow_unused=True)
    arrays.update({"D." + k: v.detach().numpy() for k, v in D.items()})
    arrays.update({f"dD.pred_fake_last.{i}": (g if g is not None else torch.zeros_like(t)).numpy() for i, (g, t) in enumerate(zip(grads, pf))})
    arrays["label"] = inputs["label"].numpy().astype(np.int16)
    arrays["ref_label"] = inputs["ref_label"].numpy().astype(np.int16)
    arrays["self_ref"] = inputs["self_ref"].numpy()
    arrays["checksum"] = np.array([float(t.detach().double().sum()) for _, t in loss_case.leaves(inputs)])
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    for name in sorted(loss_case.CASES):
        path = os.path.join(args.out, f"loss_block_{name}.npz")
        np.savez_compressed(path, **golden_arrays(name))
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
