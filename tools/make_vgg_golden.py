"""Write tests/golden/vgg19_nc0.npz and vgg19_nc1.npz: the reference's VGG19_feature_color_torchversion (correspondence.py:79-146) run
on the CPU with the seeded weights of tests/vgg_case.py — the outputs r22 r32 r42 r52 p5 of a B = 1, 40 x 40 image and the gradient of
vgg_case.loss with respect to the image, for vgg_normal_correct off and on.  Needs the reference checkout (oracle.ref_harness)."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import vgg_case  # noqa: E402
from oracle.ref_harness import load_reference  # noqa: E402


def main():
    networks = load_reference()
    torch.manual_seed(0)
    for nc in (False, True):
        net = networks.correspondence.VGG19_feature_color_torchversion(vgg_normal_correct=nc)
        net.load_state_dict(vgg_case.state_dict(), strict=True)
        x = vgg_case.input_image(nc).requires_grad_(True)
        outs = net(x, list(vgg_case.GOLDEN_KEYS), preprocess=True)
        vgg_case.loss(outs).backward()
        arrays = {"x": x.detach().numpy(), "dx": x.grad.numpy()}
        arrays.update({k: o.detach().numpy() for k, o in zip(vgg_case.GOLDEN_KEYS, outs)})
        path = os.path.join(REPO, "tests", "golden", f"vgg19_nc{int(nc)}.npz")
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
