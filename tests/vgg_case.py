"""The VGG19 golden case (tests/golden/vgg19_nc*.npz, written by tools/make_vgg_golden.py from the reference on the CPU): seeded
weights and the loss whose input gradient the files hold.  The weights are a function of a seed, so a machine without the
reference rebuilds them; the input is stored in the file."""
from __future__ import annotations

import torch

#: (name, in channels, out channels) of the sixteen 3x3 convolutions of VGG19_feature_color_torchversion
LAYERS = [("conv1_1", 3, 64), ("conv1_2", 64, 64), ("conv2_1", 64, 128), ("conv2_2", 128, 128),
          ("conv3_1", 128, 256), ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("conv3_4", 256, 256),
          ("conv4_1", 256, 512), ("conv4_2", 512, 512), ("conv4_3", 512, 512), ("conv4_4", 512, 512),
          ("conv5_1", 512, 512), ("conv5_2", 512, 512), ("conv5_3", 512, 512), ("conv5_4", 512, 512)]
#: the outputs the golden files hold, and the weight of each in the L1 loss
GOLDEN_KEYS = ("r22", "r32", "r42", "r52", "p5")
LOSS_WEIGHTS = (1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0, 1.0)
SIZE = 40          # B = 1, 40 x 40: the pooled sizes go 20, 10, 5, 2, 1 (odd sizes and W % 4 != 0 on the way)
SEED = 27


def state_dict(ic: int = 3, seed: int = SEED) -> dict:
    """He-scaled normal weights (so activations stay O(preprocessed input) through 16 layers) and small biases, fp32, CPU."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cin, cout in LAYERS:
        cin = ic if name == "conv1_1" else cin
        sd[name + ".weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd[name + ".bias"] = torch.randn(cout, generator=g) * 0.05
    return sd


def input_image(normal_correct: bool, seed: int = SEED) -> torch.Tensor:
    """[1, 3, SIZE, SIZE] in [0, 1] (in [-1, 1] with normal_correct)"""
    g = torch.Generator().manual_seed(seed + 1 + int(normal_correct))
    x = torch.rand(1, 3, SIZE, SIZE, generator=g)
    return x * 2 - 1 if normal_correct else x


def loss(outs) -> torch.Tensor:
    """A fixed weighted L1 of the golden keys' outputs."""
    return sum(w * o.abs().mean() for w, o in zip(LOSS_WEIGHTS, outs))
