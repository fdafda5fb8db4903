"""The loss-block cases (tests/golden/loss_block_*.npz, written by tools/make_loss_golden.py from the reference's own
compute_generator_loss / compute_discriminator_loss on the CPU): seeded canned network outputs, the options of each case and the stub
`self` both the reference's methods and cocosnet_amd.losses run on.  Every input is a function of a seed (CPU generator), so a
machine without the reference rebuilds it; the golden files hold the small inputs, a checksum of the large ones, the loss
dictionaries and the gradients."""
from __future__ import annotations

import argparse

import torch

VGG_KEYS = ["r12", "r22", "r32", "r42", "r52"]

_BASE = dict(warp_cycle_w=0.0, warp_patch=False, warp_stride=4, two_cycle=False, warp_self_w=0.0, weight_gan=10.0,
             no_ganFeat_loss=False, lambda_feat=10.0, lambda_vgg=10.0, fm_ratio=0.1, weight_perceptual=0.001, ctx_w=1.0,
             warp_mask_losstype="none", weight_mask=100.0, use_22ctx=False, which_perceptual="5_2", gan_mode="hinge")

#: name -> (options, nc, label size (H, W), batch, self_ref)
CASES = {
    # README ADE20k flags: --warp_mask_losstype direct, 151 classes; sample 1 holds ground-truth classes its reference lacks, sample 2
    # is all class 0 (sum of weights 0 for it)
    "ade20k": (dict(_BASE, warp_mask_losstype="direct", which_perceptual="4_2", weight_perceptual=0.01), 151, (64, 64), 3, (0.0, 1.0, 0.0)),
    # a label map whose sides are not multiples of 4 (70 x 66 -> 17 x 16 at scale 0.25)
    "ade20k_odd": (dict(_BASE, warp_mask_losstype="direct", gan_mode="ls"), 151, (70, 66), 2, (1.0, 1.0)),
    # README CelebA-HQ flags: --warp_cycle_w 1 --two_cycle, warp_self_w > 0 with mixed self_ref
    "celebahq": (dict(_BASE, warp_cycle_w=1.0, two_cycle=True, warp_self_w=1000.0, gan_mode="hinge"), 19, (64, 64), 3, (1.0, 0.0, 1.0)),
    "no_ganfeat": (dict(_BASE, no_ganFeat_loss=True, warp_cycle_w=1.0, gan_mode="original"), 19, (64, 64), 2, (0.0, 0.0)),
}
#: the canned tensors the losses are differentiated with respect to
GRAD_KEYS = ("warp_out", "warp_mask", "warp_cycle", "warp_i2r2i", "fake_features", "pred_fake")


def options(name, **over):
    return argparse.Namespace(**dict(CASES[name][0], **over))


def make_inputs(name, size=None, seed=28):
    """dict of CPU tensors for case `name`; `size` overrides the label-map size (H, W).  Images are 4x the warp grid (warp_stride)."""
    _, nc, (H, W), B, self_ref = CASES[name]
    if size is not None:
        H, W = size
    g = torch.Generator().manual_seed(seed + sorted(CASES).index(name))
    h, w = H // 4, W // 4
    rnd = lambda *s: torch.randn(*s, generator=g)
    img = lambda hh, ww: torch.rand(B, 3, hh, ww, generator=g) * 2 - 1
    blocks = lambda: torch.randint(1, nc, (B, 1, (H + 7) // 8, (W + 7) // 8), generator=g).repeat_interleave(8, 2).repeat_interleave(8, 3)[:, :, :H, :W]
    label, ref_label = blocks().contiguous(), blocks().contiguous()
    label[0, :, : H // 2] = 0                          # a region of the unknown class
    if B > 1:
        ref_label[1] = ref_label[1].clamp(max=nc // 2)  # sample 1: the upper half of the classes never occurs in its reference
    if B > 2:
        label[2] = 0                                   # sample 2: every pixel class 0
    feat_shapes = [(8, 16, 16), (16, 8, 8), (16, 4, 4), (32, 2, 2), (32, 2, 2)]
    d_shapes = [[(4, 9, 9), (8, 5, 5), (16, 4, 4), (1, 3, 3)], [(4, 5, 5), (8, 3, 3), (16, 2, 2), (1, 1, 1)]]
    # integer-rounded halves: exact ties a == b (gradient exactly 0) in the feature-matching pairs
    ties = lambda t: (t * 2).round() / 2
    return {
        "label": label, "ref_label": ref_label, "self_ref": torch.tensor(self_ref).view(B, 1, 1, 1),
        "real_image": img(4 * h, 4 * w), "ref_image": img(4 * h, 4 * w), "fake_image": img(4 * h, 4 * w),
        "warp_out": img(4 * h, 4 * w), "warp_cycle": img(h, w), "warp_i2r2i": img(h, w),
        "warp_mask": torch.softmax(rnd(B, nc, h, w) * 3, dim=1),
        "real_features": [ties(rnd(B, *s)) for s in feat_shapes], "ref_features": [rnd(B, *s) for s in feat_shapes],
        "fake_features": [ties(rnd(B, *s)) for s in feat_shapes],
        "pred_fake": [[rnd(B, *s) for s in d] for d in d_shapes], "pred_real": [[rnd(B, *s) for s in d] for d in d_shapes],
    }


def to_device(inputs, device):
    mv = lambda v: v.to(device) if torch.is_tensor(v) else [mv(x) for x in v]
    return {k: mv(v) for k, v in inputs.items()}


def leaves(inputs):
    """flat list of (name, tensor) of the tensors named by GRAD_KEYS"""
    out = []
    for k in GRAD_KEYS:
        v = inputs[k]
        if torch.is_tensor(v):
            out.append((k, v))
        else:
            flat = [t for x in v for t in (x if isinstance(x, list) else [x])]
            out += [(f"{k}.{i}", t) for i, t in enumerate(flat)]
    return out


def require_grad(inputs):
    for _, t in leaves(inputs):
        t.requires_grad_(True)
        t.grad = None
    return inputs


class StubModel:
    """What the two loss methods read from `self`, with canned networks: generate_fake / discriminate / vggnet_fix return the
    case's tensors, the contextual loss is zero."""

    def __init__(self, opt, inputs, gan_loss_cls, l1_loss_cls, float_tensor=torch.FloatTensor):
        self.opt = opt
        self.inputs = inputs
        self.FloatTensor = float_tensor
        self.criterionGAN = gan_loss_cls(opt.gan_mode, tensor=float_tensor, opt=opt)
        self.criterionFeat = l1_loss_cls()
        self.perceptual_layer = -1 if opt.which_perceptual == "5_2" else -2
        self.calls = []

    def generate_fake(self, input_semantics, real_image, ref_semantics=None, ref_image=None, self_ref=None):
        self.calls.append("generate_fake")
        i = self.inputs
        out = {k: i[k] for k in ("fake_image", "warp_out", "warp_mask", "real_features", "ref_features")}
        if self.opt.warp_cycle_w > 0:
            out["warp_cycle"] = i["warp_cycle"]
            if self.opt.two_cycle:
                out["warp_i2r2i"] = i["warp_i2r2i"]
        return out

    def discriminate(self, input_semantics, fake_image, real_image):
        self.calls.append("discriminate")
        return self.inputs["pred_fake"], self.inputs["pred_real"], None, None, None

    def vggnet_fix(self, image, keys, preprocess=True):
        self.calls.append("vggnet_fix")
        assert list(keys) == VGG_KEYS and preprocess
        return self.inputs["fake_features"]

    def get_ctx_loss(self, source, target):
        return torch.zeros((), device=source[0].device)


def run_generator(method, model):
    """`method(self, input_label, input_semantics, real_image, ref_label, ref_semantics, ref_image, self_ref)` on the stub"""
    i = model.inputs
    return method(model, i["label"], None, i["real_image"], ref_label=i["ref_label"], ref_semantics=None, ref_image=i["ref_image"],
                  self_ref=i["self_ref"])


def run_discriminator(method, model):
    i = model.inputs
    return method(model, None, i["real_image"], {"fake_image": i["fake_image"]})


def total(losses):
    """the scalar the gradients are taken of: the sum of every entry"""
    return sum(v.sum() for v in losses.values())
