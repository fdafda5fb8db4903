"""The loss block of `Pix2PixModel.compute_generator_loss` / `compute_discriminator_loss` on the K28 reduction kernels.

Boundary contract (reference models/pix2pix_model.py:205-296, util/util.py:36-43, models/networks/loss.py:15-97):
  * `weighted_l1_loss`, `mse_loss`, `L1Loss`, `GANLoss` — the reference's functions / classes, each usable on its own;
  * `generator_losses` / `discriminator_losses` — the loss dictionaries of :210-276 and :291-294 from the networks' outputs: the
    same keys under the same options, the same shapes (`GAN_Feat` stays a 1-element tensor), the same values;
  * `install_losses_into_reference(networks)` — puts all of it behind the reference's own names.

What differs is only how the numbers are formed.  The reference makes `sub`, `abs`, `expand * mul`, `mean` (and their autograd)
out of every pair of tensors, walks the discriminator's outputs with 4-5 tiny ops each, and builds the warp-mask weights in a
Python loop with `torch.unique` and one device-to-host read per label.  Here every GROUP is one launch (ops.pair_loss,
ops.gan_loss, ops.mask_nll_loss): `fm` + `perc` (the perceptual level is read once for both), `GAN_Feat`, the warp L1 terms, `GAN`,
`D_Fake`, `D_real`, `mask`.  fp64 sums, bitwise reproducible, no host synchronisation, nothing tensor-sized saved for the backward,
one gradient write per input.  `contextual` keeps calling `model.contextual_forward_loss` (K22 when installed).

Fallback: CPU tensors, non-fp32 tensors, targets or weights that need a gradient (the kernels give them none), groups wider than
a launch takes, `FUSED = False` and a kernel-side COCOS_ERR_UNSUPPORTED take the framework's ops in the reference's order; any other
kernel error raises.
"""
from __future__ import annotations

import importlib

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops

#: False: the whole block runs on the framework's ops — test / A-B hook (tools/loss_bench.py), plain module attribute read at call
#: time, in the style of vgg.FUSED
FUSED = True

_VGG_LEVEL_WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)
_VGG_KEYS = ["r12", "r22", "r32", "r42", "r52"]


def _gpu_f32(t) -> bool:
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32


def _pair_ok(a, b=None, w=None) -> bool:
    """a pair the kernels take: fp32 on the GPU, b of a's shape, one weight per sample, and neither b nor w wants a gradient"""
    if not (FUSED and _gpu_f32(a) and a.numel() > 0):
        return False
    if b is not None and not (_gpu_f32(b) and b.shape == a.shape and b.device == a.device and not b.requires_grad):
        return False
    if w is not None and not (_gpu_f32(w) and a.dim() >= 1 and w.numel() == a.shape[0] and w.device == a.device
                              and (w.dim() == 0 or w.shape[0] == a.shape[0]) and not w.requires_grad):
        return False
    return True


def _try(fused, framework):
    """fused(), or framework() when the kernel says COCOS_ERR_UNSUPPORTED"""
    try:
        return fused()
    except _lib.CocosHipError as e:
        if not e.unsupported:
            raise
    return framework()


# ---- the reference's functions and classes ----------------------------------------------------------------------------------------
def _weighted_l1_torch(input, target, weights):
    out = torch.abs(input - target)
    out = out * weights.expand_as(out)
    return out.mean()


def weighted_l1_loss(input, target, weights):
    """util.weighted_l1_loss (util/util.py:36-40): mean(|input - target| * weights), weights one per sample ([B, 1, 1, 1])."""
    if _pair_ok(input, target, weights):
        return _try(lambda: ops.pair_loss([(input, target, weights, 1.0, 0.0)])[0, 0], lambda: _weighted_l1_torch(input, target, weights))
    return _weighted_l1_torch(input, target, weights)


def mse_loss(input, target=0):
    """util.mse_loss (util/util.py:42-43): mean((input - target)^2), target a tensor or 0."""
    framework = lambda: torch.mean((input - target) ** 2)
    is_zero = not torch.is_tensor(target) and target == 0
    if (is_zero and _pair_ok(input)) or (torch.is_tensor(target) and _pair_ok(input, target)):
        return _try(lambda: ops.pair_loss([(input, None if is_zero else target, None, 0.0, 1.0)])[0, 1], framework)
    return framework()


class L1Loss(nn.Module):
    """torch.nn.L1Loss() with the default mean reduction (`criterionFeat`, pix2pix_model.py:48)."""

    reduction = "mean"

    def forward(self, input, target):
        if _pair_ok(input, target):
            return _try(lambda: ops.pair_loss([(input, target, None, 1.0, 0.0)])[0, 0], lambda: F.l1_loss(input, target))
        return F.l1_loss(input, target)


def _gan_case(gan_mode, real_label, fake_label, target_is_real, for_discriminator):
    """(kernel mode, constant label) of one GANLoss.loss call"""
    if gan_mode == "original":
        return "bce", real_label if target_is_real else fake_label
    if gan_mode == "ls":
        return "ls", real_label if target_is_real else fake_label
    if gan_mode == "hinge":
        if for_discriminator:
            return ("hinge_d_real" if target_is_real else "hinge_d_fake"), 0.0
        assert target_is_real, "The generator's hinge loss must be aiming for real"
        return "neg_mean", 0.0
    return ("neg_mean" if target_is_real else "mean"), 0.0          # wgan


def _gan_fused(gan_mode, real_label, fake_label, input, target_is_real, for_discriminator):
    """GANLoss.__call__ in one launch, or None when the input is not what the kernel takes"""
    if not FUSED or gan_mode not in ("original", "ls", "hinge", "w"):
        return None
    if isinstance(input, list):
        preds = [p[-1] if isinstance(p, list) else p for p in input]
    else:
        preds = [input]
    if not 1 <= len(preds) <= ops.GAN_LOSS_MAX_TENSORS or not all(_gpu_f32(p) and p.numel() > 0 for p in preds):
        return None
    mode, label = _gan_case(gan_mode, real_label, fake_label, target_is_real, for_discriminator)
    try:
        out = ops.gan_loss(preds, mode, label)
    except _lib.CocosHipError as e:
        if not e.unsupported:
            raise
        return None
    return out if isinstance(input, list) else out.reshape(())      # a list gives the reference's [1], a tensor its 0-dim mean


class GANLoss(nn.Module):
    """The reference's GANLoss (networks/loss.py:15-97): `gan_mode` in 'ls', 'original', 'w', 'hinge'; the input a prediction
    tensor or the multiscale discriminator's (nested) list."""

    def __init__(self, gan_mode, target_real_label=1.0, target_fake_label=0.0, tensor=torch.FloatTensor, opt=None):
        super().__init__()
        self.real_label = target_real_label
        self.fake_label = target_fake_label
        self.real_label_tensor = None
        self.fake_label_tensor = None
        self.zero_tensor = None
        self.Tensor = tensor
        self.gan_mode = gan_mode
        self.opt = opt
        if gan_mode not in ("ls", "original", "w", "hinge"):
            raise ValueError("Unexpected gan_mode {}".format(gan_mode))

    def get_target_tensor(self, input, target_is_real):
        name = "real_label_tensor" if target_is_real else "fake_label_tensor"
        if getattr(self, name) is None:
            t = self.Tensor(1).fill_(self.real_label if target_is_real else self.fake_label)
            t.requires_grad_(False)
            setattr(self, name, t)
        return getattr(self, name).expand_as(input)

    def get_zero_tensor(self, input):
        if self.zero_tensor is None:
            self.zero_tensor = self.Tensor(1).fill_(0)
            self.zero_tensor.requires_grad_(False)
        return self.zero_tensor.expand_as(input)

    def loss(self, input, target_is_real, for_discriminator=True):
        """one prediction tensor on the framework's ops (the fallback)"""
        if self.gan_mode == "original":
            return F.binary_cross_entropy_with_logits(input, self.get_target_tensor(input, target_is_real))
        if self.gan_mode == "ls":
            return F.mse_loss(input, self.get_target_tensor(input, target_is_real))
        if self.gan_mode == "hinge":
            if for_discriminator:
                arg = input - 1 if target_is_real else -input - 1
                return -torch.mean(torch.min(arg, self.get_zero_tensor(input)))
            assert target_is_real, "The generator's hinge loss must be aiming for real"
            return -torch.mean(input)
        return -input.mean() if target_is_real else input.mean()

    def __call__(self, input, target_is_real, for_discriminator=True):
        out = _gan_fused(self.gan_mode, self.real_label, self.fake_label, input, target_is_real, for_discriminator)
        if out is not None:
            return out
        if isinstance(input, list):
            loss = 0
            for pred_i in input:
                if isinstance(pred_i, list):
                    pred_i = pred_i[-1]
                loss_tensor = self.loss(pred_i, target_is_real, for_discriminator)
                bs = 1 if len(loss_tensor.size()) == 0 else loss_tensor.size(0)
                loss += torch.mean(loss_tensor.view(bs, -1), dim=1)
            return loss / len(input)
        return self.loss(input, target_is_real, for_discriminator)


def _criterion_gan(crit, input, target_is_real, for_discriminator):
    """`model.criterionGAN(...)`: fused for any criterion that carries GANLoss's three attributes, else the criterion's own call"""
    mode = getattr(crit, "gan_mode", None)
    if mode is not None and hasattr(crit, "real_label") and hasattr(crit, "fake_label"):
        out = _gan_fused(mode, crit.real_label, crit.fake_label, input, target_is_real, for_discriminator)
        if out is not None:
            return out
    return crit(input, target_is_real, for_discriminator=for_discriminator)


# ---- the loss dictionaries ------------------------------------------------------------------------------------------------------
def _sample_weights(self_ref):
    """self_ref[:, 0, 0, 0] / (sum + 1e-5) as [B, 1, 1, 1]; the sum runs over the samples in order from 0, as Python's sum() over the
    tensor does — on the device, no host read"""
    v = self_ref[:, 0, 0, 0]
    total = 0
    for i in range(v.shape[0]):
        total = total + v[i]
    return (v / (total + 1e-5)).unsqueeze(-1).unsqueeze(-1).unsqueeze(-1)


def _is_l1_mean(crit) -> bool:
    return isinstance(crit, (nn.L1Loss, L1Loss)) and getattr(crit, "reduction", "mean") == "mean"


def _warp_losses(G, opt, generate_out, real_image, ref_image, sample_weights):
    cycle, self_w = opt.warp_cycle_w > 0, opt.warp_self_w > 0
    if not (cycle or self_w):
        return
    pairs, segs = [], []          # pairs: (key, a, b, w, coefficient)
    if cycle:
        ref = ref_image if opt.warp_patch else F.avg_pool2d(ref_image, opt.warp_stride)
        pairs.append(("G_warp_cycle", generate_out["warp_cycle"], ref, None, opt.warp_cycle_w))
        if opt.two_cycle:
            pairs.append(("G_warp_cycle", generate_out["warp_i2r2i"], F.avg_pool2d(real_image, opt.warp_stride), None, opt.warp_cycle_w))
    if self_w:
        pairs.append(("G_warp_self", generate_out["warp_out"], real_image, sample_weights, opt.warp_self_w))

    def framework():
        for key, a, b, w, c in pairs:
            term = (F.l1_loss(a, b) if w is None else torch.mean(F.l1_loss(a, b, reduction="none") * w)) * c
            G[key] = G[key] + term if key in G else term

    def fused():
        out = ops.pair_loss([(a, b, w, c, 0.0) for _, a, b, w, c in pairs])
        for i, (key, *_) in enumerate(pairs):
            G[key] = G[key] + out[i, 0] if key in G else out[i, 0]

    if all(_pair_ok(a, b, w) for _, a, b, w, _ in pairs):
        _try(fused, framework)
    else:
        framework()


def _gan_feat_loss(model, opt, pred_fake, pred_real):
    num_D = len(pred_fake)
    pairs = [(pred_fake[i][j], pred_real[i][j].detach()) for i in range(num_D) for j in range(len(pred_fake[i]) - 1)]

    def framework():
        loss = model.FloatTensor(1).fill_(0)
        for a, b in pairs:
            loss += model.criterionFeat(a, b) * opt.lambda_feat / num_D
        return loss

    def fused():
        total = None
        for k in range(0, len(pairs), ops.PAIR_LOSS_MAX_SEGMENTS):
            chunk = pairs[k:k + ops.PAIR_LOSS_MAX_SEGMENTS]
            part = ops.pair_loss([(a, b, None, opt.lambda_feat / num_D, 0.0) for a, b in chunk])[len(chunk):, 0]
            total = part if total is None else total + part
        return total

    if pairs and _is_l1_mean(model.criterionFeat) and all(_pair_ok(a, b) for a, b in pairs):
        return _try(fused, framework)
    return framework()


def _vgg_losses(G, model, opt, fake_features, real_features, sample_weights):
    count = len(real_features)
    perc_layer = model.perceptual_layer

    def framework():
        loss = 0
        for i in range(count):
            loss += _VGG_LEVEL_WEIGHTS[i] * _weighted_l1_torch(fake_features[i], real_features[i].detach(), sample_weights)
        G["fm"] = loss * opt.lambda_vgg * opt.fm_ratio
        G["perc"] = torch.mean((fake_features[perc_layer] - real_features[perc_layer].detach()) ** 2) * opt.weight_perceptual

    def fused():
        p = perc_layer % count
        out = ops.pair_loss([(fake_features[i], real_features[i].detach(), sample_weights, _VGG_LEVEL_WEIGHTS[i], 1.0 if i == p else 0.0)
                             for i in range(count)])
        G["fm"] = out[count, 0] * opt.lambda_vgg * opt.fm_ratio
        G["perc"] = out[count, 1] * opt.weight_perceptual

    ok = (1 <= count <= len(_VGG_LEVEL_WEIGHTS) and -count <= perc_layer < count and len(fake_features) >= count
          and all(_pair_ok(fake_features[i], real_features[i].detach(), sample_weights) for i in range(count)))
    if ok:
        _try(fused, framework)
    else:
        framework()


def _mask_loss_torch(warp_mask, input_label, ref_label):
    """pix2pix_model.py:262-276 before `* weight_mask` on the framework's ops: a loop over the batch with a host read per label"""
    ref_small = F.interpolate(ref_label.float(), scale_factor=0.25, mode="nearest").long().squeeze(1)
    gt_small = F.interpolate(input_label.float(), scale_factor=0.25, mode="nearest").long().squeeze(1)
    weights = []
    for i in range(ref_small.shape[0]):
        in_ref = torch.unique(ref_small[i])
        weight = torch.ones_like(gt_small[i]).float()
        for label in torch.unique(gt_small[i]):
            if label not in in_ref:
                weight[gt_small[i] == label] = 0
        weight[gt_small[i] == 0] = 0          # no loss from the unknown class
        weights.append(weight.unsqueeze(0))
    weights = torch.cat(weights, dim=0)
    nll = F.nll_loss(torch.log(warp_mask + 1e-10), gt_small, reduction="none")
    return (nll * weights).sum() / (weights.sum() + 1e-5)


def _mask_loss(warp_mask, input_label, ref_label):
    def fused():
        gt = input_label if input_label.dtype == torch.int64 else input_label.long()
        ref = ref_label if ref_label.dtype == torch.int64 else ref_label.long()
        return ops.mask_nll_loss(warp_mask, gt, ref)

    ok = (FUSED and _gpu_f32(warp_mask) and warp_mask.dim() == 4 and all(
        torch.is_tensor(t) and t.is_cuda and t.dim() == 4 and t.shape[1] == 1 and t.shape[0] == warp_mask.shape[0]
        and not t.is_complex() for t in (input_label, ref_label))
        and tuple(warp_mask.shape[2:]) == (input_label.shape[2] // 4, input_label.shape[3] // 4))
    if ok:
        return _try(fused, lambda: _mask_loss_torch(warp_mask, input_label, ref_label))
    return _mask_loss_torch(warp_mask, input_label, ref_label)


def generator_losses(model, generate_out, pred_fake, pred_real, fake_features, input_label, ref_label, real_image, ref_image, self_ref):
    """The dictionary `compute_generator_loss` builds (pix2pix_model.py:210-276) from `generate_fake`'s output, the
    discriminator's predictions for the fake and the real image and the fixed VGG's features of the fake image.  `model` supplies
    `opt`, `criterionGAN`, `criterionFeat`, `perceptual_layer`, `get_ctx_loss` (and `FloatTensor` on the framework route)."""
    opt = model.opt
    G = {}
    if generate_out.get("loss_novgg_featpair") is not None:
        G["no_vgg_feat"] = generate_out["loss_novgg_featpair"]
    sample_weights = _sample_weights(self_ref)
    _warp_losses(G, opt, generate_out, real_image, ref_image, sample_weights)
    G["GAN"] = _criterion_gan(model.criterionGAN, pred_fake, True, False) * opt.weight_gan
    if not opt.no_ganFeat_loss:
        G["GAN_Feat"] = _gan_feat_loss(model, opt, pred_fake, pred_real)
    _vgg_losses(G, model, opt, fake_features, generate_out["real_features"], sample_weights)
    G["contextual"] = model.get_ctx_loss(fake_features, generate_out["ref_features"]) * opt.lambda_vgg * opt.ctx_w
    if opt.warp_mask_losstype != "none":
        G["mask"] = _mask_loss(generate_out["warp_mask"], input_label, ref_label) * opt.weight_mask
    return G


def discriminator_losses(model, pred_fake, pred_real):
    """The dictionary of `compute_discriminator_loss` (pix2pix_model.py:291-294) from the discriminator's two prediction lists."""
    opt = model.opt
    return {"D_Fake": _criterion_gan(model.criterionGAN, pred_fake, False, True) * opt.weight_gan,
            "D_real": _criterion_gan(model.criterionGAN, pred_real, True, True) * opt.weight_gan}


# ---- the reference's two methods, from their behaviour ---------------------------------------------------------------------------
def compute_generator_loss(self, input_label, input_semantics, real_image, ref_label=None, ref_semantics=None, ref_image=None, self_ref=None):
    generate_out = self.generate_fake(input_semantics, real_image, ref_semantics=ref_semantics, ref_image=ref_image, self_ref=self_ref)
    pred_fake, pred_real, *_ = self.discriminate(input_semantics, generate_out["fake_image"], real_image)
    fake_features = self.vggnet_fix(generate_out["fake_image"], list(_VGG_KEYS), preprocess=True)
    G = generator_losses(self, generate_out, pred_fake, pred_real, fake_features, input_label, ref_label, real_image, ref_image, self_ref)
    return G, generate_out


def compute_discriminator_loss(self, input_semantics, real_image, GforD, label=None):
    with torch.no_grad():
        fake_image = GforD["fake_image"].detach()
        fake_image.requires_grad_()
    pred_fake, pred_real, *_ = self.discriminate(input_semantics, fake_image, real_image)
    return discriminator_losses(self, pred_fake, pred_real)


def _reference_modules(networks_module):
    p2p = importlib.import_module(networks_module.__name__.rsplit(".", 1)[0] + ".pix2pix_model")
    return p2p, p2p.util


def install_losses_into_reference(networks_module):
    """`util.weighted_l1_loss`, `util.mse_loss`, `networks.GANLoss`, `Pix2PixModel.compute_generator_loss` and
    `.compute_discriminator_loss` -> this module's.  Returns what it replaced, for `restore_reference_losses`."""
    p2p, ref_util = _reference_modules(networks_module)
    replaced = {"weighted_l1_loss": ref_util.weighted_l1_loss, "mse_loss": ref_util.mse_loss, "GANLoss": networks_module.GANLoss,
                "compute_generator_loss": p2p.Pix2PixModel.compute_generator_loss,
                "compute_discriminator_loss": p2p.Pix2PixModel.compute_discriminator_loss}
    ref_util.weighted_l1_loss = weighted_l1_loss
    ref_util.mse_loss = mse_loss
    networks_module.GANLoss = GANLoss
    p2p.Pix2PixModel.compute_generator_loss = compute_generator_loss
    p2p.Pix2PixModel.compute_discriminator_loss = compute_discriminator_loss
    return replaced


def restore_reference_losses(networks_module, replaced):
    """Undo `install_losses_into_reference` with the dictionary it returned."""
    p2p, ref_util = _reference_modules(networks_module)
    ref_util.weighted_l1_loss = replaced["weighted_l1_loss"]
    ref_util.mse_loss = replaced["mse_loss"]
    networks_module.GANLoss = replaced["GANLoss"]
    p2p.Pix2PixModel.compute_generator_loss = replaced["compute_generator_loss"]
    p2p.Pix2PixModel.compute_discriminator_loss = replaced["compute_discriminator_loss"]
