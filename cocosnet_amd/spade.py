"""SPADE on the fused HIP kernel, for our own producers AND for the unmodified reference's translation generator.

SURVEY.md §8(f) rank 1: `PositionalNorm2d` (normalization.py:63-68) -> `SPADE.forward`'s modulation
`normalized * (1 + gamma) + beta` (:148-151) -> the `LeakyReLU(0.2)` that `SPADEResnetBlock.forward` applies right
after (architecture.py:88-95, `actvn` :107-108) are one HBM pass in K9 (`ops.pono_spade`, pono_spade.hip) instead of
~9 framework launches and their autograd.  `SPADEGenerator` (generator.py:35-45) uses 7 such blocks, each
`AdaptiveFeatureGenerator` 3 (:123-127).

`install_spade_into_reference(networks)` rebinds the two `forward` methods of the reference's own classes, so every
SPADE of an already-written training script (netG and netCorr alike) takes the fused path on the GPU; parameters,
sub-modules and `state_dict` are untouched (checkpoints load unchanged).  CPU tensors, non-fp32 tensors, the
`similarity_map` argument and norms of other classes keep the reference's arithmetic (their statistics are computed by
their own modules, only the modulation + activation are fused).  Without `--PONO`, nn.BatchNorm2d, nn.InstanceNorm2d and
dist.SyncBatchNorm2d (all parameter-free) are fused with the modulation and the activation in K26 (`ops.norm_spade`).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

LEAKY_SLOPE = 2e-1      # SPADEResnetBlock.actvn (architecture.py:107-108)
#: non-PONO SPADE: batch / sync-batch / instance norm + modulation + activation as ONE fused operator (K26, ops.norm_spade) instead
#: of the norm module followed by K17.  Test / A-B hook (tools/norm_spade_bench.py): plain module attribute, read at call time.
NORM_FUSED = True


def _hip_ok(*ts) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 for t in ts)


def _device_fp32(*ts) -> bool:
    """The tensors themselves (not the `_hip_ok` dispatch hook) are CUDA fp32: K26 also reads and updates the module's running
    buffers in place, so they have to live on the device next to x."""
    return all(t.is_cuda and t.dtype == torch.float32 for t in ts)


def _norm_spade_kind(m):
    """The kind of ops.norm_spade that computes exactly what the parameter-free norm module `m` does, or None.  Exact classes
    only: a subclass (or the reference's own SynchronizedBatchNorm2d) may do anything, so it keeps its own forward."""
    from .dist import SyncBatchNorm2d
    t = type(m)
    if t is nn.BatchNorm2d and not m.affine:
        return "batch"
    if t is nn.InstanceNorm2d and not m.affine and not m.track_running_stats:
        return "instance"
    if t is SyncBatchNorm2d and not m.affine:
        return "syncbatch"
    return None


def modulate(x, gamma, beta, pono: bool, param_free_norm=None, slope: float = 1.0):
    """leaky_relu(norm(x) * (1 + gamma) + beta, slope): the tail of SPADE.forward (+ the block's activation).
    pono: PositionalNorm2d — fused with the modulation and the activation in K9 when x is CUDA fp32.  Otherwise a batch /
    sync-batch / instance norm module of the exact classes of _norm_spade_kind is fused the same way (K26, reading and updating
    the module's running buffers); any other norm stays the module's own and the modulation + activation are K17."""
    fusible = _hip_ok(x, gamma, beta) and gamma.shape == x.shape and beta.shape == x.shape
    if pono and fusible:
        return ops.pono_spade(x, gamma, beta, slope)
    if not pono and NORM_FUSED and fusible and x.dim() == 4:
        kind = _norm_spade_kind(param_free_norm)
        m = param_free_norm
        if kind is not None and _device_fp32(x, gamma, beta, *(b for b in (m.running_mean, m.running_var) if b is not None)):
            return ops.norm_spade(x, gamma, beta, kind, m.running_mean, m.running_var, m.num_batches_tracked, m.training, m.momentum,
                                  m.eps, slope, getattr(m, "group", None))
    if pono:
        mu = x.mean(dim=1, keepdim=True)                              # normalization.py:63-68
        normalized = (x - mu) / x.var(dim=1, keepdim=True).add(1e-5).sqrt()
    else:
        normalized = param_free_norm(x)                               # instance | batch | sync-batch (normalization.py:93-101)
        if _hip_ok(normalized, gamma, beta) and gamma.shape == normalized.shape and beta.shape == normalized.shape:
            return ops.spade_modulate(normalized, gamma, beta, slope)  # K17: modulation + activation in one pass
    y = normalized * (1 + gamma) + beta                               # normalization.py:148
    return y if slope == 1.0 else F.leaky_relu(y, slope)


def label_plan(self, x, segmap):
    """(record, s) when this SPADE's `mlp_shared(resize(segmap))` can run on the label route (K35, ops.label_conv3x3), else None:
    segmap carries a fresh label record (labels.record_of), its grid is a whole multiple s of x's, x is CUDA fp32 and mlp_shared is
    Sequential(ReflectionPad2d(1), producers.Conv2d 3x3, ReLU) of a shape ops.label_conv_ok takes.  Every other mlp_shared (the
    reference's own nn.Conv2d, a 5x5 SPADE, pad_type "zero" variants) runs as it always did."""
    from . import labels, producers
    rec = labels.record_of(segmap)
    if rec is None or not _hip_ok(x) or x.dim() != 4 or producers.conv_backend() not in producers._HIP_BACKENDS:
        return None
    m = getattr(self, "mlp_shared", None)
    if not (isinstance(m, nn.Sequential) and len(m) == 3 and isinstance(m[0], nn.ReflectionPad2d) and tuple(m[0].padding) == (1, 1, 1, 1)
            and isinstance(m[1], producers.Conv2d) and type(m[2]) is nn.ReLU):
        return None
    conv = m[1]
    s = labels.whole_ratio(rec, x.shape[2:])
    if (s < 1 or conv.groups != 1 or conv.padding_mode != "zeros" or rec.index.device != x.device
            or not ops.label_conv_ok(conv.weight, rec.index, s, 1, conv.stride, conv.padding, conv.dilation, rec.nc)):
        return None
    return rec, s


def keeps_label_grid(x, segmap) -> bool:
    """A SPADEResnetBlock does NOT resize a label map that carries a fresh record whose grid is a whole multiple of x's: its SPADEs
    sample the index map themselves (a SPADE that cannot resizes the tensor itself, as the reference does)."""
    from . import labels
    rec = labels.record_of(segmap)
    return rec is not None and _hip_ok(x) and x.dim() == 4 and labels.whole_ratio(rec, x.shape[2:]) >= 1


def shared_activation(self, segmap, labels=None, sample: int = 1):
    """`self.mlp_shared(segmap)` (normalization.py:139): conv + ReLU of the label map.  Its own function so that a caller can put
    another evaluation of the same piecewise-linear map in its place.  `labels`, `sample`: what label_plan found — the reflect-padded
    3x3 convolution + ReLU of the map sampled at every `sample`-th pixel, from the record's index map (segmap itself is not read)."""
    if labels is not None:
        return self.mlp_shared[1](segmap, reflect=1, labels=labels, sample=sample, relu=True)
    return self.mlp_shared(segmap)


def spade_forward(self, x, segmap, similarity_map=None, slope: float = 1.0):
    """Drop-in for `SPADE.forward(x, segmap, similarity_map=None)` (normalization.py:129-151); works on the reference's
    module instances (attributes param_free_norm, mlp_shared, pad, mlp_gamma, mlp_beta, pad_type).  `slope`: negative
    slope of the LeakyReLU the caller would apply next (1.0 = none)."""
    plan = label_plan(self, x, segmap)
    if plan is not None:                     # K35 on the record's index map: no resize, the one-hot tensor is not read
        actv = shared_activation(self, segmap, labels=plan[0], sample=plan[1])
    else:
        if segmap.shape[2:] != x.shape[2:]:      # (spade_resnet_block_forward resizes once for the block's two or three SPADEs)
            segmap = F.interpolate(segmap, size=x.size()[2:], mode="nearest")
        actv = shared_activation(self, segmap)
    if getattr(self, "pad_type", "nozero") != "zero":
        actv = self.pad(actv)
    gamma, beta = self.mlp_gamma(actv), self.mlp_beta(actv)
    if similarity_map is not None:
        similarity_map = F.interpolate(similarity_map, size=gamma.size()[2:], mode="nearest")
        gamma, beta = gamma * similarity_map, beta * similarity_map
    pnorm = getattr(self, "param_free_norm", None)
    pono = getattr(self, "pono", None)
    if pono is None:       # the reference stores the function itself
        pono = callable(pnorm) and getattr(pnorm, "__name__", "") == "PositionalNorm2d"
    return modulate(x, gamma, beta, bool(pono), pnorm, slope)


def spade_resnet_block_forward(self, x, seg1):
    """Drop-in for `SPADEResnetBlock.forward` (architecture.py:70-95): same sub-module calls in the same order, with
    the two `actvn(norm_k(...))` pairs as one fused call each."""
    # the reference resizes the label map inside every SPADE (normalization.py:133): the block's SPADEs all see x's grid (its
    # convolutions keep the size), so ONE nearest resize serves them — and the convolutions that read it find its max|.| from the
    # first one (per module step: 24 resize kernels and as many max|.| passes less)
    if seg1.shape[2:] != x.shape[2:] and not keeps_label_grid(x, seg1):      # (a recorded label map: its SPADEs sample the index map)
        seg1 = F.interpolate(seg1, size=x.size()[2:], mode="nearest")
    x_s = self.conv_s(self.norm_s(x, seg1)) if self.learned_shortcut else x            # :97-102
    pad = self.pad if getattr(self, "pad_type", "nozero") != "zero" else (lambda t: t)
    dx = self.conv_0(pad(self.norm_0(x, seg1, slope=LEAKY_SLOPE)))
    dx = self.conv_1(pad(self.norm_1(dx, seg1, slope=LEAKY_SLOPE)))
    if self.use_se:
        dx = self.se_layar(dx)
    return x_s + dx


def install_spade_into_reference(networks_module):
    """Rebind `SPADE.forward` and `SPADEResnetBlock.forward` of the reference (`models.networks.normalization` /
    `.architecture`) to the fused versions above.  Returns the two patched classes; `uninstall` restores them."""
    import importlib
    norm = importlib.import_module(networks_module.__name__ + ".normalization")
    arch = importlib.import_module(networks_module.__name__ + ".architecture")
    for cls, fn in ((norm.SPADE, spade_forward), (arch.SPADEResnetBlock, spade_resnet_block_forward)):
        if not hasattr(cls, "_cocos_reference_forward"):
            cls._cocos_reference_forward = cls.forward
        cls.forward = fn
    return norm.SPADE, arch.SPADEResnetBlock


def uninstall_spade_from_reference(networks_module):
    import importlib
    norm = importlib.import_module(networks_module.__name__ + ".normalization")
    arch = importlib.import_module(networks_module.__name__ + ".architecture")
    for cls in (norm.SPADE, arch.SPADEResnetBlock):
        if hasattr(cls, "_cocos_reference_forward"):
            cls.forward = cls._cocos_reference_forward
            del cls._cocos_reference_forward
