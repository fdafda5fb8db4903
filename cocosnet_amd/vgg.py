"""Drop-in `VGG19_feature_color_torchversion` — the fixed VGG19 that `Pix2PixModel` runs three times per generator step.

Boundary contract (reference models/networks/correspondence.py:79-146; built at pix2pix_model.py:29-35, called at :248, :306, :311):
  * constructor `VGG19_feature_color_torchversion(pool='max', vgg_normal_correct=False, ic=3)` with the same sub-module names, so
    the `state_dict` keys and shapes equal the reference's and `models/vgg19_conv.pth` loads with `strict=True`;
  * `forward(x, out_keys, preprocess=True)` returning `[out[k] for k in out_keys]` for the keys r11 ... r54, p1 ... p5; an unknown
    key raises KeyError, as the reference's dict lookup does.

What differs is only how it gets there:
  * only the layers up to the deepest requested key run: the r12 ... r52 calls of the generator step never compute conv5_3,
    conv5_4 and pool5;
  * the convolutions are `producers.Conv2d` (K16 for fp32 GPU tensors, the framework's otherwise), and the glue between them is
    K27 (`ops.vgg_preprocess`, `ops.relu`, `ops.relu_pool2`): bitwise the framework's fp32 results, every activation written
    once, the pools' arg-max recomputed in the backward (no int64 index tensor), and each activation's max|.| left for the
    convolution that splits it next (no separate max|.| pass);
  * a ReLU that feeds a pool is fused with it; its own output is written only when that rNN key was requested.

Fallback: CPU tensors, non-fp32 tensors, pool modules of another configuration and `FUSED = False` run the reference's own ops
(`F.relu`, `self.poolN`, the framework preprocess); a kernel-side COCOS_ERR_UNSUPPORTED (a feature map smaller than one 2x2 window)
takes the same route, any other kernel error raises.  The convolutions follow `producers.Conv2d`'s own rule.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .producers import Conv2d

#: False: the glue runs on the framework's ops (the convolutions still follow producers.Conv2d) — test / A-B hook
#: (tools/vgg_bench.py), plain module attribute read at call time, in the style of spade.NORM_FUSED
FUSED = True

#: every key of the reference's forward, in the order it computes them
KEYS = ("r11", "r12", "p1", "r21", "r22", "p2", "r31", "r32", "r33", "r34", "p3",
        "r41", "r42", "r43", "r44", "p4", "r51", "r52", "r53", "r54", "p5")

_VGG_MEAN_BGR = (0.40760392, 0.45795686, 0.48501961)


def vgg_preprocess_torch(x, vgg_normal_correct: bool = False):
    """util.vgg_preprocess (util/util.py:45-54) on the framework's ops (the fallback)."""
    if vgg_normal_correct:
        x = (x + 1) / 2
    bgr = torch.cat((x[:, 2:3, :, :], x[:, 1:2, :, :], x[:, 0:1, :, :]), dim=1)
    return (bgr - torch.Tensor(list(_VGG_MEAN_BGR)).type_as(bgr).view(1, 3, 1, 1)) * 255


class VGG19_feature_color_torchversion(nn.Module):
    """The reference's VGG19 feature extractor; input RGB in [0, 1] (in [-1, 1] with vgg_normal_correct)."""

    def __init__(self, pool="max", vgg_normal_correct=False, ic=3):
        super().__init__()
        self.vgg_normal_correct = vgg_normal_correct
        self.conv1_1 = Conv2d(ic, 64, kernel_size=3, padding=1)
        self.conv1_2 = Conv2d(64, 64, kernel_size=3, padding=1)
        self.conv2_1 = Conv2d(64, 128, kernel_size=3, padding=1)
        self.conv2_2 = Conv2d(128, 128, kernel_size=3, padding=1)
        self.conv3_1 = Conv2d(128, 256, kernel_size=3, padding=1)
        self.conv3_2 = Conv2d(256, 256, kernel_size=3, padding=1)
        self.conv3_3 = Conv2d(256, 256, kernel_size=3, padding=1)
        self.conv3_4 = Conv2d(256, 256, kernel_size=3, padding=1)
        self.conv4_1 = Conv2d(256, 512, kernel_size=3, padding=1)
        self.conv4_2 = Conv2d(512, 512, kernel_size=3, padding=1)
        self.conv4_3 = Conv2d(512, 512, kernel_size=3, padding=1)
        self.conv4_4 = Conv2d(512, 512, kernel_size=3, padding=1)
        self.conv5_1 = Conv2d(512, 512, kernel_size=3, padding=1)
        self.conv5_2 = Conv2d(512, 512, kernel_size=3, padding=1)
        self.conv5_3 = Conv2d(512, 512, kernel_size=3, padding=1)
        self.conv5_4 = Conv2d(512, 512, kernel_size=3, padding=1)
        pool_cls = {"max": nn.MaxPool2d, "avg": nn.AvgPool2d}.get(pool)
        if pool_cls is not None:          # (the reference leaves the pools out for any other value: forward then fails at pool1)
            for i in range(1, 6):
                setattr(self, f"pool{i}", pool_cls(kernel_size=2, stride=2))

    # ---- glue: K27 for fp32 GPU tensors, the reference's ops otherwise ------------------------------------------------------
    @staticmethod
    def _fused(t) -> bool:
        return FUSED and t.is_cuda and t.dtype == torch.float32

    def _preprocess(self, x):
        if self._fused(x) and x.dim() == 4 and x.shape[1] == 3:
            try:
                return ops.vgg_preprocess(x, bool(self.vgg_normal_correct))
            except _lib.CocosHipError as e:
                if not e.unsupported:
                    raise
        return vgg_preprocess_torch(x, self.vgg_normal_correct)

    def _relu(self, y):
        if self._fused(y):
            try:
                return ops.relu(y)
            except _lib.CocosHipError as e:
                if not e.unsupported:
                    raise
        return F.relu(y)

    @staticmethod
    def _pool_mode(pool):
        """"max" / "avg" for a pool module that computes exactly the 2x2 / stride-2 floor pool of the kernels, else None."""
        if type(pool) is nn.MaxPool2d:
            ok = (pool.kernel_size in (2, (2, 2)) and pool.stride in (2, (2, 2)) and pool.padding in (0, (0, 0))
                  and pool.dilation in (1, (1, 1)) and not pool.ceil_mode and not pool.return_indices)
            return "max" if ok else None
        if type(pool) is nn.AvgPool2d:
            ok = (pool.kernel_size in (2, (2, 2)) and pool.stride in (2, (2, 2)) and pool.padding in (0, (0, 0))
                  and not pool.ceil_mode and pool.divisor_override is None)
            return "avg" if ok else None
        return None

    def _relu_pool(self, y, pool, keep_r: bool):
        """(relu(y) if keep_r else None, pool(relu(y)))"""
        mode = self._pool_mode(pool)
        if mode is not None and self._fused(y) and y.dim() == 4:
            try:
                out = ops.relu_pool2(y, mode, keep_r)
                return out if keep_r else (None, out)
            except _lib.CocosHipError as e:
                if not e.unsupported:
                    raise
        r = F.relu(y)
        return (r if keep_r else None), pool(r)

    def forward(self, x, out_keys, preprocess=True):
        """NOTE: input tensor should range in [0,1] (the reference's note).  Runs only up to the deepest key of `out_keys`."""
        out_keys = list(out_keys)
        for k in out_keys:
            if k not in KEYS:
                raise KeyError(k)
        if not out_keys:
            return []
        want = set(out_keys)
        last = max(KEYS.index(k) for k in out_keys)
        if preprocess:
            x = self._preprocess(x)
        out = {}
        i = 0
        while i <= last:
            key = KEYS[i]                                   # rNM: conv N_M then ReLU
            y = getattr(self, f"conv{key[1]}_{key[2]}")(x)
            if i + 1 <= last and KEYS[i + 1][0] == "p":     # the ReLU feeds the pool: fused
                pkey = KEYS[i + 1]
                r, x = self._relu_pool(y, getattr(self, f"pool{pkey[1]}"), key in want)
                out[key], out[pkey] = r, x
                i += 2
            else:
                x = out[key] = self._relu(y)
                i += 1
        return [out[k] for k in out_keys]


def install_vgg_into_reference(networks_module):
    """`models.networks.correspondence.VGG19_feature_color_torchversion` -> this class (pix2pix_model.py:29 builds the generator
    step's VGG by that name).  Returns the class."""
    import importlib
    ref_corr = importlib.import_module(networks_module.__name__ + ".correspondence")
    ref_corr.VGG19_feature_color_torchversion = VGG19_feature_color_torchversion
    return VGG19_feature_color_torchversion
