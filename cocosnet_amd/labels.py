"""Label records: a one-hot segmentation map that remembers the integer map it was built from.

Every configuration that feeds a segmentation map hands the networks a one-hot fp32 tensor [B, nc, H, W] built by `scatter_` from an
integer map [B, 1, H, W] (pix2pix_model.py:177-187).  A 3x3 convolution of such a tensor is nine table look-ups per output pixel (K35,
ops.label_conv3x3) — if the layer knows the integer map.  This module is how it gets to know: `one_hot` (or `attach`) leaves a record on
the TENSOR OBJECT, `record_of` hands it to the layers that can use it (producers.Conv2d through AdaptiveFeatureGenerator.layer1 and
SPADE.mlp_shared), and every other reader keeps reading the tensor as the dense data it still is.

The record is a plain Python attribute, `seg._cocos_labels`, in the spirit of `module._cocos_frozen`.  It holds the index map, nc and
the signature (data_ptr, _version, shape) seen when it was attached; `record_of` returns None when the signature differs, so a stale
record is never read: an in-place write (`seg[:, -3:-2] = glasses`, `seg.add_(...)`) bumps `_version`.  Views, `clone()`, `cat`,
`seg + noise` and DataParallel's scatter give new tensor objects without the attribute: they miss and take the dense route, which is
always correct.  Nothing is attached unless the user calls this module.
"""
from __future__ import annotations

import importlib
import os

import torch

#: the label route as a whole: "0" makes `record_of` return None everywhere (A/B runs).  Module attribute, read at call time.
LABEL_CONV = os.environ.get("COCOS_LABEL_CONV", "1")

_ATTR = "_cocos_labels"


def enabled() -> bool:
    return LABEL_CONV not in ("0", 0, False, "", None)


class LabelRecord:
    """index: int32 [B, H, W] on the tensor's device (-1: a pixel without a class); nc; signature of the tensor at attach time"""
    __slots__ = ("index", "nc", "signature")

    def __init__(self, index, nc, signature):
        self.index, self.nc, self.signature = index, int(nc), signature


def _signature(seg):
    return (seg.data_ptr(), seg._version, tuple(seg.shape))


def _index_of(label_map, nc):
    lab = label_map[:, 0]
    return torch.where((lab >= 0) & (lab < nc), lab, torch.full_like(lab, -1)).to(torch.int32).contiguous()


def _check_label_map(label_map):
    if not torch.is_tensor(label_map) or label_map.dim() != 4 or label_map.shape[1] != 1 or label_map.dtype != torch.int64:
        raise ValueError("labels: an int64 label map [B, 1, H, W] is expected")


def one_hot(label_map, nc: int):
    """Drop-in for `torch.zeros(B, nc, H, W).scatter_(1, label_map, 1.0)` (fp32, on label_map's device) that also attaches the
    label record.  On the GPU one kernel (K35) writes the tensor and the index map; there a label outside [0, nc) gives an all-zero
    column (index -1).  On the host it is the framework's zeros + scatter_ (which raises on such a label)."""
    _check_label_map(label_map)
    nc = int(nc)
    if label_map.is_cuda:
        from . import ops
        seg, index = ops.labels_one_hot(label_map, nc)
    else:
        B, _, H, W = label_map.shape
        seg = torch.zeros(B, nc, H, W, dtype=torch.float32, device=label_map.device).scatter_(1, label_map, 1.0)
        index = _index_of(label_map, nc)
    setattr(seg, _ATTR, LabelRecord(index, nc, _signature(seg)))
    return seg


def attach(seg, label_map, verify: bool = False):
    """Attach a record to a one-hot tensor somebody else built from `label_map`.  The CALLER asserts that seg is
    zeros.scatter_(1, label_map, 1.0) (labels outside [0, nc): all-zero columns); verify=True checks it with framework ops and raises
    ValueError otherwise (tests).  Returns seg."""
    _check_label_map(label_map)
    if seg.dim() != 4 or seg.shape[0] != label_map.shape[0] or tuple(seg.shape[2:]) != tuple(label_map.shape[2:]):
        raise ValueError(f"labels.attach: seg {tuple(seg.shape)} does not belong to a label map {tuple(label_map.shape)}")
    nc = seg.shape[1]
    index = _index_of(label_map.to(seg.device), nc)
    if verify:
        want = (index[:, None] == torch.arange(nc, device=seg.device, dtype=torch.int32)[None, :, None, None]).to(seg.dtype)
        if not torch.equal(seg, want):
            raise ValueError("labels.attach: seg is not the one-hot tensor of label_map")
    setattr(seg, _ATTR, LabelRecord(index, nc, _signature(seg)))
    return seg


def record_of(seg):
    """The record of `seg` if it has one, LABEL_CONV is on and the tensor is what it was at attach time — else None."""
    if not torch.is_tensor(seg) or not enabled():
        return None
    rec = seg.__dict__.get(_ATTR) if hasattr(seg, "__dict__") else None
    if rec is None or rec.signature != _signature(seg):
        return None
    return rec


def whole_ratio(rec, size):
    """s if the record's grid is s x the grid `size` = (h, w) on both axes (s >= 1), else 0"""
    Hs, Ws = rec.index.shape[1:]
    h, w = int(size[0]), int(size[1])
    if h < 1 or w < 1 or Hs % h or Ws % w or Hs // h != Ws // w:
        return 0
    return Hs // h


# ---- the reference's facade -------------------------------------------------------------------------------------------------------
_NO_LABEL_MODES = ("celebahq", "celebahqedge", "deepfashion")


def _pix2pix_module(networks_module):
    return importlib.import_module(networks_module.__name__.rsplit(".", 1)[0] + ".pix2pix_model")


def install_into_reference(networks_module):
    """`Pix2PixModel.preprocess_input` -> a wrapper that, in the branch that builds the one-hot maps (pix2pix_model.py:177-187),
    attaches records to the returned `input_semantics` and `ref_semantics`.  Only for dataset modes other than celebahq (whose
    glasses channel is written INTO the one-hot tensor afterwards, :189-193), celebahqedge and deepfashion (no one-hot maps).
    Returns what it replaced, for `restore_reference`."""
    p2p = _pix2pix_module(networks_module)
    original = p2p.Pix2PixModel.preprocess_input

    def preprocess_input(self, data):
        out = original(self, data)
        if self.opt.dataset_mode not in _NO_LABEL_MODES:
            label, input_semantics, _, _, _, label_ref, ref_semantics = out
            attach(input_semantics, label)
            attach(ref_semantics, label_ref)
        return out

    preprocess_input.__wrapped__ = original
    p2p.Pix2PixModel.preprocess_input = preprocess_input
    return {"preprocess_input": original}


def restore_reference(networks_module, replaced):
    """Undo `install_into_reference` with the dictionary it returned."""
    _pix2pix_module(networks_module).Pix2PixModel.preprocess_input = replaced["preprocess_input"]
