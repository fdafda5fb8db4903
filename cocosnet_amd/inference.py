"""Frozen-weight inference: everything a layer derives from its WEIGHT is prepared once and reused.

A training forward re-derives, per layer and call, max|w|, the f16 hi/lo (or bf16) operand planes and — under spectral norm — W / sigma.
With weights that do not change between calls (the `test.py` commands; the fixed `vggnet_fix` of a training step) those launches produce
the same bytes every time.  `freeze(module)` attaches a `PreparedWeight` record to every layer it knows:

  * every `producers.Conv2d` (plain, under `producers.hip_spectral_norm` or under the framework's `spectral_norm`), the layers of
    `vgg.VGG19_feature_color_torchversion` among them;
  * the theta / phi projections of `correspondence.NoVGGCorrespondence`.

The record is a plain Python attribute (`module._cocos_frozen`): no parameter, no buffer, `state_dict()` untouched.  It holds the
effective weight (W / sigma by the `eval()` rule — no power iteration — for spectral layers), its max|w| cell and the planes of every
layout a forward route has asked for (K16 / K16c / K16b planes, K0's k-padded rows, K23 / K25's fragment order); a layout is made the
first time a route asks for it (freeze() itself makes the ones it can foresee, all layers in ONE launch: ops.weight_planes_multi, K32).
Input-gradient planes are kept only for the fixed VGG, whose backward towards the image runs inside a training step.

A record is USED only when FROZEN is set, the module is in eval() mode and no gradient can reach the layer's weight tensors
(`not torch.is_grad_enabled() or not any(p.requires_grad ...)`); every use first compares (data_ptr, _version) of weight /
weight_orig / weight_u / weight_v with what the record saw — `load_state_dict`, `optimizer.step()` or a manual edit make it prepare
again (`FrozenReport.repreparations`), a stale record is never read.  In every other case the call takes the unfrozen route unchanged.

    from cocosnet_amd import inference
    report = inference.freeze(model.net)        # or any nn.Module; inference.unfreeze(...) removes the records
    inference.FROZEN = False                    # A/B switch (env COCOS_FROZEN=0): ignore attached records
"""
from __future__ import annotations

import importlib
import os

import torch
import torch.nn as nn

#: False (env COCOS_FROZEN=0): attached records are ignored — every call takes the unfrozen route (A/B runs).  This only bypasses
#: records that freeze() attached explicitly; nothing is frozen by default.  Module attribute, read at call time.
FROZEN = os.environ.get("COCOS_FROZEN", "1") != "0"

_ATTR = "_cocos_frozen"


class FrozenReport:
    """What freeze() did, and what happened to the records since (`repreparations` counts up while the model is used)."""

    def __init__(self):
        self.layers = 0              # records attached
        self.spectral = 0            # ... of which under spectral norm (W / sigma folded)
        self.skipped = []            # qualified names of layers left alone (a spectral-norm hook of an unknown class)
        self.launches = 0            # kernel launches freeze() itself made (K21 per spectral layer + the K32 tables)
        self.repreparations = 0      # records found stale at use time and prepared again
        self.records = []            # the records, in module order

    def __repr__(self):
        return (f"FrozenReport(layers={self.layers}, spectral={self.spectral}, skipped={len(self.skipped)}, launches={self.launches}, "
                f"repreparations={self.repreparations})")


def _spectral_hook(module):
    """(hook, known) of a spectral norm on `weight`, or (None, False).  Known: the HIP hook, the framework's own class (freeze() re-classes
    it to producers._SpectralNormRecord, same arithmetic + the record lookup) or that class already."""
    from . import producers
    for hook in module._forward_pre_hooks.values():
        if isinstance(hook, producers._sn_mod.SpectralNorm) and hook.name == "weight":
            return hook, type(hook) in (producers._SpectralNormHIP, producers._SpectralNormRecord, producers._sn_mod.SpectralNorm)
    return None, False


class PreparedWeight:
    """The prepared-weight record of one layer.  `prepare(record)` fills `weight` and `amax` from the module's tensors (the default
    runs on the GPU; tests pass their own)."""

    def __init__(self, module, report=None, keep_dgrad=False, prepare=None, name=""):
        self.module = module
        self.report = report if report is not None else FrozenReport()
        self.keep_dgrad = bool(keep_dgrad)          # the input-gradient planes may be served from the record (the fixed VGG)
        self.name = name
        self.hook = _spectral_hook(module)[0]
        self._prepare = prepare if prepare is not None else _prepare_on_device
        self.weight = None                          # effective weight (detached): W, or W / sigma
        self.amax = None                            # its max|w| cell (1-element device tensor)
        self._layouts = {}                          # (layout, aux) -> (hi, lo, scale)
        self._sig = None                            # what sources() looked like when the record was prepared
        self.handed = False                         # the spectral hook validated the record for the call in progress

    # ---- what the record watches ---------------------------------------------------------------------------------------------
    def sources(self):
        """the tensors the effective weight is a function of"""
        m = self.module
        if self.hook is not None:
            return [getattr(m, "weight_orig"), getattr(m, "weight_u"), getattr(m, "weight_v")]
        return [m.weight]

    def params(self):
        """the layer's weight tensors a gradient could be wanted for"""
        return [self.sources()[0]]

    def signature(self):
        return tuple((t.data_ptr(), t._version) for t in self.sources())

    @property
    def prepared(self) -> bool:
        return self._sig is not None

    def stale(self) -> bool:
        """the tensors changed (or moved) since the record was prepared"""
        return self._sig is not None and self._sig != self.signature()

    def eligible(self) -> bool:
        """FROZEN, eval() mode, and no gradient can reach the weight tensors"""
        return (FROZEN and not self.module.training
                and (not torch.is_grad_enabled() or not any(p.requires_grad for p in self.params())))

    # ---- use -----------------------------------------------------------------------------------------------------------------
    def ensure(self):
        """prepare now if never prepared; prepare AGAIN (and count it) if stale"""
        sig = self.signature()
        if self._sig == sig:
            return self
        if self._sig is not None:
            self.report.repreparations += 1
        self._layouts = {}
        self.weight = self.amax = None
        self._prepare(self)
        self._sig = sig
        return self

    def use(self):
        """the record, fresh, if this call may use it — else None (the caller takes the unfrozen route)"""
        if not self.eligible():
            return None
        w = self.sources()[0]
        if not (w.is_cuda and w.dtype == torch.float32):
            return None
        return self.ensure()

    def planes(self, layout: str, aux: int = 0):
        """(hi, lo, scale) of `layout` (ops.weight_planes_multi), made on first request and kept"""
        key = (layout, int(aux))
        got = self._layouts.get(key)
        if got is None:
            from . import ops
            (got,), _ = ops.weight_planes_multi([(self.weight, None if layout.endswith("bf16") else self.amax, layout, aux)])
            self._layouts[key] = got
        return got


def _effective_weight(rec):
    """(weight, max|w| cell or None) as the unfrozen eval() route forms them: the parameter itself, or the spectral hook's W / sigma
    without power iteration (K21 where the hook takes it, the framework's ops otherwise) — K21 leaves the cell as a by-product."""
    from . import ops
    m = rec.module
    with torch.no_grad():
        if rec.hook is None:
            return m.weight.detach().contiguous(), None
        w = getattr(rec.hook, "compute_weight_unfrozen", rec.hook.compute_weight)(m, False).detach().contiguous()
    return w, ops._recall_amax(w)


def _prepare_on_device(rec):
    from . import ops
    rec.weight, rec.amax = _effective_weight(rec)
    if rec.amax is None:
        (rec.amax,), _ = ops.weight_absmax_multi([rec.weight])


def _foreseen_layouts(rec):
    """the layouts the layer's default route will ask for, as far as they do not depend on the input's shape"""
    from . import ops, producers
    m, w = rec.module, rec.weight
    if w.dim() != 4:
        return []
    k, hip = tuple(w.shape[2:]), ops.CONV_PRECISION in ("f16x3", "bf16")
    if not isinstance(m, producers.Conv2d):                 # theta / phi: K23 / K25's fragment order
        return [("frag", 0)] if k == (1, 1) and w.shape[0] == ops.FUSED_K and w.shape[1] <= 4096 else []
    if not hip or (k == (1, 1) and m.stride[0] == 1 and m.padding[0] == 0):      # (1x1: K0, rows padded by the grid's rule: on request)
        return []
    bf = "_bf16" if ops.CONV_PRECISION == "bf16" else ""
    out = [("conv_fwd" + bf, 0)]
    if rec.keep_dgrad and m.stride[0] == 1 and k[0] == k[1]:
        out.append(("conv_dgrad" + bf, 0))
    return out


def _prepare_many(records, report):
    """every record that lives on the GPU, together: K21 per spectral layer, ONE max|w| table, ONE plane table (K32)"""
    from . import ops
    todo = []
    for rec in records:
        w = rec.sources()[0]
        if w.is_cuda and w.dtype == torch.float32:
            todo.append(rec)
    if not todo:
        return
    for rec in todo:
        rec.weight, rec.amax = _effective_weight(rec)
        if rec.hook is not None:
            report.launches += 1
    need = [r for r in todo if r.amax is None]
    by_dev = {}
    for r in need:
        by_dev.setdefault(r.weight.device, []).append(r)
    for rs in by_dev.values():
        cells, n = ops.weight_absmax_multi([r.weight for r in rs])
        report.launches += n
        for r, c in zip(rs, cells):
            r.amax = c
    reqs = [(r, lay, aux) for r in todo for lay, aux in _foreseen_layouts(r)]
    if reqs:
        got, n = ops.weight_planes_multi([(r.weight, None if lay.endswith("bf16") else r.amax, lay, aux) for r, lay, aux in reqs])
        report.launches += n
        for (r, lay, aux), g in zip(reqs, got):
            r._layouts[(lay, int(aux))] = g
    for rec in todo:
        rec._sig = rec.signature()


def _modules_of(target):
    if isinstance(target, nn.Module):
        return [("", target)]
    if isinstance(target, dict) or hasattr(target, "items"):
        return [(str(k), v) for k, v in target.items() if isinstance(v, nn.Module)]
    raise TypeError(f"freeze: expected an nn.Module or a dictionary of networks, got {type(target).__name__}")


def record_of(module):
    """the record freeze() attached to `module`, or None"""
    return module.__dict__.get(_ATTR)


def usable_record(module):
    """the record of `module`, validated, if this call may use it (see PreparedWeight.use) — else None"""
    rec = module.__dict__.get(_ATTR)
    return None if rec is None else rec.use()


def freeze(module, prepare=None) -> FrozenReport:
    """Attach a prepared-weight record to every layer of `module` (an nn.Module, or the `net` dictionary of a Pix2PixModel) that has a
    frozen route; layers that already carry one get a new one.  Records of layers on the GPU are prepared here (a handful of launches
    for a whole model); the others the first time they are used.  `prepare`: a callable(record) that fills record.weight and
    record.amax instead of the device routine (tests).  Opt-in: nothing changes for modules nobody freezes."""
    from . import correspondence, producers, vgg
    report = FrozenReport()
    for prefix, root in _modules_of(module):
        in_vgg = set()
        for m in root.modules():
            if isinstance(m, vgg.VGG19_feature_color_torchversion):
                in_vgg.update(id(c) for c in m.modules())
        projections = set()
        for m in root.modules():
            if isinstance(m, correspondence.NoVGGCorrespondence):
                projections.update((id(m.theta), id(m.phi)))
        for name, m in root.named_modules():
            if not (isinstance(m, producers.Conv2d) or id(m) in projections) or not isinstance(m, nn.Conv2d):
                continue
            full = f"{prefix}.{name}" if prefix and name else (prefix or name)
            hook, hip = _spectral_hook(m)
            if hook is not None and not hip:
                report.skipped.append(full)
                continue
            if type(hook) is producers._sn_mod.SpectralNorm:      # the framework's hook: same arithmetic + the record lookup
                hook.__class__ = producers._SpectralNormRecord
            rec = PreparedWeight(m, report, keep_dgrad=id(m) in in_vgg, prepare=prepare, name=full)
            m.__dict__[_ATTR] = rec
            report.layers += 1
            report.spectral += hook is not None
            report.records.append(rec)
    if prepare is None:
        _prepare_many(report.records, report)
    return report


def unfreeze(module) -> int:
    """Remove the records below `module` (an nn.Module or a dictionary of networks).  Returns how many there were."""
    from . import producers
    n = 0
    for _, root in _modules_of(module):
        for m in root.modules():
            if m.__dict__.pop(_ATTR, None) is not None:
                n += 1
                hook = _spectral_hook(m)[0]
                if type(hook) is producers._SpectralNormRecord:
                    hook.__class__ = producers._sn_mod.SpectralNorm
    return n


# ---- the reference's facade -------------------------------------------------------------------------------------------------------
def _pix2pix_module(networks_module):
    return importlib.import_module(networks_module.__name__.rsplit(".", 1)[0] + ".pix2pix_model")


def install_inference_into_reference(networks_module):
    """`Pix2PixModel.initialize_networks` -> a wrapper that, for `opt.isTrain == False`, freezes the networks after they are built and
    loaded (the report is left in `model.frozen_report`).  Returns what it replaced, for `restore_reference_inference`.  A training
    user freezes the fixed VGG alone: `inference.freeze(model.vggnet_fix)`."""
    p2p = _pix2pix_module(networks_module)
    original = p2p.Pix2PixModel.initialize_networks

    def initialize_networks(self, opt):
        net = original(self, opt)
        if not opt.isTrain:
            self.__dict__["frozen_report"] = freeze(net)
        return net

    initialize_networks.__wrapped__ = original
    p2p.Pix2PixModel.initialize_networks = initialize_networks
    return {"initialize_networks": original}


def restore_reference_inference(networks_module, replaced):
    """Undo `install_inference_into_reference` with the dictionary it returned."""
    _pix2pix_module(networks_module).Pix2PixModel.initialize_networks = replaced["initialize_networks"]
