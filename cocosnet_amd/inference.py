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

`prepare_exemplar(net, ref_img, ref_seg_map)` does the same for everything a `NoVGGCorrespondence` derives from the EXEMPLAR (one
style image against many label maps): see PreparedExemplar.
"""
from __future__ import annotations

import importlib
import os

import torch
import torch.nn as nn

#: False (env COCOS_FROZEN=0): attached records are ignored — every call takes the unfrozen route (A/B runs) — and so is a prepared
#: exemplar handed to forward(exemplar=...).  This only bypasses records that freeze() attached / the caller passed explicitly;
#: nothing is frozen by default.  Module attribute, read at call time.
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

    def label_table(self):
        """the tap-major table of K35 (ops.label_conv_table) of the effective weight, made on first request and kept like the planes"""
        key = ("label_taps", 0)
        got = self._layouts.get(key)
        if got is None:
            from . import ops
            got = self._layouts[key] = ops.label_conv_table(self.weight)
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


# ---- prepared exemplars ------------------------------------------------------------------------------------------------------------
class PreparedExemplar:
    """Everything `NoVGGCorrespondence.forward` derives from the EXEMPLAR (ref_img, ref_seg_map) alone, made once and reused for any
    number of content inputs — see prepare_exemplar().  Holds the exemplar stream's features behind `self.layer` and, made the first
    time a route asks for them (as PreparedWeight._layouts), the products of the route in force (an ops.PreparedKeys):

      fused match_kernel 1 (split flavour)   position-major hi / lo key planes of kn and its row norms — the fp32 kn never exists
      fused match_kernel 3 (_BoxedCorr)      phi_raw's position-major hi / lo planes, their scale cell and its (nu, b) statistics
      every other back end                   phi_raw as fp32 (generic, WTA, return_corr, COCOS_PRECISION=fp32)
      always                                 the row pass's value tensor (pooled image or its patches + the sampled direct mask, i.e.
                                             the resized ref_seg of warp_mask / show_warpmask) with its max|v| cell and, on the split
                                             flavour, its hi / lo planes and the lo-plane block mask

    It keeps references to ref_img and ref_seg_map and watches (data_ptr, _version) of both and of every parameter and buffer of
    adaptive_model_img, layer and phi: a record found stale at use time prepares again (`repreparations` counts it) — a stale record
    is never read.  `batch` (Be) is the exemplar batch: a forward with B inputs takes Be == B or Be == 1 (one exemplar for all)."""

    def __init__(self, net, ref_img, ref_seg_map):
        self.net, self.ref_img, self.ref_seg_map = net, ref_img, ref_seg_map
        self.repreparations = 0
        self._sig = None
        self.feat = None            # the exemplar stream behind self.layer [Be, cl, fh, fw]
        self.keys = None            # ops.PreparedKeys on the GPU (fp32); None on the CPU
        self._phi_raw = None        # CPU / fp64: the projection itself

    batch = property(lambda self: self.ref_img.shape[0])

    def sources(self):
        net = self.net
        out = [self.ref_img, self.ref_seg_map]
        for m in (net.adaptive_model_img, net.layer, net.phi):
            out += list(m.parameters()) + list(m.buffers())
        return out

    def signature(self):
        return tuple((t.data_ptr(), t._version) for t in self.sources())

    def stale(self) -> bool:
        return self._sig is not None and self._sig != self.signature()

    def ensure(self):
        """prepare now if never prepared; prepare AGAIN (and count it) if a watched tensor changed or moved"""
        if self.net.training:
            raise ValueError("PreparedExemplar: the network must be in eval() mode")
        sig = self.signature()
        if self._sig == sig:
            return self
        if self._sig is not None:
            self.repreparations += 1
        self.feat = self.keys = self._phi_raw = None
        self._prepare()
        self._sig = sig
        return self

    def phi_raw(self):
        """the exemplar's fp32 projection [Be,256,fh,fw]"""
        return self._phi_raw if self.keys is None else self.keys.phi_raw()

    # ---- the exemplar stream (correspondence.py project(), exemplar side) -----------------------------------------------------------
    def _prepare(self):
        from . import ops
        net = self.net
        with torch.no_grad():
            ref = self.feat = net.exemplar_stream(self.ref_img, self.ref_seg_map)
            if not (ref.is_cuda and ref.dtype == torch.float32):
                self._phi_raw = net.phi(ref)      # CPU / fp64: producer parity tests only (the hot path needs a GPU and fp32)
                return
        rec = self
        ref_img, ref_seg_map = self.ref_img, self.ref_seg_map
        lazy = lambda: ops.LazyProj1x1(ref, net.phi.weight.detach(), None if net.phi.bias is None else net.phi.bias.detach(),
                                       usable_record(net.phi))

        def make_phi_raw():
            return lazy().raw()

        def make_split():      # K23 with one problem where it takes the shape, else K0 + K1's planes flavour
            p = lazy()
            if ops.proj_norm_fused_ok(p):
                return ops.proj_center_l2norm_planes_one(p, 1)
            x = rec.keys.phi_raw()
            return ops.center_l2norm_planes_fwd(x.reshape(x.shape[0], x.shape[1], -1), 1)

        def make_box():
            x = rec.keys.phi_raw()
            B, C, h, w = x.shape
            nu, b = ops.unfold3_stats(x, float(C * 9))
            xf = x.reshape(B, C, h * w)
            kh, kl, ks = ops.split_f16(xf, True, amax=ops.absmax(xf))
            return kh, kl, ks, nu, b

        def make_values(down, patch, direct_mask):
            from .hot_path import exemplar_values
            return exemplar_values(ref_img, ref_seg_map, down, patch, direct_mask)

        B, _, fh, fw = ref.shape
        self.keys = ops.PreparedKeys(B, (B, net.phi.weight.shape[0], fh, fw), ref_img.shape[2:], make_phi_raw, make_split, make_box,
                                     make_values)


def prepare_exemplar(net, ref_img, ref_seg_map) -> PreparedExemplar:
    """Run the exemplar stream of a `NoVGGCorrespondence` once: `net.forward(None, real_img, seg_map, None, exemplar=record)` then
    runs the content stream alone.  Requires `net.eval()` (ValueError otherwise) and runs under torch.no_grad().

    The stream includes the `noise_for_mask` draw of the maskmix concat: that noise is FIXED at preparation time — every forward with
    the record sees the same draw (the ordinary route draws per call); a record that prepares again (see PreparedExemplar) draws again.
    `COCOS_FROZEN=0` / `inference.FROZEN = False` makes forward ignore the record and run the ordinary route from the record's stored
    ref_img / ref_seg_map."""
    from . import correspondence
    if not isinstance(net, correspondence.NoVGGCorrespondence):
        raise TypeError(f"prepare_exemplar: expected a NoVGGCorrespondence, got {type(net).__name__}")
    if net.training:
        raise ValueError("prepare_exemplar: the network must be in eval() mode")
    if ref_img is None or ref_seg_map is None or ref_img.shape[0] != ref_seg_map.shape[0]:
        raise ValueError("prepare_exemplar: ref_img and ref_seg_map of one batch size are required")
    return PreparedExemplar(net, ref_img, ref_seg_map).ensure()


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
