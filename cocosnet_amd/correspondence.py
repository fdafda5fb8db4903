"""Drop-in `NoVGGCorrespondence` — the reference's correspondence network with its hot path on HIP.

Boundary contract (reference models/networks/correspondence.py:148-374):
  * constructor `NoVGGCorrespondence(opt)` with the same side effects on `opt` (sets/deletes
    `opt.spade_ic`, sets `opt.down`; :154-166), same sub-module and parameter names, so
    `state_dict()` round-trips with the reference's `*_net_Corr.pth` checkpoints;
  * `forward(ref_img, real_img, seg_map, ref_seg_map, temperature=0.01, detach_flag=False,
    WTA_scale_weight=1, alpha=1, return_corr=False)` returning the same `coor_out` dict (or the
    scaled correlation tensor when `return_corr`), fresh autograd-tracked fp32 NCHW tensors;
  * `print_network()` / `init_weights(init_type, gain)` as `BaseNetwork` provides them
    (base_network.py:18-59), because `networks.create_network` calls both.

Everything up to `self.theta(...)` / `self.phi(...)` is stock PyTorch (cocosnet_amd.producers);
from there on (`correspondence.py:272-372`) it is `cocosnet_amd.hot_path` = HIP kernels.
To plug into the unmodified reference, see INTEGRATION.md (`install_into_reference()`).
"""
from __future__ import annotations

import argparse

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn import init

from . import inference, ops
from .hot_path import (HotPathConfig, _box3_scope, _flow_scope, _max_dist, _nll_scope, _no_patchmatch_with, _refine_scope, _restrict_scope,
                       _sparse_scope, _sparse_search, _topk_arg, _transport_dict, _transport_scope, _upsample, correspondence_flow, correspondence_flow_box3,
                       correspondence_hot_path, correspondence_match, correspondence_match_box3, correspondence_mutual, correspondence_nll, correspondence_nll_box3,
                       correspondence_sparse, correspondence_sparse_box3,
                       correspondence_transport, correspondence_transport_box3)
from .producers import AdaptiveFeatureGenerator, ResidualBlock

_EPS = __import__("sys").float_info.epsilon
#: the four shared ResidualBlocks see content and exemplar features as ONE batch (False: two calls, as the reference writes it —
#: a test / A-B hook, no environment variable)
BATCH_SHARED_LAYERS = True


def feature_normalize(x):
    """util.feature_normalize (util/util.py:31-34): x / (||x||_2 over channels + epsilon)."""
    if x.is_cuda and x.dtype == torch.float32:      # K1 without the centring: one HBM pass instead of four
        return ops.feature_normalize(x, _EPS)
    return x / (torch.norm(x, 2, 1, keepdim=True) + _EPS)   # CPU / fp64: producer parity tests only (the fp64 arbiter of tests/)


class NetworkBase(nn.Module):
    """The two `BaseNetwork` services `create_network` relies on (base_network.py:18-59)."""

    def print_network(self):
        n = sum(p.numel() for p in self.parameters())
        print("Network [%s] was created. Total number of parameters: %.1f million. "
              "To see the architecture, do print(network)." % (type(self).__name__, n / 1e6))

    def init_weights(self, init_type="normal", gain=0.02):
        def init_one(m):
            cname = m.__class__.__name__
            if "BatchNorm2d" in cname:
                if getattr(m, "weight", None) is not None:
                    init.normal_(m.weight.data, 1.0, gain)
                if getattr(m, "bias", None) is not None:
                    init.constant_(m.bias.data, 0.0)
            elif hasattr(m, "weight") and ("Conv" in cname or "Linear" in cname):
                # NB (faithful to the reference): on spectral-normed layers `m.weight` is the
                # derived tensor, so their `weight_orig` keeps PyTorch's default initialisation
                w = m.weight.data
                if init_type == "normal":
                    init.normal_(w, 0.0, gain)
                elif init_type == "xavier":
                    init.xavier_normal_(w, gain=gain)
                elif init_type == "xavier_uniform":
                    init.xavier_uniform_(w, gain=1.0)
                elif init_type == "kaiming":
                    init.kaiming_normal_(w, a=0, mode="fan_in")
                elif init_type == "orthogonal":
                    init.orthogonal_(w, gain=gain)
                elif init_type == "none":
                    m.reset_parameters()
                else:
                    raise NotImplementedError(f"initialization method [{init_type}] is not implemented")
                if getattr(m, "bias", None) is not None:
                    init.constant_(m.bias.data, 0.0)
        self.apply(init_one)
        for child in self.children():
            if hasattr(child, "init_weights"):
                child.init_weights(init_type, gain)


class NoVGGCorrespondence(NetworkBase):
    def __init__(self, opt):
        self.opt = opt
        super().__init__()
        # the adaptors read opt.spade_ic at construction (:154-158)
        opt.spade_ic = opt.semantic_nc
        self.adaptive_model_seg = AdaptiveFeatureGenerator(opt)
        opt.spade_ic = 3
        self.adaptive_model_img = AdaptiveFeatureGenerator(opt)
        del opt.spade_ic
        if opt.weight_domainC > 0 and (not opt.domain_rela):
            raise NotImplementedError("DomainClassifier (--weight_domainC > 0) is outside the MI355X "
                                      "hot-path scope (SURVEY.md §2 row 3)")
        if "down" not in opt:
            opt.down = 4
        if opt.warp_stride == 2:
            opt.down = 2
        assert opt.down in (2, 4)
        self.down = opt.down
        self.feature_channel = 64
        self.in_channels = self.feature_channel * 4
        self.inter_channels = 256

        cl = self.in_channels + (opt.semantic_nc if opt.maskmix else 0) + (3 if opt.use_coordconv else 0)
        self.layer = nn.Sequential(*[ResidualBlock(cl, cl, kernel_size=3, padding=1, stride=1)
                                     for _ in range(4)])
        self.phi = nn.Conv2d(cl, self.inter_channels, kernel_size=1, stride=1, padding=0)
        self.theta = nn.Conv2d(cl, self.inter_channels, kernel_size=1, stride=1, padding=0)
        # parameter-free; kept as attributes because the reference has them (:184-188)
        self.upsampling_bi = nn.Upsample(scale_factor=opt.down, mode="bilinear")
        self.upsampling = (nn.Upsample(scale_factor=opt.down, mode="bilinear") if opt.warp_bilinear
                           else nn.Upsample(scale_factor=opt.down))
        self.zero_tensor = None

    @staticmethod
    def addcoords(x):
        """CoordConv channels x, y in [-1, 1] and their radius (:202-220)."""
        B, _, h, w = x.shape
        xs = torch.arange(w, dtype=x.dtype, device=x.device) / (w - 1) * 2 - 1
        ys = torch.arange(h, dtype=x.dtype, device=x.device) / (h - 1) * 2 - 1
        xx = xs.view(1, 1, 1, w).expand(B, 1, h, w)
        yy = ys.view(1, 1, h, 1).expand(B, 1, h, w)
        return torch.cat((x, xx, yy, torch.sqrt(xx ** 2 + yy ** 2)), dim=1)

    def exemplar_stream(self, ref_img, ref_seg_map):
        """The exemplar side of project() up to and including `self.layer` (:240-266): adaptive_model_img, feature_normalize,
        coord-conv, the maskmix concat (with its noise_for_mask draw) and the four shared ResidualBlocks.  What
        inference.prepare_exemplar runs once; the ordinary route keeps its own (batched) copy in project()."""
        opt = self.opt
        feat_img = feature_normalize(self.adaptive_model_img(ref_img, ref_img))
        if opt.use_coordconv:
            feat_img = self.addcoords(feat_img)
        if opt.maskmix:
            ref_seg = F.interpolate(ref_seg_map, size=feat_img.shape[2:], mode="nearest")
            if opt.noise_for_mask and ((not opt.isTrain) or (opt.isTrain and opt.epoch > opt.mask_epoch)):
                noise = torch.randn_like(ref_seg, requires_grad=False) * 0.01
                ref_in = torch.cat((feat_img, noise), 1)
            else:
                ref_in = torch.cat((feat_img, ref_seg), 1)
        else:
            ref_in = feat_img
        return self.layer(ref_in)

    def _check_exemplar(self, exemplar, batch):
        """the record, fresh — or ValueError where a record cannot stand in for the exemplar stream"""
        opt = self.opt
        if not isinstance(exemplar, inference.PreparedExemplar) or exemplar.net is not self:
            raise ValueError("exemplar: expected the record inference.prepare_exemplar(net, ...) made for THIS network")
        if self.training:
            raise ValueError("exemplar: a prepared exemplar needs net.eval()")
        if (torch.is_grad_enabled() and opt.isTrain) or opt.warp_cycle_w > 0 or (opt.isTrain and opt.novgg_featpair > 0):
            # the cycle terms (warp_cycle_w, and two_cycle, which only exists with it) and novgg_featpair are training terms whose
            # gradient runs through the exemplar side; the path computes the cycle terms whenever warp_cycle_w > 0.  THE rule: the
            # hot path itself only insists on torch.no_grad()
            raise ValueError("exemplar: a prepared exemplar is inference-only (grad mode with isTrain, warp_cycle_w / two_cycle and "
                             "novgg_featpair need the exemplar stream)")
        if exemplar.batch not in (batch, 1):
            raise ValueError(f"exemplar: prepared for a batch of {exemplar.batch}, used with {batch} inputs (expected {batch} or 1)")
        return exemplar.ensure() if inference.FROZEN else exemplar      # (ignored under COCOS_FROZEN=0: nothing is prepared for it)

    def _project_content(self, seg_map, exemplar, lazy):
        """project() with a prepared exemplar: the content stream alone (`self.layer` sees cont_in alone)."""
        opt = self.opt
        if opt.mask_noise:
            noise = torch.randn_like(seg_map, requires_grad=False) * 0.1
            noise[seg_map == 0] = 0
            seg_input = seg_map + noise
        else:
            seg_input = seg_map
        feat_seg = feature_normalize(self.adaptive_model_seg(seg_input, seg_input))
        if opt.use_coordconv:
            feat_seg = self.addcoords(feat_seg)
        if opt.maskmix:
            seg = F.interpolate(seg_map, size=feat_seg.shape[2:], mode="nearest")
            cont = self.layer(torch.cat((feat_seg, seg), 1))
        else:
            cont = self.layer(feat_seg)
        if cont.is_cuda and cont.dtype == torch.float32:
            rt = inference.usable_record(self.theta)
            if lazy:
                return ops.LazyProj1x1(cont, self.theta.weight, self.theta.bias, rt), exemplar.keys
            return ops.proj1x1(cont, self.theta.weight, self.theta.bias, rt), exemplar.phi_raw()
        return self.theta(cont), exemplar.phi_raw()

    def project(self, ref_img, real_img, seg_map, ref_seg_map, coor_out=None, lazy=False, *, exemplar=None):
        """Everything BEFORE the hot path (:239-272, :282): returns (theta_raw, phi_raw).  `exemplar`: a record of
        inference.prepare_exemplar — ref_img / ref_seg_map may then be None, only the content stream runs and phi_raw is the record's
        (with inference.FROZEN off the record is ignored: the ordinary route, from the record's stored inputs)."""
        opt = self.opt
        if exemplar is not None:
            exemplar = self._check_exemplar(exemplar, seg_map.shape[0])
            if inference.FROZEN:
                return self._project_content(seg_map, exemplar, lazy)
            ref_img, ref_seg_map = _stored_inputs(exemplar, seg_map.shape[0])
        elif ref_img is None or ref_seg_map is None:
            raise ValueError("project: ref_img and ref_seg_map are required without a prepared exemplar")
        if opt.mask_noise:
            noise = torch.randn_like(seg_map, requires_grad=False) * 0.1
            noise[seg_map == 0] = 0
            seg_input = seg_map + noise
        else:
            seg_input = seg_map
        feat_seg = feature_normalize(self.adaptive_model_seg(seg_input, seg_input))
        feat_img = feature_normalize(self.adaptive_model_img(ref_img, ref_img))
        if opt.isTrain and opt.novgg_featpair > 0 and coor_out is not None:
            pair = feature_normalize(self.adaptive_model_img(real_img, real_img))
            coor_out["loss_novgg_featpair"] = F.l1_loss(feat_seg, pair) * opt.novgg_featpair
        if opt.use_coordconv:
            feat_seg, feat_img = self.addcoords(feat_seg), self.addcoords(feat_img)
        seg = F.interpolate(seg_map, size=feat_seg.shape[2:], mode="nearest")
        ref_seg = F.interpolate(ref_seg_map, size=feat_img.shape[2:], mode="nearest")
        if opt.maskmix:
            cont_in = torch.cat((feat_seg, seg), 1)
            if opt.noise_for_mask and ((not opt.isTrain) or (opt.isTrain and opt.epoch > opt.mask_epoch)):
                noise = torch.randn_like(ref_seg, requires_grad=False) * 0.01
                ref_in = torch.cat((feat_img, noise), 1)
            else:
                ref_in = torch.cat((feat_img, ref_seg), 1)
        else:
            cont_in, ref_in = feat_seg, feat_img
        if BATCH_SHARED_LAYERS and cont_in.is_cuda and cont_in.shape == ref_in.shape:
            # `self.layer` (four ResidualBlocks, shared weights) is applied to both streams (:258-266): every op in it is
            # per-sample (convolution, InstanceNorm2d, PReLU), so ONE pass over the concatenated batch gives the same values
            # with half the launches — one weight-plane preparation, one weight gradient and one split-K reduction per
            # convolution instead of two
            both = self.layer(torch.cat((cont_in, ref_in), 0))
            cont, ref = both[:cont_in.shape[0]], both[cont_in.shape[0]:]
        else:
            cont, ref = self.layer(cont_in), self.layer(ref_in)
        if cont.is_cuda and cont.dtype == torch.float32:   # :272 / :282 on K0 (same parameters: checkpoints are unaffected)
            # (frozen-weight inference: the projections' records, when freeze() attached them and this call may use them)
            rt, rp = inference.usable_record(self.theta), inference.usable_record(self.phi)
            if lazy:      # forward(): the hot path decides — K23 (projection + K1 fused, no fp32 theta / phi) or K0 (ops.LazyProj1x1)
                return (ops.LazyProj1x1(cont, self.theta.weight, self.theta.bias, rt),
                        ops.LazyProj1x1(ref, self.phi.weight, self.phi.bias, rp))
            return (ops.proj1x1(cont, self.theta.weight, self.theta.bias, rt),
                    ops.proj1x1(ref, self.phi.weight, self.phi.bias, rp))
        return self.theta(cont), self.phi(ref)   # CPU / fp64: producer parity tests only; the hot path needs a GPU and fp32

    def forward(self, ref_img, real_img, seg_map, ref_seg_map, temperature=0.01, detach_flag=False,
                WTA_scale_weight=1, alpha=1, return_corr=False, *, exemplar=None):
        coor_out = {}
        keys = None
        if exemplar is not None:
            exemplar = self._check_exemplar(exemplar, seg_map.shape[0])
            if inference.FROZEN:
                with torch.no_grad():
                    theta_raw, keys = self._project_content(seg_map, exemplar, lazy=True)
                phi_raw = ref_img = ref_seg_map = None
            else:
                ref_img, ref_seg_map = _stored_inputs(exemplar, seg_map.shape[0])
        elif ref_img is None or ref_seg_map is None:
            raise ValueError("forward: ref_img and ref_seg_map are required without a prepared exemplar")
        if keys is None:
            theta_raw, phi_raw = self.project(ref_img, real_img, seg_map, ref_seg_map, coor_out, lazy=True)
        cfg = HotPathConfig.from_opt(self.opt, down=self.opt.down)
        kw = dict(temperature=temperature, detach_flag=detach_flag, WTA_scale_weight=WTA_scale_weight, return_corr=return_corr)
        if keys is None:      # (the ordinary call, argument for argument as before)
            res = correspondence_hot_path(theta_raw, phi_raw, ref_img, real_img, seg_map, ref_seg_map, cfg, **kw)
        else:
            with torch.no_grad():      # a record's route is forward-only
                res = correspondence_hot_path(theta_raw, None, None, real_img, seg_map, None, cfg, exemplar=keys, **kw)
        if return_corr:
            return res
        coor_out.update(res)
        return coor_out

    def match(self, ref_img, seg_map, ref_seg_map, temperature=0.01, *, exemplar=None, direction="rows", hard_warp=False, topk=1,
              blend="topk", refine=0, refine_temperature=None, restrict=None):
        """Where each position matched, and how sure the match is — the hard readout of the correlation that
        `forward(..., return_corr=True)` returns as a [B,HW,HW] matrix (:305-306), without that matrix wherever the fused
        match_kernel-1 back end runs, and with one HWxHW tensor (the x-box correlation T, read once) instead of two logit matrices
        wherever the fused match_kernel-3 back end runs (hot_path.correspondence_match).  Forward only.

        direction="rows": per content position its best exemplar position; "cols": per exemplar position its best content position.
        Returns {match_index [B,h,w] int64 (flat position on the other side's grid), match_xy [B,2,h,w] (x, y), match_prob (the
        match's softmax weight), match_lse} and, with `hard_warp`, warp_hard [B,3,H,W]: every content cell filled with the
        down x down patch of ref_img at its match (rows only).  `exemplar`: a record of inference.prepare_exemplar in place of
        ref_img / ref_seg_map (both None).

        `topk` = k in 2..8 (at most the number of positions; else ValueError) returns the k best candidates per position, best
        first, ties in favour of the lower index: match_index [B,k,h,w], match_xy [B,k,2,h,w], match_prob [B,k,h,w] (each
        candidate's softmax weight among ALL positions), match_lse [B,h,w]; nothing HWxHW on the fused match_kernel-1 route,
        the one T = xbox(C) read once on the fused match_kernel-3 route (K41), the logits matrix read once everywhere else.  With `hard_warp` also warp_hard (the rank-0 gather, as with topk = 1)
        and warp_topk [B,3,H,W]: per cell the blend of the k candidates' full-resolution patches, weighted by `blend` =
        "topk" (softmax over the k logits: the weights sum to 1 — a k-sparse softmax) or "full" (match_prob itself: the true
        softmax weights, which sum to <= 1).  An unknown `blend` raises ValueError.

        `refine` = r in 1..3 (K44; 0, the default, changes nothing) refines the top-1 match below the feature grid: a softmax at
        `refine_temperature` (None: `temperature`) over the (2 r + 1)^2 window of positions around the match gives match_offset
        [B,2,h,w] (x, y; in cells, |offset| <= r), match_xy_sub = match_xy + match_offset (fp32) and match_window_prob [B,h,w], the
        window's share of the position's softmax mass; with `hard_warp` also warp_sub [B,3,H,W], ref_img sampled bilinearly at the
        refined position (warp_hard stays).  Scope: topk = 1, no prepared exemplar, the fused match_kernel-1 route (PONO_C,
        COCOS_PRECISION=f16x3, ops.MATCH_FUSED); everything else raises ValueError before the network runs.

        `restrict` (K47; None, the default, changes nothing): "label" picks every position's candidates only among the positions of
        the other side that carry its class — the majority class of each feature cell of seg_map / ref_seg_map
        (hot_path.cell_labels); a pair (q_labels [B,h,w], k_labels [B,h,w]) of int32 / int64 tensors, content side first, says
        "this region takes from that region" with any labels (a negative content label: unrestricted).  match_prob and match_lse
        are then over the ALLOWED positions, not all of them; warp_hard / warp_topk work unchanged from the restricted indices.  A
        position whose label has fewer than topk positions on the other side falls back to the unrestricted scan; match_restricted
        [B,h,w] bool says which positions were restricted.  Scope: the fused match_kernel-1 route (PONO_C, COCOS_PRECISION=f16x3,
        ops.MATCH_FUSED), no prepared exemplar, refine = 0; everything else raises a ValueError naming restrict before the network runs."""
        if direction not in ("rows", "cols"):
            raise ValueError(f"match: direction {direction!r}: expected 'rows' or 'cols'")
        if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= ops.MATCH_TOPK_MAX:
            raise ValueError(f"match: topk={topk!r}: expected an integer in 1..{ops.MATCH_TOPK_MAX}")
        if blend not in ("topk", "full"):
            raise ValueError(f"match: blend {blend!r}: expected 'topk' or 'full'")
        if hard_warp and direction == "cols":
            raise ValueError("match: hard_warp gathers exemplar patches for the content grid: it needs direction='rows'")
        cfg = HotPathConfig.from_opt(self.opt, down=self.opt.down)
        _restrict_scope("match", cfg, restrict, exemplar is not None, refine, channels=self.inter_channels)
        _refine_scope("match", cfg, refine, refine_temperature, topk, exemplar is not None, self.inter_channels)
        keys = phi_raw = None
        with torch.no_grad():
            if exemplar is not None:
                exemplar = self._check_exemplar(exemplar, seg_map.shape[0])
                if inference.FROZEN:
                    theta_raw, keys = self._project_content(seg_map, exemplar, lazy=True)
                    phi_raw, ref_img = None, exemplar.ref_img
                    if not isinstance(keys, ops.PreparedKeys):      # CPU / fp64 content: the record's projection itself — the
                        phi_raw, keys = keys, None                  # readout then refuses the tensors ("no CPU fallback")
                else:
                    ref_img, ref_seg_map = _stored_inputs(exemplar, seg_map.shape[0])
            elif ref_img is None or ref_seg_map is None:
                raise ValueError("match: ref_img and ref_seg_map are required without a prepared exemplar")
            if keys is None and phi_raw is None:      # (real_img: project() reads it for the training-time featpair term only)
                theta_raw, phi_raw = self.project(ref_img, None, seg_map, ref_seg_map, None, lazy=True)
            if restrict is None:
                m = correspondence_match(theta_raw, phi_raw, cfg, temperature, exemplar=keys, direction=direction, topk=topk, refine=refine,
                                         refine_temperature=refine_temperature)
            else:
                m = correspondence_match(theta_raw, phi_raw, cfg, temperature, exemplar=keys, direction=direction, topk=topk, refine=refine,
                                         refine_temperature=refine_temperature, restrict=restrict, seg_map=seg_map, ref_seg_map=ref_seg_map)
            out = {"match_index": m.index, "match_xy": m.xy(), "match_prob": m.prob, "match_lse": m.lse}
            if restrict is not None:
                out["match_restricted"] = m.restricted
            if refine:
                out.update(match_offset=m.offset, match_xy_sub=m.xy_sub(), match_window_prob=m.window_prob)
            if hard_warp and topk == 1:
                fh, fw = m.index.shape[1:]
                out["warp_hard"] = ops.gather_patches(ref_img, m.index, fh, fw, self.opt.down)
                if refine:
                    off = m.offset.permute(0, 2, 3, 1).reshape(m.index.shape[0], fh * fw, 2)
                    out["warp_sub"] = ops.gather_patches_subcell(ref_img, m.index, off, (fh, fw), m.grid, self.opt.down)
            elif hard_warp:
                fh, fw = m.index.shape[2:]
                out["warp_hard"] = ops.gather_patches(ref_img, m.index[:, 0], fh, fw, self.opt.down)
                weights = torch.softmax(m.logit, dim=1) if blend == "topk" else m.prob
                out["warp_topk"] = ops.gather_blend_patches(ref_img, m.index, weights, fh, fw, self.opt.down)
        return out

    def mutual_match(self, ref_img, seg_map, ref_seg_map, temperature=0.01, *, exemplar=None, max_dist=0, hard_warp=False):
        """Where each position matched AND whether the match is confirmed from the other side (K48, hot_path.correspondence_mutual):
        content position i goes to exemplar position j = match_index, j goes back to content position match_round_trip, and the match
        counts as mutual when that lies within `max_dist` cells (Chebyshev; 0, the default: exactly i — mutual nearest neighbours) of
        i.  One projection of the network, under torch.no_grad(); where the fused match_kernel-1 route runs, ONE sweep of the
        correlation serves both directions (every other route, prepared exemplars included, pays two readouts).  Returns
        match_index [B,h,w] int64 / match_xy [B,2,h,w] / match_prob / match_lse: match(direction="rows")'s, bit for bit;
        back_index [B,gh,gw] / back_xy / back_prob / back_lse: the column direction, per exemplar position its best content position;
        match_round_trip [B,h,w] int64, match_cycle_dist [B,h,w] int32, match_mutual [B,h,w] bool on the content grid;
        back_cycle_dist, back_mutual [B,gh,gw] on the exemplar grid;
        with `hard_warp`: warp_hard [B,3,H,W] as match() returns it and warp_valid [B,1,H,W] fp32, match_mutual up-sampled by `down`
        (nearest neighbour): the full-resolution cells whose source is confirmed.
        `exemplar`: a record of inference.prepare_exemplar in place of ref_img / ref_seg_map, as for match().  `max_dist` must be a
        non-negative integer (ValueError before the network runs).  match(), forward(), sparse_warp() and flow_warp() are unaffected."""
        max_dist = _max_dist("mutual_match", max_dist)
        cfg = HotPathConfig.from_opt(self.opt, down=self.opt.down)
        keys = phi_raw = None
        with torch.no_grad():
            if exemplar is not None:
                exemplar = self._check_exemplar(exemplar, seg_map.shape[0])
                if inference.FROZEN:
                    theta_raw, keys = self._project_content(seg_map, exemplar, lazy=True)
                    phi_raw, ref_img = None, exemplar.ref_img
                    if not isinstance(keys, ops.PreparedKeys):      # CPU / fp64 content: as match() — the readout refuses the tensors
                        phi_raw, keys = keys, None
                else:
                    ref_img, ref_seg_map = _stored_inputs(exemplar, seg_map.shape[0])
            elif ref_img is None or ref_seg_map is None:
                raise ValueError("mutual_match: ref_img and ref_seg_map are required without a prepared exemplar")
            if keys is None and phi_raw is None:
                theta_raw, phi_raw = self.project(ref_img, None, seg_map, ref_seg_map, None, lazy=True)
            m = correspondence_mutual(theta_raw, phi_raw, cfg, temperature, exemplar=keys, max_dist=max_dist)
            out = {"match_index": m.rows.index, "match_xy": m.rows.xy(), "match_prob": m.rows.prob, "match_lse": m.rows.lse,
                   "back_index": m.cols.index, "back_xy": m.cols.xy(), "back_prob": m.cols.prob, "back_lse": m.cols.lse,
                   "match_round_trip": m.rows_back, "match_cycle_dist": m.rows_dist, "match_mutual": m.rows_mutual,
                   "back_cycle_dist": m.cols_dist, "back_mutual": m.cols_mutual}
            if hard_warp:
                fh, fw = m.rows.index.shape[1:]
                out["warp_hard"] = ops.gather_patches(ref_img, m.rows.index, fh, fw, self.opt.down)
                out["warp_valid"] = _upsample(m.rows_mutual.to(torch.float32).unsqueeze(1).contiguous(), self.opt.down, False)
        return out

    def transport_match(self, ref_img, seg_map, ref_seg_map, temperature=0.01, *, iters=5, tau=1.0, topk=1, hard_warp=False):
        """match() on the entropic transport plan instead of the row softmax (K50, hot_path.correspondence_transport; UNITE's
        replacement of this block's softmax): `iters` log-domain Sinkhorn iterations under uniform marginals (tau = 1 balanced, 0 < tau
        < 1 KL-relaxed) give the potentials f, g, and every content position reads the row of z_ij = s_ij + g_j — an exemplar
        position that many content positions want is priced out, so one exemplar cell no longer serves hundreds of queries.  One
        projection of the network, under torch.no_grad(); nothing HWxHW.  Returns match()'s keys computed on z: match_index [B,h,w]
        int64 ([B,k,h,w] with topk = k > 1), match_xy, match_prob = exp(z - match_lse), match_lse = log sum_j exp z_ij; with
        `hard_warp` warp_hard and, for topk > 1, warp_topk (the blend weighted by the softmax over the k values of z); and
        potential_q [B,h,w], potential_k [B,gh,gw], match_mass [B,h,w] (1 where the row marginal is met), key_mass [B,gh,gw] (the
        transported mass each exemplar position receives over its fair share; 1 under tau = 1).  Scope: sparse_warp's (match_kernel 1
        with PONO_C on the plain flag set, COCOS_PRECISION=f16x3, no prepared exemplar); everything else raises a ValueError naming
        transport before the network runs.  match(), mutual_match(), forward() and sparse_warp() are unaffected."""
        k = _topk_arg("transport_match", topk)
        cfg = HotPathConfig.from_opt(self.opt, down=self.opt.down)
        _transport_scope("transport_match", cfg, {"iters": iters, "tau": tau}, False, channels=self.inter_channels)
        if ref_img is None or ref_seg_map is None:
            raise ValueError("transport_match: ref_img and ref_seg_map are required (a prepared exemplar is out of scope)")
        with torch.no_grad():
            theta_raw, phi_raw = self.project(ref_img, None, seg_map, ref_seg_map, None, lazy=True)
            res = correspondence_transport(theta_raw, phi_raw, cfg, temperature, iters=iters, tau=tau, topk=k)
            m = res.pop("readout")
            out = {"match_index": m.index, "match_xy": m.xy(), "match_prob": m.prob, "match_lse": m.lse, **res}
            if hard_warp and k == 1:
                fh, fw = m.index.shape[1:]
                out["warp_hard"] = ops.gather_patches(ref_img, m.index, fh, fw, self.opt.down)
            elif hard_warp:
                fh, fw = m.index.shape[2:]
                out["warp_hard"] = ops.gather_patches(ref_img, m.index[:, 0], fh, fw, self.opt.down)
                out["warp_topk"] = ops.gather_blend_patches(ref_img, m.index, torch.softmax(m.logit, dim=1), fh, fw, self.opt.down)
        return out

    def sparse_warp(self, ref_img, real_img, seg_map, ref_seg_map, temperature=0.01, *, topk=4, search="dense", search_opts=None,
                    restrict=None, transport=None):
        """The trainable k-sparse warp (hot_path.correspondence_sparse): per content position the `topk` best exemplar positions are
        selected without gradient, and a softmax over those k logits alone blends the pooled exemplar (and, under
        --warp_mask_losstype direct, the exemplar's labels) — attention over k keys instead of all HW, with gradients to the whole
        network through theta and phi and nothing HWxHW in memory.  Returns {warp_out [B,3,H,W], warp_mask [B,nc,h,w] (direct),
        match_index [B,k,h,w] int64, match_weight [B,k,h,w]} (+ loss_novgg_featpair where project() makes it).  Scope: match_kernel 1
        with PONO_C on the plain flag set; everything else raises ValueError (no fall-back).  forward() and match() are unaffected.
        `search` / `search_opts`: the candidate selector, "dense" (default: the scan over all keys) or "patchmatch" (K43) with its
        schedule, as hot_path.correspondence_sparse takes them.  `restrict` (K47; None changes nothing): "label" or a pair of label
        tensors, as match() takes them — the candidates come from the exemplar positions of the content position's label (dense
        selector only), the result gains match_restricted [B,h,w], and the gradients are the same: the indices are data.
        `transport` (K50; None changes nothing): dict(iters=, tau=) — the candidates are the top-k of the transport plan's rows and the
        blend is the biased softmax over them, with the Sinkhorn potentials detached (gradients reach the network through the k pair
        logits and the values only); the result gains potential_k [B,gh,gw] and match_mass [B,h,w].  Dense selector, no restrict."""
        cfg = HotPathConfig.from_opt(self.opt, down=self.opt.down)
        _transport_scope("sparse_warp", cfg, transport, False, search, restrict, self.inter_channels)
        _restrict_scope("sparse_warp", cfg, restrict, False, 0, search, self.inter_channels)
        _sparse_scope(cfg, topk)                  # out-of-scope flags are refused before the network runs
        _sparse_search(search, search_opts)
        if ref_img is None or ref_seg_map is None:
            raise ValueError("sparse_warp: ref_img and ref_seg_map are required (a prepared exemplar is out of scope)")
        coor_out = {}
        theta_raw, phi_raw = self.project(ref_img, real_img, seg_map, ref_seg_map, coor_out, lazy=True)
        kw = {} if restrict is None else {"restrict": restrict}
        if transport is not None:
            kw["transport"] = transport
        coor_out.update(correspondence_sparse(theta_raw, phi_raw, ref_img, seg_map, ref_seg_map, cfg, temperature, topk, search=search,
                                              search_opts=search_opts, **kw))
        return coor_out

    def transport_match_box3(self, ref_img, seg_map, ref_seg_map, temperature=0.01, *, iters=5, tau=1.0, topk=1, hard_warp=False):
        """transport_match on the reference's default route, match_kernel 3 (K54, hot_path.correspondence_transport_box3): the Sinkhorn
        iteration runs on the one x-box tensor T of the box logits — one correlation GEMM, 2 iters + 1 streaming reads of T — and every
        content position reads the row of z + g.  One projection of the network, under torch.no_grad(); one HWxHW tensor alive at a
        time, none after return.  Returns transport_match's keys: match_index [B,h,w] int64 ([B,k,h,w] with topk = k > 1), match_xy,
        match_prob, match_lse, potential_q, potential_k, match_mass, key_mass, and with `hard_warp` warp_hard (topk > 1: also
        warp_topk).  Scope: match_kernel 3 with PONO_C on the plain flag set, COCOS_PRECISION=f16x3, no prepared exemplar; everything
        else raises a ValueError naming box transport before the network runs.  transport_match() is unaffected."""
        cfg = HotPathConfig.from_opt(self.opt, down=self.opt.down)
        got = _box3_scope("transport_match_box3", "transport_box3", cfg, False, self.inter_channels, topk=topk, sinkhorn=(iters, tau))
        k, (iters, tau) = got["topk"], got["sinkhorn"]
        if ref_img is None or ref_seg_map is None:
            raise ValueError("transport_match_box3: ref_img and ref_seg_map are required (a prepared exemplar is out of scope)")
        with torch.no_grad():
            theta_raw, phi_raw = self.project(ref_img, None, seg_map, ref_seg_map, None, lazy=True)
            res = correspondence_transport_box3(theta_raw, phi_raw, cfg, temperature, iters=iters, tau=tau, topk=k)
            m = res.pop("readout")
            out = {"match_index": m.index, "match_xy": m.xy(), "match_prob": m.prob, "match_lse": m.lse, **res}
            if hard_warp and k == 1:
                fh, fw = m.index.shape[1:]
                out["warp_hard"] = ops.gather_patches(ref_img, m.index, fh, fw, self.opt.down)
            elif hard_warp:
                fh, fw = m.index.shape[2:]
                out["warp_hard"] = ops.gather_patches(ref_img, m.index[:, 0], fh, fw, self.opt.down)
                out["warp_topk"] = ops.gather_blend_patches(ref_img, m.index, torch.softmax(m.logit, dim=1), fh, fw, self.opt.down)
        return out

    def match_box3(self, ref_img, seg_map, ref_seg_map, temperature=0.01, *, direction="rows", hard_warp=False, topk=1, blend="topk",
                   restrict="label"):
        """match(restrict=) on the reference's default route, match_kernel 3 (K55, hot_path.correspondence_match_box3): every
        position's candidates are picked only among the positions of the other side that carry its class — `restrict` = "label": the
        majority class of each feature cell of seg_map / ref_seg_map; a pair (q_labels [B,h,w], k_labels [B,h,w]) of int32 / int64
        tensors, content side first: any labels (a negative content label: unrestricted) — with the mask inside the scan of the one
        x-box tensor T: one correlation GEMM, one launch, nothing HWxHW after return.  One projection of the network, under
        torch.no_grad().  Returns match()'s keys plus match_restricted [B,h,w] bool (a position whose label has fewer than topk
        positions on the other side falls back to the unrestricted scan): match_index [B,h,w] int64 ([B,k,h,w] with topk = k > 1),
        match_xy, match_prob and match_lse over the ALLOWED positions, and with `hard_warp` warp_hard (topk > 1: also warp_topk,
        weighted by `blend`) from the restricted indices.  `restrict` = None is match() on the same arguments.  Scope: match_kernel 3
        with PONO_C, COCOS_PRECISION=f16x3, ops.MATCH_FUSED, no prepared exemplar; everything else raises a ValueError naming restrict
        before the network runs.  match() is unaffected."""
        if restrict is None:
            return self.match(ref_img, seg_map, ref_seg_map, temperature, direction=direction, hard_warp=hard_warp, topk=topk, blend=blend)
        if direction not in ("rows", "cols"):
            raise ValueError(f"match_box3: direction {direction!r}: expected 'rows' or 'cols'")
        k = _topk_arg("match_box3", topk)
        if blend not in ("topk", "full"):
            raise ValueError(f"match_box3: blend {blend!r}: expected 'topk' or 'full'")
        if hard_warp and direction == "cols":
            raise ValueError("match_box3: hard_warp gathers exemplar patches for the content grid: it needs direction='rows'")
        cfg = HotPathConfig.from_opt(self.opt, down=self.opt.down)
        _box3_scope("match_box3", "restrict_box3", cfg, False, self.inter_channels, plain_flags=False, restrict=restrict, transport=None)
        if ref_img is None or ref_seg_map is None:
            raise ValueError("match_box3: restrict: ref_img and ref_seg_map are required (a prepared exemplar is out of scope)")
        with torch.no_grad():
            theta_raw, phi_raw = self.project(ref_img, None, seg_map, ref_seg_map, None, lazy=True)
            m = correspondence_match_box3(theta_raw, phi_raw, cfg, temperature, direction=direction, topk=k, restrict=restrict,
                                          seg_map=seg_map, ref_seg_map=ref_seg_map)
            out = {"match_index": m.index, "match_xy": m.xy(), "match_prob": m.prob, "match_lse": m.lse, "match_restricted": m.restricted}
            if hard_warp and k == 1:
                fh, fw = m.index.shape[1:]
                out["warp_hard"] = ops.gather_patches(ref_img, m.index, fh, fw, self.opt.down)
            elif hard_warp:
                fh, fw = m.index.shape[2:]
                out["warp_hard"] = ops.gather_patches(ref_img, m.index[:, 0], fh, fw, self.opt.down)
                weights = torch.softmax(m.logit, dim=1) if blend == "topk" else m.prob
                out["warp_topk"] = ops.gather_blend_patches(ref_img, m.index, weights, fh, fw, self.opt.down)
        return out

    def sparse_warp_box3(self, ref_img, real_img, seg_map, ref_seg_map, temperature=0.01, *, topk=4, transport=None, restrict=None,
                         search="dense", search_opts=None):
        """sparse_warp on the reference's default route, match_kernel 3 (K51, hot_path.correspondence_sparse_box3): per content position
        the `topk` best exemplar positions are selected without gradient, as match(topk=topk) selects them, and a softmax over those k
        box logits alone blends the pooled exemplar (and, under --warp_mask_losstype direct, the exemplar's labels), with gradients to
        the whole network through theta and phi and nothing HWxHW kept for the backward.  Returns sparse_warp's dictionary: {warp_out
        [B,3,H,W], warp_mask [B,nc,h,w] (direct), match_index [B,k,h,w] int64, match_weight [B,k,h,w]} (+ loss_novgg_featpair where
        project() makes it).  Scope: match_kernel 3 with PONO_C on the plain flag set; everything else raises ValueError before the
        network runs (no fall-back).  forward(), match() and sparse_warp() are unaffected.  `transport` (K54; None changes nothing):
        dict(iters=, tau=) — the candidates are the top-k of the box transport plan's rows and the blend is the biased softmax over
        them, with the Sinkhorn potentials detached; the result gains potential_k and match_mass.  `restrict` (K55; None changes nothing):
        "label" or a pair of integer label tensors as for match_box3 — the candidates are the restricted top-k; the result gains
        match_restricted; restrict together with transport raises ValueError.  `search` / `search_opts` (K57; "dense" changes nothing):
        "patchmatch" selects the candidates with ops.patchmatch_topk_box3 — no HWxHW tensor of the full grid, any grid sizes — as
        hot_path.correspondence_sparse_box3 takes them; together with restrict or transport it raises a ValueError naming search."""
        cfg = HotPathConfig.from_opt(self.opt, down=self.opt.down)
        _no_patchmatch_with("sparse_warp_box3", search, restrict, transport)
        if restrict is not None:      # (first: every scope message of a restricted call names restrict)
            _topk_arg("sparse_warp_box3", topk)
            _box3_scope("sparse_warp_box3", "restrict_box3", cfg, False, self.inter_channels, restrict=restrict, transport=transport)
        _box3_scope("sparse_warp_box3", "sparse_box3", cfg, False, self.inter_channels, topk=topk)      # refused before the network runs
        _sparse_search(search, search_opts, "sparse_warp_box3")
        if transport is not None:
            _transport_dict("sparse_warp_box3", transport)
        if ref_img is None or ref_seg_map is None:
            raise ValueError("sparse_warp_box3: ref_img and ref_seg_map are required (a prepared exemplar is out of scope)")
        coor_out = {}
        theta_raw, phi_raw = self.project(ref_img, real_img, seg_map, ref_seg_map, coor_out, lazy=True)
        kw = {} if transport is None else {"transport": transport}
        if restrict is not None:
            kw["restrict"] = restrict
        if search != "dense":
            kw.update(search=search, search_opts=search_opts)
        coor_out.update(correspondence_sparse_box3(theta_raw, phi_raw, ref_img, seg_map, ref_seg_map, cfg, temperature, topk, **kw))
        return coor_out

    def flow_warp(self, ref_img, real_img, seg_map, ref_seg_map, temperature=0.01, *, radius=1, refine_temperature=None):
        """The trainable sub-cell correspondence (hot_path.correspondence_flow): per content position the best exemplar position is
        selected without gradient, a softmax at `refine_temperature` (None: `temperature`) over the (2 radius + 1)^2 window around it
        gives a sub-cell offset, and ref_img is sampled bilinearly at the refined position — with gradients to the whole network
        through theta and phi (none to ref_img), so a photometric loss on warp_out or a regression loss on match_offset trains the
        field below the feature grid.  Returns {warp_out [B,3,H,W], match_index [B,h,w] int64, match_offset [B,2,h,w],
        match_xy_sub [B,2,h,w], match_window_prob [B,h,w]} (+ loss_novgg_featpair where project() makes it); match_index and
        match_offset are match(refine=radius)'s bit for bit.  Scope: sparse_warp's (match_kernel 1 with PONO_C on the plain flag set),
        radius in 1..3; everything else raises ValueError before the network runs.  forward() and match() are unaffected."""
        cfg = HotPathConfig.from_opt(self.opt, down=self.opt.down)
        _flow_scope(cfg, radius, refine_temperature)      # out-of-scope flags are refused before the network runs
        if ref_img is None or ref_seg_map is None:
            raise ValueError("flow_warp: ref_img and ref_seg_map are required (a prepared exemplar is out of scope)")
        coor_out = {}
        theta_raw, phi_raw = self.project(ref_img, real_img, seg_map, ref_seg_map, coor_out, lazy=True)
        coor_out.update(correspondence_flow(theta_raw, phi_raw, ref_img, cfg, temperature, radius=radius,
                                            refine_temperature=refine_temperature))
        return coor_out

    def flow_warp_box3(self, ref_img, real_img, seg_map, ref_seg_map, temperature=0.01, *, radius=1, refine_temperature=None):
        """flow_warp on the reference's default route, match_kernel 3 (K52, hot_path.correspondence_flow_box3): per content position
        the best exemplar position is selected without gradient, as match() selects it, a softmax at `refine_temperature` (None:
        `temperature`) over the box logits of the (2 radius + 1)^2 window around it gives a sub-cell offset, and ref_img is sampled
        bilinearly at the refined position — with gradients to the whole network through theta and phi (none to ref_img) and nothing
        HWxHW kept for the backward.  Returns flow_warp's dictionary: {warp_out [B,3,H,W], match_index [B,h,w] int64, match_offset
        [B,2,h,w], match_xy_sub [B,2,h,w], match_window_prob [B,h,w]} (+ loss_novgg_featpair where project() makes it).  Under
        torch.no_grad() this is the forward-only readout of the route.  Scope: match_kernel 3 with PONO_C on the plain flag set,
        radius in 1..3; everything else raises ValueError before the network runs (no fall-back).  forward(), match(), flow_warp() and
        sparse_warp_box3() are unaffected."""
        cfg = HotPathConfig.from_opt(self.opt, down=self.opt.down)
        # out-of-scope flags are refused before the network runs
        _box3_scope("flow_warp_box3", "flow_box3", cfg, False, self.inter_channels, radius=radius, refine_temperature=refine_temperature)
        if ref_img is None or ref_seg_map is None:
            raise ValueError("flow_warp_box3: ref_img and ref_seg_map are required (a prepared exemplar is out of scope)")
        coor_out = {}
        theta_raw, phi_raw = self.project(ref_img, real_img, seg_map, ref_seg_map, coor_out, lazy=True)
        coor_out.update(correspondence_flow_box3(theta_raw, phi_raw, ref_img, cfg, temperature, radius=radius,
                                                 refine_temperature=refine_temperature))
        return coor_out

    def match_loss(self, ref_img, real_img, seg_map, ref_seg_map, target, temperature=0.01, *, weight=None, symmetric=True):
        """The supervised correspondence loss (hot_path.correspondence_nll, K49): `target` [B,h,w] int64 / int32 names, per content
        cell, the flat exemplar position y * w + x it should match (negative: unsupervised) — from a self-pair, keypoints, a flow field
        or the confirmed pairs of mutual_match — and the result holds the negative log-likelihood of that position under the row softmax
        (match_nll [B,h,w]) and of the content cell under the column softmax of its target (back_nll [B,h,w]), both 0 where
        unsupervised, match_lse [B,h,w] and back_lse [B,gh,gw] (mutual_match's), match_target_prob = exp(-match_nll) (detached) and
            loss_match = sum_i w_i (match_nll_i + [symmetric] back_nll_i) / max(sum of w over the supervised cells, tiny)
        with `weight` [B,h,w] fp32 >= 0 (None: 1), + loss_novgg_featpair where project() makes it.  The projection runs with gradients,
        as in sparse_warp: loss_match.backward() reaches the whole network through theta and phi, and nothing HWxHW is allocated.
        With no supervised cell the loss is 0 with zero gradients.  Scope: sparse_warp's (match_kernel 1 with PONO_C on the plain flag
        set, COCOS_PRECISION=f16x3, no prepared exemplar); everything else raises ValueError before the network runs.  forward(),
        match(), mutual_match(), sparse_warp() and flow_warp() are unaffected."""
        cfg = HotPathConfig.from_opt(self.opt, down=self.opt.down)
        _nll_scope(cfg, symmetric)                # out-of-scope flags are refused before the network runs
        if ref_img is None or ref_seg_map is None:
            raise ValueError("match_loss: ref_img and ref_seg_map are required (a prepared exemplar is out of scope)")
        if not torch.is_tensor(target) or target.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"match_loss: target must be an int32 or int64 tensor, got "
                            f"{target.dtype if torch.is_tensor(target) else type(target).__name__}")
        coor_out = {}
        theta_raw, phi_raw = self.project(ref_img, real_img, seg_map, ref_seg_map, coor_out, lazy=True)
        coor_out.update(correspondence_nll(theta_raw, phi_raw, target, cfg, temperature, weight=weight, symmetric=symmetric))
        return coor_out

    def match_loss_box3(self, ref_img, real_img, seg_map, ref_seg_map, target, temperature=0.01, *, weight=None, symmetric=True):
        """match_loss on the reference's default route, match_kernel 3 (K53, hot_path.correspondence_nll_box3): the same targets, the
        same dictionary — match_nll, back_nll [B,h,w] (0 where unsupervised), match_lse, back_lse (match()'s, bit for bit),
        match_target_prob (detached), loss_match, + loss_novgg_featpair where project() makes it — on the box logits of the 3x3-unfolded
        vectors.  loss_match.backward() reaches the whole network through theta and phi.  The x-box tensor T is kept for the backward
        and its gradient is allocated there: two HWxHW tensors, the dense match_kernel-3 step's budget.  match_nll is not clamped: on a
        one-hot row it can come out slightly negative (the target logit is fp32, the lse split-precision).  With no supervised cell
        the loss is 0 with zero gradients.  Scope: match_kernel 3 with PONO_C on the plain flag set, COCOS_PRECISION=f16x3, equal 64-
        or 128-wide grids, no prepared exemplar; everything else raises ValueError before the network runs (no fall-back).
        match_loss(), match(), forward(), sparse_warp_box3() and flow_warp_box3() are unaffected."""
        cfg = HotPathConfig.from_opt(self.opt, down=self.opt.down)
        _box3_scope("match_loss_box3", "nll_box3", cfg, False, self.inter_channels, symmetric=symmetric)      # out-of-scope flags are refused before the network runs
        if ref_img is None or ref_seg_map is None:
            raise ValueError("match_loss_box3: ref_img and ref_seg_map are required (a prepared exemplar is out of scope)")
        if not torch.is_tensor(target) or target.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"match_loss_box3: target must be an int32 or int64 tensor, got "
                            f"{target.dtype if torch.is_tensor(target) else type(target).__name__}")
        coor_out = {}
        theta_raw, phi_raw = self.project(ref_img, real_img, seg_map, ref_seg_map, coor_out, lazy=True)
        coor_out.update(correspondence_nll_box3(theta_raw, phi_raw, target, cfg, temperature, weight=weight, symmetric=symmetric))
        return coor_out


def _stored_inputs(exemplar, batch):
    """(ref_img, ref_seg_map) of a record for the ordinary route: one exemplar for all inputs is repeated"""
    ref_img, ref_seg_map = exemplar.ref_img, exemplar.ref_seg_map
    if ref_img.shape[0] != batch:
        ref_img = ref_img.expand(batch, -1, -1, -1).contiguous()
        ref_seg_map = ref_seg_map.expand(batch, -1, -1, -1).contiguous()
    return ref_img, ref_seg_map


def base_options(**overrides) -> argparse.Namespace:
    """`opt` with the defaults of options/base_options.py for every field the network reads."""
    opt = argparse.Namespace(
        semantic_nc=151, ngf=64, norm_E="spectralinstance", norm_G="spectralspadesyncbatch3x3",
        eqlr_sn=False, apex=False, PONO=False, PONO_C=False, adaptor_kernel=3, adaptor_se=False,
        adaptor_nonlocal=False, adaptor_res_deeper=False, dilation_conv=False, warp_stride=4,
        weight_domainC=0.0, domain_rela=False, use_coordconv=False, maskmix=False, warp_bilinear=False,
        mask_noise=False, noise_for_mask=False, isTrain=False, epoch=0, mask_epoch=-1,
        novgg_featpair=0.0, match_kernel=3, warp_patch=False, show_corr=False,
        warp_mask_losstype="none", show_warpmask=False, warp_cycle_w=0.0, two_cycle=False,
        CBN_intype="warp_mask", use_attention=False, init_type="xavier", init_variance=0.02,
        crop_size=256, aspect_ratio=1.0, gpu_ids=[0])
    for k, v in overrides.items():
        setattr(opt, k, v)
    return opt


def ade20k_options(**overrides) -> argparse.Namespace:
    """README.md:45 flag set: --use_attention --maskmix --warp_mask_losstype direct --PONO --PONO_C
    (label_nc 150 + dontcare -> semantic_nc 151)."""
    o = dict(semantic_nc=151, use_attention=True, maskmix=True, warp_mask_losstype="direct", PONO=True,
             PONO_C=True)
    o.update(overrides)
    return base_options(**o)


def celebahq_edge_options(**overrides) -> argparse.Namespace:
    """README.md:62,106: --use_attention --maskmix --PONO --PONO_C --warp_bilinear --adaptor_kernel 4
    (+ training: --warp_cycle_w 1); label_nc 15, no dontcare."""
    o = dict(semantic_nc=15, use_attention=True, maskmix=True, PONO=True, PONO_C=True, warp_bilinear=True,
             adaptor_kernel=4)
    o.update(overrides)
    return base_options(**o)


def deepfashion_options(**overrides) -> argparse.Namespace:
    """README.md:69,115: --use_attention --PONO --PONO_C --warp_bilinear --no_flip --warp_patch
    --video_like --adaptor_kernel 4; label_nc 20."""
    o = dict(semantic_nc=20, use_attention=True, PONO=True, PONO_C=True, warp_bilinear=True, warp_patch=True,
             adaptor_kernel=4)
    o.update(overrides)
    return base_options(**o)


def install_into_reference(networks_module):
    """Make the unmodified reference build THIS network: `networks.define_Corr(opt)` looks up a
    class named `novggcorrespondence` in `models.networks.correspondence` and asserts it subclasses
    the reference's `BaseNetwork` (networks/__init__.py:18-26,76-78).  Returns the injected class."""
    import importlib
    ref_corr = importlib.import_module(networks_module.__name__ + ".correspondence")
    base = networks_module.BaseNetwork
    cls = type("NoVGGCorrespondence", (NoVGGCorrespondence, base), {"__doc__": NoVGGCorrespondence.__doc__})
    ref_corr.NoVGGCorrespondence = cls
    return cls
