"""Host-side orchestration of the correspondence hot path (correspondence.py:271-372).

Takes the outputs of the `theta` / `phi` 1x1 convolutions and returns the reference's `coor_out`
dictionary.  Every correlation / softmax / warp product is a HIP kernel call (cocosnet_amd.ops);
the only PyTorch ops left are the tiny, shape-only ones the survey keeps on the stock backend:
avg-pool / nearest-resize of the 3..151-channel inputs, fold/unfold of patches and the final
x`down` up-sampling.

Pass structure on the fused path (K == 256).  The reference materialises f once and reuses it;
here each use is one fused launch that recomputes its logits tiles (f never reaches HBM), with all
the channel groups that share a softmax concatenated into a single V:
    R1  rows    softmax_j(f)    V = [exemplar rgb | ref_seg (direct mask)]        :318, :334
    C1  columns softmax_i(f^T)  V = [seg (cycle mask) | y (warp_cycle) | real]    :338-343, :351-367
        — the same kernel with theta/phi swapped (SURVEY.md §7 design notes)
    R2  rows    softmax_j(f)    V = [C1's mask | C1's i2r]                        :344, :369
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from . import ops


@dataclass
class HotPathConfig:
    """The `opt` fields the hot path reads, detached from argparse."""
    match_kernel: int = 3
    PONO_C: bool = False
    down: int = 4
    warp_patch: bool = False
    warp_bilinear: bool = False
    isTrain: bool = False
    show_corr: bool = False
    warp_mask_losstype: str = "none"
    show_warpmask: bool = False
    warp_cycle_w: float = 0.0
    two_cycle: bool = False

    @classmethod
    def from_opt(cls, opt, down=None):
        g = lambda k, d: getattr(opt, k, d)
        return cls(match_kernel=int(g("match_kernel", 3)), PONO_C=bool(g("PONO_C", False)),
                   down=int(down if down is not None else g("down", 4)),
                   warp_patch=bool(g("warp_patch", False)),
                   warp_bilinear=bool(g("warp_bilinear", False)), isTrain=bool(g("isTrain", False)),
                   show_corr=bool(g("show_corr", False)),
                   warp_mask_losstype=str(g("warp_mask_losstype", "none")),
                   show_warpmask=bool(g("show_warpmask", False)),
                   warp_cycle_w=float(g("warp_cycle_w", 0.0)), two_cycle=bool(g("two_cycle", False)))


class _SplitChannels(torch.autograd.Function):
    """x[:, :n], x[:, n:] whose backward is ONE concatenation of the two gradients.  Plain slicing makes autograd
    build two zero-filled full-size tensors, copy a slice into each and add them: five kernels and 100 MB of traffic
    for the 20 MB gradient of the row pass (37 us per step at the benchmark shape, now 12)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.shapes = (x.shape, int(n))
        return x[:, :n], x[:, n:]

    @staticmethod
    def backward(ctx, ga, gb):
        shape, n = ctx.shapes
        parts = []
        for g, c in ((ga, n), (gb, shape[1] - n)):
            parts.append(g if g is not None else torch.zeros((shape[0], c) + tuple(shape[2:]), device=(ga if ga is not None else gb).device,
                                                             dtype=(ga if ga is not None else gb).dtype))
        if ga is not None and gb is not None and ga.is_cuda and ga.dtype == torch.float32 and gb.dtype == torch.float32:
            return ops.concat_channels_amax(ga, gb), None      # one kernel, and max|.| for the K2 backward's f16 split
        return torch.cat(parts, dim=1), None


def _split_channels(x, n):
    return _SplitChannels.apply(x, n)


def _hip_fp32(t):
    return t is not None and t.is_cuda and t.dtype == torch.float32


def _flat(x):
    """[B,C,h,w] -> channel-major [B,C,h*w] (a view when contiguous)."""
    return x.reshape(x.shape[0], x.shape[1], -1)


def _upsample(y, down, bilinear):
    if bilinear:   # nn.Upsample(scale_factor, mode='bilinear'), align_corners=False (:184-186)
        return F.interpolate(y, scale_factor=down, mode="bilinear", align_corners=False)
    if y.is_cuda and y.dtype == torch.float32 and (y.shape[3] * down) % 4 == 0:
        return ops.upsample_nearest(y, down)                     # :188 (K11)
    return F.interpolate(y, scale_factor=down, mode="nearest")


class _Attention:
    """The two softmax directions of one correlation.  Three back ends:
       fused      K = 256 logits computed inside the kernels (match_kernel 1);
       streamed   logits materialised once per orientation, softmax + warp fused (match_kernel 3);
       generic    materialised logits -> row softmax -> GEMM (return_corr / WTA / everything else)."""

    def __init__(self, qn=None, kn=None, inv_t=1.0, f_scaled=None, logits_q=None, logits_k=None, boxed=None, planes=None):
        self.qn, self.kn, self.inv_t = qn, kn, inv_t
        self.fused = qn is not None
        self._boxed = boxed                          # match_kernel 3 fused (K19 / K20): a _BoxedCorr
        self._f = f_scaled
        self._lq, self._lk = logits_q, logits_k      # providers: query-major f / key-major f^T
        self._cache = {}
        # f16 operand planes of theta/phi, shared by the row / column / second row pass of THIS forward call
        # (per-call object: nothing is cached across calls or threads)
        self._planes = (planes if planes is not None else ops.OperandPlanes()) if self.fused else None

    def _get(self, name, fn):
        if name not in self._cache:
            self._cache[name] = fn()
        return self._cache[name]

    @property
    def f_scaled(self):
        return self._f if self._f is not None else self._get("lq", self._lq)

    def rows(self, v):
        """softmax over exemplar positions, then @ v   (f_div_C @ v, :307/:318)."""
        if isinstance(v, ops.PreparedValues):      # a record's value tensor on a back end without a native broadcast
            v = v.expanded(self._batch())
        if self.fused:
            return ops.corr_softmax_warp(self.qn, self.kn, v, self.inv_t, self._planes)
        if self._boxed is not None:
            return self._boxed.rows(v)
        if self._lk is not None:
            return ops.logits_softmax_warp(self._get("lk", self._lk), v)
        return ops.warp_materialized(self._get("p_row", lambda: ops.row_softmax(self._f)), v)

    def _batch(self):
        """B of this call, for a record's value tensor that has to be expanded"""
        if self.fused:
            return self.qn.shape[0]
        if self._boxed is not None:
            return self._boxed.th.shape[0]
        return (self._f if self._f is not None else self._get("lk" if self._lk is not None else "lq", self._lk or self._lq)).shape[0]

    def cols(self, v):
        """softmax over content positions of f^T, then @ v   (f_div_C_v @ v, :338/:351)."""
        if self.fused:
            return ops.corr_softmax_warp(self.kn, self.qn, v, self.inv_t, self._planes)
        if self._boxed is not None:
            return self._boxed.cols(v)
        if self._lq is not None:   # f itself is the key-major logit matrix of the swapped problem
            return ops.logits_softmax_warp(self._get("lq", self._lq), v)
        return ops.warp_materialized(
            self._get("p_col", lambda: ops.row_softmax(self._f.transpose(1, 2).contiguous())), v)


class _SharedAttention(_Attention):
    """The fused back end of a call with a prepared exemplar (ops.PreparedKeys): the row pass over the record's own value tensor
    reads the record's key / value planes in place (cocos_corr_softmax_warp_fwd_f16x3_shared: ONE set for all B inputs when the
    record's batch is 1).  Every other pass (cycle mask: columns, second row pass) runs the ordinary kernels over per-call
    OperandPlanes, made the first time such a pass comes: handles for qn / kn and the record's key planes, expanded to B."""

    def __init__(self, qh, ql, keys, inv_t):
        super().__init__(inv_t=inv_t)
        self._qh, self._ql, self._keys = qh, ql, keys

    def _ordinary(self):
        if not self.fused:
            B, N, C = self._qh.shape
            kh, kl, _ = self._keys.split_planes(B)
            self._planes = ops.OperandPlanes()
            # (handles: fp32 tensors that stand for the planes and are never written or read — see ops._CenterL2NormPlanes)
            self.qn = torch.empty((B, C, N), device=self._qh.device, dtype=torch.float32)
            self.kn = torch.empty((B, C, kh.shape[1]), device=self._qh.device, dtype=torch.float32)
            self._planes.put(self.qn, True, ops.SPLIT_OPERAND_SCALE, self._qh, self._ql)
            self._planes.put(self.kn, True, ops.SPLIT_OPERAND_SCALE, kh, kl)
            self.fused = True

    def rows(self, v):
        if isinstance(v, ops.PreparedValues) and v.v.shape[1] <= ops.MAX_FUSED_SPLIT_CV:
            return ops.corr_softmax_warp_shared(self._qh, self._ql, self._keys, v, self.inv_t)
        self._ordinary()
        return super().rows(v)

    def cols(self, v):
        self._ordinary()
        return super().cols(v)


class _BoxedCorr:
    """match_kernel 3, PONO_C, 64- or 128-wide grid: the statistics of the unfolded vectors (K12) and, per orientation that is
    actually used, T = xbox(C_raw) from the correlation GEMM's epilogue; every softmax + warp pass then reads T three
    blocks at a time (K19).  Nothing box-filtered and no logits matrix reaches HBM."""

    def __init__(self, theta_raw, phi_raw, inv_t, prepared_k=None, share_sink=None):
        _, C, self.fh, self.fw = theta_raw.shape
        self.kc = float(C * 9)
        self._cache = {}
        self._raw_planes = None
        if prepared_k is not None:
            # a prepared exemplar (inference only): phi's planes and (nu, b) are the record's, `phi_raw` is a handle that stands for
            # them; theta alone goes through K0, K12 and the operand split — the key side is not touched
            kh, kl, ks, nu, b = prepared_k
            if isinstance(theta_raw, ops.LazyProj1x1):
                theta_raw = theta_raw.raw()
            theta_raw = theta_raw.detach()
            B = theta_raw.shape[0]
            mu, a = ops.unfold3_stats(theta_raw, self.kc)
            tf = theta_raw.reshape(B, C, -1)
            qh, ql, qs = ops.split_f16(tf, True, amax=ops.absmax(tf))
            self._raw_planes = ops.Box3RawPlanes()
            self._raw_planes.put(theta_raw, qh, ql, None, None, qs)
            self._raw_planes.put(phi_raw, kh, kl, None, None, ks)
            self._cache["q"], self._cache["k"] = (mu, a), (nu, b)
        elif isinstance(theta_raw, ops.LazyProj1x1) and ops.proj_raw_fused_ok(theta_raw, phi_raw):
            # round 6, K25: ONE launch from the features of both tensors to the operand planes of the raw projections and the sums
            # behind K12's statistics — the fp32 projections never exist; theta_raw / phi_raw are autograd handles from here on
            self._raw_planes = ops.Box3RawPlanes()
            (theta_raw, mu, a), (phi_raw, nu, b) = ops.proj_raw_planes_stats_pair(theta_raw, phi_raw, self.kc, self._raw_planes)
            self._cache["q"], self._cache["k"] = (mu, a), (nu, b)
        elif isinstance(theta_raw, ops.LazyProj1x1):
            # round 6: projection + K12 statistics as ONE autograd node per tensor (ops.proj_unfold3_stats): its backward folds K12's
            # backward and the sum of theta_raw's two gradients into the projection's input gradient (K24)
            if ops.PROJ_PRECISION == "f16x3":      # max|.| of both feature tensors and both weights in one launch
                # (a projection with a frozen record brings its weight's cell: only the features are measured)
                ops.prefetch_amax([theta_raw.x, None if theta_raw.prepared is not None else theta_raw.weight.reshape(C, -1),
                                   phi_raw.x, None if phi_raw.prepared is not None else phi_raw.weight.reshape(C, -1)])
            theta_raw, mu, a = ops.proj_unfold3_stats(theta_raw, self.kc)
            phi_raw, nu, b = ops.proj_unfold3_stats(phi_raw, self.kc)
            self._cache["q"], self._cache["k"] = (mu, a), (nu, b)
        self.th, self.ph, self.inv_t = theta_raw, phi_raw, inv_t
        # round 4: ONE T for both orientations (xbox(C)^T = xbox(C^T): the column pass reads it transposed) and one gradient
        # buffer for all passes over it — no second correlation GEMM, one box adjoint and one pair of GEMMs in the backward
        # (`share_sink`: None = the ops.BOX3_SHARE_T switch; True: always, for a caller whose passes are made to share one G — K53)
        self._sink = ops.Box3GradSink() if (ops.BOX3_SHARE_T if share_sink is None else share_sink) else None

    def _get(self, name, fn):
        if name not in self._cache:
            self._cache[name] = fn()
        return self._cache[name]

    def _t(self):
        """T = xbox(C_raw) of the row orientation, made once: every pass and every readout reads it (the column direction transposed)"""
        return self._get("t_rows", lambda: ops.box3_corr_xbox(self.th, self.ph, self._sink, self._raw_planes))

    def stats(self):
        """((mu, a), (nu, b)) of theta and phi, with autograd where the operands carry it"""
        return self._get("q", lambda: _unfold3_stats(self.th, self.kc)), self._get("k", lambda: _unfold3_stats(self.ph, self.kc))

    def _sides(self, rows: bool):
        """(the statistics of the side that asks, of the other side, T): theta's first for rows, phi's otherwise — T is then read
        transposed"""
        q, k = self.stats()
        return (q, k, self._t()) if rows else (k, q, self._t())

    def rows(self, v):
        q, k, t = self._sides(True)
        return ops.box3_softmax_warp(t, *q, *k, v, self.fh, self.fw, self.kc, self.inv_t, sink=self._sink)

    def cols(self, v):   # the same operator with the roles of theta and phi exchanged
        if self._sink is not None:
            q, k, t = self._sides(False)
            return ops.box3_softmax_warp(t, *q, *k, v, self.fh, self.fw, self.kc, self.inv_t, transposed=True, sink=self._sink)
        (mu, a), (nu, b) = self.stats()
        t = self._get("t_cols", lambda: ops.box3_corr_xbox(self.ph, self.th, None, self._raw_planes))
        return ops.box3_softmax_warp(t, nu, b, mu, a, v, self.fh, self.fw, self.kc, self.inv_t)

    def match(self, rows: bool, k: int = 1):
        """(idx int32, max, lse) [B,N] of the rows of the logits (rows) or of their transpose (not rows): K37 on the row pass's T —
        read transposed for the column direction, with or without a gradient sink (nothing is differentiated).  k > 1: the k best
        per row, (idx [B,N,k], val [B,N,k], lse [B,N]), from K41 on the same T and the same cached statistics."""
        q, kk, t = self._sides(rows)
        if k == 1:
            return ops.box3_match(t, *q, *kk, self.fh, self.fw, self.kc, self.inv_t, transposed=not rows)
        return ops.box3_topk(t, *q, *kk, self.fh, self.fw, self.kc, self.inv_t, k, transposed=not rows)

    def match_biased(self, rows: bool, bias, k: int = 1):
        """match(rows, k) over z + bias[key] (K54, ops.box3_topk_biased) -> (idx [B,N,k], val, lse), on the same T and the same cached
        statistics; `bias` [B,N] fp32 belongs to the keys of the direction read (phi's positions for rows, theta's otherwise)"""
        q, kk, t = self._sides(rows)
        return ops.box3_topk_biased(t, *q, *kk, bias, self.fh, self.fw, self.kc, self.inv_t, k, transposed=not rows)

    def match_labelled(self, rows: bool, q_label, k_label, k: int = 1):
        """match(rows, k) over the keys each query's label allows (K55, ops.box3_topk_labelled) -> (idx [B,N,k], val, lse), on the same
        T and the same cached statistics; q_label [B,N] belongs to the positions that ask in the direction read (theta's for rows,
        phi's otherwise), k_label to the other side: the caller passes them in that order, statistics and T's orientation follow"""
        q, kk, t = self._sides(rows)
        return ops.box3_topk_labelled(t, *q, *kk, q_label, k_label, self.fh, self.fw, self.kc, self.inv_t, k, transposed=not rows)

    def sinkhorn(self, iters: int, tau: float = 1.0, readout: bool = False):
        """(f, g, row_lse) [B,N] of ops.box3_sinkhorn on the row pass's T and the cached statistics (K54): 2 iters + 1 launches, no
        second correlation GEMM.  `readout`: (f, g, idx [B,N,1], val [B,N,1], row_lse) — the last launch is the k = 1 readout of z + g"""
        iters, tau = ops._sinkhorn_args("box3_sinkhorn", iters, tau)
        q, kk, t = self._sides(True)
        out = ops._box3_sinkhorn_readout(t, *q, *kk, self.fh, self.fw, self.kc, self.inv_t, iters, tau)
        return out if readout else (out[0], out[1], out[4])

    def lse(self, rows: bool):
        """match(rows)'s lse [B,N] bit for bit, WITH a gradient (K53, ops.box3_lse): the passes over the one T share its gradient sink"""
        q, kk, t = self._sides(rows)
        return ops.box3_lse(t, *q, *kk, self.fh, self.fw, self.kc, self.inv_t, transposed=not rows, sink=self._sink)


def _box_sum3(x):
    """zero-padded 3x3 box SUM of a [B,1,h,w] map."""
    return F.avg_pool2d(x, 3, stride=1, padding=1, divisor_override=1)


def _unfold3_stats(x_raw, k_unfolded):
    """mean and 1/(norm+eps) of the zero-padded 3x3-unfolded, centred vectors of x_raw [B,C,h,w]
    WITHOUT unfolding: box sums of the per-position channel sums / sums of squares (:276-280)."""
    if x_raw.is_cuda and x_raw.dtype == torch.float32:
        return ops.unfold3_stats(x_raw, k_unfolded)                  # K12: one pass over x, fwd and bwd
    s1 = x_raw.sum(dim=1, keepdim=True)
    s2 = (x_raw * x_raw).sum(dim=1, keepdim=True)
    mu = _box_sum3(s1) / k_unfolded
    nrm = torch.sqrt(torch.clamp(_box_sum3(s2) - k_unfolded * mu * mu, min=0.0))
    B = x_raw.shape[0]
    return mu.reshape(B, -1), (1.0 / (nrm + ops.NORM_EPS)).reshape(B, -1)


def _box3_logits(theta_raw, phi_raw, scale, transposed=False):
    """match_kernel 3, PONO_C: f (or f^T) * scale from the K = 256 correlation, no unfold (K6)."""
    B, C, fh, fw = theta_raw.shape
    kc = float(C * 9)
    mu, a = _unfold3_stats(theta_raw, kc)
    nu, b = _unfold3_stats(phi_raw, kc)
    if transposed:   # f^T[q,p]: the same operator with the roles of theta and phi exchanged
        c_raw = ops.corr_materialize(_flat(phi_raw), _flat(theta_raw), 1.0)
        return ops.box3_logits(c_raw, nu, mu, b, a, fh, fw, kc, scale)
    c_raw = ops.corr_materialize(_flat(theta_raw), _flat(phi_raw), 1.0)
    return ops.box3_logits(c_raw, mu, nu, a, b, fh, fw, kc, scale)


def _scaled_logits(theta_raw, phi_raw, cfg, inv_t, detach_flag, wta):
    """Materialised, query-major f_WTA / temperature (:272-304) for the generic back end."""
    mk = cfg.match_kernel
    wta_on = wta != 1
    pre_scaled = not (wta_on or detach_flag)
    if mk == 3 and cfg.PONO_C:
        f = _box3_logits(theta_raw, phi_raw, inv_t if pre_scaled else 1.0)
    else:
        if mk == 1:
            theta, phi = _flat(theta_raw), _flat(phi_raw)
        else:
            theta = F.unfold(theta_raw, kernel_size=mk, padding=mk // 2)
            phi = F.unfold(phi_raw, kernel_size=mk, padding=mk // 2)
        qn = ops.center_l2norm(theta, cfg.PONO_C)
        kn = ops.center_l2norm(phi, cfg.PONO_C)
        f = ops.corr_materialize(qn, kn, inv_t if pre_scaled else 1.0)      # :291 (+ :304)
    if pre_scaled:
        return f
    if detach_flag:                                                          # :292-293
        f = f.detach()
    if wta_on:
        return ops.wta_scale(f, wta, inv_t)                                  # :300-303 + :304 (K8)
    return f * inv_t                                                         # :304 (detached: no graph)


def _row_values(ref_img, ref_seg_map, down, patch, direct_mask, fused_values):
    """(V of the row pass [B,Cv,HW], number of image channels): pooled exemplar (or its patches) + the sampled direct mask"""
    if fused_values:
        # pooled image (or its patches, --warp_patch) + sampled mask in one kernel (K14)
        v1 = _flat(ops.warp_values(ref_img, ref_seg_map if direct_mask else None, down, patch=patch))
        return v1, ref_img.shape[1] * (down * down if patch else 1)
    if patch:
        ref = F.unfold(ref_img, down, stride=down)                    # [B, 3*down^2, HW]
    else:
        ref = _flat(F.avg_pool2d(ref_img, down))                      # [B, 3, HW]
    v_r1 = [ref]
    if direct_mask:
        ref_seg = F.interpolate(ref_seg_map, scale_factor=1 / down, mode="nearest")
        v_r1.append(_flat(ref_seg))
    return (torch.cat(v_r1, dim=1) if len(v_r1) > 1 else ref), ref.shape[1]


def _fused_values_ok(ref_img, ref_seg_map, down, patch, direct_mask, modes):
    H, W = ref_img.shape[2], ref_img.shape[3]
    return bool((modes or (direct_mask and not patch)) and _hip_fp32(ref_img) and not ref_img.requires_grad
                and (not direct_mask or (_hip_fp32(ref_seg_map) and not ref_seg_map.requires_grad))
                and H % down == 0 and W % down == 0)


def exemplar_values(ref_img, ref_seg_map, down, patch, direct_mask) -> "ops.PreparedValues":
    """The row pass's value tensor as a prepared exemplar keeps it (inference.PreparedExemplar): the same tensor the ordinary route
    forms per call (its max|v| cell is taken when the split flavour first asks for the planes)."""
    modes = ops.WARP_HEAD_MODES and _hip_fp32(ref_img)
    v1, n_ref = _row_values(ref_img, ref_seg_map, down, patch, direct_mask,
                            _fused_values_ok(ref_img, ref_seg_map, down, patch, direct_mask, modes))
    v1 = v1.contiguous()
    return ops.PreparedValues(v1, n_ref)


def _attention_with_exemplar(theta_raw, keys, cfg, inv_t, WTA_scale_weight, return_corr):
    """The _Attention of a forward call whose exemplar side is a record (ops.PreparedKeys): the query side is made here, per call;
    key planes / statistics / phi_raw come from the record — in place on the fused match_kernel-1 back end (any record batch),
    expanded to B once per record on the others."""
    B, C, fh, fw = theta_raw.shape
    N = fh * fw
    mk = cfg.match_kernel
    keys.check(B)
    if keys.shape[1:] != theta_raw.shape[1:]:
        raise ValueError(f"prepared exemplar: feature grid {tuple(keys.shape)} does not match the content's {tuple(theta_raw.shape)}")
    plain = WTA_scale_weight == 1 and not return_corr
    if (mk == 1 and C == ops.FUSED_K and plain and cfg.PONO_C and _hip_fp32(theta_raw)
            and ops.corr_split_ok(B, C, N, N, 1, False)):
        if isinstance(theta_raw, ops.LazyProj1x1) and ops.proj_norm_fused_ok(theta_raw):
            qh, ql, _ = ops.proj_center_l2norm_planes_one(theta_raw, 1)      # K23, theta alone
        else:
            th = theta_raw.raw() if isinstance(theta_raw, ops.LazyProj1x1) else theta_raw
            qh, ql, _ = ops.center_l2norm_planes_fwd(_flat(th), 1)
        return _SharedAttention(qh, ql, keys, inv_t)
    theta = theta_raw.raw() if isinstance(theta_raw, ops.LazyProj1x1) else theta_raw
    if mk == 3 and cfg.PONO_C and plain and _hip_fp32(theta) and ops.box3_fused_ok(B, C, fh, fw):
        pk = keys.box_planes(B)
        theta = theta.detach()
        ph = theta.view_as(theta)      # a handle for phi's planes (another object of theta's shape, no memory): never read
        return _Attention(inv_t=inv_t, boxed=_BoxedCorr(theta, ph, inv_t, prepared_k=pk))
    return None      # every other back end reads phi_raw as fp32: the caller continues on the ordinary route with keys.phi_raw(B)


def correspondence_hot_path(theta_raw, phi_raw, ref_img, real_img, seg_map, ref_seg_map,
                            cfg: HotPathConfig, temperature=0.01, detach_flag=False,
                            WTA_scale_weight=1, return_corr=False, *, exemplar=None):
    """correspondence.py:272-372 from the theta/phi conv outputs onward.

    theta_raw, phi_raw: [B,256,h,w] CUDA fp32.  Returns the `coor_out` dict of the reference
    (or the scaled correlation [B,HW,HW] when return_corr, :305-306).

    `exemplar`: the ops.PreparedKeys of a prepared exemplar (inference.PreparedExemplar) IN PLACE of phi_raw, ref_img and
    ref_seg_map (all three None): the key side and the row pass's value tensor are the record's.  Forward only (no autograd
    graph is built)."""
    B, C, fh, fw = theta_raw.shape
    down, mk = cfg.down, cfg.match_kernel
    attn = None
    if exemplar is not None:
        if phi_raw is not None or ref_img is not None or ref_seg_map is not None:
            raise ValueError("correspondence_hot_path: a prepared exemplar stands in place of phi_raw, ref_img and ref_seg_map")
        if torch.is_grad_enabled():      # (which configurations may use a record at all: NoVGGCorrespondence._check_exemplar)
            raise ValueError("correspondence_hot_path: a prepared exemplar is forward-only (call under torch.no_grad())")
        H, W = exemplar.image_size
        attn = _attention_with_exemplar(theta_raw, exemplar, cfg, 1.0 / temperature, WTA_scale_weight, return_corr)
        if attn is None:
            theta_raw = theta_raw.raw() if isinstance(theta_raw, ops.LazyProj1x1) else theta_raw
            phi_raw = exemplar.phi_raw(B)
    else:
        H, W = ref_img.shape[2], ref_img.shape[3]
    out = {}

    inv_t = 1.0 / temperature
    fused = (mk == 1) and (C == ops.FUSED_K) and WTA_scale_weight == 1 and not return_corr
    # round 6: theta / phi may arrive as LAZY projections (ops.LazyProj1x1: the 1x1 convolutions of :272 / :282 not run yet).  On the
    # fused match_kernel-1 / PONO_C path K23 then goes from the features straight to the correlation kernels' operand planes
    # (projection + centring + normalisation in one launch for both tensors: the fp32 projections never exist); every other
    # back end asks for the projections (K0) and continues as before.
    lazy = attn is None and isinstance(theta_raw, ops.LazyProj1x1) and isinstance(phi_raw, ops.LazyProj1x1)
    if attn is None and lazy != (isinstance(theta_raw, ops.LazyProj1x1) or isinstance(phi_raw, ops.LazyProj1x1)):
        raise TypeError("correspondence_hot_path: theta and phi must both be tensors or both be ops.LazyProj1x1")
    k23 = boxed_lazy = False
    if lazy:
        keep = torch.is_grad_enabled() and not detach_flag and (theta_raw.requires_grad or phi_raw.requires_grad)
        k23 = (fused and cfg.PONO_C and theta_raw.x.shape == phi_raw.x.shape and ops.proj_norm_fused_ok(theta_raw)
               and ops.proj_norm_fused_ok(phi_raw) and ops.corr_split_ok(B, C, fh * fw, fh * fw, 1, keep))
        # match_kernel 3, fused family: the projections stay lazy up to _BoxedCorr, which makes (theta_raw, mu, a) in one autograd node
        boxed_lazy = (mk == 3 and cfg.PONO_C and WTA_scale_weight == 1 and not return_corr and _hip_fp32(theta_raw)
                      and ops.PROJ_BWD_FUSED and ops.box3_fused_ok(B, C, fh, fw))
        if not (k23 or boxed_lazy):
            theta_raw, phi_raw = theta_raw.raw(), phi_raw.raw()
    if attn is not None:
        pass      # (a prepared exemplar's: made above)
    elif k23:
        th_l, ph_l = (theta_raw.detach(), phi_raw.detach()) if detach_flag else (theta_raw, phi_raw)   # :292-293 `f = f.detach()`
        planes = ops.OperandPlanes()
        qn, kn = ops.proj_center_l2norm_planes_pair(th_l, ph_l, 1, planes, want_chan=keep)
        attn = _Attention(qn=qn, kn=kn, inv_t=inv_t, planes=planes)
    elif fused:
        # :272-289 — flatten, centre, L2-normalise; the rest happens inside the fused kernels
        th_f, ph_f = _flat(theta_raw), _flat(phi_raw)
        if detach_flag:   # :292-293 `f = f.detach()`: nothing upstream of f receives a gradient
            th_f, ph_f = th_f.detach(), ph_f.detach()
        keep = torch.is_grad_enabled() and (th_f.requires_grad or ph_f.requires_grad)
        planes = ops.OperandPlanes()
        if (cfg.PONO_C and _hip_fp32(theta_raw)
                and ops.corr_split_ok(B, C, fh * fw, fh * fw, 1, keep)):
            # K1 writes the operand planes of the split kernels itself: fp32 qn / kn never exist (ops.center_l2norm_planes)
            # (channel-major planes of BOTH operands whenever either is differentiated: the K2 backward reads both)
            qn = ops.center_l2norm_planes(th_f, 1, planes, want_chan=keep)
            kn = ops.center_l2norm_planes(ph_f, 1, planes, want_chan=keep)
        else:
            qn = ops.center_l2norm(th_f, cfg.PONO_C)
            kn = ops.center_l2norm(ph_f, cfg.PONO_C)
        attn = _Attention(qn=qn, kn=kn, inv_t=inv_t, planes=planes)
    elif (mk == 3 and cfg.PONO_C and WTA_scale_weight == 1 and not return_corr and _hip_fp32(theta_raw)
          and ops.box3_fused_ok(B, C, fh, fw)):
        # the reference's default: 3x3 neighbourhoods, fused (round 3): x box in the correlation GEMM, y box + softmax + warp
        # in one kernel — see _BoxedCorr
        th, ph = (theta_raw.detach(), phi_raw.detach()) if detach_flag else (theta_raw, phi_raw)
        attn = _Attention(inv_t=inv_t, boxed=_BoxedCorr(th, ph, inv_t))
    elif mk == 3 and cfg.PONO_C and WTA_scale_weight == 1:
        # every other shape / the exact-fp32 flavour: logits = diagonal box filter of the K = 256
        # correlation, materialised once per orientation that is actually used, then streamed.
        th, ph = (theta_raw.detach(), phi_raw.detach()) if detach_flag else (theta_raw, phi_raw)
        attn = _Attention(inv_t=inv_t,
                          logits_q=lambda: _box3_logits(th, ph, inv_t, transposed=False),
                          logits_k=lambda: _box3_logits(th, ph, inv_t, transposed=True))
    else:
        attn = _Attention(inv_t=inv_t,
                          f_scaled=_scaled_logits(theta_raw, phi_raw, cfg, inv_t, detach_flag, WTA_scale_weight))
    if return_corr:
        return attn.f_scaled

    # ---- R1: exemplar colours (+ direct mask) through the row softmax  (:309-336) ----------------
    direct_mask = cfg.warp_mask_losstype == "direct" or cfg.show_warpmask
    if exemplar is not None:
        modes = ops.WARP_HEAD_MODES and _hip_fp32(theta_raw)
        v1 = exemplar.values(down, cfg.warp_patch, direct_mask)      # an ops.PreparedValues: _Attention.rows knows it
        n_ref = v1.n_ref
    else:
        # K30: the head and the value kernels on every flag set (ops.WARP_HEAD_MODES; CPU / non-fp32 tensors keep the framework route)
        modes = ops.WARP_HEAD_MODES and _hip_fp32(theta_raw) and _hip_fp32(ref_img)
        v1, n_ref = _row_values(ref_img, ref_seg_map, down, cfg.warp_patch, direct_mask,
                                _fused_values_ok(ref_img, ref_seg_map, down, cfg.warp_patch, direct_mask, modes))
    o_r1 = attn.rows(v1)
    want_cycle = cfg.warp_cycle_w > 0
    show_bi = (not cfg.isTrain) and cfg.show_corr
    # round 6: when the row pass's output goes to the up-sampling and the direct mask and nowhere else, both come from one op whose
    # backward hands the K2 / K19 backward its d out, max|d out| and D in ONE kernel (ops.warp_head).  K30: the same op up-samples
    # bilinearly or folds patches, works without mask channels, and with cycle terms also returns the image channels as a view whose
    # gradient (from the column pass) its backward adds in the same pass.
    head_mode = "patch" if cfg.warp_patch else ("bilinear" if cfg.warp_bilinear else "nearest")
    if modes:
        head = (ops.warp_head_ok(o_r1, n_ref, fh, fw, down, head_mode) and (fh * down, fw * down) == (H, W)
                and (direct_mask or n_ref == o_r1.shape[1]))
    else:
        head = (direct_mask and not cfg.warp_patch and not cfg.warp_bilinear and not want_cycle
                and not show_bi and ops.warp_head_ok(o_r1, n_ref, fh, fw, down) and n_ref < o_r1.shape[1])
    if head:
        want_bi = show_bi and head_mode == "nearest"
        res = ops.warp_head(o_r1, n_ref, fh, fw, down, mode=head_mode, want_y=want_cycle, want_bi=want_bi)
        if show_bi:               # (bilinear / patch mode: warp_out is the side output already, :326-327)
            out["warp_out_bi"] = res[-1] if want_bi else res[0]
        out["warp_out"] = y_img = res[0]
        if direct_mask:
            out["warp_mask"] = res[1]
        y = res[2] if want_cycle else None
    else:
        y, o_mask = _split_channels(o_r1, n_ref) if direct_mask else (o_r1, None)   # [B, ch, HW], [B, nc, HW]
        if cfg.warp_patch:
            y_img = F.fold(y, (H, W), down, stride=down)                  # reference hard-codes 256 (:321)
        else:
            y_img = y.reshape(B, n_ref, fh, fw)
        if show_bi:
            out["warp_out_bi"] = y_img if cfg.warp_patch else _upsample(y_img, down, True)
        out["warp_out"] = y_img if cfg.warp_patch else _upsample(y_img, down, cfg.warp_bilinear)
        if direct_mask:
            out["warp_mask"] = o_mask.reshape(B, -1, fh, fw)

    # ---- C1: everything that goes through the column softmax  (:337-343, :350-367) ---------------
    cycle_mask = (not direct_mask) and cfg.warp_mask_losstype == "cycle"
    want_two = want_cycle and cfg.two_cycle and not cfg.warp_patch
    v_c1, names = [], []
    if cycle_mask:
        seg = F.interpolate(seg_map, scale_factor=1 / down, mode="nearest")
        v_c1.append(_flat(seg)); names.append("mask")
    if want_cycle:
        # (:353 unfolds the fold of y: non-overlapping patches, so that is y itself, bit for bit)
        yy = F.unfold(y_img, down, stride=down) if cfg.warp_patch and not modes else y
        v_c1.append(yy); names.append("cycle")
    if want_two:
        if modes and _hip_fp32(real_img) and not real_img.requires_grad and H % down == 0 and W % down == 0:
            v_c1.append(_flat(ops.warp_values(real_img, None, down))); names.append("i2r")
        else:
            v_c1.append(_flat(F.avg_pool2d(real_img, down))); names.append("i2r")
    if v_c1:
        o_c1 = attn.cols(torch.cat(v_c1, dim=1) if len(v_c1) > 1 else v_c1[0])
        # K30: the fold of the column pass's output (:357) is the head in patch mode without mask channels — its backward leaves
        # d o, max|d o| and D for the column pass's backward
        cycle_head = (modes and cfg.warp_patch and names == ["cycle"] and (fh * down, fw * down) == (H, W)
                      and ops.warp_head_ok(o_c1, o_c1.shape[1], fh, fw, down, "patch"))
        if cycle_head:
            parts = {"cycle": o_c1}
        else:
            parts = dict(zip(names, torch.split(o_c1, [t.shape[1] for t in v_c1], dim=1)))
        if want_cycle:
            wc = parts["cycle"]
            if cycle_head:
                out["warp_cycle"] = ops.warp_head(wc, wc.shape[1], fh, fw, down, mode="patch")[0]
            else:
                out["warp_cycle"] = (F.fold(wc, (H, W), down, stride=down) if cfg.warp_patch
                                     else wc.reshape(B, -1, fh, fw))
        if want_two:
            out["warp_i2r"] = parts["i2r"].reshape(B, -1, fh, fw)

        # ---- R2: second trip through the row softmax  (:344, :369) --------------------------------
        v_r2 = [parts[n] for n in ("mask", "i2r") if n in parts]
        if v_r2:
            o_r2 = attn.rows(torch.cat(v_r2, dim=1) if len(v_r2) > 1 else v_r2[0])
            pos = 0
            if cycle_mask:
                nm = parts["mask"].shape[1]
                out["warp_mask"] = o_r2[:, :nm].reshape(B, nm, fh, fw)
                pos = nm
            if want_two:
                out["warp_i2r2i"] = o_r2[:, pos:].reshape(B, -1, fh, fw)
    return out


# ---- K36: match readout ---------------------------------------------------------------------------------------------------------
@dataclass
class MatchReadout:
    """Where every position matched and how sure the match is (correspondence_match): per position of the [fh, fw] grid of the
    side that asks, `index` the flat position y * gw + x of its best match on the other side's [gh, gw] grid (int64), `max_logit`
    the logit of that match (cosine / temperature), `lse` the log-sum-exp of the position's logits and `prob` = exp(max_logit - lse),
    the match's softmax weight — each [B,fh,fw]."""
    index: torch.Tensor
    prob: torch.Tensor
    max_logit: torch.Tensor
    lse: torch.Tensor
    grid: tuple = None      # (gh, gw) of the side the indices point into; None = the same as index.shape[1:]
    # with refine = r > 0 (K44): `offset` [B,2,fh,fw] the (x, y) soft-argmax offset, in cells, over the (2 r + 1)^2 window of the other
    # side's grid around the match; `window_prob` [B,fh,fw] = exp(lse_win - lse), the share of the position's full softmax mass that
    # lies in the window (meaningful when the refinement runs at the readout's temperature)
    offset: torch.Tensor = None
    window_prob: torch.Tensor = None
    # with restrict (K47): bool [B,fh,fw], the positions whose candidates were restricted to their label (the others fell back to
    # the scan over all positions); index, prob, max_logit and lse are then over the allowed set
    restricted: torch.Tensor = None

    def xy(self):
        """[B,2,fh,fw] int64: (x, y) of the match on the other side's grid — index = y * gw + x"""
        gw = (self.grid or tuple(self.index.shape[1:]))[1]
        return torch.stack((self.index % gw, torch.div(self.index, gw, rounding_mode="floor")), dim=1)

    def xy_sub(self):
        """[B,2,fh,fw] fp32: the sub-cell position xy() + offset (a readout made with refine > 0)"""
        if self.offset is None:
            raise ValueError("MatchReadout.xy_sub: the readout holds no offset (correspondence_match(refine=r > 0) makes one)")
        return self.xy().float() + self.offset


@dataclass
class TopkMatchReadout:
    """The k best candidates of every position (correspondence_match with topk = k > 1), best first — logit descending and, among
    bitwise-equal logits, the lower index first: `index` [B,k,fh,fw] int64 the flat positions y * gw + x on the other side's
    [gh, gw] grid (pairwise distinct per position for finite input), `logit` [B,k,fh,fw] their logits (cosine / temperature),
    `prob` = exp(logit - lse) their softmax weights (they sum to <= 1 over k), `lse` [B,fh,fw] the log-sum-exp of ALL of the
    position's logits.  Rank 0 is what MatchReadout holds."""
    index: torch.Tensor
    prob: torch.Tensor
    logit: torch.Tensor
    lse: torch.Tensor
    grid: tuple = None      # (gh, gw) of the side the indices point into; None = the same as index.shape[2:]
    restricted: torch.Tensor = None     # with restrict (K47): as MatchReadout.restricted; prob and lse are over the allowed set

    def xy(self):
        """[B,k,2,fh,fw] int64: (x, y) of every candidate on the other side's grid — index = y * gw + x"""
        gw = (self.grid or tuple(self.index.shape[2:]))[1]
        return torch.stack((self.index % gw, torch.div(self.index, gw, rounding_mode="floor")), dim=2)


# ---- what the family's entry points share: argument checks, the fused-route scope, the operand planes, the readouts ----------------
#: why each member refuses what lies off the fused match_kernel-1 route: the sentence its scope messages end in (_route_scope)
_ROUTE = {"refine": ": the sub-cell refinement (refine > 0) runs on the fused match_kernel 1 route only",
          "restrict": ": restrict runs on the fused match_kernel 1 route only",
          "sparse": " (the sparse warp runs on the fused match_kernel 1 route)",
          "nll": " (the loss runs on the fused match_kernel 1 route)",
          "transport": " (transport runs on the fused match_kernel 1 route)",
          "sparse_box3": " (the box sparse warp runs on the match_kernel 3 route)",
          "flow_box3": " (the box sub-cell flow runs on the match_kernel 3 route)",
          "nll_box3": " (the box match loss runs on the match_kernel 3 route)",
          "transport_box3": " (box transport runs on the match_kernel 3 route)",
          "restrict_box3": " (the box restrict runs on the match_kernel 3 route)"}


def _route_scope(name: str, cfg: HotPathConfig, member: str, *, plain_flags: bool, match_fused: bool, kernel: int = 1):
    """ValueError for a flag set off the fused match_kernel-1 route (`kernel` = 3: the match_kernel-3 route of K51), in this order:
    match_kernel, PONO_C, with `plain_flags` the warp modes and the cycle terms, COCOS_PRECISION, with `match_fused` the
    ops.MATCH_FUSED switch; every message ends in _ROUTE[member]"""
    route = _ROUTE[member]
    if cfg.match_kernel != kernel:
        raise ValueError(f"{name}: match_kernel {cfg.match_kernel} is out of scope{route}")
    if not cfg.PONO_C:
        raise ValueError(f"{name}: needs PONO_C{route}")
    if plain_flags:
        for flag in ("warp_patch", "warp_bilinear"):
            if getattr(cfg, flag):
                raise ValueError(f"{name}: {flag} is out of scope{route}")
        if cfg.warp_cycle_w > 0 or cfg.two_cycle or cfg.warp_mask_losstype == "cycle":
            raise ValueError(f"{name}: the cycle terms (warp_cycle_w, two_cycle, warp_mask_losstype='cycle') are out of scope{route}")
    if ops.PRECISION != "f16x3":
        raise ValueError(f"{name}: COCOS_PRECISION={ops.PRECISION} is out of scope{route}")
    if match_fused and not ops.MATCH_FUSED:
        raise ValueError(f"{name}: ops.MATCH_FUSED = False (the materialised readout) is out of scope{route}")


def _route_channels(name: str, member: str, channels):
    if channels is not None and channels != ops.FUSED_K:
        raise ValueError(f"{name}: needs {ops.FUSED_K} channels, got {channels}{_ROUTE[member]}")


_EXEMPLAR_FWD_ONLY = "a prepared exemplar is out of scope (it is forward-only; the {} differentiates phi)"
#: the match_kernel-3 members (K51 - K55): what its route messages carry after the name, whether ops.MATCH_FUSED belongs to the scope,
#: why a prepared exemplar is refused (None: the member takes no such argument), the member's own arguments checked before the flag
#: set and after the channels (_BOX3_ARG)
_BOX3_MEMBER = {"sparse_box3": ("", False, _EXEMPLAR_FWD_ONLY.format("sparse warp"), ("topk",), ()),
                "flow_box3": ("", False, _EXEMPLAR_FWD_ONLY.format("refinement"), (), ("radius", "refine_temperature")),
                "nll_box3": ("", False, _EXEMPLAR_FWD_ONLY.format("loss"), ("symmetric",), ()),
                "transport_box3": (": transport", True, "transport with a prepared exemplar is out of scope (not built)"
                                   + _ROUTE["transport_box3"], ("topk", "sinkhorn"), ()),
                "restrict_box3": (": restrict", True, None, ("restrict", "transport"), ())}


def _topk_arg(name: str, topk):
    if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= ops.MATCH_TOPK_MAX:
        raise ValueError(f"{name}: topk={topk!r}: expected an integer in 1..{ops.MATCH_TOPK_MAX}")
    return topk


def _refine_temperature_arg(name: str, refine_temperature):
    if refine_temperature is not None and not (isinstance(refine_temperature, (int, float)) and not isinstance(refine_temperature, bool)
                                               and refine_temperature > 0):
        raise ValueError(f"{name}: refine_temperature={refine_temperature!r}: expected a positive number (None: the readout's temperature)")


def _radius_arg(name: str, radius):
    top = ops.MATCH_REFINE_MAX_RADIUS
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= top:
        raise ValueError(f"{name}: radius={radius!r}: expected an integer in 1..{top}")


def _symmetric_arg(name: str, symmetric):
    if not isinstance(symmetric, bool):
        raise ValueError(f"{name}: symmetric={symmetric!r}: expected True or False")


def _restrict_arg(name: str, restrict):
    """ValueError for a `restrict` that is neither "label" nor a pair of tensors, TypeError for a pair of another dtype"""
    pair = isinstance(restrict, (tuple, list)) and len(restrict) == 2 and all(torch.is_tensor(t) for t in restrict)
    if not (pair or (isinstance(restrict, str) and restrict == "label")):
        what = repr(restrict) if isinstance(restrict, str) else type(restrict).__name__
        raise ValueError(f"{name}: restrict={what}: expected None, 'label' or a pair (q_labels, k_labels) of integer tensors")
    if pair and any(t.dtype not in (torch.int32, torch.int64) for t in restrict):
        raise TypeError(f"{name}: restrict: the labels must be int32 or int64 tensors, got {restrict[0].dtype} and {restrict[1].dtype}")


def _no_transport_arg(name: str, transport):
    if transport is not None:
        raise ValueError(f"{name}: restrict with transport is out of scope (not built){_ROUTE['restrict_box3']}")


#: the checks of the members' own arguments: (name, value) -> what the caller goes on with, or None
_BOX3_ARG = {"topk": _topk_arg, "radius": _radius_arg, "refine_temperature": _refine_temperature_arg, "symmetric": _symmetric_arg,
             "sinkhorn": lambda name, v: ops._sinkhorn_args(f"{name}: transport", *v), "restrict": _restrict_arg,
             "transport": _no_transport_arg}


def _box3_scope(name: str, member: str, cfg: HotPathConfig, has_exemplar: bool = False, channels=None, *, plain_flags: bool = True, **args):
    """ValueError (TypeError for labels of another dtype) for everything outside the scope of a match_kernel-3 member, before any
    tensor is looked at, in _BOX3_MEMBER[member]'s order: the member's own arguments (`args`, by name), the flag set (_route_scope
    with kernel = 3: match_kernel 3, PONO_C, with `plain_flags` the plain flags, COCOS_PRECISION=f16x3, ops.MATCH_FUSED where it
    belongs), a prepared exemplar, the channels (`channels` may be a callable: no tensor is looked at before this step), the arguments
    that come last -> {argument: what its check returned}"""
    tag, match_fused, no_exemplar, before, after = _BOX3_MEMBER[member]
    got = {a: _BOX3_ARG[a](name, args[a]) for a in before}
    _route_scope(name + tag, cfg, member, plain_flags=plain_flags, match_fused=match_fused, kernel=3)
    if has_exemplar and no_exemplar is not None:
        raise ValueError(f"{name}: {no_exemplar}")
    _route_channels(name + tag, member, channels() if callable(channels) else channels)
    got.update({a: _BOX3_ARG[a](name, args[a]) for a in after})
    return got


def _box3_fused_shapes(name: str, member: str, B, C, fh, fw, gh, gw, k=1):
    """ValueError unless the grids are equal, ops.box3_fused_ok takes them and ops.box3_topk_ok serves k: the members that read T have
    no materialised fall-back"""
    if (gh, gw) != (fh, fw) or not ops.box3_fused_ok(B, C, fh, fw) or not ops.box3_topk_ok(k):
        raise ValueError(f"{name}{_BOX3_MEMBER[member][0]}: the fused box route does not take a {fh}x{fw} content grid with a {gh}x{gw} "
                         f"exemplar grid at topk={k} (equal 64- or 128-wide grids, positions a multiple of 256), and there is no "
                         f"materialised fall-back{_ROUTE[member]}")


def _raw(t):
    """the fp32 projection of a LazyProj1x1 (K0, computed once and cached by it); a tensor as it is"""
    return t.raw() if isinstance(t, ops.LazyProj1x1) else t


def _same_kind(name: str, theta_raw, phi_raw):
    if isinstance(theta_raw, ops.LazyProj1x1) != isinstance(phi_raw, ops.LazyProj1x1):
        raise TypeError(f"{name}: theta and phi must both be tensors or both be ops.LazyProj1x1")


def _grids(theta_raw, phi_raw, exemplar=None):
    """(B, C, fh, fw, gh, gw, N, Nk): the content grid of theta, the exemplar grid of phi (a prepared exemplar: the content's)"""
    B, C, fh, fw = theta_raw.shape
    gh, gw = (fh, fw) if exemplar is not None else tuple(phi_raw.shape[2:])
    return B, C, fh, fw, gh, gw, fh * fw, gh * gw


def _fused_width(name: str, theta_raw, phi_raw):
    if theta_raw.shape[1] != ops.FUSED_K or phi_raw.shape[:2] != theta_raw.shape[:2]:
        raise ValueError(f"{name}: needs theta / phi with {ops.FUSED_K} channels and one batch, got {tuple(theta_raw.shape)} and "
                         f"{tuple(phi_raw.shape)}")


def _operand_planes(theta_raw, phi_raw, planes, *, detach: bool, want_chan, pair: bool = True):
    """The one producer of the family's operand planes -> the handles (qn, kn) of theta's and phi's planes, registered in `planes`.
    Two LazyProj1x1 of one input shape that ops.proj_norm_fused_ok takes go through K23 in one launch (`pair` False: never — the
    caller's route projects and runs K1); everything else is projected where lazy (K0) and goes through K1 twice.  Every entry point
    selects from these planes, which is what makes their indices and log-sum-exps agree bit for bit.  `detach`: a forward-only caller —
    no graph, no channel-major planes; otherwise the handles carry the graph, K23 writes the channel-major planes on `want_chan`
    and K1 for a side that requires a gradient."""
    if (pair and isinstance(theta_raw, ops.LazyProj1x1) and theta_raw.x.shape == phi_raw.x.shape and ops.proj_norm_fused_ok(theta_raw)
            and ops.proj_norm_fused_ok(phi_raw)):
        if detach:
            theta_raw, phi_raw = theta_raw.detach(), phi_raw.detach()
        return ops.proj_center_l2norm_planes_pair(theta_raw, phi_raw, 1, planes, want_chan=want_chan)      # K23
    if detach:      # side by side: theta's projection and K1, then phi's
        return tuple(ops.center_l2norm_planes(_flat(_raw(t)).detach(), 1, planes, want_chan=False) for t in (theta_raw, phi_raw))
    theta_raw, phi_raw = _raw(theta_raw), _raw(phi_raw)     # both projections, then K1 twice
    return ops.center_l2norm_planes(_flat(theta_raw), 1, planes), ops.center_l2norm_planes(_flat(phi_raw), 1, planes)


def _readout(idx, mx, lse, shape, other):
    """the MatchReadout of a kernel's (idx int32, max, lse) on the [B,h,w] `shape` of the side that asks; `other`: the grid indexed"""
    return MatchReadout(index=idx.to(torch.int64).reshape(shape), prob=torch.exp(mx - lse).reshape(shape), max_logit=mx.reshape(shape),
                        lse=lse.reshape(shape), grid=other)


def _rank_first(t, shape, k):
    """a [B,N,k] kernel output (tiny) with the rank in front of the [B,h,w] `shape`: [B,k,h,w]"""
    return t.reshape(tuple(shape) + (k,)).permute(0, 3, 1, 2).contiguous()


def _match_result(idx, val, lse, shape, other, restricted=None):
    """The readout of a kernel's (idx int32 [B,N,k], val [B,N,k], lse [B,N]) on the [B,h,w] `shape` of the side that asks: a MatchReadout
    for k = 1, a TopkMatchReadout otherwise; `other`: the grid indexed, `restricted` [B,N] bool or None (K47, K55)"""
    k = idx.shape[-1]
    restricted = None if restricted is None else restricted.reshape(shape)
    if k == 1:
        m = _readout(idx[..., 0], val[..., 0], lse, shape, other)
        m.restricted = restricted
        return m
    lse = lse.reshape(shape)
    val = _rank_first(val, shape, k)
    return TopkMatchReadout(index=_rank_first(idx.to(torch.int64), shape, k), prob=torch.exp(val - lse.unsqueeze(1)), logit=val, lse=lse,
                            grid=other, restricted=restricted)


def _boxed(theta_raw, phi_raw, inv_t, *, exemplar=None, grad: bool = False):
    """The _BoxedCorr of a (theta_raw, phi_raw) pair as correspondence_hot_path makes it: a lazy pair stays lazy where
    ops.PROJ_BWD_FUSED lets _BoxedCorr take it (K25 / proj_unfold3_stats inside), everything else is projected first (K0).  Forward
    only — the operands are detached — unless `grad` (K53: autograd stays, and the lse passes share one gradient sink).  `exemplar`: a
    prepared exemplar in place of phi_raw — the record's planes and (nu, b): the key side is not recomputed."""
    if exemplar is not None:
        th = _raw(theta_raw).detach()
        return _BoxedCorr(th, th.view_as(th), inv_t, prepared_k=exemplar.box_planes(th.shape[0]))
    if not (isinstance(theta_raw, ops.LazyProj1x1) and ops.PROJ_BWD_FUSED):
        theta_raw, phi_raw = _raw(theta_raw), _raw(phi_raw)
    if grad:
        return _BoxedCorr(theta_raw, phi_raw, inv_t, share_sink=True)
    return _BoxedCorr(theta_raw.detach(), phi_raw.detach(), inv_t)


def _refine_scope(name: str, cfg: HotPathConfig, refine, refine_temperature, topk, has_exemplar: bool, channels=None):
    """ValueError for a `refine` that is no radius, and — with refine > 0 — for everything outside the sub-cell refinement's scope (K44:
    top-1 on the fused match_kernel-1 route, no prepared exemplar); checked before any tensor is looked at.  `channels`: the width of
    theta / phi where the caller knows it."""
    top = ops.MATCH_REFINE_MAX_RADIUS
    if isinstance(refine, bool) or not isinstance(refine, int) or not 0 <= refine <= top:
        raise ValueError(f"{name}: refine={refine!r}: expected an integer in 0..{top} (0: no refinement)")
    _refine_temperature_arg(name, refine_temperature)
    if refine == 0:
        return
    if topk != 1:
        raise ValueError(f"{name}: refine={refine} with topk={topk}: the refinement is built for the single best match (topk = 1)")
    if has_exemplar:
        raise ValueError(f"{name}: refine={refine} with a prepared exemplar is out of scope (not built)")
    _route_scope(name, cfg, "refine", plain_flags=False, match_fused=True)
    _route_channels(name, "refine", channels)


# ---- K47: label-restricted candidates ---------------------------------------------------------------------------------------------
def cell_labels(seg_map, down):
    """int64 [B,h,w]: the majority class of every down x down cell of a one-hot (or soft) label map seg_map [B,nc,h*down,w*down]; among
    equally frequent classes the lower one (torch glue: the labels of correspondence_match / correspondence_sparse with
    restrict="label")."""
    if not torch.is_tensor(seg_map) or seg_map.dim() != 4:
        raise ValueError("cell_labels: expected a label map [B,nc,H,W]")
    if isinstance(down, bool) or not isinstance(down, int) or down < 1 or seg_map.shape[2] % down or seg_map.shape[3] % down:
        raise ValueError(f"cell_labels: down={down!r} does not divide the {tuple(seg_map.shape[2:])} label map")
    return F.avg_pool2d(seg_map.float(), down).argmax(1)


def _restrict_scope(name: str, cfg: HotPathConfig, restrict, has_exemplar: bool, refine=0, search="dense", channels=None):
    """ValueError for a `restrict` that is neither None, "label" nor a pair of integer tensors (TypeError for another dtype), and — with
    a restriction — for everything outside its scope (K47: the fused match_kernel-1 route, no prepared exemplar, no refinement, the
    dense selector); checked before any tensor is looked at.  Every message names `restrict`."""
    if restrict is None:
        return
    _restrict_arg(name, restrict)
    _route_scope(name, cfg, "restrict", plain_flags=False, match_fused=True)
    if has_exemplar:
        raise ValueError(f"{name}: restrict with a prepared exemplar is out of scope (not built)")
    if refine:
        raise ValueError(f"{name}: restrict with refine={refine!r} is out of scope (not built)")
    if search != "dense":
        raise ValueError(f"{name}: restrict with search={search!r} is out of scope: the label mask lives in the dense scan")
    _route_channels(name, "restrict", channels)


def _restrict_labels(name: str, restrict, seg_map, ref_seg_map, down, B, content_grid, exemplar_grid):
    """(content labels [B,fh*fw], exemplar labels [B,gh*gw]) of a restriction _restrict_scope accepted: cell_labels of the two label
    maps, or the given pair; ValueError for what does not fit the grids"""
    (fh, fw), (gh, gw) = content_grid, exemplar_grid
    if isinstance(restrict, str):
        for what, seg, (h, w) in (("seg_map", seg_map, content_grid), ("ref_seg_map", ref_seg_map, exemplar_grid)):
            if not torch.is_tensor(seg) or seg.dim() != 4 or seg.shape[0] != B or tuple(seg.shape[2:]) != (h * down, w * down):
                got = tuple(seg.shape) if torch.is_tensor(seg) else type(seg).__name__
                raise ValueError(f"{name}: restrict='label' needs {what} [B={B},nc,{h * down},{w * down}] (down={down} times the {h}x{w} "
                                 f"grid), got {got}")
        if seg_map.shape[1] != ref_seg_map.shape[1]:
            raise ValueError(f"{name}: restrict='label': seg_map has {seg_map.shape[1]} classes, ref_seg_map {ref_seg_map.shape[1]}")
        q_lab, k_lab = cell_labels(seg_map, down), cell_labels(ref_seg_map, down)
    else:
        q_lab, k_lab = restrict
        if tuple(q_lab.shape) != (B, fh, fw) or tuple(k_lab.shape) != (B, gh, gw):
            raise ValueError(f"{name}: restrict: labels {tuple(q_lab.shape)}, {tuple(k_lab.shape)} do not fit the content grid "
                             f"{(B, fh, fw)} and the exemplar grid {(B, gh, gw)}")
    return q_lab.reshape(B, fh * fw), k_lab.reshape(B, gh * gw)


def restrict_fallback(q_lab, k_lab, k):
    """The fallback rule of a restriction: asking position i of sample b is restricted only if the other side holds at least k
    positions of its label in that sample (a negative label: never).  q_lab [B,Nq], k_lab [B,Nk] integer tensors of one device ->
    (q_eff, k_eff, restricted): int32 labels for ops.corr_topk_labelled — dense ids of the labels that occur, so any int64 ids
    survive the narrowing; -1 for an unrestricted asking position and for a negative label of the other side — and restricted bool
    [B,Nq].  So no row of the readout is short or empty.  Counts: a scatter_add over b * L + id."""
    B, Nq = q_lab.shape
    ids, inv = torch.unique(torch.cat((q_lab, k_lab), 1).to(torch.int64), return_inverse=True)
    L = ids.numel()
    q_id, k_id = inv[:, :Nq], inv[:, Nq:]
    k_valid = k_lab >= 0
    at = torch.arange(B, device=q_lab.device).view(B, 1) * L
    counts = torch.zeros(B * L, dtype=torch.int64, device=q_lab.device)
    counts.scatter_add_(0, (at + k_id).reshape(-1), k_valid.reshape(-1).to(torch.int64))
    restricted = (q_lab >= 0) & (counts.view(B, L).gather(1, q_id) >= k)
    minus = torch.full_like(q_id, -1)
    return (torch.where(restricted, q_id, minus).to(torch.int32).contiguous(),
            torch.where(k_valid, k_id, torch.full_like(k_id, -1)).to(torch.int32).contiguous(), restricted)


def correspondence_match(theta_raw, phi_raw, cfg: HotPathConfig, temperature=0.01, *, exemplar=None, direction="rows", topk=1, refine=0,
                         refine_temperature=None, restrict=None, seg_map=None, ref_seg_map=None):
    """The hard readout of the correlation of correspondence.py:272-304: argmax, maximum and log-sum-exp of every row of the scaled
    matrix f / temperature that forward(return_corr=True) returns (:305-306) — `direction="rows"`: per CONTENT position over the
    exemplar positions; "cols": per EXEMPLAR position over the content positions (the rows of f^T).  Returns a MatchReadout.

    theta_raw, phi_raw: [B,256,h,w] CUDA fp32 or ops.LazyProj1x1, as for correspondence_hot_path; `exemplar`: the ops.PreparedKeys
    of a prepared exemplar in place of phi_raw (None).  Routes mirror correspondence_hot_path's: where its fused match_kernel-1
    back end runs (C == 256, PONO_C, the split-precision kernels) the operand planes go to K36a and nothing HWxHW is allocated;
    where its fused match_kernel-3 back end runs (PONO_C, equal 64- or 128-wide grids: ops.box3_fused_ok) the one HWxHW tensor is
    T = xbox(C) from the correlation GEMM's epilogue, which K37 reads once (the column direction reads the same T transposed; a
    prepared exemplar brings its key planes and statistics);
    everywhere else (other match_kernel-3 shapes, no PONO_C, COCOS_PRECISION=fp32, odd sizes, ops.MATCH_FUSED = False) the logits
    are materialised as for return_corr and read in one sweep by K36b.  Forward only: runs under torch.no_grad().

    `topk` = k > 1 (at most ops.MATCH_TOPK_MAX and the number of positions asked about, else ValueError) returns a TopkMatchReadout:
    the k best candidates per position.  The fused match_kernel-1 route then runs K39a (ops.corr_topk_ok(k); still nothing HWxHW)
    and the fused match_kernel-3 route K41 (ops.box3_topk_ok(k): the same one T, read once, K37's kernel with a candidate list per
    lane); every other route materialises its logits and reads them in one sweep with K39b.

    `refine` = r in 1..ops.MATCH_REFINE_MAX_RADIUS (K44; 0, the default, changes nothing) adds a sub-cell position to the top-1 readout:
    a softmax at `refine_temperature` (None: `temperature`) over the logits of the (2 r + 1)^2 window of the other side's grid around
    every match — positions outside the grid are left out — whose expected offset becomes MatchReadout.offset, with
    MatchReadout.window_prob the window's share of the full softmax mass; the same operand planes serve the scan and the window.
    Scope: topk = 1, no prepared exemplar, the fused match_kernel-1 route (PONO_C, 256 channels, COCOS_PRECISION=f16x3,
    ops.MATCH_FUSED); everything else raises ValueError — nothing falls back.

    `restrict` (K47; None, the default, is the code path above, untouched) keeps every position's candidates inside its own region:
    "label" takes the majority class of each cell of the one-hot `seg_map` / `ref_seg_map` [B,nc,h*down,w*down] (cell_labels, with
    cfg.down); a pair (q_labels [B,h,w], k_labels [B,gh,gw]) of int32 / int64 tensors — content side first, whatever the direction —
    is taken as given (face-parsing parts, instance ids, scribbles; a negative content label: unrestricted).  The mask is applied
    inside the scan (ops.corr_topk_labelled): index, logit, prob and lse are then over the ALLOWED positions, and still nothing HWxHW
    exists.  A position whose label has fewer than topk positions on the other side of its sample falls back to the unrestricted scan
    (restrict_fallback), so no row is short; the readout's `restricted` says which positions were restricted.  Scope: the fused
    match_kernel-1 route (PONO_C, 256 channels, COCOS_PRECISION=f16x3, ops.MATCH_FUSED, ops.corr_split_ok shapes), no prepared
    exemplar, refine = 0; everything else raises a ValueError that names restrict — nothing falls back to a materialised matrix."""
    if direction not in ("rows", "cols"):
        raise ValueError(f"correspondence_match: direction {direction!r}: expected 'rows' or 'cols'")
    k = _topk_arg("correspondence_match", topk)
    _restrict_scope("correspondence_match", cfg, restrict, exemplar is not None, refine, channels=theta_raw.shape[1])
    _refine_scope("correspondence_match", cfg, refine, refine_temperature, topk, exemplar is not None, theta_raw.shape[1])
    if (exemplar is None) == (phi_raw is None):
        raise ValueError("correspondence_match: pass phi_raw or a prepared exemplar in its place (not both)")
    B, C, fh, fw, gh, gw, N, Nk = _grids(theta_raw, phi_raw, exemplar)
    mk, inv_t = cfg.match_kernel, 1.0 / temperature
    rows = direction == "rows"
    if exemplar is not None:
        exemplar.check(B)
        if exemplar.shape[1:] != theta_raw.shape[1:]:
            raise ValueError(f"prepared exemplar: feature grid {tuple(exemplar.shape)} does not match the content's {tuple(theta_raw.shape)}")
    else:
        _same_kind("correspondence_match", theta_raw, phi_raw)
    if k > (Nk if rows else N):
        raise ValueError(f"correspondence_match: topk={k} exceeds the {Nk if rows else N} positions each row of direction={direction!r} ranges over")
    labels = None
    if restrict is not None:
        labels = _restrict_labels("correspondence_match", restrict, seg_map, ref_seg_map, cfg.down, B, (fh, fw), (gh, gw))
    with torch.no_grad():
        if not _hip_fp32(theta_raw):
            raise ops._lib.CocosHipError("correspondence_match: expected CUDA/HIP fp32 tensors; the correspondence hot path has no CPU fallback")
        fused = (ops.MATCH_FUSED and mk == 1 and C == ops.FUSED_K and cfg.PONO_C and ops.corr_split_ok(B, C, N, Nk, 1, False)
                 and (k == 1 or ops.corr_topk_ok(k)))
        if refine and not fused:
            raise ValueError(f"correspondence_match: refine={refine}: the fused match_kernel 1 route does not take B={B}, {fh}x{fw} content "
                             f"and {gh}x{gw} exemplar positions (ops.corr_split_ok), and the refinement runs on no other route")
        if restrict is not None and not fused:
            raise ValueError(f"correspondence_match: restrict: the fused match_kernel 1 route does not take B={B}, {fh}x{fw} content and "
                             f"{gh}x{gw} exemplar positions, topk={k} (ops.corr_split_ok, ops.corr_topk_ok), and restrict runs on no other route")
        off = lse_win = restricted = None
        if fused and exemplar is not None:
            # the query side as _attention_with_exemplar makes it; the record's key planes are read in place
            if isinstance(theta_raw, ops.LazyProj1x1) and ops.proj_norm_fused_ok(theta_raw):
                qh, ql, _ = ops.proj_center_l2norm_planes_one(theta_raw, 1)      # K23, theta alone
            else:
                qh, ql, _ = ops.center_l2norm_planes_fwd(_flat(_raw(theta_raw)), 1)
            if rows:
                idx, mx, lse = ops.corr_match_shared(qh, ql, exemplar, inv_t) if k == 1 else ops.corr_topk_shared(qh, ql, exemplar, inv_t, k)
            else:       # the exemplar's positions ask: B different key sets (the contents), so the record's planes are needed per sample
                kh, kl, _ = exemplar.split_planes(B)
                idx, mx, lse = ops._corr_match_planes(kh, kl, qh, ql, inv_t) if k == 1 else ops._corr_topk_planes(kh, kl, qh, ql, inv_t, k)
        elif fused:
            planes = ops.OperandPlanes()
            qn, kn = _operand_planes(theta_raw, phi_raw, planes, detach=True, want_chan=False)
            if labels is not None:      # K47: the side that asks brings its labels, operands and label tensors swap together
                asks, other_side = (qn, kn) if rows else (kn, qn)
                q_eff, k_eff, restricted = restrict_fallback(*(labels if rows else labels[::-1]), k)
                idx, mx, lse = ops.corr_topk_labelled(asks, other_side, q_eff, k_eff, inv_t, k, planes)
            elif k == 1:
                idx, mx, lse = ops.corr_match(qn, kn, inv_t, planes) if rows else ops.corr_match(kn, qn, inv_t, planes)
                if refine:      # K44: the window scores come from the operand planes that chose the centre
                    inv_rt = inv_t if refine_temperature is None else 1.0 / refine_temperature
                    asks, other_side, kgrid = (qn, kn, (gh, gw)) if rows else (kn, qn, (fh, fw))
                    off, lse_win = ops.match_refine(asks, other_side, idx, kgrid, inv_rt, refine, planes)
            else:
                idx, mx, lse = ops.corr_topk(qn, kn, inv_t, k, planes) if rows else ops.corr_topk(kn, qn, inv_t, k, planes)
        elif ((k == 1 or ops.box3_topk_ok(k)) and ops.MATCH_FUSED and mk == 3 and cfg.PONO_C and (gh, gw) == (fh, fw)
              and ops.box3_fused_ok(B, C, fh, fw)):
            # the reference's default on the fused family's shapes: ONE HWxHW tensor (T, from the x-box GEMM's epilogue), read once
            # by K37 (k > 1: K41) — the _BoxedCorr is made as correspondence_hot_path / _attention_with_exemplar make theirs
            boxed = _boxed(theta_raw, phi_raw, inv_t, exemplar=exemplar)
            idx, mx, lse = boxed.match(rows, k)
            del boxed
        else:
            th = _raw(theta_raw).detach()
            ph = (exemplar.phi_raw(B) if exemplar is not None else _raw(phi_raw)).detach()
            if mk == 3 and cfg.PONO_C:
                f = _box3_logits(th, ph, inv_t, transposed=not rows)
            else:   # f^T is the same matrix with the operands exchanged (centring and normalisation are per tensor)
                f = _scaled_logits(th, ph, cfg, inv_t, False, 1) if rows else _scaled_logits(ph, th, cfg, inv_t, False, 1)
            idx, mx, lse = ops.row_argmax_lse(f) if k == 1 else ops.row_topk_lse(f, k)
            del f
        own, other = ((fh, fw), (gh, gw)) if rows else ((gh, gw), (fh, fw))
        shape = (B,) + own
        m = _match_result(idx.reshape(B, -1, k), mx.reshape(B, -1, k), lse, shape, other, restricted)
        if refine:
            m.offset = _rank_first(off, shape, 2)
            m.window_prob = torch.exp(lse_win - lse).reshape(shape)
        return m


# ---- K48: mutual match — both directions and the round trip ---------------------------------------------------------------------
@dataclass
class MutualMatchReadout:
    """Both directions of the hard readout and their round trip (correspondence_mutual).  `rows`: the MatchReadout of the content
    positions (into the exemplar grid), `cols`: of the exemplar positions (into the content grid), each exactly as
    correspondence_match builds it.  rows_back [B,fh,fw] int64: where a content position comes back to on its OWN grid
    (cols.index at rows.index), rows_dist int32 the Chebyshev distance in cells between that and the position itself, rows_mutual
    bool = rows_dist <= max_dist (max_dist = 0: mutual nearest neighbours); cols_back / cols_dist / cols_mutual [B,gh,gw] the same
    for the exemplar positions."""
    rows: MatchReadout
    cols: MatchReadout
    rows_back: torch.Tensor
    cols_back: torch.Tensor
    rows_dist: torch.Tensor
    cols_dist: torch.Tensor
    rows_mutual: torch.Tensor
    cols_mutual: torch.Tensor
    max_dist: int = 0


def _max_dist(name: str, max_dist):
    if isinstance(max_dist, bool) or not isinstance(max_dist, int) or max_dist < 0:
        raise ValueError(f"{name}: max_dist={max_dist!r}: expected a non-negative integer (cells; 0: mutual nearest neighbours)")
    return max_dist


def mutual_fused_route(cfg: HotPathConfig, B, C, N, Nk, has_exemplar: bool) -> bool:
    """correspondence_mutual sweeps the correlation once: where correspondence_match's fused match_kernel-1 route runs, without a
    prepared exemplar, on the shapes the mutual kernel takes, and with both switches on"""
    return bool(ops.MATCH_FUSED and ops.MATCH_MUTUAL_FUSED and not has_exemplar and cfg.match_kernel == 1 and C == ops.FUSED_K
                and cfg.PONO_C and ops.PRECISION == "f16x3" and ops.corr_split_ok(B, C, N, Nk, 1, False)
                and ops.corr_match_mutual_ok(B, N, Nk))


def correspondence_mutual(theta_raw, phi_raw, cfg: HotPathConfig, temperature=0.01, *, exemplar=None, max_dist=0):
    """The round-trip test of the hard correspondence: content position i goes to its best exemplar position j
    (correspondence_match, direction="rows"), j goes to its best content position i' (direction="cols"), and the match is confirmed
    when i' is i or within `max_dist` cells of it (Chebyshev, on the content grid) — an occlusion / "nothing to copy from" mask, the
    hard-readout counterpart of the cycle terms (warp_cycle_w, correspondence.py:350-372).  Returns a MutualMatchReadout.  Arguments
    as correspondence_match; `max_dist` must be a non-negative integer (ValueError, before any tensor is looked at).  Forward only.

    Routes.  FUSED: where correspondence_match's fused match_kernel-1 route runs (ops.MATCH_FUSED, match_kernel 1, 256 channels,
    PONO_C, COCOS_PRECISION=f16x3) with no prepared exemplar, ops.MATCH_MUTUAL_FUSED on and shapes ops.corr_match_mutual_ok takes,
    the operand planes are made once (the K23 pair where it applies) and the correlation is swept ONCE: K48's kernel reads every
    S^T tile along the keys and along the queries (ops.corr_match_mutual).  `rows` is then correspondence_match's readout bit for
    bit; `cols` holds the same logits reduced in another order: its index is the exchanged call's except among logits closer than
    the kernel's rounding, its lse within the same error bound.  EVERYWHERE ELSE (the fused match_kernel-3 route, the
    materialised routes, prepared exemplars, ops.MATCH_MUTUAL_FUSED = False) this makes two correspondence_match calls on the same
    theta_raw / phi_raw, rows then cols: those routes pay two readouts (two projections' worth of centring / normalisation, two
    sweeps or two reads of their matrix) — sharing T or the operand planes between the two calls is out of scope here.  Every route
    ends in the same round-trip kernel (ops.match_round_trip)."""
    name = "correspondence_mutual"
    max_dist = _max_dist(name, max_dist)
    if (exemplar is None) == (phi_raw is None):
        raise ValueError(f"{name}: pass phi_raw or a prepared exemplar in its place (not both)")
    B, C, fh, fw, gh, gw, N, Nk = _grids(theta_raw, phi_raw, exemplar)
    inv_t = 1.0 / temperature
    with torch.no_grad():
        fused = (exemplar is None and isinstance(theta_raw, ops.LazyProj1x1) == isinstance(phi_raw, ops.LazyProj1x1)
                 and _hip_fp32(theta_raw) and mutual_fused_route(cfg, B, C, N, Nk, False))
        if fused:
            planes = ops.OperandPlanes()
            qn, kn = _operand_planes(theta_raw, phi_raw, planes, detach=True, want_chan=False)      # correspondence_match's planes
            (ri, rm, rl), (ci, cm, cl) = ops.corr_match_mutual(qn, kn, inv_t, planes)
            rows = _readout(ri, rm, rl, (B, fh, fw), (gh, gw))
            cols = _readout(ci, cm, cl, (B, gh, gw), (fh, fw))
        else:      # two readouts; every refusal (CPU tensors, mixed operand kinds, a stale record) is correspondence_match's
            rows = correspondence_match(theta_raw, phi_raw, cfg, temperature, exemplar=exemplar, direction="rows")
            cols = correspondence_match(theta_raw, phi_raw, cfg, temperature, exemplar=exemplar, direction="cols")
            ri, ci = rows.index.reshape(B, N), cols.index.reshape(B, Nk)
        q_back, q_dist, k_back, k_dist = ops.match_round_trip(ri, ci, (fh, fw), (gh, gw))
        q_dist, k_dist = q_dist.reshape(B, fh, fw), k_dist.reshape(B, gh, gw)
        return MutualMatchReadout(rows=rows, cols=cols, rows_back=q_back.to(torch.int64).reshape(B, fh, fw),
                                  cols_back=k_back.to(torch.int64).reshape(B, gh, gw), rows_dist=q_dist, cols_dist=k_dist,
                                  rows_mutual=q_dist <= max_dist, cols_mutual=k_dist <= max_dist, max_dist=max_dist)


# ---- K42: differentiable k-sparse warp over the top-k matches ---------------------------------------------------------------------
def _sparse_scope(cfg: HotPathConfig, topk):
    """ValueError for every flag outside correspondence_sparse's scope (checked before any tensor is looked at) -> k"""
    k = _topk_arg("correspondence_sparse", topk)
    _route_scope("correspondence_sparse", cfg, "sparse", plain_flags=True, match_fused=False)
    return k


def _sparse_search(search, search_opts, name="correspondence_sparse"):
    """ValueError for a selector correspondence_sparse (`name`: correspondence_sparse_box3) does not have, or options it does not know
    -> the PatchMatch schedule (None for the dense scan); checked after the route's scope, before any tensor is looked at"""
    if search not in ("dense", "patchmatch"):
        raise ValueError(f"{name}: search={search!r}: expected 'dense' or 'patchmatch'")
    opts = dict(search_opts or {})
    if search == "dense":
        if opts:
            raise ValueError(f"{name}: search_opts {sorted(opts)} given with search='dense' (the dense scan has no options)")
        return None
    unknown = sorted(set(opts) - set(ops.PATCHMATCH_DEFAULTS))
    if unknown:
        raise ValueError(f"{name}: unknown search_opts {unknown}: expected a subset of {sorted(ops.PATCHMATCH_DEFAULTS)}")
    return dict(ops.PATCHMATCH_DEFAULTS, **opts)


def _patchmatch_coarse_init(theta_raw, phi_raw, inv_t, k):
    """The starting candidates of the PatchMatch selector, [B,N,k] int64, or "random" where the half grid is out of the dense readout's
    reach (an odd side, half-grid positions that are no multiple of 4, fewer than k half-grid keys): theta / phi averaged over 2 x 2
    cells (torch glue), K1 planes of the pooled features, the dense top-k (K39a) at a quarter of the positions on each side — a
    sixteenth of the full scan — and every coarse candidate (ky, kx) of coarse query (y / 2, x / 2) expanded to the fine key
    (2 ky + y % 2, 2 kx + x % 2): the key that lies in its coarse cell where the query lies in its own."""
    B, C, fh, fw = theta_raw.shape
    gh, gw = phi_raw.shape[2:]
    if fh % 2 or fw % 2 or gh % 2 or gw % 2:
        return "random"
    Nc, Nkc = (fh // 2) * (fw // 2), (gh // 2) * (gw // 2)
    if k > Nkc or not ops.corr_split_ok(B, C, Nc, Nkc, 1, False) or not ops.corr_topk_ok(k):
        return "random"
    planes = ops.OperandPlanes()
    pool = lambda t: _flat(torch.nn.functional.avg_pool2d(t.detach(), 2))
    qc = ops.center_l2norm_planes(pool(theta_raw), 1, planes, want_chan=False)
    kc = ops.center_l2norm_planes(pool(phi_raw), 1, planes, want_chan=False)
    coarse, _, _ = ops.corr_topk(qc, kc, inv_t, k, planes)                          # [B,Nc,k] int32
    return _patchmatch_expand(coarse.to(torch.int64).reshape(B, fh // 2, fw // 2, k), fh, fw, gw)


def _patchmatch_expand(coarse, fh, fw, gw):
    """coarse [B,fh/2,fw/2,k] int64, keys of the half exemplar grid (width gw / 2) -> [B,fh*fw,k] int64 on the full grids: every
    coarse candidate (ky, kx) of coarse query (y / 2, x / 2) moved to the fine key (2 ky + y % 2, 2 kx + x % 2)"""
    B, k = coarse.shape[0], coarse.shape[3]
    coarse = coarse.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)         # the coarse query of every fine query
    dev = coarse.device
    py = (torch.arange(fh, device=dev) % 2).view(1, fh, 1, 1)
    px = (torch.arange(fw, device=dev) % 2).view(1, 1, fw, 1)
    cky, ckx = torch.div(coarse, gw // 2, rounding_mode="floor"), coarse % (gw // 2)
    return ((2 * cky + py) * gw + 2 * ckx + px).reshape(B, fh * fw, k)


def correspondence_sparse(theta_raw, phi_raw, ref_img, seg_map, ref_seg_map, cfg: HotPathConfig, temperature=0.01, topk=4, *,
                          exemplar=None, search="dense", search_opts=None, restrict=None, transport=None):
    """The k-sparse, trainable variant of correspondence_hot_path's row pass (CoCosNet-v2 style): per content position the `topk` best
    exemplar positions are SELECTED without gradient by the match readout (K23 / K1 planes -> K39a, as correspondence_match), then a
    softmax over those k logits alone blends their values — ops.sparse_softmax_warp (K42), with gradients to theta_raw and phi_raw
    through ops.center_l2norm_planes (K1, whose planes serve both steps).  Nothing HWxHW is allocated, forward or backward.

    theta_raw, phi_raw: [B,256,h,w] CUDA fp32 (or ops.LazyProj1x1, projected here).  Returns {warp_out [B,3,H,W] (nearest
    up-sampling of the blend of the pooled exemplar), warp_mask [B,nc,h,w] when cfg.warp_mask_losstype == "direct" (or show_warpmask),
    match_index [B,k,h,w] int64, match_weight [B,k,h,w] (the k-sparse softmax weights; no gradient)}.

    Scope: match_kernel 1, PONO_C, 256 channels, shapes ops.corr_split_ok and ops.corr_topk_ok(k) accept, COCOS_PRECISION=f16x3, plain
    flag set (no warp_patch / warp_bilinear / cycle terms), no prepared exemplar: everything else raises ValueError — there is no
    fall-back route.  CPU tensors raise CocosHipError.

    `search`: how the k candidates are found.  "dense" (the default) is the scan over all keys above.  "patchmatch" (K43) starts from
    the dense top-k of the 2 x 2 average-pooled features (_patchmatch_coarse_init; a random start where the half grid is out of the
    readout's reach) and runs ops.patchmatch_topk on the full-grid planes: propagation from the grid neighbours plus a random search,
    O(N k) dot products per iteration whatever the number of keys.  Its candidates are the best of what it looked at, not of all keys
    (DESIGN.md 3.27 records recall and cost against the dense scan); scope and refusals are the dense selector's.  `search_opts`
    overrides entries of ops.PATCHMATCH_DEFAULTS: strides (one iteration per entry), radii, radius0, seed.

    `restrict` (K47; None, the default, is the code path above, untouched): "label" or a pair (q_labels [B,h,w], k_labels [B,gh,gw]),
    as correspondence_match takes them — the k candidates are selected among the exemplar positions of the content position's label
    (ops.corr_topk_labelled; positions whose label has fewer than topk exemplar positions fall back to the scan over all), and the
    warp and its gradients are the same K42 on those indices.  The result gains match_restricted [B,h,w] bool.  Scope: the dense
    selector of the scope above; everything else raises a ValueError that names restrict.

    `transport` (K50; None, the default, is the code path above, untouched): dict(iters=, tau=) — the softmax is replaced by entropic
    optimal transport over the same correlation.  ops.corr_sinkhorn runs `iters` log-domain Sinkhorn iterations (tau = 1: balanced,
    tau < 1: KL-relaxed) on the operand planes, the k candidates are the top-k of z_ij = s_ij + g_j (ops.corr_topk_biased) and the blend
    is the biased softmax over them (ops.sparse_softmax_warp(k_bias=g)): the row-conditional transport plan on its k largest entries.
    The potentials are DETACHED: gradients reach theta, phi and the values through the k pair logits and the blend, with g a constant —
    nothing differentiates through the iterations.  The result gains potential_k [B,gh,gw] (g) and match_mass [B,h,w] (1 where the row
    marginal is met).  Scope: the dense selector of the scope above, restrict = None; everything else raises a ValueError that names
    transport."""
    _transport_scope("correspondence_sparse", cfg, transport, exemplar is not None, search, restrict, theta_raw.shape[1])
    _restrict_scope("correspondence_sparse", cfg, restrict, exemplar is not None, 0, search, theta_raw.shape[1])
    k = _sparse_scope(cfg, topk)
    pm = _sparse_search(search, search_opts)
    if exemplar is not None:
        raise ValueError("correspondence_sparse: a prepared exemplar is out of scope (it is forward-only; the sparse warp differentiates phi)")
    _same_kind("correspondence_sparse", theta_raw, phi_raw)
    B, C, fh, fw, gh, gw, N, Nk = _grids(theta_raw, phi_raw)
    down = cfg.down
    _fused_width("correspondence_sparse", theta_raw, phi_raw)
    if k > Nk:
        raise ValueError(f"correspondence_sparse: topk={k} exceeds the {Nk} exemplar positions")
    if tuple(ref_img.shape[2:]) != (gh * down, gw * down) or ref_img.shape[3] % 4 != 0:
        raise ValueError(f"correspondence_sparse: ref_img {tuple(ref_img.shape)} is not down={down} times the exemplar grid "
                         f"{(gh, gw)} (width a multiple of 4)")
    labels = None
    if restrict is not None:
        labels = _restrict_labels("correspondence_sparse", restrict, seg_map, ref_seg_map, down, B, (fh, fw), (gh, gw))
    if not (_hip_fp32(theta_raw) and _hip_fp32(ref_img)):
        raise ops._lib.CocosHipError("correspondence_sparse: expected CUDA/HIP fp32 tensors; the correspondence hot path has no CPU fallback")
    if not ops.corr_split_ok(B, C, N, Nk, 1, False) or not ops.corr_topk_ok(k):
        raise ValueError(f"correspondence_sparse: the fused top-k readout does not take B={B}, {N} x {Nk} positions, k={k} "
                         "(positions must be multiples of 4)" + ("; restrict runs on no other route" if restrict is not None else "")
                         + ("; transport runs on no other route" if transport is not None else ""))
    # K1 with autograd (_operand_planes without the K23 pair: lazy operands are projected): the position-major operand planes are
    # written once and serve the selection and the warp alike (the same planes, so the same candidates as correspondence_match, bit
    # for bit); qn / kn are the handles of those planes, and each keeps its channel-major planes for its own backward when it is
    # differentiated
    planes = ops.OperandPlanes()
    qn, kn = _operand_planes(theta_raw, phi_raw, planes, detach=False, want_chan=None, pair=False)
    inv_t = 1.0 / temperature
    direct_mask = cfg.warp_mask_losstype == "direct" or cfg.show_warpmask
    with torch.no_grad():
        restricted = g = None
        if labels is not None:      # K47: the same selection among the exemplar positions of the position's label
            q_eff, k_eff, restricted = restrict_fallback(*labels, k)
            idx, _, _ = ops.corr_topk_labelled(qn, kn, q_eff, k_eff, inv_t, k, planes)
        elif transport is not None:      # K50: the potentials (no gradient), then the k largest entries of every row of the plan
            f, g, _ = ops.corr_sinkhorn(qn, kn, inv_t, transport["iters"], transport["tau"], planes)
            idx, _, row_lse = ops.corr_topk_biased(qn, kn, g, inv_t, k, planes)
        elif pm is None:
            idx, _, _ = ops.corr_topk(qn, kn, inv_t, k, planes)                # selection: no gradient
        else:
            idx, _ = ops.patchmatch_topk(qn, kn, inv_t, k, ((fh, fw), (gh, gw)),
                                         _patchmatch_coarse_init(_raw(theta_raw), _raw(phi_raw), inv_t, k), pm["strides"],
                                         (pm["radii"], pm["radius0"]), pm["seed"], planes)
        v = _flat(ops.warp_values(ref_img, ref_seg_map if direct_mask else None, down))
    if g is None:
        o, w = ops.sparse_softmax_warp(qn, kn, v, idx, inv_t, planes, return_weights=True)
    else:
        o, w = ops.sparse_softmax_warp(qn, kn, v, idx, inv_t, planes, return_weights=True, k_bias=g)
    n_ref = ref_img.shape[1]
    y, o_mask = _split_channels(o, n_ref) if direct_mask else (o, None)
    out = {"warp_out": ops.upsample_nearest(y.reshape(B, n_ref, fh, fw), down)}
    if direct_mask:
        out["warp_mask"] = o_mask.reshape(B, -1, fh, fw)
    out["match_index"] = _rank_first(idx.to(torch.int64), (B, fh, fw), k)
    out["match_weight"] = _rank_first(w, (B, fh, fw), k)
    if restricted is not None:
        out["match_restricted"] = restricted.reshape(B, fh, fw)
    if g is not None:
        out["potential_k"] = g.reshape(B, gh, gw)
        out["match_mass"] = torch.exp(f + row_lse + math.log(N)).reshape(B, fh, fw)
    return out


# ---- K51 / K52: the trainable routes on match_kernel 3 (the k-sparse warp, the sub-cell flow) -----------------------------------------
def _no_patchmatch_with(name: str, search, restrict, transport):
    """ValueError naming search: on the match_kernel-3 route the label mask and the transport bias live in the scan of T, which
    search="patchmatch" does not make"""
    if search == "patchmatch" and (restrict is not None or transport is not None):
        what = "restrict" if restrict is not None else "transport"
        raise ValueError(f"{name}: search='patchmatch' with {what} is out of scope (not built): {what} selects inside the dense scan of T"
                         f"{_ROUTE['sparse_box3']}")


def _box3_select_and_stats(theta_raw, phi_raw, select):
    """The prologue of the trainable routes -> (th, ph, mu, a, nu, b, what `select` returned).  Lazy operands are projected first, with
    autograd (K0; the handle caches the projection, so this must not happen inside the selection's no_grad block); `select()` — the
    member's selector: correspondence_match, _restrict_box3_select or _transport_box3_select on the operands as they came, so its
    candidates are that entry point's bit for bit — runs without gradient and drops its T inside.  What it returns (a few [B,·,h,w]
    tensors) lives across the two statistics launches, which run before the caller's warp_values: the same launches, reordered."""
    th, ph = _raw(theta_raw), _raw(phi_raw)
    with torch.no_grad():
        picked = select()
    kc = float(th.shape[1] * 9)
    mu, a = _unfold3_stats(th, kc)      # K12 with autograd: the statistics' share of the gradient goes back through its backward
    nu, b = _unfold3_stats(ph, kc)
    return th, ph, mu, a, nu, b, picked


#: the largest materialised matrix the coarse start of search="patchmatch" may build at the half grid, per matrix (the chain builds
#: two): a condition on the shapes, not a measurement
PATCHMATCH_BOX3_COARSE_CAP = 256 << 20


def _patchmatch_coarse_route_box3(B, C, fh, fw, gh, gw, k):
    """How search="patchmatch" starts on the match_kernel-3 route, as a pure function of the shapes -> "fused", "materialised" or
    "random".  The start is correspondence_match(topk=k) on the 2 x 2 average-pooled features, so it needs even sides and k half-grid
    keys.  "fused": the half grids are equal and pass ops.box3_fused_ok and ops.box3_topk_ok(k) (with ops.MATCH_FUSED) — the readout
    from one T of the half grid (256x256 -> 128x128, 128x128 -> 64x64).  "materialised": the chain at the half grid stays small,
    B * Nc * Nkc * 4 bytes <= PATCHMATCH_BOX3_COARSE_CAP (256 MiB) per matrix.  "random" for everything else: an odd side, k above the
    number of half-grid keys, a half grid that is too large, and unequal grids (the dense box readout, fused or materialised, is
    built for equal grids: ops.box3_logits filters a square matrix)."""
    if fh % 2 or fw % 2 or gh % 2 or gw % 2 or (gh, gw) != (fh, fw):
        return "random"
    ch, cw = fh // 2, fw // 2
    Nc = ch * cw
    if k > Nc:
        return "random"
    if ops.MATCH_FUSED and ops.box3_fused_ok(B, C, ch, cw) and ops.box3_topk_ok(k):
        return "fused"
    return "materialised" if B * Nc * Nc * 4 <= PATCHMATCH_BOX3_COARSE_CAP else "random"


def _patchmatch_coarse_init_box3(theta_raw, phi_raw, cfg, temperature, k):
    """The starting candidates of the PatchMatch selector on the match_kernel-3 route, [B,N,k] int64, or "random"
    (_patchmatch_coarse_route_box3 decides from the shapes alone): theta / phi averaged over 2 x 2 cells (torch glue),
    correspondence_match(topk=k) on the pooled features — K41 on the half grid's T where the fused family takes it, the materialised
    chain where that stays below 256 MiB per matrix — and every coarse candidate expanded as _patchmatch_coarse_init does.  Runs
    without gradient; whatever HWxHW tensor of the HALF grid the readout made is gone on return."""
    B, C, fh, fw = theta_raw.shape
    gh, gw = phi_raw.shape[2:]
    if _patchmatch_coarse_route_box3(B, C, fh, fw, gh, gw, k) == "random":
        return "random"
    with torch.no_grad():
        pool = lambda t: F.avg_pool2d(t.detach(), 2)
        m = correspondence_match(pool(theta_raw), pool(phi_raw), cfg, temperature, topk=k)
        coarse = m.index.reshape(B, k, fh // 2, fw // 2).permute(0, 2, 3, 1)
        del m
        return _patchmatch_expand(coarse, fh, fw, gw)


def correspondence_sparse_box3(theta_raw, phi_raw, ref_img, seg_map, ref_seg_map, cfg: HotPathConfig, temperature=0.01, topk=4, *,
                               exemplar=None, transport=None, restrict=None, search="dense", search_opts=None):
    """correspondence_sparse on the reference's default route, match_kernel 3 (K51): per content position the `topk` best exemplar
    positions are SELECTED without gradient exactly as correspondence_match(theta_raw, phi_raw, cfg, temperature, topk=topk) selects
    them (that function is called: K41 on the one x-box tensor T where ops.box3_fused_ok and ops.box3_topk_ok(topk) hold, the
    materialised chain elsewhere; T is gone when it returns), then a softmax over those k box logits alone blends their values —
    ops.box3_sparse_softmax_warp, with gradients to theta_raw and phi_raw through the pair logits and through the statistics of the
    unfolded vectors (K12, made here with autograd).  Nothing HWxHW is kept for, or allocated in, the backward.

    theta_raw, phi_raw: [B,256,h,w] CUDA fp32 (or ops.LazyProj1x1: the selection takes them as correspondence_match does, the warp
    projects them).  Returns correspondence_sparse's dictionary: {warp_out [B,3,H,W], warp_mask [B,nc,h,w] when
    cfg.warp_mask_losstype == "direct" (or show_warpmask), match_index [B,k,h,w] int64, match_weight [B,k,h,w] (no gradient)}.

    Scope: match_kernel 3, PONO_C, 256 channels, COCOS_PRECISION=f16x3, plain flag set (no warp_patch / warp_bilinear / cycle terms),
    no prepared exemplar: everything else raises ValueError — there is no fall-back route.  CPU tensors raise CocosHipError.  Not built
    on this route: refine.

    `search` (K57; "dense", the default, is the route as it was, launch for launch): "patchmatch" finds the k candidates without any
    HWxHW tensor of the full grid — the K12 statistics are made once (with autograd; the selector reads their detached values, the
    warp the same tensors), the start is _patchmatch_coarse_init_box3 (the dense readout of the 2 x 2 pooled features, or a random
    start), then ops.patchmatch_topk_box3 runs the schedule on the box logit of single pairs; the warp and its gradients are the same
    K51 on those indices.  The 64- / 128-wide grid requirement of the dense selector is dropped: any grids, equal or not.  Its
    candidates are the best of what it looked at, not of all keys.  `search_opts` overrides entries of
    ops.PATCHMATCH_DEFAULTS.  search="patchmatch" together with restrict or transport raises a ValueError that names search.

    `restrict` (K55; None is the route as it was, launch for launch): "label" or a pair (q_labels [B,h,w], k_labels [B,h,w]) as for
    correspondence_match_box3 — the k candidates are its restricted top-k (the label mask inside the scan of T), the warp and its
    gradients are the same K51 on those indices (idx is data).  It needs the grids the fused box route takes and a topk that
    ops.box3_topk_ok serves (ValueError naming restrict); the result gains match_restricted [B,h,w] bool.  restrict together with
    transport raises ValueError.

    `transport` (K54; None is the route as it was, launch for launch): dict(iters=, tau=) — the candidates are
    correspondence_transport_box3's top-k of z + g and the blend is the softmax over the k pair logits plus g (ops.box3_sparse_softmax_warp
    with k_bias = g).  The potentials are detached: gradients reach theta_raw, phi_raw and the values through the k pair logits and the
    K12 statistics only.  It needs the grids the fused box route takes and a topk that ops.box3_topk_ok serves (ValueError); the result
    gains potential_k [B,h,w] and match_mass [B,h,w]."""
    name = "correspondence_sparse_box3"
    _no_patchmatch_with(name, search, restrict, transport)
    if restrict is not None:      # (first: every scope message of a restricted call names restrict)
        _topk_arg(name, topk)
        _box3_scope(name, "restrict_box3", cfg, False, theta_raw.shape[1], restrict=restrict, transport=transport)
    k = _box3_scope(name, "sparse_box3", cfg, exemplar is not None, theta_raw.shape[1], topk=topk)["topk"]
    pm = _sparse_search(search, search_opts, name)
    if transport is not None:
        iters, tau = _transport_dict(name, transport)
    _same_kind(name, theta_raw, phi_raw)
    B, C, fh, fw, gh, gw, N, Nk = _grids(theta_raw, phi_raw)
    down = cfg.down
    _fused_width(name, theta_raw, phi_raw)
    if k > Nk:
        raise ValueError(f"{name}: topk={k} exceeds the {Nk} exemplar positions")
    if tuple(ref_img.shape[2:]) != (gh * down, gw * down) or ref_img.shape[3] % 4 != 0:
        raise ValueError(f"{name}: ref_img {tuple(ref_img.shape)} is not down={down} times the exemplar grid {(gh, gw)} (width a multiple of 4)")
    if not (_hip_fp32(theta_raw) and _hip_fp32(ref_img)):
        raise ops._lib.CocosHipError(f"{name}: expected CUDA/HIP fp32 tensors; the correspondence hot path has no CPU fallback")
    direct_mask = cfg.warp_mask_losstype == "direct" or cfg.show_warpmask
    extra, g = {}, None
    if restrict is not None:
        labels = _restrict_labels(name, restrict, seg_map, ref_seg_map, down, B, (fh, fw), (gh, gw))
        _box3_fused_shapes(name, "restrict_box3", B, C, fh, fw, gh, gw, k)
        *operands, (idx, _, _, restricted) = _box3_select_and_stats(
            theta_raw, phi_raw, lambda: _restrict_box3_select(theta_raw, phi_raw, 1.0 / temperature, True, labels, k))
        extra = {"match_restricted": restricted.reshape(B, fh, fw)}
        idx = idx.to(torch.int64).contiguous()
    elif pm is not None:      # K57: the statistics first (once, with autograd), the selection on their detached values
        th, ph = _raw(theta_raw), _raw(phi_raw)
        kc = float(C * 9)
        operands = [th, ph, *_unfold3_stats(th, kc), *_unfold3_stats(ph, kc)]
        with torch.no_grad():
            idx, _ = ops.patchmatch_topk_box3(*operands, 1.0 / temperature, k, _patchmatch_coarse_init_box3(th, ph, cfg, temperature, k),
                                              pm["strides"], (pm["radii"], pm["radius0"]), pm["seed"])
            idx = idx.to(torch.int64)
    elif transport is None:
        *operands, m = _box3_select_and_stats(theta_raw, phi_raw, lambda: correspondence_match(theta_raw, phi_raw, cfg, temperature, topk=k))
        with torch.no_grad():
            idx = m.index.reshape(B, k, N).permute(0, 2, 1).contiguous()
            del m
    else:
        _box3_fused_shapes(name, "transport_box3", B, C, fh, fw, gh, gw, k)
        *operands, (f, g, idx, _, row_lse, _) = _box3_select_and_stats(
            theta_raw, phi_raw, lambda: _transport_box3_select(theta_raw, phi_raw, 1.0 / temperature, iters, tau, k, key_mass=False))
        extra = {"potential_k": g.reshape(B, gh, gw), "match_mass": torch.exp(f + row_lse + math.log(N)).reshape(B, fh, fw)}
        idx = idx.to(torch.int64).contiguous()
    with torch.no_grad():
        v = _flat(ops.warp_values(ref_img, ref_seg_map if direct_mask else None, down))
    o, w = ops.box3_sparse_softmax_warp(*operands, v, idx, 1.0 / temperature, return_weights=True, k_bias=g)
    n_ref = ref_img.shape[1]
    y, o_mask = _split_channels(o, n_ref) if direct_mask else (o, None)
    out = {"warp_out": ops.upsample_nearest(y.reshape(B, n_ref, fh, fw), down)}
    if direct_mask:
        out["warp_mask"] = o_mask.reshape(B, -1, fh, fw)
    out["match_index"] = _rank_first(idx, (B, fh, fw), k)
    out["match_weight"] = _rank_first(w, (B, fh, fw), k)
    out.update(extra)
    return out


# ---- K55: label-restricted candidates on the match_kernel-3 route — the mask inside the scan of T ---------------------------------
def _restrict_box3_select(theta_raw, phi_raw, inv_t, rows: bool, labels, k):
    """One _BoxedCorr as correspondence_match's fused match_kernel-3 branch makes it (lazy projections through K25 where allowed), one
    x-box GEMM and one labelled launch -> (idx int32 [B,N,k], val, lse, restricted bool [B,N]), all without gradient; `labels`
    (content, exemplar) [B,N] — the side that asks brings its labels, statistics and labels swap together; T is dropped on return"""
    with torch.no_grad():
        q_eff, k_eff, restricted = restrict_fallback(*(labels if rows else labels[::-1]), k)
        boxed = _boxed(theta_raw, phi_raw, inv_t)
        idx, val, lse = boxed.match_labelled(rows, q_eff, k_eff, k)
        del boxed
        return idx, val, lse, restricted


def correspondence_match_box3(theta_raw, phi_raw, cfg: HotPathConfig, temperature=0.01, *, direction="rows", topk=1, restrict=None,
                              seg_map=None, ref_seg_map=None):
    """correspondence_match(restrict=) on the reference's default route, match_kernel 3 (K55): the hard readout of the box logits with
    every position's candidates kept inside its own region.  `restrict` = None calls correspondence_match on the same arguments
    (its result bit for bit).  "label" takes the majority class of each cell of seg_map / ref_seg_map (cell_labels with cfg.down); a
    pair (q_labels [B,h,w], k_labels [B,h,w]) of int32 / int64 tensors — content side first, whatever the direction — is taken as
    given (a negative content label: unrestricted).  The mask is applied inside the scan of the one x-box tensor T
    (ops.box3_topk_labelled): one x-box GEMM, one labelled launch, T dropped on return; index, logit, prob and lse are over the
    ALLOWED positions.  A position whose label has fewer than topk positions on the other side falls back to the unrestricted scan
    (restrict_fallback); `restricted` [B,h,w] bool says which positions were restricted.  Forward only.  Returns a MatchReadout
    (a TopkMatchReadout for topk > 1).

    Scope: match_kernel 3, PONO_C, COCOS_PRECISION=f16x3, ops.MATCH_FUSED, 256 channels, no prepared exemplar — anything else raises
    a ValueError naming restrict before any tensor is looked at; then equal grids that ops.box3_fused_ok takes and a topk that
    ops.box3_topk_ok serves (ValueError: there is no materialised fall-back).  CPU tensors raise CocosHipError.  Not built:
    restriction together with transport, the flow warp, the match loss or a prepared exemplar."""
    name = "correspondence_match_box3"
    if restrict is None:
        return correspondence_match(theta_raw, phi_raw, cfg, temperature, direction=direction, topk=topk)
    if direction not in ("rows", "cols"):
        raise ValueError(f"{name}: direction {direction!r}: expected 'rows' or 'cols'")
    k = _topk_arg(name, topk)
    _box3_scope(name, "restrict_box3", cfg, False, theta_raw.shape[1], plain_flags=False, restrict=restrict, transport=None)
    _same_kind(name, theta_raw, phi_raw)
    B, C, fh, fw, gh, gw, N, Nk = _grids(theta_raw, phi_raw)
    _fused_width(name, theta_raw, phi_raw)
    rows = direction == "rows"
    if k > (Nk if rows else N):
        raise ValueError(f"{name}: topk={k} exceeds the {Nk if rows else N} positions each row of direction={direction!r} ranges over")
    labels = _restrict_labels(name, restrict, seg_map, ref_seg_map, cfg.down, B, (fh, fw), (gh, gw))
    if not _hip_fp32(theta_raw):
        raise ops._lib.CocosHipError(f"{name}: expected CUDA/HIP fp32 tensors; the correspondence hot path has no CPU fallback")
    _box3_fused_shapes(name, "restrict_box3", B, C, fh, fw, gh, gw, k)
    idx, val, lse, restricted = _restrict_box3_select(theta_raw, phi_raw, 1.0 / temperature, rows, labels, k)
    with torch.no_grad():
        own, other = ((fh, fw), (gh, gw)) if rows else ((gh, gw), (fh, fw))
        return _match_result(idx, val, lse, (B,) + own, other, restricted)


# ---- K54: transport on the match_kernel-3 route — Sinkhorn from one T -------------------------------------------------------------
def _transport_box3_select(theta_raw, phi_raw, inv_t, iters, tau, k, key_mass: bool):
    """One _BoxedCorr as correspondence_match's fused match_kernel-3 branch makes it (lazy projections through K25 where allowed), one
    x-box GEMM, 2 iters + 1 biased launches, one top-k launch when k > 1, one column launch when `key_mass` -> (f, g, idx [B,N,k],
    z [B,N,k], lse [B,N] of z + g, col_lse or None), all without gradient; T is dropped on return"""
    with torch.no_grad():
        boxed = _boxed(theta_raw, phi_raw, inv_t)
        f, g, idx, z, lse = boxed.sinkhorn(iters, tau, readout=True)
        if k > 1:
            idx, z, lse = boxed.match_biased(True, g, k)      # (lse is the last launch's bit for bit)
        col_lse = boxed.match_biased(False, f, 1)[2] if key_mass else None
        del boxed
        return f, g, idx, z, lse, col_lse


def correspondence_transport_box3(theta_raw, phi_raw, cfg: HotPathConfig, temperature=0.01, *, iters=5, tau=1.0, topk=1):
    """correspondence_transport on the reference's default route, match_kernel 3 (K54): the match readout of the entropic transport
    plan over the box logits z — the rows of softmax_q(z[p,q] + g_q) with g the exemplar-side potential of `iters` log-domain Sinkhorn
    iterations under uniform marginals (ops.box3_sinkhorn; tau = 1 balanced, tau < 1 KL-relaxed).  Forward only.  One x-box GEMM, then
    2 iters + 1 biased launches over the one T (the last is the topk = 1 readout), one top-k launch when topk > 1, one column launch
    for key_mass; only one HWxHW tensor is ever alive and it is dropped on return.

    theta_raw, phi_raw: [B,256,h,w] CUDA fp32 or ops.LazyProj1x1.  Returns correspondence_transport's dictionary: `readout` (a
    MatchReadout, or a TopkMatchReadout for topk > 1, over z + g), potential_q (f) and potential_k (g) [B,h,w], match_mass [B,h,w] =
    exp(f + lse) N, key_mass [B,h,w] = exp(g + log sum_p exp(z + f)) N (1 under tau = 1).

    Scope: match_kernel 3, PONO_C, the plain flag set, COCOS_PRECISION=f16x3, ops.MATCH_FUSED, 256 channels, no prepared exemplar —
    anything else raises a ValueError naming box transport before any tensor is looked at; then equal grids that ops.box3_fused_ok
    takes and a topk that ops.box3_topk_ok serves (ValueError: there is no materialised fall-back).  CPU tensors raise CocosHipError."""
    name = "correspondence_transport_box3"
    got = _box3_scope(name, "transport_box3", cfg, False, theta_raw.shape[1], topk=topk, sinkhorn=(iters, tau))
    k, (iters, tau) = got["topk"], got["sinkhorn"]
    _same_kind(name, theta_raw, phi_raw)
    B, C, fh, fw, gh, gw, N, Nk = _grids(theta_raw, phi_raw)
    _fused_width(name, theta_raw, phi_raw)
    if k > Nk:
        raise ValueError(f"{name}: topk={k} exceeds the {Nk} exemplar positions")
    if not _hip_fp32(theta_raw):
        raise ops._lib.CocosHipError(f"{name}: expected CUDA/HIP fp32 tensors; the correspondence hot path has no CPU fallback")
    _box3_fused_shapes(name, "transport_box3", B, C, fh, fw, gh, gw, k)
    f, g, idx, z, lse, col_lse = _transport_box3_select(theta_raw, phi_raw, 1.0 / temperature, iters, tau, k, key_mass=True)
    with torch.no_grad():
        shape = (B, fh, fw)
        return {"readout": _match_result(idx, z, lse, shape, (gh, gw)), "potential_q": f.reshape(shape), "potential_k": g.reshape(B, gh, gw),
                "match_mass": torch.exp(f + lse + math.log(N)).reshape(shape),
                "key_mass": torch.exp(g + col_lse + math.log(Nk)).reshape(B, gh, gw)}


# ---- K50: transport match — entropic optimal transport over the correlation instead of the row softmax ---------------------------
def _transport_dict(name: str, transport):
    """ValueError unless `transport` is a dict with exactly the keys iters (integer in 1..ops.SINKHORN_MAX_ITERS) and tau (0 < tau <= 1)
    -> (iters, tau); the check both transport routes make of the argument"""
    if not isinstance(transport, dict) or set(transport) != {"iters", "tau"}:
        what = sorted(transport) if isinstance(transport, dict) else type(transport).__name__
        raise ValueError(f"{name}: transport={what}: expected None or dict(iters=, tau=)")
    return ops._sinkhorn_args(f"{name}: transport", transport["iters"], transport["tau"])


def _transport_scope(name: str, cfg: HotPathConfig, transport, has_exemplar: bool, search="dense", restrict=None, channels=None):
    """ValueError for a `transport` that is neither None nor a dict with exactly the keys iters (integer in 1..ops.SINKHORN_MAX_ITERS)
    and tau (0 < tau <= 1), and — with one — for everything outside its scope (K50: sparse_warp's route, no prepared exemplar, the
    dense selector, no restriction); checked before any tensor is looked at.  Every message names `transport`."""
    if transport is None:
        return
    _transport_dict(name, transport)
    _route_scope(f"{name}: transport", cfg, "transport", plain_flags=True, match_fused=False)
    if has_exemplar:
        raise ValueError(f"{name}: transport with a prepared exemplar is out of scope (not built)")
    if search != "dense":
        raise ValueError(f"{name}: transport with search={search!r} is out of scope: the potentials live in the dense scan")
    if restrict is not None:
        raise ValueError(f"{name}: transport with restrict is out of scope (not built)")
    _route_channels(f"{name}: transport", "transport", channels)


def correspondence_transport(theta_raw, phi_raw, cfg: HotPathConfig, temperature=0.01, *, iters=5, tau=1.0, topk=1):
    """The match readout of the entropic transport plan over the correlation (K50; UNITE's replacement of CoCosNet's softmax): where
    correspondence_match reads the rows of softmax_j(s_ij), this reads the rows of softmax_j(s_ij + g_j) with g the exemplar-side
    potential of `iters` log-domain Sinkhorn iterations under uniform marginals (ops.corr_sinkhorn; tau = 1 balanced, tau < 1
    KL-relaxed) — an exemplar position that many content positions want pays for it in g.  Forward only, nothing HWxHW.

    theta_raw, phi_raw: [B,256,h,w] CUDA fp32 or ops.LazyProj1x1 (planes from _operand_planes, correspondence_match's producer).
    Returns a dict: `readout`, a MatchReadout (topk = 1) or TopkMatchReadout over z = s + g — index, max_logit / logit = z,
    prob = exp(z - lse), lse = log sum_j exp z_ij; potential_q [B,h,w] (f) and potential_k [B,gh,gw] (g); match_mass [B,h,w] =
    exp(f_i + lse_i) / mu_i, 1 where the row marginal is met; key_mass [B,gh,gw] = exp(g_j + log sum_i exp(s_ij + f_i)) / nu_j, the
    same for the columns (one more column launch): the transported mass each exemplar position receives, 1 under tau = 1.
    Launches: the planes' producer, 2 iters + 1 for the potentials, one top-k over z (topk > 1; with topk = 1 the last row launch
    serves), one column launch.

    Scope: correspondence_sparse's (match_kernel 1, PONO_C, the plain flag set, COCOS_PRECISION=f16x3, 256 channels, positions a
    multiple of 4, no prepared exemplar); everything else raises a ValueError that names transport.  CPU tensors raise CocosHipError."""
    name = "correspondence_transport"
    k = _topk_arg(name, topk)
    _transport_scope(name, cfg, {"iters": iters, "tau": tau}, False, channels=theta_raw.shape[1])
    _same_kind(name, theta_raw, phi_raw)
    B, C, fh, fw, gh, gw, N, Nk = _grids(theta_raw, phi_raw)
    _fused_width(name, theta_raw, phi_raw)
    if k > Nk:
        raise ValueError(f"{name}: topk={k} exceeds the {Nk} exemplar positions")
    if not _hip_fp32(theta_raw):
        raise ops._lib.CocosHipError(f"{name}: expected CUDA/HIP fp32 tensors; the correspondence hot path has no CPU fallback")
    if N % 4 or Nk % 4 or not ops.corr_split_ok(B, C, N, Nk, 1, False) or not ops.corr_topk_ok(k):
        raise ValueError(f"{name}: transport: the fused readout does not take B={B}, {N} x {Nk} positions, topk={k} (positions must be "
                         "multiples of 4), and transport runs on no other route")
    inv_t = 1.0 / temperature
    with torch.no_grad():
        planes = ops.OperandPlanes()
        qn, kn = _operand_planes(theta_raw, phi_raw, planes, detach=True, want_chan=False)
        f, g, row_lse = ops.corr_sinkhorn(qn, kn, inv_t, iters, tau, planes)
        idx, z, lse = ops.corr_topk_biased(qn, kn, g, inv_t, k, planes)       # (k = 1: lse is row_lse bit for bit)
        _, _, col_lse = ops.corr_topk_biased(kn, qn, f, inv_t, 1, planes)
        shape = (B, fh, fw)
        return {"readout": _match_result(idx, z, lse, shape, (gh, gw)), "potential_q": f.reshape(shape), "potential_k": g.reshape(B, gh, gw),
                "match_mass": torch.exp(f + row_lse + math.log(N)).reshape(shape),
                "key_mass": torch.exp(g + col_lse + math.log(Nk)).reshape(B, gh, gw)}


# ---- K46: trainable sub-cell correspondence (a flow-style readout with gradients) --------------------------------------------------
def _flow_scope(cfg: HotPathConfig, radius, refine_temperature):
    """ValueError for everything outside correspondence_flow's scope: correspondence_sparse's flag checks (_sparse_scope, in its words),
    then the window radius and the refinement temperature; checked before any tensor is looked at"""
    _sparse_scope(cfg, 1)
    _radius_arg("correspondence_flow", radius)
    _refine_temperature_arg("correspondence_flow", refine_temperature)


def _flow_result(ref_img, idx, off, lse_win, lse, grid, kgrid, down):
    """correspondence_flow's dictionary (and correspondence_flow_box3's) from the selected centres idx [B,N] (int32 or int64), the refined
    offset off [B,N,2] (with gradient), the window's log-sum-exp and the selection's lse [B,N]"""
    (fh, fw), (gh, gw), B = grid, kgrid, idx.shape[0]
    warp = ops.subcell_warp(ref_img, idx, off, (fh, fw), (gh, gw), down)
    index = idx.to(torch.int64).reshape(B, fh, fw)
    offset = _rank_first(off, (B, fh, fw), 2)
    xy = torch.stack((index % gw, torch.div(index, gw, rounding_mode="floor")), dim=1)
    return {"warp_out": warp, "match_index": index, "match_offset": offset, "match_xy_sub": xy.float() + offset,
            "match_window_prob": torch.exp(lse_win.detach() - lse).reshape(B, fh, fw)}


def correspondence_flow(theta_raw, phi_raw, ref_img, cfg: HotPathConfig, temperature=0.01, *, radius=1, refine_temperature=None,
                        exemplar=None):
    """The trainable sub-cell correspondence (K46): per content position the best exemplar position is SELECTED without gradient (the
    top-1 of ops.corr_topk: correspondence_match's centre), a softmax at `refine_temperature` (None: `temperature`) over the
    (2 radius + 1)^2 window of exemplar positions around it gives a sub-cell offset — ops.soft_match_offset, with gradients to
    theta_raw and phi_raw through the producer of the operand planes, which serve selection and refinement alike — and the exemplar
    is sampled bilinearly at the refined position — ops.subcell_warp, with a gradient to the offset.  A photometric loss on warp_out
    or a regression loss on match_offset therefore trains theta and phi below the feature grid.  Nothing HWxHW is allocated.

    theta_raw, phi_raw: [B,256,h,w] CUDA fp32 or ops.LazyProj1x1; the planes come from _operand_planes, correspondence_match's producer (K23 from a
    lazy pair it takes, K1 otherwise), so match_index and match_offset are correspondence_match(refine=radius)'s bit for bit.
    ref_img [B,3,H,W] gets no gradient (one that requires it raises ValueError).  Returns {warp_out [B,3,H,W], match_index [B,h,w]
    int64, match_offset [B,2,h,w] (x, y; in cells; with gradient), match_xy_sub [B,2,h,w] = match_xy + match_offset (with gradient),
    match_window_prob [B,h,w] (the window's share of the softmax mass; no gradient)}.

    Scope and refusals: correspondence_sparse's (match_kernel 1, PONO_C, the plain flag set, COCOS_PRECISION=f16x3, 256 channels,
    positions a multiple of 4, no prepared exemplar), radius in 1..ops.MATCH_REFINE_MAX_RADIUS: everything else raises ValueError — there
    is no fall-back route.  CPU tensors raise CocosHipError."""
    name = "correspondence_flow"
    _flow_scope(cfg, radius, refine_temperature)
    if exemplar is not None:
        raise ValueError(f"{name}: a prepared exemplar is out of scope (it is forward-only; the refinement differentiates phi)")
    _same_kind(name, theta_raw, phi_raw)
    B, C, fh, fw, gh, gw, N, Nk = _grids(theta_raw, phi_raw)
    down = cfg.down
    _fused_width(name, theta_raw, phi_raw)
    if ref_img.dim() != 4 or ref_img.shape[0] != B or tuple(ref_img.shape[2:]) != (gh * down, gw * down):
        raise ValueError(f"{name}: ref_img {tuple(ref_img.shape)} is not a batch of {B} images of down={down} times the exemplar grid "
                         f"{(gh, gw)}")
    if ref_img.requires_grad:
        raise ValueError(f"{name}: ref_img requires a gradient, and the gradient to the exemplar image is not built (pass ref_img.detach())")
    if not (_hip_fp32(theta_raw) and _hip_fp32(ref_img)):
        raise ops._lib.CocosHipError(f"{name}: expected CUDA/HIP fp32 tensors; the correspondence hot path has no CPU fallback")
    if not ops.corr_split_ok(B, C, N, Nk, 1, False) or not ops.corr_topk_ok(1):
        raise ValueError(f"{name}: the fused readout does not take B={B}, {N} x {Nk} positions (positions must be multiples of 4)")
    planes = ops.OperandPlanes()
    keep = torch.is_grad_enabled() and (theta_raw.requires_grad or phi_raw.requires_grad)
    qn, kn = _operand_planes(theta_raw, phi_raw, planes, detach=False, want_chan=keep)
    inv_t = 1.0 / temperature
    inv_rt = inv_t if refine_temperature is None else 1.0 / refine_temperature
    with torch.no_grad():
        idx, _, lse = ops.corr_topk(qn, kn, inv_t, 1, planes)                  # selection: no gradient
        idx = idx.reshape(B, N)
    off, lse_win = ops.soft_match_offset(qn, kn, idx, (gh, gw), inv_rt, radius, planes)
    return _flow_result(ref_img, idx, off, lse_win, lse.reshape(B, N), (fh, fw), (gh, gw), down)


# ---- K52: the trainable sub-cell correspondence on the match_kernel-3 route ----------------------------------------------------------
def correspondence_flow_box3(theta_raw, phi_raw, ref_img, cfg: HotPathConfig, temperature=0.01, *, radius=1, refine_temperature=None,
                             exemplar=None):
    """correspondence_flow on the reference's default route, match_kernel 3 (K52): per content position the best exemplar position is
    SELECTED without gradient exactly as correspondence_match(theta_raw, phi_raw, cfg, temperature) selects it (that function is
    called: K37 on the one x-box tensor T where ops.box3_fused_ok holds, the materialised chain elsewhere; T is gone when it
    returns), a softmax at `refine_temperature` (None: `temperature`) over the box logits of the (2 radius + 1)^2 window of exemplar
    positions around it gives a sub-cell offset — ops.box3_soft_match_offset, with gradients to theta_raw and phi_raw through the pair
    logits and through the statistics of the unfolded vectors (K12, made here with autograd) — and the exemplar is sampled bilinearly
    at the refined position — ops.subcell_warp, with a gradient to the offset.  Nothing HWxHW is kept for, or allocated in, the backward.

    theta_raw, phi_raw: [B,256,h,w] CUDA fp32 (or ops.LazyProj1x1: the selection takes them as correspondence_match does, the
    refinement projects them).  ref_img [B,3,H,W] gets no gradient (one that requires it raises ValueError).  Returns
    correspondence_flow's dictionary: {warp_out [B,3,H,W], match_index [B,h,w] int64, match_offset [B,2,h,w] (x, y; in cells; with
    gradient), match_xy_sub [B,2,h,w] = match_xy + match_offset (with gradient), match_window_prob [B,h,w] = exp(lse_win - the
    selection's lse) (no gradient)}.

    Scope: match_kernel 3, PONO_C, 256 channels, COCOS_PRECISION=f16x3, plain flag set (no warp_patch / warp_bilinear / cycle terms),
    no prepared exemplar, radius in 1..ops.MATCH_REFINE_MAX_RADIUS: everything else raises ValueError — there is no fall-back route.
    CPU tensors raise CocosHipError.  Not built on this route: top-k centres, restrict, transport, search="patchmatch"."""
    name = "correspondence_flow_box3"
    _box3_scope(name, "flow_box3", cfg, exemplar is not None, theta_raw.shape[1], radius=radius, refine_temperature=refine_temperature)
    _same_kind(name, theta_raw, phi_raw)
    B, C, fh, fw, gh, gw, N, Nk = _grids(theta_raw, phi_raw)
    down = cfg.down
    _fused_width(name, theta_raw, phi_raw)
    if ref_img.dim() != 4 or ref_img.shape[0] != B or tuple(ref_img.shape[2:]) != (gh * down, gw * down):
        raise ValueError(f"{name}: ref_img {tuple(ref_img.shape)} is not a batch of {B} images of down={down} times the exemplar grid "
                         f"{(gh, gw)}")
    if ref_img.requires_grad:
        raise ValueError(f"{name}: ref_img requires a gradient, and the gradient to the exemplar image is not built (pass ref_img.detach())")
    if not (_hip_fp32(theta_raw) and _hip_fp32(ref_img)):
        raise ops._lib.CocosHipError(f"{name}: expected CUDA/HIP fp32 tensors; the correspondence hot path has no CPU fallback")
    inv_rt = 1.0 / (temperature if refine_temperature is None else refine_temperature)
    *operands, m = _box3_select_and_stats(theta_raw, phi_raw, lambda: correspondence_match(theta_raw, phi_raw, cfg, temperature))
    idx, lse = m.index.reshape(B, N), m.lse.reshape(B, N)
    del m
    off, lse_win = ops.box3_soft_match_offset(*operands, idx, (fh, fw), (gh, gw), inv_rt, radius)
    return _flow_result(ref_img, idx, off, lse_win, lse, (fh, fw), (gh, gw), down)


# ---- K49: trainable match readout — the correspondence negative log-likelihood in both softmax directions ---------------------------
def _nll_scope(cfg: HotPathConfig, symmetric=True):
    """ValueError for every flag outside correspondence_nll's scope — correspondence_sparse's, in messages that name match_loss;
    checked before any tensor is looked at"""
    _symmetric_arg("match_loss", symmetric)
    _route_scope("match_loss", cfg, "nll", plain_flags=True, match_fused=False)


def _nll_targets(target, weight, B, fh, fw, Nk, name="match_loss"):
    """target [B,h,w] int32 / int64 with values below Nk (negative: unsupervised), weight [B,h,w] fp32 >= 0 or None — TypeError /
    ValueError in messages that name match_loss (`name`: match_loss_box3's)"""
    if not torch.is_tensor(target) or target.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{name}: target must be an int32 or int64 tensor, got {target.dtype if torch.is_tensor(target) else type(target).__name__}")
    if tuple(target.shape) != (B, fh, fw):
        raise ValueError(f"{name}: target is {tuple(target.shape)}, expected {(B, fh, fw)} (one exemplar position per content cell)")
    if target.numel() and int(target.max()) >= Nk:
        raise ValueError(f"{name}: target holds {int(target.max())}, expected flat exemplar positions below {Nk} (negative: unsupervised)")
    if weight is not None:
        if not torch.is_tensor(weight) or weight.dtype != torch.float32:
            raise TypeError(f"{name}: weight must be a float32 tensor or None, got {weight.dtype if torch.is_tensor(weight) else type(weight).__name__}")
        if tuple(weight.shape) != (B, fh, fw):
            raise ValueError(f"{name}: weight is {tuple(weight.shape)}, expected {(B, fh, fw)}")
        if weight.requires_grad:
            raise ValueError(f"{name}: weight requires a gradient; it is data")
        if weight.numel() and not bool((torch.isfinite(weight) & (weight >= 0)).all()):
            raise ValueError(f"{name}: weight must be finite and >= 0")


def nll_reduce(row_nll, col_nll, target, weight, symmetric: bool):
    """loss_match = sum_i w_i (row_nll_i + [symmetric] col_nll_i) / max(sum over the supervised positions of w_i, tiny); with no
    supervised position the numerator is a sum of zeros that still hangs on the graph: 0 with zero gradients.  Elementwise glue on
    [B,N] tensors."""
    sup = (target >= 0).reshape(row_nll.shape)
    w = sup.to(row_nll.dtype) if weight is None else torch.where(sup, weight.reshape(row_nll.shape), torch.zeros_like(row_nll))
    per = row_nll + col_nll if symmetric else row_nll
    return (w * per).sum() / w.sum().clamp_min(torch.finfo(torch.float32).tiny)


def correspondence_nll(theta_raw, phi_raw, target, cfg: HotPathConfig, temperature=0.01, *, weight=None, symmetric=True, exemplar=None):
    """The supervised correspondence loss (K49): with s_ij = <qn_i, kn_j> / temperature over the projected, centred and normalised
    features, the negative log-likelihood that content position i picks its target t_i among all exemplar positions (match_nll, the
    row softmax) and that exemplar position t_i picks i among all content positions (back_nll, the column softmax) —
    ops.corr_pair_nll, with gradients to theta_raw and phi_raw through the producer of the operand planes.  Nothing HWxHW is
    allocated, forward or backward.

    theta_raw, phi_raw: [B,256,h,w] CUDA fp32 or ops.LazyProj1x1 (planes from _operand_planes, correspondence_mutual's producer: match_lse /
    back_lse are its bit for bit).  target [B,h,w] int32 / int64: flat exemplar position per content cell, negative =
    unsupervised; weight [B,h,w] fp32 >= 0 or None.  Returns {match_nll, back_nll [B,h,w] (0 where unsupervised), match_lse [B,h,w],
    back_lse [B,gh,gw], match_target_prob = exp(-match_nll) (detached), loss_match (see nll_reduce)}.

    Scope and refusals: correspondence_sparse's (match_kernel 1, PONO_C, the plain flag set, COCOS_PRECISION=f16x3, 256 channels,
    positions a multiple of 4, no prepared exemplar); everything else raises ValueError in a message that names match_loss — there is
    no fall-back route.  CPU tensors raise CocosHipError."""
    name = "match_loss"
    _nll_scope(cfg, symmetric)
    if exemplar is not None:
        raise ValueError(f"{name}: a prepared exemplar is out of scope (it is forward-only; the loss differentiates phi)")
    _same_kind(name, theta_raw, phi_raw)
    B, C, fh, fw, gh, gw, N, Nk = _grids(theta_raw, phi_raw)
    _fused_width(name, theta_raw, phi_raw)
    _nll_targets(target, weight, B, fh, fw, Nk)
    if not (_hip_fp32(theta_raw) and target.is_cuda and (weight is None or weight.is_cuda)):
        raise ops._lib.CocosHipError(f"{name}: expected CUDA/HIP tensors (fp32 features); the correspondence hot path has no CPU fallback")
    if not ops.corr_split_ok(B, C, N, Nk, 1, False) or not ops.corr_match_mutual_ok(B, N, Nk):
        raise ValueError(f"{name}: the fused sweep does not take B={B}, {N} x {Nk} positions (positions must be multiples of 4)")
    planes = ops.OperandPlanes()
    keep = torch.is_grad_enabled() and (theta_raw.requires_grad or phi_raw.requires_grad)
    qn, kn = _operand_planes(theta_raw, phi_raw, planes, detach=False, want_chan=keep)
    tgt = target.reshape(B, N)
    row_nll, col_nll, row_lse, col_lse = ops.corr_pair_nll(qn, kn, tgt, 1.0 / temperature, planes, return_lse=True, check_target=False)
    return {"match_nll": row_nll.reshape(B, fh, fw), "back_nll": col_nll.reshape(B, fh, fw), "match_lse": row_lse.reshape(B, fh, fw),
            "back_lse": col_lse.reshape(B, gh, gw), "match_target_prob": torch.exp(-row_nll.detach()).reshape(B, fh, fw),
            "loss_match": nll_reduce(row_nll, col_nll, tgt, weight, symmetric)}


# ---- K53: the supervised match loss on the match_kernel-3 route ----------------------------------------------------------------------
def correspondence_nll_box3(theta_raw, phi_raw, target, cfg: HotPathConfig, temperature=0.01, *, weight=None, symmetric=True, exemplar=None):
    """correspondence_nll on the reference's default route, match_kernel 3 (K53): with z[p,q] the box logit of the 3x3-unfolded,
    centred, normalised vectors over the temperature, match_nll = lse_q z[p,.] - z[p,t_p] and back_nll = lse_p z[.,t_p] - z[p,t_p].
    The two log-sum-exp vectors are read from the one x-box tensor T exactly as correspondence_match reads them (ops.box3_lse: K37's
    launch; the column direction reads T transposed), the target logit comes from the pair unit on fp32 rows (ops.box3_pair_logits),
    and the column lse is gathered at the target in a fixed order (ops.box3_gather_keys).  In the backward both lse passes write into
    ONE gradient of T (cocos_box3_lse_bwd_f16x3 under the Box3GradSink), so one box adjoint and one pair of GEMMs serve them.

    Memory: T is saved for the backward and its gradient G is allocated there — two HWxHW fp32 tensors, the dense match_kernel-3
    step's budget (unlike correspondence_nll, whose route keeps nothing HWxHW).  Precision: the target logit is formed in fp32 rows,
    the lse from the f16x3 T, so on a one-hot row match_nll can come out slightly NEGATIVE; it is not clamped.

    theta_raw, phi_raw: [B,256,h,w] CUDA fp32 or ops.LazyProj1x1, equal grids; target [B,h,w] int32 / int64: flat exemplar position
    per content cell, negative = unsupervised; weight [B,h,w] fp32 >= 0 or None.  Returns correspondence_nll's dictionary.  With
    symmetric=False the column direction is out of the loss: back_lse / back_nll are still reported, detached, at the cost of one
    more forward-only readout launch over T (K37, transposed) — no second lse backward, no accumulate pass.

    Scope: match_kernel 3, PONO_C, 256 channels, COCOS_PRECISION=f16x3, the plain flag set, no prepared exemplar, equal 64- or
    128-wide grids that ops.box3_fused_ok takes: everything else raises ValueError in a message that names match_loss_box3 — there is
    no fall-back to the materialised chain.  CPU tensors raise CocosHipError."""
    name = "match_loss_box3"
    _box3_scope(name, "nll_box3", cfg, exemplar is not None, lambda: theta_raw.shape[1], symmetric=symmetric)
    _same_kind(name, theta_raw, phi_raw)
    B, C, fh, fw, gh, gw, N, Nk = _grids(theta_raw, phi_raw)
    _fused_width(name, theta_raw, phi_raw)
    _nll_targets(target, weight, B, fh, fw, Nk, name)
    if not (_hip_fp32(theta_raw) and _hip_fp32(phi_raw) and target.is_cuda and (weight is None or weight.is_cuda)):
        raise ops._lib.CocosHipError(f"{name}: expected CUDA/HIP tensors (fp32 features); the correspondence hot path has no CPU fallback")
    _box3_fused_shapes(name, "nll_box3", B, C, fh, fw, gh, gw)
    inv_t = 1.0 / temperature
    th, ph = _raw(theta_raw), _raw(phi_raw)      # the fp32 projections the pair unit reads (K0 with autograd; cached by the handle)
    # T and the statistics as correspondence_match makes them (the lse vectors are its readout's bit for bit), with autograd
    boxed = _boxed(theta_raw, phi_raw, inv_t, grad=True)      # the lse passes share one G
    (mu, a), (nu, b) = boxed.stats()
    tgt = target.reshape(B, N)
    row_lse = boxed.lse(True)
    col_lse = boxed.lse(False) if symmetric else None
    z_t = ops.box3_pair_logits(th, ph, mu, a, nu, b, tgt, inv_t)
    sup = tgt >= 0
    zero = torch.zeros((), device=z_t.device, dtype=z_t.dtype)
    row_nll = torch.where(sup, row_lse - z_t, zero)
    if symmetric:
        col_nll = torch.where(sup, ops.box3_gather_keys(col_lse, tgt) - z_t, zero)
    else:
        with torch.no_grad():
            col_lse = boxed.match(False)[2]
            col_nll = torch.where(sup, torch.gather(col_lse, 1, tgt.clamp_min(0).long()) - z_t.detach(), zero)
    return {"match_nll": row_nll.reshape(B, fh, fw), "back_nll": col_nll.reshape(B, fh, fw), "match_lse": row_lse.reshape(B, fh, fw),
            "back_lse": col_lse.reshape(B, gh, gw), "match_target_prob": torch.exp(-row_nll.detach()).reshape(B, fh, fw),
            "loss_match": nll_reduce(row_nll, col_nll, tgt, weight, symmetric)}
