"""torch.autograd bindings of the HIP kernels (host side above the C ABI).

PyTorch here is plumbing only: it owns device memory, the stream and the autograd graph; every
piece of arithmetic on the path is a hand-written gfx950 kernel reached through ctypes.
All feature tensors are channel-major [B, C, positions] fp32 — what `x.view(B, C, -1)` gives in
the reference (models/networks/correspondence.py:274,284).
"""
from __future__ import annotations

import ctypes
import math
import os
import sys
import threading
import weakref

import torch

from . import _lib

_C = _lib.CONSTANTS      # the integer #defines of include/cocos_hip.h
#: K1's `center_over_channels`: the mean over the positions of a channel, over the channels of a position (PONO_C), or none
CENTER_POSITIONS, CENTER_CHANNELS, CENTER_NONE = _C["COCOS_CENTER_POSITIONS"], _C["COCOS_CENTER_CHANNELS"], _C["COCOS_CENTER_NONE"]
#: `sys.float_info.epsilon`, the constant the reference adds to the norm (correspondence.py:279,288)
NORM_EPS = sys.float_info.epsilon
#: widest V the fused kernel takes in one launch (5 blocks of 32 channels)
MAX_FUSED_CV = 160
#: ... of the split-precision forward: one padding channel of the V tile carries the softmax row sums
MAX_FUSED_SPLIT_CV = 159
#: largest dS^T scratch (bytes) the EXACT-FP32 backward may allocate to replace the second logits recompute by
#: a GEMM; above it (e.g. 128x128 grids at large batch) the flash-style key kernel is used
MAX_DS_WORKSPACE_BYTES = 16 << 30
#: split flavour: a training forward SAVES its logits (B*Nq*Nk*4 bytes, and the backward as much again for the dS'' planes)
#: only up to this size; above it the forward keeps the row LSE alone and the backward RECOMPUTES the logits, one chunk of keys
#: at a time (round 4: _corr_bwd_recompute — same kernels, HWxHW scratch bounded by RECOMPUTE_CHUNK_BYTES per matrix).
#: Measured A/B at the three BASELINE shapes (profiles/r04_configs_bench.json): the saved-logits chain is 24 % (cfg2), 33 % (cfg3)
#: and 45-68 % (cfg5) FASTER where it fits, so the default is speed first on a 288 GB part — 16 GiB, the cap of rounds 1-3, beyond
#: which this route now replaces the exact-fp32 flash kernels; COCOS_MAX_SAVED_LOGITS_BYTES=1073741824 puts BASELINE config 5
#: (1 GiB of logits PER SAMPLE) on the bounded-memory route: 4.3 -> 2.5 GiB peak.  Module attribute, read at call time.
MAX_SAVED_LOGITS_BYTES = int(os.environ.get("COCOS_MAX_SAVED_LOGITS_BYTES", 16 << 30))
#: ... the recomputed logits / dS'' / P planes of one key chunk (bytes per matrix).  1 GiB: at HW = 16384, B = 2 a chunk is 8192
#: keys — the key-side GEMM of a chunk still has 128 workgroups (512 MiB chunks: 64 workgroups, its time tripled)
RECOMPUTE_CHUNK_BYTES = int(os.environ.get("COCOS_RECOMPUTE_CHUNK_BYTES", 1 << 30))
#: split K2 backward: D = sum_c dout * out per query from a streaming kernel (cocos_rowdot_f64) instead of the query kernel's own
#: serial fp64 prologue; "0": the round-3 form (A/B runs)
BWD_D_PRECOMPUTED = True
#: channel count the fused kernels are specialised for (self.inter_channels, correspondence.py:170)
FUSED_K = 256
#: where the K2 forward's products run: "fp32" = v_mfma_f32_32x32x2_f32 (exact fp32 operands);
#: "f16x3" = v_mfma_f32_32x32x16_f16 on f16 hi+lo planes, 3 terms per product, fp32 accumulate
#: (fp32-class accuracy, ~1/5 of the matrix-pipe time).  Module attribute, read at call time.
PRECISION = os.environ.get("COCOS_PRECISION", "f16x3")
#: K0 (theta/phi 1x1 projections): "fp32" = the fp32-MFMA GEMM (on par with rocBLAS); "f16x3" = split products on
#: the f16 MFMA — the streaming kernels below at the reference's shapes, else the split GEMM of sgemm_f16x3.hip
#: (operands split on the fly, staged pieces converted/committed between MFMAs).
PROJ_PRECISION = os.environ.get("COCOS_PROJ_PRECISION", "f16x3")
# ---- switches below WITHOUT an environment variable are test / A-B hooks: plain module attributes, read at call time, every
# ---- non-default value covered by a GPU test (the env surface is COCOS_PRECISION, COCOS_PROJ_PRECISION,
# ---- COCOS_CONV, COCOS_MAX_SAVED_LOGITS_BYTES, COCOS_RECOMPUTE_CHUNK_BYTES and COCOS_LIB_PATH)
#: K2 split kernels: test V's f16 lo plane per 32-channel block and skip all-zero blocks (exact label / mask channels)
VALUE_LO_SKIP = True
#: K2 split forward: True = the QK MFMAs of key tile t+1 run under the softmax arithmetic of tile t ("QK ahead", whole-tile key counts
#: of the unit-norm flavour); False = QK, softmax, P.V of a tile in turn.  Bit-identical results (tests/test_gpu_fwd_qk_ahead.py); the
#: default is the library's (COCOS_FWD_QK_AHEAD_DEFAULT), the selection is handed to it before every forward call
FWD_QK_AHEAD = bool(_lib.CONSTANTS["COCOS_FWD_QK_AHEAD_DEFAULT"])
#: K0 at the reference's own shapes (<= 416 input channels, HW % 64 == 0): y = W x and dx = W^T dy on the streaming
#: kernel (proj_stream_f16x3.hip: weight planes resident in the accumulator file, x / y touched once), dw + db as one
#: streaming reduction (proj_dw_f16x3.hip).  "0" = the general split GEMM everywhere (A/B, tests).
PROJ_STREAM = True
#: power-of-two pre-scale of the unit-norm operands before the f16 split (keeps the lo plane normal)
SPLIT_OPERAND_SCALE = 16.0
#: K36 match readout (hot_path.correspondence_match): True = the fused kernel (K36a: nothing HWxHW in memory) wherever the
#: split-precision correlation runs; False = every route materialises its logits and reads them with K36b
MATCH_FUSED = True


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _select_fwd_schedule():
    """FWD_QK_AHEAD -> the library's process-wide selection (a host-side store: no launch, no device memory)"""
    _lib.load().cocos_corr_fwd_f16x3_qk_ahead(1 if FWD_QK_AHEAD else 0)


class KernelTimer:
    """Brackets every C-ABI call with HIP events on the stream the kernels are launched on (torch's
    current stream) and reports the average device time per entry point — bench.py's live source
    for `roofline.achieved`.  Use as a context manager; call summary() after a synchronize."""

    active = None

    def __init__(self, tags=None):
        """`tags`: only these entry-point tags are bracketed (every HIP event is a marker packet in the queue that
        serialises the dispatch around it: ~3.5 us each, 8 % of the benchmark step when all ~40 calls are
        bracketed); None = all."""
        self.events = {}
        self.tags = None if tags is None else frozenset(tags)

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *exc):
        KernelTimer.active = None

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for tag, evs in self.events.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            out[tag] = {"calls": len(ms), "avg_ms": sum(ms) / len(ms), "total_ms": sum(ms), "min_ms": min(ms)}
        return out


def _call(tag, name, *args):
    t = KernelTimer.active
    if t is None or (t.tags is not None and tag not in t.tags):
        return _lib.call(name, *args)
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.call(name, *args)
    e1.record()
    t.events.setdefault(tag, []).append((e0, e1))


def _chk(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.CocosHipError(
            f"{name}: expected a CUDA/HIP tensor; the correspondence hot path has no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    return t.contiguous()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------
# K1  centre + L2-normalise            (correspondence.py:277-280, :287-289)
# ------------------------------------------------------------------------------------------
class _CenterL2Norm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, center_over_channels: int, eps: float):
        x = _chk(x, "center_l2norm: x")
        B, K, N = x.shape
        y = torch.empty_like(x)
        norm = torch.empty((B, N), device=x.device, dtype=torch.float32)
        center_over_channels = int(center_over_channels)      # CENTER_*
        row_ws = None if center_over_channels != CENTER_POSITIONS else torch.empty((B, K), device=x.device,
                                                                dtype=torch.float32)
        _call("center_l2norm_fwd", "cocos_center_l2norm_fwd", x.data_ptr(), y.data_ptr(), norm.data_ptr(),
                  _ptr(row_ws), B, K, N, int(center_over_channels), float(eps), _stream())
        ctx.save_for_backward(y, norm)
        ctx.cfg = (center_over_channels, float(eps))
        return y

    @staticmethod
    def backward(ctx, dy):
        y, norm = ctx.saved_tensors
        center_over_channels, eps = ctx.cfg
        dy = _chk(dy, "center_l2norm: dy")
        B, K, N = y.shape
        dx = torch.empty_like(y)
        col_ws = row_ws = None
        if center_over_channels == CENTER_POSITIONS:
            col_ws = torch.empty((B, N), device=y.device, dtype=torch.float32)
            row_ws = torch.empty((B, K), device=y.device, dtype=torch.float32)
        # max|dx| as a by-product: K0's backward (the consumer on the theta/phi path) needs it.  Mode 2
        # (feature_normalize) feeds MIOpen convolutions: nobody would pick the value up
        if PROJ_PRECISION == "f16x3" and center_over_channels != CENTER_NONE:
            cell = _zero_cell(dx.device)
            _call("center_l2norm_bwd", "cocos_center_l2norm_bwd_amax", y.data_ptr(), norm.data_ptr(), dy.data_ptr(),
                  dx.data_ptr(), _ptr(col_ws), _ptr(row_ws), B, K, N, int(center_over_channels), eps,
                  cell.data_ptr(), _stream())
            _remember_amax(dx, cell)
        else:
            _call("center_l2norm_bwd", "cocos_center_l2norm_bwd", y.data_ptr(), norm.data_ptr(), dy.data_ptr(),
                  dx.data_ptr(), _ptr(col_ws), _ptr(row_ws), B, K, N, int(center_over_channels),
                  eps, _stream())
        return dx, None, None


def center_l2norm(x: torch.Tensor, center_over_channels, eps: float = NORM_EPS):
    """x [B,K,N] -> (x - mean) / (||x - mean||_2 over K + eps); mean over K (True / 1: PONO_C), over N
    (False / 0) or no centring at all (2): CENTER_CHANNELS, CENTER_POSITIONS, CENTER_NONE."""
    return _CenterL2Norm.apply(x, int(center_over_channels), eps)


def feature_normalize(x: torch.Tensor, eps: float = NORM_EPS):
    """util.feature_normalize (util/util.py:31-34): x [B,C,h,w] / (||x||_2 over C + eps) — K1 without
    the centring; used on the adaptor outputs right before the ResidualBlocks (correspondence.py:247-248)."""
    B, C = x.shape[:2]
    return _CenterL2Norm.apply(x.reshape(B, C, -1), CENTER_NONE, eps).reshape(x.shape)




class _CenterL2NormPlanes(torch.autograd.Function):
    """K1 for the split flavour: x [B,256,N] -> operand planes (handed to the caller's OperandPlanes) + norms.  The autograd
    OUTPUT is only a handle: a view of x (no new memory) whose VALUES are x's, not the normalised tensor's — the split
    correlation kernels never read it, they read the planes; its gradient (d qn from K2's backward) comes back here."""

    @staticmethod
    def forward(ctx, x, center_over_channels: int, eps: float, planes, want_chan: bool):
        x = _chk(x, "center_l2norm_planes: x")
        B, K, N = x.shape
        half = dict(device=x.device, dtype=torch.float16)
        norm = torch.empty((B, N), device=x.device, dtype=torch.float32)
        ph, pl = torch.empty((B, N, K), **half), torch.empty((B, N, K), **half)
        ch = cl = None
        if want_chan:
            ch, cl = torch.empty((B, K, N), **half), torch.empty((B, K, N), **half)
        _call("center_l2norm_fwd", "cocos_center_l2norm_fwd_planes", x.data_ptr(), norm.data_ptr(), ph.data_ptr(),
              pl.data_ptr(), _ptr(ch), _ptr(cl), B, K, N, int(center_over_channels), float(eps), SPLIT_OPERAND_SCALE, _stream())
        handle = x.view_as(x)
        planes.put(handle, True, SPLIT_OPERAND_SCALE, ph, pl)
        if want_chan:
            planes.put(handle, False, SPLIT_OPERAND_SCALE, ch, cl)
        ctx.save_for_backward(norm, ch, cl)
        ctx.cfg = (int(center_over_channels), float(eps))
        return handle

    @staticmethod
    def backward(ctx, dy):
        norm, ch, cl = ctx.saved_tensors
        mode, eps = ctx.cfg
        dy = _chk(dy, "center_l2norm_planes: dy")
        B, K, N = dy.shape
        if ch is None:
            raise _lib.CocosHipError("center_l2norm_planes: backward without the channel-major planes (forward ran without grad)")
        dx = torch.empty_like(dy)
        cell = _zero_cell(dx.device) if PROJ_PRECISION == "f16x3" else None
        _call("center_l2norm_bwd", "cocos_center_l2norm_bwd_planes", ch.data_ptr(), cl.data_ptr(), norm.data_ptr(),
              dy.data_ptr(), dx.data_ptr(), B, K, N, mode, eps, SPLIT_OPERAND_SCALE, _ptr(cell), _stream())
        if cell is not None:
            _remember_amax(dx, cell)
        return dx, None, None, None, None


def center_l2norm_planes(x: torch.Tensor, center_over_channels, planes: OperandPlanes, eps: float = NORM_EPS,
                         want_chan=None):
    """K1 whose only products are the operand planes of the split correlation kernels (registered in `planes`) — see
    _CenterL2NormPlanes.  Returns the autograd handle to pass to corr_softmax_warp(..., planes=planes) as qn / kn.  Only
    for callers that take the split path (corr_split_ok).

    `want_chan`: also write the channel-major planes.  The K2 backward reads them of BOTH operands as soon as EITHER
    theta or phi is differentiated (d qn contracts dS with kn's planes and vice versa), so a caller with two operands
    passes its `keep` (= either requires grad) for both; None = this tensor's own requires_grad (single-operand use)."""
    if want_chan is None:
        want_chan = torch.is_grad_enabled() and x.requires_grad
    return _CenterL2NormPlanes.apply(x, int(center_over_channels), eps, planes, bool(want_chan))


def center_l2norm_planes_fwd(x: torch.Tensor, center_over_channels, eps: float = NORM_EPS):
    """K1's planes flavour, forward only and without an autograd node (inference with a prepared exemplar): x [B,256,N] ->
    (pos_hi, pos_lo [B,N,256] of SPLIT_OPERAND_SCALE * y, norm [B,N]).  Only on the split path (corr_split_ok)."""
    x = _chk(x.detach(), "center_l2norm_planes: x")
    B, K, N = x.shape
    norm = torch.empty((B, N), device=x.device, dtype=torch.float32)
    ph = torch.empty((B, N, K), device=x.device, dtype=torch.float16)
    pl = torch.empty((B, N, K), device=x.device, dtype=torch.float16)
    _call("center_l2norm_fwd", "cocos_center_l2norm_fwd_planes", x.data_ptr(), norm.data_ptr(), ph.data_ptr(), pl.data_ptr(), None, None,
          B, K, N, int(center_over_channels), float(eps), SPLIT_OPERAND_SCALE, _stream())
    return ph, pl, norm


def corr_split_ok(B, K, Nq, Nk, Cv, keep: bool) -> bool:
    """True when corr_softmax_warp takes the split-precision kernels for this shape (forward and, when `keep`, backward):
    the condition under which qn / kn may exist as operand planes only."""
    chunk = min(Cv, MAX_FUSED_SPLIT_CV)
    return (PRECISION == "f16x3" and K == FUSED_K and Nk % 4 == 0 and Nq % 4 == 0
            and (not keep or (_split_bwd_ok(B, Nq, Nk, chunk) and _split_bwd_ok(B, Nk, Nq, chunk))))


# ------------------------------------------------------------------------------------------
# K2  fused correlation -> softmax -> warp     (correspondence.py:291,:304,:307,:318)
# ------------------------------------------------------------------------------------------
class OperandPlanes:
    """f16 hi/lo operand planes of the theta/phi tensors of ONE forward call, made on first use and shared by the up
    to three launches that read them (row pass, column pass, second row pass).  Owned by the caller (hot_path's
    _Attention), so there is no process-global cache: under the reference's DataParallelWithCallback every replica
    thread has its own object (SURVEY.md §8b threading contract)."""

    def __init__(self):
        self._planes = {}

    def put(self, x: torch.Tensor, transpose: bool, scale: float, hi: torch.Tensor, lo: torch.Tensor):
        """Planes a producer kernel wrote itself (K1's planes flavour): later get() calls for `x` return them."""
        self._planes[(id(x), bool(transpose), float(scale))] = (x, x._version, hi, lo, True)

    def get(self, x: torch.Tensor, transpose: bool, scale: float):
        key = (id(x), bool(transpose), float(scale))
        ent = self._planes.get(key)
        if ent is not None and ent[0] is x and len(ent) > 4:
            # producer-made planes: x is only a handle (its VALUES are not what the planes hold), they cannot be re-made
            if ent[1] != x._version:
                raise _lib.CocosHipError("OperandPlanes: the tensor behind producer-made operand planes was modified in place")
            return ent[2], ent[3]
        if ent is None and any(k[0] == id(x) and len(e) > 4 and e[0] is x for k, e in self._planes.items()):
            # x is a producer's HANDLE (its values are the raw features, not the normalised tensor): splitting it here
            # would hand the kernels planes of the wrong tensor — the producer must be asked for this orientation
            raise _lib.CocosHipError(
                f"OperandPlanes: {'position' if transpose else 'channel'}-major planes (scale {scale}) of a tensor that exists "
                "as producer-made planes only were not written by the producer (center_l2norm_planes(..., want_chan=True))")
        if ent is None or ent[0] is not x or ent[1] != x._version:
            hi, lo = split_f16(x, transpose, scale)
            ent = self._planes[key] = (x, x._version, hi, lo)     # holds x: its id cannot be recycled meanwhile
        return ent[2], ent[3]

    def get_scaled(self, x: torch.Tensor, transpose: bool):
        """Planes with a DEVICE-side power-of-two scale from max|x| (operands without an a-priori magnitude):
        (hi, lo, scale_tensor).  The scale depends on x only, so both orientations of x share it."""
        key = (id(x), bool(transpose), "amax")
        ent = self._planes.get(key)
        if ent is None or ent[0] is not x or ent[1] != x._version:
            am = self._planes.get((id(x), "amax_cell"))
            if am is None or am[0] is not x or am[1] != x._version:
                am = self._planes[(id(x), "amax_cell")] = (x, x._version, absmax(x))
            hi, lo, sc = split_f16(x, transpose, amax=am[2])
            ent = self._planes[key] = (x, x._version, hi, lo, sc)
        return ent[2], ent[3], ent[4]

    def has(self, x: torch.Tensor) -> bool:
        return any(k[0] == id(x) and e[0] is x for k, e in self._planes.items())

    def __len__(self):
        return len(self._planes)


def split_f16(x: torch.Tensor, transpose: bool, scale: float = 1.0, cpad=None, amax=None):
    """x [B,C,N] fp32 -> (hi, lo) f16 planes with x*scale ~= hi + lo; [B,N,C] when `transpose`.
    `cpad` (transpose only): rows padded with zero channels to cpad.  `amax`: a 1-element CUDA tensor
    holding max|x|; the scale is then chosen on the device (power of two, max -> [2^9, 2^10)) and the
    call returns (hi, lo, scale_tensor)."""
    x = _chk(x, "split_f16: x")
    B, C, N = x.shape
    if cpad is not None or amax is not None:
        cp = C if cpad is None else int(cpad)
        shape = (B, N, cp) if transpose else (B, C, N)
        hi = torch.empty(shape, device=x.device, dtype=torch.float16)
        lo = torch.empty(shape, device=x.device, dtype=torch.float16)
        sc = torch.empty(1, device=x.device, dtype=torch.float32) if amax is not None else None
        _call("split_f16", "cocos_split_f16_ex", x.data_ptr(), hi.data_ptr(), lo.data_ptr(), B, C, N, cp,
              int(bool(transpose)), float(scale), _ptr(amax), _ptr(sc), _stream())
        return (hi, lo, sc) if amax is not None else (hi, lo)
    shape = (B, N, C) if transpose else (B, C, N)
    hi = torch.empty(shape, device=x.device, dtype=torch.float16)
    lo = torch.empty(shape, device=x.device, dtype=torch.float16)
    _call("split_f16", "cocos_split_f16", x.data_ptr(), hi.data_ptr(), lo.data_ptr(), B, C, N, int(bool(transpose)),
          float(scale), _stream())
    return hi, lo


def split_f16_chan_mask(x: torch.Tensor, amax: torch.Tensor, want_mask: bool):
    """x [B,C,N] -> (hi, lo, scale_tensor, mask_cell | None): the channel-major planes of split_f16(x, False, amax=amax) and,
    when `want_mask`, f16_plane_block_mask(lo), in ONE launch (cocos_split_f16_chan_mask; N % 4 == 0, else two launches)."""
    x = _chk(x, "split_f16_chan_mask: x")
    B, C, N = x.shape
    if N % 4 != 0 or C > 1024 or x.data_ptr() % 16 != 0:
        hi, lo, sc = split_f16(x, False, amax=amax)
        return hi, lo, sc, (f16_plane_block_mask(lo) if want_mask else None)
    hi = torch.empty((B, C, N), device=x.device, dtype=torch.float16)
    lo = torch.empty((B, C, N), device=x.device, dtype=torch.float16)
    sc = torch.empty(1, device=x.device, dtype=torch.float32)
    mask = _zero_cell(x.device) if want_mask else None          # fp32 zero = integer zero
    _call("split_f16", "cocos_split_f16_chan_mask", x.data_ptr(), hi.data_ptr(), lo.data_ptr(), B, C, N, amax.data_ptr(),
          sc.data_ptr(), _ptr(mask), _stream())
    return hi, lo, sc, mask


def f16_plane_block_mask(plane: torch.Tensor) -> torch.Tensor:
    """plane [B,C,N] f16 (channel-major) -> 1-element int32 CUDA tensor whose bit (c >> 5) says "channel block c//32 has
    a non-zero element" (cocos_f16_plane_block_mask; no host sync)."""
    B, C, N = plane.shape
    cell = _zero_cell(plane.device)                      # fp32 zero = integer zero
    _call("f16_plane_block_mask", "cocos_f16_plane_block_mask", plane.data_ptr(), B, C, N, cell.data_ptr(), _stream())
    return cell


def _recompute_chunk(B, Nq, Nk):
    """Keys per chunk of the recompute backward: whole 128-key groups (blocked planes), RECOMPUTE_CHUNK_BYTES per matrix."""
    per_key = max(B * Nq * 4, 1)
    nchunks = max(1, -(-(per_key * Nk) // max(RECOMPUTE_CHUNK_BYTES, 1)))      # equal chunks: the last one is not a sliver
    kc = max(128, -(-Nk // nchunks) // 128 * 128 + (128 if (-(-Nk // nchunks)) % 128 else 0))
    return min(kc, (Nk + 127) // 128 * 128)


def _saves_logits(B, Nq, Nk) -> bool:
    """Split flavour: does a training forward of this shape save its logits (else: LSE only, chunked recompute)?"""
    return (B * Nq * Nk * 4 <= MAX_SAVED_LOGITS_BYTES
            and _lib.load().cocos_corr_softmax_warp_saved_logits_bytes(1, Nq, Nk) < 2 ** 31 - 1)


def _split_bwd_ok(B, Nq, Nk, Cv):
    """Shapes the split-precision K2 backward takes (cocos_corr_softmax_warp_bwd_query_f16x3 + the planes GEMM) — with saved
    logits, or by recomputing them chunk by chunk (any size whose per-sample chunk stays below 2 GiB)."""
    if not (Nk % 8 == 0 and Nq % 8 == 0 and Cv <= MAX_FUSED_CV):
        return False
    if _saves_logits(B, Nq, Nk):
        return True
    return Nk % 128 == 0 and Nq % 32 == 0 and Nq * _recompute_chunk(B, Nq, Nk) * 4 < 2 ** 31 - 1


GEMM_SPLIT_K_BELOW = 200      # workgroups: a backward GEMM with fewer tiles than this splits its reduction (256 CUs to fill)


def _hgemm_planes(timer, ah, al, bh, bl, out, M, n, Kred, host, dev1, dev2, bmode, st):
    """out[b] (M x n) = A[b] (M x Kred) . B[b] (Kred x n) on the split GEMM (cocos_hgemm_f16x3), A = channel-major planes [B,M,Kred].
    With [query][key]-blocked B planes (bmode 2) and too few 256 x 128 output tiles to fill the chip (the Attention block:
    M = C/8 rows, B = 4 samples -> 128 workgroups on 256 CUs, each streaming all of Kred) the reduction is cut into S
    contiguous slices that run as S * B "samples" (a slice of a blocked plane is contiguous, so only A is re-laid out) and the
    S partial products are summed in a fixed order: deterministic."""
    B = out.shape[0]
    tiles = B * ((M + 255) // 256) * ((n + 127) // 128)
    S = 1
    while bmode == 2 and tiles * S < GEMM_SPLIT_K_BELOW and S < 8 and Kred % (64 * S) == 0:
        S *= 2
    if S == 1:
        _call(timer, "cocos_hgemm_f16x3", ah.data_ptr(), al.data_ptr(), bh.data_ptr(), bl.data_ptr(), out.data_ptr(), B, M, n, Kred,
              host, _ptr(dev1), _ptr(dev2), bmode, st)
        return
    a2h = ah.view(B, M, S, Kred // S).transpose(1, 2).contiguous()
    a2l = al.view(B, M, S, Kred // S).transpose(1, 2).contiguous()
    part = torch.empty((B, S, M, n), device=out.device, dtype=torch.float32)
    _call(timer, "cocos_hgemm_f16x3", a2h.data_ptr(), a2l.data_ptr(), bh.data_ptr(), bl.data_ptr(), part.data_ptr(), B * S, M, n,
          Kred // S, host, _ptr(dev1), _ptr(dev2), bmode, st)
    torch.sum(part, dim=1, out=out)


def _key_gemm(qch, qcl, dsh, dsl, dk, n, Nq, k_active, qks, ds_scale, gemm_b, st):
    """dk[b] = (q_scale qn)[b] . dS''[b] on the split GEMM (K5's key side); qch / qcl / dk have the REAL channel count (the
    magnitude-free flavour's K < 256: M = K rows, see _hgemm_planes for what that means for the launch)."""
    K = dk.shape[1]
    assert qch.shape[1] == K and (not k_active or k_active == K)
    _hgemm_planes("corr_softmax_warp_bwd_key_from_ds", qch, qcl, dsh, dsl, dk, K, n, Nq, 1.0 if qks else 1.0 / SPLIT_OPERAND_SCALE,
                  ds_scale, qks[0] if qks else None, gemm_b, st)


class _CorrSoftmaxWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qn, kn, v, inv_temperature: float, keep_logits: bool, planes=None):
        qn, kn, v = _chk(qn, "qn"), _chk(kn, "kn"), _chk(v, "v")
        B, K, Nq = qn.shape
        Bk, Kk, Nk = kn.shape
        Bv, Cv, Nv = v.shape
        if (Bk, Kk) != (B, K) or (Bv, Nv) != (B, Nk):
            raise ValueError(f"corr_softmax_warp: shape mismatch qn{tuple(qn.shape)} "
                             f"kn{tuple(kn.shape)} v{tuple(v.shape)}")
        out = torch.empty((B, Cv, Nq), device=qn.device, dtype=torch.float32)
        lse = torch.empty((B, Nq), device=qn.device, dtype=torch.float32)
        # training: keep the logits for the query-side backward (cheaper than recomputing them, see
        # corr_fused_fwd.hip); inference never materialises anything HWxHW
        logits_t = None
        ctx.split = planes is not None
        ctx.v_amax = None
        ctx.v_lomask = None
        if planes is not None:       # split-precision flavour: same outputs, f16x3 matrix products
            qh, ql, kh, kl, vh, vl, v_scale, v_amax, v_lomask = planes[:9]
            qk_scales = planes[13] if len(planes) > 13 else None      # (q_scale, k_scale) device scalars, or None
            ctx.k_active = planes[14] if len(planes) > 14 else 0     # K < 256 (magnitude-free flavour): planes zero-padded to 256
            Kp = FUSED_K if ctx.k_active else K
            ctx.recompute = bool(keep_logits) and not _saves_logits(B, Nq, Nk)
            if keep_logits and not ctx.recompute:   # the forward's private tile-blocked layout (cocos_hip.h), opaque here
                nbytes = _lib.load().cocos_corr_softmax_warp_saved_logits_bytes(B, Nq, Nk)
                logits_t = torch.empty(nbytes // 4, device=qn.device, dtype=torch.float32)
            # magnitude-free flavour (device-side operand scales): per-row (m, r) for its backward (cocos_hip.h)
            ctx.rowstat = torch.empty((B, 3, Nq), device=qn.device, dtype=torch.float32) if (qk_scales and keep_logits) else None
            # ... and, with saved logits (which this flavour stores RELATIVE to the running maximum), that maximum per 32-key tile
            ctx.mtile = (torch.empty((B, (Nk + 31) // 32, 2, Nq), device=qn.device, dtype=torch.float32)
                         if (qk_scales and logits_t is not None) else None)
            _select_fwd_schedule()
            _call("corr_softmax_warp_fwd", "cocos_corr_softmax_warp_fwd_f16x3_ex", qh.data_ptr(), ql.data_ptr(),
                  kh.data_ptr(), kl.data_ptr(), vh.data_ptr(), vl.data_ptr(), out.data_ptr(), lse.data_ptr(),
                  _ptr(logits_t), v_scale.data_ptr(), _ptr(v_lomask), B, Kp, Nq, Nk, Cv, float(inv_temperature),
                  SPLIT_OPERAND_SCALE, _ptr(qk_scales[0] if qk_scales else None), _ptr(qk_scales[1] if qk_scales else None),
                  _ptr(ctx.rowstat), _ptr(ctx.mtile), ctx.k_active, _stream())
            ctx.v_amax = v_amax
            ctx.v_lomask = v_lomask
            ctx.qk_scales = qk_scales
        else:
            keep = (keep_logits and B * Nq * Nk * 4 <= MAX_DS_WORKSPACE_BYTES and Nq * Nk * 4 < 2 ** 31 - 1)
            logits_t = torch.empty((B, Nk, Nq), device=qn.device, dtype=torch.float32) if keep else None
            _call("corr_softmax_warp_fwd", "cocos_corr_softmax_warp_fwd", qn.data_ptr(), kn.data_ptr(),
                  v.data_ptr(), out.data_ptr(), lse.data_ptr(), _ptr(logits_t), B, K, Nq, Nk, Cv,
                  float(inv_temperature), _stream())
        ctx.save_for_backward(qn, kn, v, out, lse)
        ctx.logits_t = logits_t
        ctx.inv_t = float(inv_temperature)
        # channel-major planes of k_scale*qn, k_scale*kn for the split-precision backward (when given); the recompute
        # backward also needs the position-major ones the forward multiplied
        recompute = planes is not None and getattr(ctx, "recompute", False)
        ctx.cplanes = planes[9:13] if (planes is not None and len(planes) > 9 and (logits_t is not None or recompute)) else None
        ctx.pplanes = planes[0:4] if recompute else None
        return out

    @staticmethod
    def backward(ctx, dout):
        qn, kn, v, out, lse = ctx.saved_tensors
        dout = _chk(dout, "dout")
        B, K, Nq = qn.shape
        Nk, Cv = kn.shape[2], v.shape[1]
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        dqn = torch.empty_like(qn) if need_q else None
        dkn = torch.empty_like(kn) if (need_k or need_v) else None
        dv = torch.empty_like(v) if need_v else None
        st = _stream()
        logits_t = ctx.logits_t
        if ctx.split and getattr(ctx, "recompute", False):
            return _CorrSoftmaxWarp._backward_recompute(ctx, qn, kn, v, out, lse, dout, dqn, dkn, dv, need_k)
        if ctx.split and logits_t is not None:
            # split-precision backward: everything on the f16 MFMA, fp32-class accuracy (see cocos_hip.h).  The
            # forward only takes this flavour (and saves its private logits layout) for shapes this branch takes.
            qch, qcl, kch, kcl = ctx.cplanes
            qks = ctx.qk_scales
            cvp = (Cv + 31) // 32 * 32
            g_amax, v_amax = _recall_amax(dout), ctx.v_amax   # max|v| was taken once, by the forward; max|dout| comes
            if g_amax is None:                                # with dout when concat_channels_amax produced it
                g_amax = absmax(dout)
            (gph, gpl, g_scale), (vph, vpl, v_scale) = _split_pair_transposed(dout, g_amax, v, v_amax, cvp)
            half = dict(device=qn.device, dtype=torch.float16)
            want_k = dkn is not None
            dsh = dsl = psh = psl = None
            if want_k:
                dsh, dsl = torch.empty((B, Nk, Nq), **half), torch.empty((B, Nk, Nq), **half)
            if dv is not None:      # cycle terms: V itself is differentiated, the key side needs P as well
                psh, psl = torch.empty((B, Nk, Nq), **half), torch.empty((B, Nk, Nq), **half)
            ds_scale = torch.empty(1, device=qn.device, dtype=torch.float32)
            blocked = int(Nk % 128 == 0 and Nq % 32 == 0)     # [query][key]-blocked dS'' / P planes (see cocos_hip.h)
            gemm_b = 2 * blocked                               # ... which the GEMM reads as b_blocked = 2
            ka = getattr(ctx, "k_active", 0)
            Kp = FUSED_K if ka else K
            if ka:                   # the kernel writes all 256 channel rows (zeros past K): dqn is the view of the real ones
                dqn_buf = torch.empty((B, Kp, Nq), device=qn.device, dtype=torch.float32)
                dqn = dqn_buf[:, :K] if dqn is not None else None
            elif dqn is None:        # the query kernel always accumulates dqn; scratch when nobody wants it
                dqn_buf = torch.empty_like(qn)
            else:
                dqn_buf = dqn
            d_pre = _rowdot_cached(dout, out) if BWD_D_PRECOMPUTED else None
            _call("corr_softmax_warp_bwd_query", "cocos_corr_softmax_warp_bwd_query_f16x3_ex", kch.data_ptr(),
                  kcl.data_ptr(), vph.data_ptr(), vpl.data_ptr(), gph.data_ptr(), gpl.data_ptr(),
                  g_scale.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), logits_t.data_ptr(),
                  dqn_buf.data_ptr(), _ptr(dsh), _ptr(dsl), _ptr(psh), _ptr(psl), v_amax.data_ptr(),
                  v_scale.data_ptr(), ds_scale.data_ptr(), _ptr(ctx.v_lomask), B, Kp, Nq, Nk, Cv, cvp, ctx.inv_t,
                  SPLIT_OPERAND_SCALE, _ptr(qks[0] if qks else None), _ptr(qks[1] if qks else None), blocked,
                  _ptr(getattr(ctx, "rowstat", None)), _ptr(getattr(ctx, "mtile", None)), _ptr(d_pre), ka, st)
            if want_k:    # A = the channel-major planes of q_scale * qn
                _key_gemm(qch, qcl, dsh, dsl, dkn, Nk, Nq, ka, qks, ds_scale, gemm_b, st)
            if dv is not None:      # dv[c,j] = sum_i dout[c,i] P[i,j]
                gch, gcl, _ = split_f16(dout, False, amax=g_amax)
                _hgemm_planes("corr_softmax_warp_bwd_dv", gch, gcl, psh, psl, dv, Cv, Nk, Nq, 1.0 / 16384.0, g_scale, None, gemm_b, st)
            return dqn, (dkn if need_k else None), dv, None, None, None
        # key side: GEMM over a materialised dS^T when it pays and fits (see cocos_hip.h), else the
        # flash-style kernel that recomputes the logits (always when dv is wanted: it needs P)
        ds_bytes = B * Nq * Nk * 4
        via_gemm = (dqn is not None and dkn is not None and dv is None
                    and ds_bytes <= MAX_DS_WORKSPACE_BYTES and Nq * Nk * 4 < 2 ** 31 - 1)
        key_recompute = dkn is not None and not via_gemm
        dvec = None
        if key_recompute or (dqn is not None and logits_t is None):
            dvec = torch.empty((B, Nq), device=qn.device, dtype=torch.float32)
            _call("corr_softmax_warp_bwd_prepare", "cocos_corr_softmax_warp_bwd_prepare",
                  out.data_ptr(), dout.data_ptr(), dvec.data_ptr(), B, Nq, Cv, st)
        dims = (B, K, Nq, Nk, Cv, ctx.inv_t, st)
        ds_t = torch.empty((B, Nk, Nq), device=qn.device, dtype=torch.float32) if via_gemm else None
        if dqn is not None:
            _call("corr_softmax_warp_bwd_query", "cocos_corr_softmax_warp_bwd_query", qn.data_ptr(),
                  kn.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), dout.data_ptr(),
                  _ptr(dvec), _ptr(logits_t), _ptr(dqn), _ptr(ds_t), *dims)
        if via_gemm:
            _call("corr_softmax_warp_bwd_key_from_ds", "cocos_corr_softmax_warp_bwd_key_from_ds",
                  qn.data_ptr(), ds_t.data_ptr(), dkn.data_ptr(), B, K, Nq, Nk, st)
        elif dkn is not None:
            _call("corr_softmax_warp_bwd_key", "cocos_corr_softmax_warp_bwd_key", qn.data_ptr(),
                  kn.data_ptr(), v.data_ptr(), lse.data_ptr(), dout.data_ptr(), dvec.data_ptr(),
                  _ptr(dkn), _ptr(dv), *dims)
        return dqn, (dkn if need_k else None), dv, None, None, None


def _corr_bwd_recompute(ctx, qn, kn, v, out, lse, dout, dqn, dkn, dv, need_k):
    """Split-precision backward WITHOUT saved logits (the forward kept the row LSE only): the keys are walked in chunks of
    _recompute_chunk() keys; per chunk the forward kernel is run again on the resident operand planes just for its logits
    (one zero value channel: 6 instead of 30 P.V MFMAs per tile; its softmax output is discarded — the RAW logits it
    saves do not depend on it), then the query kernel (global LSE and D: a chunk's dS'' is exact) and the key-side GEMM(s)
    for that slice of d kn / d v; d qn accumulates over the chunks.  HWxHW scratch: RECOMPUTE_CHUNK_BYTES per matrix
    instead of B*Nq*Nk*4 — BASELINE config 5 (HW = 16384, B = 2): 2 x 0.5 GiB instead of 2 x 2 GiB.  Same kernels, same
    arithmetic per element as the saved-logits chain (bit-identical dS'')."""
    qh, ql, kh, kl = ctx.pplanes
    qch, qcl, kch, kcl = ctx.cplanes
    qks = ctx.qk_scales
    B, K, Nq = qn.shape
    Nk, Cv = kn.shape[2], v.shape[1]
    st = _stream()
    lib = _lib.load()
    cvp = (Cv + 31) // 32 * 32
    g_amax, v_amax = _recall_amax(dout), ctx.v_amax
    if g_amax is None:
        g_amax = absmax(dout)
    gph, gpl, g_scale = split_f16(dout, True, cpad=cvp, amax=g_amax)
    vph, vpl, v_scale = split_f16(v, True, cpad=cvp, amax=v_amax)
    gch = gcl = None
    if dv is not None:
        gch, gcl, _ = split_f16(dout, False, amax=g_amax)
    dev, half = qn.device, dict(device=qn.device, dtype=torch.float16)
    want_k = dkn is not None
    kc = _recompute_chunk(B, Nq, Nk)
    ds_scale = torch.empty(1, device=dev, dtype=torch.float32)
    d_pre = _rowdot(dout, out) if BWD_D_PRECOMPUTED else None
    ka = getattr(ctx, "k_active", 0)
    Kp = FUSED_K if ka else K        # (K < 256, magnitude-free flavour: the planes are zero-padded to the kernels' 256 channels)
    dq_acc = None
    # scratch shared by the chunks (sized for a full chunk)
    o1 = torch.empty((B, 1, Nq), device=dev, dtype=torch.float32)
    l1 = torch.empty((B, Nq), device=dev, dtype=torch.float32)
    for k0 in range(0, Nk, kc):
        n = min(kc, Nk - k0)
        khc, klc = kh[:, k0:k0 + n].contiguous(), kl[:, k0:k0 + n].contiguous()
        vz = torch.zeros((B, 1, n), **half)                  # one zero value channel (hi and lo plane alike)
        lg = torch.empty(lib.cocos_corr_softmax_warp_saved_logits_bytes(B, Nq, n) // 4, device=dev, dtype=torch.float32)
        rowstat = getattr(ctx, "rowstat", None)           # magnitude-free flavour: relative logits + their per-tile reference
        mt = torch.empty((B, (n + 31) // 32, 2, Nq), device=dev, dtype=torch.float32) if rowstat is not None else None
        _select_fwd_schedule()
        _call("corr_softmax_warp_recompute", "cocos_corr_softmax_warp_fwd_f16x3_ex", qh.data_ptr(), ql.data_ptr(), khc.data_ptr(),
              klc.data_ptr(), vz.data_ptr(), vz.data_ptr(), o1.data_ptr(), l1.data_ptr(), lg.data_ptr(), None, None, B, Kp, Nq, n, 1,
              ctx.inv_t, SPLIT_OPERAND_SCALE, _ptr(qks[0] if qks else None), _ptr(qks[1] if qks else None), None, _ptr(mt), ka, st)
        kchc, kclc = kch[:, :, k0:k0 + n].contiguous(), kcl[:, :, k0:k0 + n].contiguous()
        vphc, vplc = vph[:, k0:k0 + n].contiguous(), vpl[:, k0:k0 + n].contiguous()
        dsh = dsl = psh = psl = None
        if want_k:
            dsh, dsl = torch.empty((B, n, Nq), **half), torch.empty((B, n, Nq), **half)
        if dv is not None:
            psh, psl = torch.empty((B, n, Nq), **half), torch.empty((B, n, Nq), **half)
        blocked = int(n % 128 == 0 and Nq % 32 == 0)
        dq_c = torch.empty((B, Kp, Nq), device=dev, dtype=torch.float32)
        _call("corr_softmax_warp_bwd_query", "cocos_corr_softmax_warp_bwd_query_f16x3_ex", kchc.data_ptr(), kclc.data_ptr(),
              vphc.data_ptr(), vplc.data_ptr(), gph.data_ptr(), gpl.data_ptr(), g_scale.data_ptr(), out.data_ptr(), dout.data_ptr(),
              lse.data_ptr(), lg.data_ptr(), dq_c.data_ptr(), _ptr(dsh), _ptr(dsl), _ptr(psh), _ptr(psl), v_amax.data_ptr(),
              v_scale.data_ptr(), ds_scale.data_ptr(), _ptr(ctx.v_lomask), B, Kp, Nq, n, Cv, cvp, ctx.inv_t, SPLIT_OPERAND_SCALE,
              _ptr(qks[0] if qks else None), _ptr(qks[1] if qks else None), blocked, _ptr(rowstat), _ptr(mt), _ptr(d_pre), ka, st)
        del lg
        if ka:                   # (only the real rows are written, see cocos_hip.h)
            dq_c = dq_c[:, :K]
        dq_acc = dq_c if dq_acc is None else dq_acc.add_(dq_c)
        if want_k:
            dk_c = dkn if n == Nk else torch.empty((B, K, n), device=dev, dtype=torch.float32)
            _key_gemm(qch, qcl, dsh, dsl, dk_c, n, Nq, ka, qks, ds_scale, 2 * blocked, st)
            if dk_c is not dkn:
                dkn[:, :, k0:k0 + n] = dk_c
        if dv is not None:
            dv_c = dv if n == Nk else torch.empty((B, Cv, n), device=dev, dtype=torch.float32)
            _hgemm_planes("corr_softmax_warp_bwd_dv", gch, gcl, psh, psl, dv_c, Cv, n, Nq, 1.0 / 16384.0, g_scale, None, 2 * blocked, st)
            if dv_c is not dv:
                dv[:, :, k0:k0 + n] = dv_c
    if dqn is not None:
        dqn = dq_acc
    return dqn, (dkn if need_k else None), dv, None, None, None


_CorrSoftmaxWarp._backward_recompute = staticmethod(_corr_bwd_recompute)


def _rowdot(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """D[b,i] = sum_c a[b,c,i] b[b,c,i] (fp64 accumulation) -> [B,N]: the D of the softmax backward (cocos_rowdot_f64)."""
    B, C, N = a.shape
    d = torch.empty((B, N), device=a.device, dtype=torch.float32)
    _call("rowdot", "cocos_rowdot_f64", a.data_ptr(), b.data_ptr(), d.data_ptr(), B, C, N, _stream())
    return d


def _rowdot_cached(dout: torch.Tensor, out: torch.Tensor):
    """D of the softmax backward: the one the producer of `dout` left behind (warp_head's backward computes it in the pass that
    writes dout), else one cocos_rowdot_f64 pass."""
    ent, _tls.known_rowdot = _tls.known_rowdot, None
    if ent is not None:
        ref, version, out_ptr, d = ent
        src = ref()
        if (src is not None and src.data_ptr() == dout.data_ptr() and src.shape == dout.shape and dout._version == version
                and out.data_ptr() == out_ptr and dout.is_contiguous()):
            return d
    return _rowdot(dout, out)


def _split_pair_transposed(x0, amax0, x1, amax1, cpad):
    """split_f16(x0, True, cpad=cpad, amax=amax0) and the same of x1 (same shape) in ONE launch: ((hi, lo, scale), (hi, lo, scale))."""
    x0, x1 = _chk(x0, "split_f16: x"), _chk(x1, "split_f16: x")
    B, C, N = x0.shape
    if x1.shape != x0.shape or 2 * B > 65535:
        return split_f16(x0, True, cpad=cpad, amax=amax0), split_f16(x1, True, cpad=cpad, amax=amax1)
    half = dict(device=x0.device, dtype=torch.float16)
    res, args = [], []
    for x, am in ((x0, amax0), (x1, amax1)):
        hi, lo = torch.empty((B, N, cpad), **half), torch.empty((B, N, cpad), **half)
        sc = torch.empty(1, device=x0.device, dtype=torch.float32)
        res.append((hi, lo, sc))
        args += [x.data_ptr(), hi.data_ptr(), lo.data_ptr(), am.data_ptr(), sc.data_ptr()]
    _call("split_f16", "cocos_split_f16_transpose_pair", *args, B, C, N, int(cpad), _stream())
    return res[0], res[1]


def _wants_logits(qn, kn):
    # decided OUTSIDE the Function (inside it grad mode is always off): only a pass that will be
    # differentiated w.r.t. theta/phi saves the logits; inference never materialises anything HWxHW
    return torch.is_grad_enabled() and (qn.requires_grad or kn.requires_grad)


def corr_softmax_warp(qn, kn, v, inv_temperature: float, planes: OperandPlanes | None = None, operand_amax: bool = False,
                      precision: str | None = None):
    """out[b,c,i] = sum_j softmax_j(<qn[b,:,i], kn[b,:,j]> * inv_temperature) * v[b,c,j].

    qn [B,256,Nq], kn [B,256,Nk], v [B,Cv,Nk] -> [B,Cv,Nq].  Wider V is processed in chunks of
    159 channels (each chunk recomputes the logits; no materialisation).  `planes`: the caller's per-forward
    OperandPlanes (theta/phi planes shared by several launches); None = made for this call only.  `operand_amax`: qn / kn
    are NOT unit-norm columns (softmax_attention): their planes get device-side power-of-two scales from max|.| instead of
    the fixed SPLIT_OPERAND_SCALE (split flavour only; raises if this shape cannot take it).  `precision`: overrides the
    module-level PRECISION for this call (a per-call argument, not a global: threads do not see each other's choice).
    With operand_amax K may be < 256 (softmax_attention: K = C/8): the planes are zero-padded and the kernels' K = 32 / 64
    instantiations skip the matrix steps, fragment reads and fetches of the padding."""
    B, K, Nq = qn.shape
    Nk, Cv = kn.shape[2], v.shape[1]
    keep = _wants_logits(qn, kn)
    if operand_amax and not keep and torch.is_grad_enabled() and v.requires_grad:
        # only V is differentiated (frozen / detached theta, phi of an Attention block): the backward still needs P, and for K < 256
        # only the split chain (saved logits -> P planes -> the dv GEMM) exists — the exact-fp32 kernels are K = 256 only
        keep = True
    prec = PRECISION if precision is None else precision
    if prec not in ("fp32", "f16x3"):
        raise ValueError(f"cocosnet_amd.ops.PRECISION = {prec!r}: expected 'fp32' or 'f16x3'")
    chunk = min(Cv, MAX_FUSED_SPLIT_CV)
    # the split flavour saves its logits in a private layout only its own backward reads: a training pass takes it
    # only for shapes that backward takes too (otherwise the exact-fp32 kernels run, forward and backward)
    split = (prec == "f16x3" and (K == FUSED_K or (operand_amax and K < FUSED_K)) and Nk % 4 == 0
             and (not keep or _split_bwd_ok(B, Nq, Nk, chunk)))
    if planes is None:
        planes = OperandPlanes()
    if operand_amax and not split:
        raise _lib.CocosHipError("corr_softmax_warp: operand_amax needs the split-precision kernels for this shape")
    if not split and (planes.has(qn) or planes.has(kn)):
        raise _lib.CocosHipError("corr_softmax_warp: qn / kn exist as operand planes only (center_l2norm_planes) but this "
                                 "shape does not take the split-precision kernels")

    qk_made = []

    def qk_planes():
        # the magnitude-free flavour's q / k planes, once per call (the value chunks share them).  K <= 256 real channels:
        # the position-major planes the forward multiplies are written zero-padded to 256 by the split kernel itself; of the
        # channel-major ones (backward) q's keep the real K rows (the key-side GEMM's M) and k's are padded (the query
        # kernel stages 256-row tiles, fetching only the real rows)
        if not qk_made:
            qa, ka_ = absmax(qn), absmax(kn)
            qh, ql, qs = split_f16(qn, True, cpad=FUSED_K, amax=qa)
            kh, kl, ks = split_f16(kn, True, cpad=FUSED_K, amax=ka_)
            cpl = (None,) * 4
            if keep:
                qch, qcl, _ = split_f16(qn, False, amax=qa)
                kch, kcl, _ = split_f16(kn, False, amax=ka_)
                if K < FUSED_K:
                    pad = lambda t: torch.cat([t, t.new_zeros((B, FUSED_K - K, Nk))], dim=1)
                    kch, kcl = pad(kch), pad(kcl)
                cpl = (qch, qcl, kch, kcl)
            qk_made.append((qh, ql, kh, kl, *cpl, (qs, ks), K if K < FUSED_K else 0))
        return qk_made[0]

    def run(vv):
        pl = None
        if split:   # operand planes: theta/phi once per forward (shared through `planes`), V per launch
            with torch.no_grad():
                # V has no a-priori magnitude in a general forward() call: its planes are normalised by a
                # device-side power of two like every other operand (one max|v| pass, reused by the backward)
                v_amax = _recall_amax(vv)
                if v_amax is None:
                    v_amax = absmax(vv)
                # V planes, and which 32-channel blocks of V have a non-zero lo plane (one-hot labels / masks are exact in
                # f16: theirs is all zero and the kernels skip it) — the same launch, only when it can pay
                # (the magnitude-free flavour — operand_amax — takes no lo mask: its kernels are the single-flavour instantiations)
                vh, vl, v_scale, v_lomask = split_f16_chan_mask(vv, v_amax, VALUE_LO_SKIP and vv.shape[1] > 32 and not operand_amax)
                if operand_amax:
                    pl = (*qk_planes()[:4], vh, vl, v_scale, v_amax, v_lomask, *qk_planes()[4:])
                else:
                    pl = (*planes.get(qn, True, SPLIT_OPERAND_SCALE), *planes.get(kn, True, SPLIT_OPERAND_SCALE),
                          vh, vl, v_scale, v_amax, v_lomask)
                    if keep:   # the backward wants the channel-major planes as well
                        pl += (*planes.get(qn, False, SPLIT_OPERAND_SCALE), *planes.get(kn, False, SPLIT_OPERAND_SCALE))
        return _CorrSoftmaxWarp.apply(qn, kn, vv, inv_temperature, keep, pl)

    limit = MAX_FUSED_SPLIT_CV if split else MAX_FUSED_CV
    if Cv <= limit:
        return run(v)
    return torch.cat([run(v[:, c0:c0 + limit]) for c0 in range(0, Cv, limit)], dim=1)


class PreparedValues:
    """The value tensor of the row pass of a prepared exemplar (inference.PreparedExemplar): v [Be,Cv,N] fp32 with its max|v| cell
    and, made on first use by the split flavour, its channel-major hi / lo planes, their scale cell and the lo-plane block mask.
    `n_ref`: how many leading channels are image (the rest is the direct mask)."""

    def __init__(self, v: torch.Tensor, n_ref: int):
        self.v, self.n_ref = v, int(n_ref)
        self.amax = None            # max|v| cell: taken when the split flavour first asks for the planes
        self._split = None
        self._expanded = {}         # B -> the copy for B query batches (kept, as PreparedKeys keeps its copies)

    def split(self):
        """(vh, vl, scale cell, lo mask | None): what corr_softmax_warp's run() makes of V per launch, made once"""
        if self._split is None:
            self.amax = absmax(self.v)
            self._split = split_f16_chan_mask(self.v, self.amax, VALUE_LO_SKIP and self.v.shape[1] > 32)
        return self._split

    def expanded(self, B: int) -> torch.Tensor:
        """v for B query batches: itself, or ONE exemplar's copied B times, once per record (the routes without a native broadcast:
        their kernels measure and split V per call, as for any other value tensor)"""
        Be = self.v.shape[0]
        if Be == B:
            return self.v
        if Be != 1:
            raise ValueError(f"prepared exemplar of batch {Be} used with {B} inputs (expected {B} or 1)")
        if B not in self._expanded:
            self._expanded[B] = self.v.expand(B, -1, -1).contiguous()
        return self._expanded[B]


class PreparedKeys:
    """The key side and the value side of a correlation that outlive ONE forward call — the halves of what ops.OperandPlanes (a
    per-call object) holds that depend on the exemplar alone.  Owned by an inference.PreparedExemplar, which fills it through the
    `make_*` callables it passes in; every product is made the first time a route asks for it and kept until the record finds its
    sources changed (it then builds a new PreparedKeys: nothing here is ever updated in place).  Inference only: nothing in it
    carries an autograd graph.  `Be` is the exemplar batch: the number of query batches B, or 1 = all of them share one exemplar."""

    def __init__(self, Be: int, shape, image_size, make_phi_raw, make_split, make_box, make_values):
        self.Be = int(Be)
        self.shape = torch.Size(shape)            # of phi_raw: [Be, 256, fh, fw]
        self.image_size = tuple(image_size)       # (H, W) of ref_img
        self._make = dict(phi_raw=make_phi_raw, split=make_split, box=make_box, values=make_values)
        self._got = {}

    def _get(self, key, fn):
        if key not in self._got:
            with torch.no_grad():
                self._got[key] = fn()
        return self._got[key]

    def check(self, B: int):
        if self.Be not in (B, 1):
            raise ValueError(f"prepared exemplar of batch {self.Be} used with {B} inputs (expected {B} or 1)")

    def _bcast(self, key, t, B):
        """t [Be,...] for B query batches: expand().contiguous() once per call site and record state (kept: the next call reuses it)"""
        if t is None or t.shape[0] == B:
            return t
        return self._get((key, "x", B), lambda: t.expand(B, *t.shape[1:]).contiguous())

    def phi_raw(self, B=None):
        """the fp32 projection [Be,256,fh,fw] (generic back end, WTA, return_corr, the fp32 flavour); [B,...] when B is given"""
        t = self._get("phi_raw", self._make["phi_raw"])
        return t if B is None else self._bcast("phi_raw", t, B)

    def split_planes(self, B=None):
        """(kh, kl, norm): position-major planes [Be,N,256] of SPLIT_OPERAND_SCALE * kn and the row norms (fused match_kernel 1)"""
        got = self._get("split", self._make["split"])
        return got if B is None else tuple(self._bcast(("split", i), t, B) for i, t in enumerate(got))

    def box_planes(self, B=None):
        """(kh, kl, scale cell, nu, b): phi_raw's position-major planes and its K12 statistics (fused match_kernel 3)"""
        got = self._get("box", self._make["box"])
        if B is None:
            return got
        return tuple(t if i == 2 else self._bcast(("box", i), t, B) for i, t in enumerate(got))

    def values(self, down: int, patch: bool, direct_mask: bool) -> PreparedValues:
        key = ("values", int(down), bool(patch), bool(direct_mask))
        return self._get(key, lambda: self._make["values"](int(down), bool(patch), bool(direct_mask)))


def corr_softmax_warp_shared(qh, ql, keys: PreparedKeys, values: PreparedValues, inv_temperature: float):
    """corr_softmax_warp(qn, kn, v, ...) of the split flavour, forward only, with the key planes and V of a prepared exemplar:
    qh, ql [B,Nq,256] (this call's query planes); keys / values of batch B or 1 — with 1 every query batch reads the ONE key /
    value set (batch stride 0 in cocos_corr_softmax_warp_fwd_f16x3_shared: no copies).  Cv <= MAX_FUSED_SPLIT_CV."""
    B, Nq, K = qh.shape
    kh, kl, _ = keys.split_planes()
    vh, vl, v_scale, v_lomask = values.split()
    Be, Nk = kh.shape[0], kh.shape[1]
    Cv = vh.shape[1]
    if Be not in (B, 1) or vh.shape[0] != Be or vh.shape[2] != Nk or kh.shape[2] != K:
        raise ValueError(f"corr_softmax_warp_shared: shape mismatch q{tuple(qh.shape)} k{tuple(kh.shape)} v{tuple(vh.shape)}")
    dense = Be == B
    out = torch.empty((B, Cv, Nq), device=qh.device, dtype=torch.float32)
    lse = torch.empty((B, Nq), device=qh.device, dtype=torch.float32)
    _select_fwd_schedule()
    _call("corr_softmax_warp_fwd", "cocos_corr_softmax_warp_fwd_f16x3_shared", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(),
          kl.data_ptr(), vh.data_ptr(), vl.data_ptr(), out.data_ptr(), lse.data_ptr(), None, v_scale.data_ptr(), _ptr(v_lomask),
          B, K, Nq, Nk, Cv, float(inv_temperature), SPLIT_OPERAND_SCALE, Nk * K if dense else 0, Cv * Nk if dense else 0, _stream())
    return out


# ------------------------------------------------------------------------------------------
# K36  match readout: row maximum, its index and the row log-sum-exp   (correspondence.py:291,:304-307 + the caller's max / argmax)
# ------------------------------------------------------------------------------------------
def _readout_planes(name: str, qh, ql, kh, kl):
    """what K36a and K39a ask of their operand planes -> (B, K, Nq, Nk, key batch stride: 0 = one key set for all samples)"""
    for t in (qh, ql, kh, kl):
        if not t.is_cuda:
            raise _lib.CocosHipError(f"{name}: expected CUDA/HIP operand planes; the correspondence hot path has no CPU fallback")
        if t.dtype != torch.float16 or not t.is_contiguous():
            raise TypeError(f"{name}: operand planes are contiguous float16 tensors")
    B, Nq, K = qh.shape
    Be, Nk = kh.shape[0], kh.shape[1]
    if Be not in (B, 1) or kh.shape[2] != K or ql.shape != qh.shape or kl.shape != kh.shape:
        raise ValueError(f"{name}: shape mismatch q{tuple(qh.shape)} k{tuple(kh.shape)}")
    return B, K, Nq, Nk, Nk * K if Be == B else 0


def _readout_outputs(lead, k, device):
    """(idx int32, val, lse) for a readout kernel to fill: idx and val `lead` (+ (k,) with k candidates per row), lse `lead`"""
    full = tuple(lead) + ((k,) if k else ())
    return (torch.empty(full, device=device, dtype=torch.int32), torch.empty(full, device=device, dtype=torch.float32),
            torch.empty(tuple(lead), device=device, dtype=torch.float32))


def _is_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


def _grid_pair(name: str, what: str, grid):
    try:
        h, w = grid
    except (TypeError, ValueError):
        h = w = None
    if not (_is_int(h) and _is_int(w) and h >= 1 and w >= 1):
        raise ValueError(f"{name}: {what}={grid!r}: expected a pair (h, w) of positive integers")
    return h, w


def _int_table(name: str, what: str, t, shape=None, any_int: bool = False):
    """An index or label table -> contiguous int32.  TypeError unless `t` is an int32 / int64 tensor (`any_int`: any integer dtype),
    ValueError unless it has `shape` (None: the caller's own check); the device is the caller's next refusal.  Wider types are
    narrowed after a clamp into int32's range, which keeps a negative entry negative and a large one out of any range a kernel
    clamps to (two label classes above 2^31 - 2 would collide: no label map has them)."""
    if not torch.is_tensor(t) or ((t.dtype.is_floating_point or t.dtype == torch.bool or t.dtype.is_complex) if any_int
                                  else t.dtype not in (torch.int32, torch.int64)):
        raise TypeError(f"{name}: {what} must be an {'integer' if any_int else 'int32 or int64'} tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {what} is {tuple(t.shape)}, expected {tuple(shape)}")
    return (t if t.dtype == torch.int32 else t.clamp(-1, 2 ** 31 - 1).to(torch.int32)).contiguous()


def _gate(name: str, tensors, needs_f16x3: bool):
    """The refusals that follow every TypeError / ValueError of an argument: each (tensor, what) lives on the GPU, then — where only
    the split-precision kernel exists — the flavour"""
    for t, what in tensors:
        if not t.is_cuda:
            raise _lib.CocosHipError(f"{name}: {what}: expected a CUDA/HIP tensor; the correspondence hot path has no CPU fallback")
    if needs_f16x3 and PRECISION != "f16x3":
        raise _lib.CocosHipError(f"{name}: only the split-precision flavour exists (COCOS_PRECISION=f16x3)")


def _operand_shapes(name: str, qn, kn, nq=None, nk=None, fit: str = "", width: bool = True):
    """qn [B,256,Nq] and kn [B,256,Nk] of one batch and width (`nq` / `nk`: the positions a grid asks for, `fit` names it; `width`:
    256 channels) -> (B, Nq, Nk); ValueError"""
    if (qn.dim() != 3 or kn.dim() != 3 or qn.shape[:2] != kn.shape[:2] or (nq is not None and qn.shape[2] != nq)
            or (nk is not None and kn.shape[2] != nk)):
        raise ValueError(f"{name}: expected qn [B,256,Nq] and kn [B,256,Nk]{fit}, got {tuple(qn.shape)} and {tuple(kn.shape)}")
    if width and qn.shape[1] != FUSED_K:
        raise ValueError(f"{name}: needs {FUSED_K} channels, got {qn.shape[1]}")
    return qn.shape[0], qn.shape[2], kn.shape[2]


def _fetch_planes(name: str, qn, kn, planes, detach: bool, same_batch: bool = False):
    """(qn, kn, (qh, ql, kh, kl)): the position-major operand planes of the two operands — a producer's, where the handle is
    registered in `planes`, else split here from the fp32 tensor (`detach`: a forward-only caller's)"""
    if planes is None:
        planes = OperandPlanes()
    qn, kn = (t if planes.has(t) else _chk(t.detach() if detach else t, f"{name}: {what}") for t, what in ((qn, "qn"), (kn, "kn")))
    with torch.no_grad():
        pl = (*planes.get(qn, True, SPLIT_OPERAND_SCALE), *planes.get(kn, True, SPLIT_OPERAND_SCALE))
    if same_batch and pl[2].shape[0] != pl[0].shape[0]:
        raise ValueError(f"{name}: query and key batch differ")
    return qn, kn, pl


def _corr_match_planes(qh, ql, kh, kl, inv_temperature: float):
    """K36a on operand planes: qh, ql [B,Nq,256], kh, kl [B or 1,Nk,256] (1: every sample reads the one key set, batch stride 0)
    -> (idx int32, max, lse), each [B,Nq]."""
    B, K, Nq, Nk, k_stride = _readout_planes("corr_match", qh, ql, kh, kl)
    idx, mx, lse = _readout_outputs((B, Nq), None, qh.device)
    _call("corr_match", "cocos_corr_match_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(), idx.data_ptr(),
          mx.data_ptr(), lse.data_ptr(), B, K, Nq, Nk, float(inv_temperature), SPLIT_OPERAND_SCALE, k_stride, _stream())
    return idx, mx, lse


def corr_match(qn, kn, inv_temperature: float, planes: OperandPlanes | None = None):
    """(idx int32, max, lse), each [B,Nq]: max[b,i] = max_j <qn[b,:,i], kn[b,:,j]> * inv_temperature, idx its (lowest) j, lse the
    row log-sum-exp — corr_softmax_warp's logits without its value tensor (K36a; forward only).  qn [B,256,Nq], kn [B,256,Nk]
    unit-norm columns, or the handles of producer-made planes registered in `planes` (center_l2norm_planes, K23), as for
    corr_softmax_warp.  Shapes the kernel does not take (K != 256, Nk % 4 != 0) raise: materialise and use row_argmax_lse."""
    _gate("corr_match", ((qn, "qn"), (kn, "kn")), False)
    with torch.no_grad():
        return _corr_match_planes(*_fetch_planes("corr_match", qn, kn, planes, True)[2], inv_temperature)


def corr_match_shared(qh, ql, keys: PreparedKeys, inv_temperature: float):
    """corr_match with the key planes of a prepared exemplar read in place: qh, ql [B,Nq,256] (this call's query planes), a record
    of batch B or 1 — with 1 every query batch reads the one key set (batch stride 0: no copies)."""
    kh, kl, _ = keys.split_planes()
    with torch.no_grad():
        return _corr_match_planes(qh, ql, kh, kl, inv_temperature)


def _readout_rows(name: str, f: torch.Tensor):
    """what K36b and K39b ask of a logit matrix -> (f, its leading shape, B, Nq, Nk)"""
    f = _chk(f.detach(), f"{name}: f")
    if f.dim() < 2 or f.numel() == 0:
        raise ValueError(f"{name}: expected a non-empty [..., Nq, Nk] tensor, got {tuple(f.shape)}")
    Nk, Nq = f.shape[-1], f.shape[-2]
    return f, f.shape[:-1], f.numel() // (Nq * Nk), Nq, Nk


def row_argmax_lse(f: torch.Tensor):
    """(idx int32, max, lse), each f.shape[:-1], of the rows of a materialised logit matrix f [..., Nk] in one sweep (K36b):
    torch.max(f, -1) (the lowest index among equal maxima) and torch.logsumexp(f, -1).  Forward only."""
    f, lead, B, Nq, Nk = _readout_rows("row_argmax_lse", f)
    idx, mx, lse = _readout_outputs(lead, None, f.device)
    _call("row_argmax_lse", "cocos_row_argmax_lse", f.data_ptr(), idx.data_ptr(), mx.data_ptr(), lse.data_ptr(), B, Nq, Nk, _stream())
    return idx, mx, lse


def _gather_gate(name: str, img, idx):
    """What the copy and the blend refuse alike before their shapes, in this order: img fp32 on the GPU, idx on the GPU and of an
    integer type -> img detached and contiguous"""
    img = _chk(img.detach(), f"{name}: img")
    _gate(name, ((idx, "idx"),), False)
    if idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise TypeError(f"{name}: idx must be an integer tensor, got {idx.dtype}")
    return img


def gather_patches(img: torch.Tensor, idx: torch.Tensor, h: int, w: int, down: int):
    """The hard warp (K36c): out [B,C,H,W] whose cell (y, x) of the h x w grid is the down x down patch of img at the cell idx[b, y*w+x]
    — a bitwise copy.  img [Be,C,H,W] fp32 with H == h*down, W == w*down and Be == B or 1 (one exemplar for all); idx [B,h*w] or
    [B,h,w], any integer type (values outside [0, h*w) are clamped into it)."""
    img = _gather_gate("gather_patches", img, idx)
    Be, C, H, W = img.shape
    B = idx.shape[0]
    if (H, W) != (h * down, w * down) or idx.numel() != B * h * w or Be not in (B, 1):
        raise ValueError(f"gather_patches: img{tuple(img.shape)} idx{tuple(idx.shape)} do not fit a {h}x{w} grid with down={down}")
    idx = idx.reshape(B, h * w).to(torch.int32).contiguous()
    out = torch.empty((B, C, H, W), device=img.device, dtype=torch.float32)
    _call("gather_patches", "cocos_gather_patches", img.data_ptr(), idx.data_ptr(), out.data_ptr(), B, C, H, W, int(down),
          C * H * W if Be == B else 0, _stream())
    return out


# ------------------------------------------------------------------------------------------
# K39  top-k match readout: the k best candidates per position and the row log-sum-exp   (:304-307 + the caller's topk / logsumexp)
# ------------------------------------------------------------------------------------------
#: the largest k of the readout (COCOS_MATCH_TOPK_MAX of cocos_hip.h)
MATCH_TOPK_MAX = _lib.CONSTANTS["COCOS_MATCH_TOPK_MAX"]


def _check_topk(name: str, k, Nk: int) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MATCH_TOPK_MAX or k > Nk:
        raise ValueError(f"{name}: k={k!r}: expected an integer in 1..{MATCH_TOPK_MAX} that does not exceed the {Nk} keys")
    return k


def corr_topk_ok(k: int) -> bool:
    """K39a ships a fused instantiation that serves k candidates (one ships only with zero scratch at two waves per SIMD and when it
    beats materialise + row_topk_lse at the benchmark shape: DESIGN.md 3.24); above it the readout materialises (K39b)."""
    return 1 <= k <= _lib.load().cocos_corr_topk_max_k()


def _corr_topk_planes(qh, ql, kh, kl, inv_temperature: float, k: int):
    """K39a on operand planes (as _corr_match_planes) -> (idx int32 [B,Nq,k], val [B,Nq,k], lse [B,Nq])."""
    B, K, Nq, Nk, k_stride = _readout_planes("corr_topk", qh, ql, kh, kl)
    k = _check_topk("corr_topk", k, Nk)
    idx, val, lse = _readout_outputs((B, Nq), k, qh.device)
    _call("corr_topk", "cocos_corr_topk_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(), idx.data_ptr(),
          val.data_ptr(), lse.data_ptr(), B, K, Nq, Nk, k, float(inv_temperature), SPLIT_OPERAND_SCALE, k_stride, _stream())
    return idx, val, lse


def corr_topk(qn, kn, inv_temperature: float, k: int, planes: OperandPlanes | None = None):
    """(idx int32 [B,Nq,k], val [B,Nq,k], lse [B,Nq]): per query the k largest logits <qn[b,:,i], kn[b,:,j]> * inv_temperature, in
    descending order (the lower j first among bitwise-equal logits), their j, and the row log-sum-exp (K39a; forward only).  Rank 0
    and lse are corr_match's outputs bit for bit.  Operands as corr_match.  1 <= k <= MATCH_TOPK_MAX, k <= Nk (ValueError); a k that
    corr_topk_ok refuses and the shapes corr_match refuses raise: materialise and use row_topk_lse."""
    _gate("corr_topk", ((qn, "qn"), (kn, "kn")), False)
    with torch.no_grad():
        return _corr_topk_planes(*_fetch_planes("corr_topk", qn, kn, planes, True)[2], inv_temperature, k)


def corr_topk_shared(qh, ql, keys: PreparedKeys, inv_temperature: float, k: int):
    """corr_topk with the key planes of a prepared exemplar read in place (as corr_match_shared)."""
    kh, kl, _ = keys.split_planes()
    with torch.no_grad():
        return _corr_topk_planes(qh, ql, kh, kl, inv_temperature, k)


# K47  label-restricted readout: the same scan over the keys each query's label allows
def _corr_topk_labels_planes(qh, ql, kh, kl, q_label, k_label, inv_temperature: float, k: int):
    """K47 on operand planes (as _corr_topk_planes) and int32 contiguous labels [B,Nq], [Be,Nk] on their device"""
    B, K, Nq, Nk, k_stride = _readout_planes("corr_topk_labelled", qh, ql, kh, kl)
    k = _check_topk("corr_topk_labelled", k, Nk)
    if tuple(q_label.shape) != (B, Nq) or tuple(k_label.shape) != (kh.shape[0], Nk):
        raise ValueError(f"corr_topk_labelled: labels {tuple(q_label.shape)}, {tuple(k_label.shape)} do not fit q{tuple(qh.shape)} k{tuple(kh.shape)}")
    idx, val, lse = _readout_outputs((B, Nq), k, qh.device)
    _call("corr_topk_labelled", "cocos_corr_topk_labels_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(),
          q_label.data_ptr(), k_label.data_ptr(), idx.data_ptr(), val.data_ptr(), lse.data_ptr(), B, K, Nq, Nk, k, float(inv_temperature),
          SPLIT_OPERAND_SCALE, k_stride, _stream())
    return idx, val, lse


def corr_topk_labelled(qn, kn, q_label, k_label, inv_temperature: float, k: int, planes: OperandPlanes | None = None):
    """corr_topk over the keys each query's label allows (K47; forward only) -> (idx int32 [B,Nq,k], val [B,Nq,k], lse [B,Nq]).
    q_label [B,Nq], k_label [B,Nk] int32 / int64: key j is allowed for query i when q_label[b,i] < 0 (unrestricted) or
    q_label[b,i] == k_label[b,j]; a negative key label is matched by unrestricted queries only.  The mask is applied to the logits
    inside the scan, before the candidate list and the log-sum-exp: lse is over the allowed keys, idx / val their k best in corr_topk's
    order.  A row with fewer than k allowed keys has val = -inf on the missing ranks (idx stays inside [0, Nk)); a row with none has
    lse = -inf.  With nothing restricted the outputs are corr_topk's bit for bit.  Operands, k and refusals as corr_topk; labels of
    another dtype raise TypeError, of another shape ValueError."""
    name = "corr_topk_labelled"
    B, Nq, Nk = _operand_shapes(name, qn, kn, width=False)
    q_label = _int_table(name, "q_label", q_label, (B, Nq))
    k_label = _int_table(name, "k_label", k_label, (B, Nk))
    _check_topk(name, k, Nk)
    _gate(name, ((qn, "qn"), (kn, "kn"), (q_label, "q_label"), (k_label, "k_label")), True)
    with torch.no_grad():
        return _corr_topk_labels_planes(*_fetch_planes(name, qn, kn, planes, True)[2], q_label, k_label, inv_temperature, k)


# ------------------------------------------------------------------------------------------
# K50  biased readout and the Sinkhorn iteration on top of it: entropic optimal transport over the correlation, no HW x HW
# ------------------------------------------------------------------------------------------
#: the largest number of Sinkhorn iterations corr_sinkhorn runs (two launches each)
SINKHORN_MAX_ITERS = 64


def _corr_topk_bias_planes(qh, ql, kh, kl, k_bias, inv_temperature: float, k: int, name: str = "corr_topk_biased"):
    """K50 on operand planes (as _corr_topk_planes) and a contiguous fp32 bias [Be,Nk] on their device (Be: the key planes' batch)"""
    B, K, Nq, Nk, k_stride = _readout_planes(name, qh, ql, kh, kl)
    k = _check_topk(name, k, Nk)
    if tuple(k_bias.shape) != (kh.shape[0], Nk):
        raise ValueError(f"{name}: k_bias {tuple(k_bias.shape)} does not fit k{tuple(kh.shape)}")
    idx, val, lse = _readout_outputs((B, Nq), k, qh.device)
    _call("corr_topk_biased", "cocos_corr_topk_bias_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(), k_bias.data_ptr(),
          idx.data_ptr(), val.data_ptr(), lse.data_ptr(), B, K, Nq, Nk, k, float(inv_temperature), SPLIT_OPERAND_SCALE, k_stride, _stream())
    return idx, val, lse


def _bias_table(name: str, k_bias, shape):
    """A per-key bias -> contiguous fp32 without a graph.  TypeError unless it is a float32 tensor, ValueError unless it has `shape` and
    needs no gradient (it is a constant of every op that takes it); the device is the caller's next refusal."""
    if not torch.is_tensor(k_bias) or k_bias.dtype != torch.float32:
        raise TypeError(f"{name}: k_bias must be a float32 tensor, got {k_bias.dtype if torch.is_tensor(k_bias) else type(k_bias).__name__}")
    if tuple(k_bias.shape) != tuple(shape):
        raise ValueError(f"{name}: k_bias is {tuple(k_bias.shape)}, expected {tuple(shape)}")
    if k_bias.requires_grad:
        raise ValueError(f"{name}: k_bias requires a gradient; the bias is not differentiable (pass k_bias.detach())")
    return k_bias.contiguous()


def corr_topk_biased(qn, kn, k_bias, inv_temperature: float, k: int, planes: OperandPlanes | None = None):
    """corr_topk over z_ij = inv_temperature <qn_i, kn_j> + k_bias[b,j] (K50; forward only) -> (idx int32 [B,Nq,k], val [B,Nq,k] = z,
    lse [B,Nq] = log sum_j exp z_ij).  k_bias [B,Nk] float32: finite values of any sign, or -inf to exclude a key (a row with every key
    excluded has lse = val = -inf and indices in range; no NaN from finite or -inf input).  The bias is added to the logits inside the
    scan, before the candidate list and the sum; a bias of zeros gives corr_topk's outputs bit for bit.  Operands, k and refusals as
    corr_topk_labelled; a bias of another dtype raises TypeError, of another shape or one that requires a gradient ValueError."""
    name = "corr_topk_biased"
    B, Nq, Nk = _operand_shapes(name, qn, kn, width=False)
    k_bias = _bias_table(name, k_bias, (B, Nk))
    _check_topk(name, k, Nk)
    _gate(name, ((qn, "qn"), (kn, "kn"), (k_bias, "k_bias")), True)
    with torch.no_grad():
        return _corr_topk_bias_planes(*_fetch_planes(name, qn, kn, planes, True)[2], k_bias, inv_temperature, k)


def _sinkhorn_args(name: str, iters, tau):
    """ValueError unless `iters` is an integer in 1..SINKHORN_MAX_ITERS and 0 < tau <= 1 -> (iters, tau)"""
    if not _is_int(iters) or not 1 <= iters <= SINKHORN_MAX_ITERS:
        raise ValueError(f"{name}: iters={iters!r}: expected an integer in 1..{SINKHORN_MAX_ITERS}")
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not 0 < tau <= 1:
        raise ValueError(f"{name}: tau={tau!r}: expected a number in (0, 1] (1: balanced transport)")
    return iters, float(tau)


def _sinkhorn_planes(qh, ql, kh, kl, inv_temperature: float, iters: int, tau: float):
    """The iteration of corr_sinkhorn on dense operand planes [B,Nq,256], [B,Nk,256] -> (f [B,Nq], g [B,Nk], row_lse [B,Nq])"""
    name = "corr_sinkhorn"
    B, Nq, Nk = qh.shape[0], qh.shape[1], kh.shape[1]
    log_mu, log_nu = -math.log(Nq), -math.log(Nk)
    g = torch.zeros((B, Nk), device=qh.device, dtype=torch.float32)
    for _ in range(iters):
        f = tau * (log_mu - _corr_topk_bias_planes(qh, ql, kh, kl, g, inv_temperature, 1, name)[2])       # rows: sum over the keys
        g = tau * (log_nu - _corr_topk_bias_planes(kh, kl, qh, ql, f, inv_temperature, 1, name)[2])       # columns: operands exchanged
    return f, g, _corr_topk_bias_planes(qh, ql, kh, kl, g, inv_temperature, 1, name)[2]


def corr_sinkhorn(qn, kn, inv_temperature: float, iters: int, tau: float = 1.0, planes: OperandPlanes | None = None):
    """Log-domain Sinkhorn over s_ij = inv_temperature <qn_i, kn_j> with uniform marginals mu = 1 / Nq, nu = 1 / Nk (K50; forward only,
    under torch.no_grad()) -> (f [B,Nq], g [B,Nk], row_lse [B,Nq]).  With g = 0, `iters` times:
        f_i = tau (log mu_i - log sum_j exp(s_ij + g_j)),   g_j = tau (log nu_j - log sum_i exp(s_ij + f_i))
    tau = 1 is balanced entropic transport (the column marginals of P_ij = exp(s_ij + f_i + g_j) are exact after every iteration),
    tau < 1 the KL-relaxed form rho / (rho + eps).  row_lse_i = log sum_j exp(s_ij + g_j) against the FINAL g: the normaliser of the
    row-conditional plan softmax_j(s_ij + g_j), and exp(f_i + row_lse_i) / mu_i is the row's mass (1 where its marginal is met).
    The operand planes are made once; every half-step is one launch of the K = 1 biased readout (the column half-step with the two
    plane pairs exchanged and f as the key bias), the affine update runs in torch on [B,N] vectors, row_lse costs one more launch:
    2 iters + 1 launches, nothing Nq x Nk.  Operands as corr_topk (dense keys of the queries' batch); iters an integer in
    1..SINKHORN_MAX_ITERS, 0 < tau <= 1, Nq and Nk multiples of 4 (ValueError)."""
    name = "corr_sinkhorn"
    B, Nq, Nk = _operand_shapes(name, qn, kn, width=False)
    iters, tau = _sinkhorn_args(name, iters, tau)
    if Nq % 4 or Nk % 4:
        raise ValueError(f"{name}: Nq={Nq} and Nk={Nk} must be multiples of 4 (each side is the key side of one half-step)")
    _gate(name, ((qn, "qn"), (kn, "kn")), True)
    with torch.no_grad():
        pl = _fetch_planes(name, qn, kn, planes, True, same_batch=True)[2]
        return _sinkhorn_planes(*pl, float(inv_temperature), iters, tau)


# ------------------------------------------------------------------------------------------
# K48  mutual match: both softmax directions from one correlation sweep, and the round trip
# ------------------------------------------------------------------------------------------
#: hot_path.correspondence_mutual: True = one sweep of the fused kernel serves both directions where it runs; False = every call
#: makes two readouts (rows, then cols).  The default follows profiles/k48_match_mutual.txt (tools/match_mutual_bench.py; B = 8, 64 x 64
#: grid): the fused kernel plus its finishing kernel 0.2570 ms against 0.3505 ms for two cocos_corr_match_f16x3 calls, a difference of
#: 0.0934 ms where the spread of the two-call windows is 0.0027 ms — above the spread, hence True.
MATCH_MUTUAL_FUSED = True


def corr_match_mutual_ok(B: int, Nq: int, Nk: int) -> bool:
    """the fused mutual kernel takes [B,Nq,256] x [B,Nk,256] planes: Nq and Nk multiples of 4 (dense keys, 256 channels)"""
    return (B >= 1 and Nq >= 4 and Nk >= 4 and Nq % 4 == 0 and Nk % 4 == 0
            and _lib.load().cocos_corr_match_mutual_workspace_bytes(int(B), int(Nq), int(Nk)) > 0)


def _corr_match_mutual_planes(qh, ql, kh, kl, inv_temperature: float):
    """K48 on operand planes qh, ql [B,Nq,256], kh, kl [B,Nk,256] -> ((row_idx, row_max, row_lse) [B,Nq], (col_idx, col_max, col_lse)
    [B,Nk])"""
    B, K, Nq, Nk, k_stride = _readout_planes("corr_match_mutual", qh, ql, kh, kl)
    if k_stride == 0 and B != 1:
        raise ValueError("corr_match_mutual: one key set for all samples is out of scope (dense keys only)")
    dev = qh.device
    rows, cols = _readout_outputs((B, Nq), None, dev), _readout_outputs((B, Nk), None, dev)
    nbytes = _lib.load().cocos_corr_match_mutual_workspace_bytes(B, Nq, Nk)
    ws = torch.empty((max(nbytes, 4) // 4,), device=dev, dtype=torch.float32)
    _call("corr_match_mutual", "cocos_corr_match_mutual_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(),
          rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(), cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(),
          ws.data_ptr(), ws.numel() * 4, B, K, Nq, Nk, float(inv_temperature), SPLIT_OPERAND_SCALE, _stream())
    return rows, cols


def corr_match_mutual(qn, kn, inv_temperature: float, planes: OperandPlanes | None = None):
    """Both directions of corr_match from ONE sweep of the correlation (K48; forward only) -> ((row_idx int32, row_max, row_lse), each
    [B,Nq], (col_idx int32, col_max, col_lse), each [B,Nk]).  The row triple is corr_match(qn, kn)'s bit for bit; the column triple is
    what corr_match(kn, qn) computes — per key the largest logit over the queries, its query (the lowest among bitwise-equal logits)
    and the column log-sum-exp — from the same tile registers: col_max is an element of the tile, so a mutual pair has bitwise-equal
    row_max and col_max; col_lse's summation order differs from the exchanged call's (within the same error bound).  Operands as
    corr_match.  Shapes the kernel does not take (corr_match_mutual_ok) raise: make two corr_match calls."""
    name = "corr_match_mutual"
    for t, what in ((qn, "qn"), (kn, "kn")):
        if not torch.is_tensor(t):
            raise TypeError(f"{name}: {what}: expected a tensor, got {type(t).__name__}")
    if planes is None or not (planes.has(qn) or planes.has(kn)):
        _operand_shapes(name, qn, kn, width=False)
    _gate(name, ((qn, "qn"), (kn, "kn")), True)
    with torch.no_grad():
        return _corr_match_mutual_planes(*_fetch_planes(name, qn, kn, planes, True)[2], inv_temperature)


# ------------------------------------------------------------------------------------------
# K49  trainable match readout: the two log-sum-exp vectors with gradients, and the correspondence NLL on top
# ------------------------------------------------------------------------------------------
def _corr_lse_bwd_planes(qh, ql, kh, kl, row_lse, col_lse, g_row, g_col, inv_temperature: float):
    """K49's sweep on operand planes -> out_t [B,Nq,256] = inv_t sum_j (g_row_i exp(s_ij - row_lse_i) + g_col_j exp(s_ij - col_lse_j)) kn_j;
    g_row [B,Nq] / g_col [B,Nk] fp32 contiguous or None (not both).  The key side is the same call with everything exchanged."""
    B, Nq, K = qh.shape
    Nk = kh.shape[1]
    out_t = torch.empty((B, Nq, K), device=qh.device, dtype=torch.float32)
    _call("corr_lse_bwd", "cocos_corr_lse_bwd_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(), row_lse.data_ptr(),
          col_lse.data_ptr(), _ptr(g_row), _ptr(g_col), out_t.data_ptr(), B, K, Nq, Nk, float(inv_temperature), SPLIT_OPERAND_SCALE, _stream())
    return out_t


def _lse_grads(planes4, row_lse, col_lse, g_row, g_col, inv_t: float, need_q: bool, need_k: bool):
    """(dq_t [B,Nq,256] | None, dk_t [B,Nk,256] | None) of sum g_row row_lse + sum g_col col_lse; both g None: zeros"""
    qh, ql, kh, kl = planes4
    dq_t = dk_t = None
    if g_row is None and g_col is None:
        if need_q:
            dq_t = torch.zeros(qh.shape, device=qh.device, dtype=torch.float32)
        if need_k:
            dk_t = torch.zeros(kh.shape, device=kh.device, dtype=torch.float32)
        return dq_t, dk_t
    if need_q:
        dq_t = _corr_lse_bwd_planes(qh, ql, kh, kl, row_lse, col_lse, g_row, g_col, inv_t)
    if need_k:
        dk_t = _corr_lse_bwd_planes(kh, kl, qh, ql, col_lse, row_lse, g_col, g_row, inv_t)
    return dq_t, dk_t


def _grad_vec(g, name: str):
    return None if g is None else _chk(g, name)


class _CorrLse(torch.autograd.Function):
    """K49.  qn / kn are only the autograd inputs; saved: the four planes and the two lse vectors."""

    @staticmethod
    def forward(ctx, qn, kn, inv_t: float, qh, ql, kh, kl):
        rows, cols = _corr_match_mutual_planes(qh, ql, kh, kl, inv_t)
        ctx.save_for_backward(qh, ql, kh, kl, rows[2], cols[2])
        ctx.inv_t = float(inv_t)
        ctx.set_materialize_grads(False)
        return rows[2], cols[2]

    @staticmethod
    def backward(ctx, g_row, g_col):
        qh, ql, kh, kl, row_lse, col_lse = ctx.saved_tensors
        need_q, need_k = ctx.needs_input_grad[:2]
        dq_t, dk_t = _lse_grads((qh, ql, kh, kl), row_lse, col_lse, _grad_vec(g_row, "corr_lse: d row_lse"),
                                _grad_vec(g_col, "corr_lse: d col_lse"), ctx.inv_t, need_q, need_k)
        return (_transpose(dq_t) if need_q else None, _transpose(dk_t) if need_k else None, None, None, None, None, None)


def _pair_logits_planes(qh, ql, kh, kl, target, inv_temperature: float):
    """s [B,Nq] = inv_t <qn_i, kn_target(i)> from the planes, K42's logit of the pair bit for bit; target int32 [B,Nq], negative: 0"""
    B, Nq, K = qh.shape
    s = torch.empty((B, Nq), device=qh.device, dtype=torch.float32)
    _call("pair_logits", "cocos_pair_logits_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(), target.data_ptr(),
          s.data_ptr(), B, K, Nq, kh.shape[1], float(inv_temperature), SPLIT_OPERAND_SCALE, _stream())
    return s


class _CorrPairNll(torch.autograd.Function):
    """K49.  Saved for the backward: the four planes, row_lse [B,Nq], col_lse [B,Nk] and the table [B,Nq] — nothing with an Nq x Nk
    extent.  Outputs: row_nll, col_nll and, without gradient, row_lse, col_lse."""

    @staticmethod
    def forward(ctx, qn, kn, target, inv_t: float, qh, ql, kh, kl):
        rows, cols = _corr_match_mutual_planes(qh, ql, kh, kl, inv_t)
        row_lse, col_lse = rows[2], cols[2]
        s = _pair_logits_planes(qh, ql, kh, kl, target, inv_t)
        sup = target >= 0
        zero = torch.zeros_like(s)
        row_nll = torch.where(sup, row_lse - s, zero)
        col_nll = torch.where(sup, col_lse.gather(1, target.clamp(min=0).long()) - s, zero)
        ctx.save_for_backward(qh, ql, kh, kl, row_lse, col_lse, target)
        ctx.inv_t = float(inv_t)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(row_lse, col_lse)
        return row_nll, col_nll, row_lse, col_lse

    @staticmethod
    def backward(ctx, g_r, g_c, _gl_r, _gl_c):
        qh, ql, kh, kl, row_lse, col_lse, target = ctx.saved_tensors
        need_q, need_k = ctx.needs_input_grad[:2]
        none = (None,) * 8
        if not (need_q or need_k):
            return none
        B, Nq, K = qh.shape
        Nk = kh.shape[1]
        dev = qh.device
        sup = target >= 0
        zero = torch.zeros((B, Nq), device=dev, dtype=torch.float32)
        # d row_lse_i = g_r, d col_lse_{t(i)} += g_c, d s_i = -(g_r + g_c), all on the supervised positions only
        g_r = None if g_r is None else torch.where(sup, _chk(g_r, "corr_pair_nll: d row_nll"), zero)
        g_c = None if g_c is None else torch.where(sup, _chk(g_c, "corr_pair_nll: d col_nll"), zero)
        if g_r is None and g_c is None:
            return (torch.zeros((B, K, Nq), device=dev) if need_q else None, torch.zeros((B, K, Nk), device=dev) if need_k else None) + none[2:]
        ds = -(g_r if g_c is None else g_c if g_r is None else g_r + g_c)
        dims = (B, K, Nq, Nk, 1, 1, ctx.inv_t, SPLIT_OPERAND_SCALE, _stream())
        # the key side of the pair terms walks the inverse table of the targets in a fixed order (K42's key backward at k = 1, Cv = 1):
        # dk_pair[j] = inv_t sum_{t(i) = j} ds_i qn_i, and the same walk sums g_c over a key's queries — what the gather col_lse[t(i)]
        # sends back to col_lse[j].  Unsupervised positions sit in key 0's list with ds = g_c = 0.
        g_col = dk_pair = None
        if need_k or g_c is not None:
            entries, offsets = _inverse_index_table(target.clamp(min=0).view(B, Nq, 1), Nk)
            dk_pair = torch.empty((B, Nk, K), device=dev, dtype=torch.float32) if need_k else None
            g_col = torch.empty((B, Nk), device=dev, dtype=torch.float32) if g_c is not None else None
            ones = torch.full((B, Nq), 1.0, device=dev, dtype=torch.float32)
            _call("corr_pair_nll_bwd_key", "cocos_sparse_softmax_warp_bwd_key_f16x3", qh.data_ptr(), ql.data_ptr(), ones.data_ptr(),
                  ds.data_ptr(), (g_c if g_c is not None else ones).data_ptr(), entries.data_ptr(), offsets.data_ptr(), _ptr(dk_pair),
                  _ptr(g_col), *dims)
            del entries, offsets, ones
        dq_t, dk_t = _lse_grads((qh, ql, kh, kl), row_lse, col_lse, g_r, g_col, ctx.inv_t, need_q, need_k)
        dqn = dkn = None
        if need_q:
            _call("pair_logits_bwd_query", "cocos_pair_logits_bwd_query_f16x3", kh.data_ptr(), kl.data_ptr(), target.data_ptr(), ds.data_ptr(),
                  dq_t.data_ptr(), B, K, Nq, Nk, ctx.inv_t, SPLIT_OPERAND_SCALE, 1, _stream())
            dqn = _transpose(dq_t)
            del dq_t
        if need_k:
            dk_t.add_(dk_pair)
            del dk_pair
            dkn = _transpose(dk_t)
        return (dqn, dkn) + none[2:]


def _lse_operands(name: str, qn, kn):
    """the argument checks corr_lse and corr_pair_nll share, in corr_match_mutual's order (the shape refusal included)"""
    for t, what in ((qn, "qn"), (kn, "kn")):
        if not torch.is_tensor(t):
            raise TypeError(f"{name}: {what}: expected a tensor, got {type(t).__name__}")
    return _operand_shapes(name, qn, kn)


def _lse_device(name: str, qn, kn, extra=()):
    _gate(name, ((qn, "qn"), (kn, "kn")) + tuple(extra), True)
    B, Nq, Nk = qn.shape[0], qn.shape[2], kn.shape[2]
    if not corr_match_mutual_ok(B, Nq, Nk):
        raise ValueError(f"{name}: B={B} Nq={Nq} Nk={Nk}: the sweep takes Nq and Nk that are multiples of 4 (corr_match_mutual_ok)")


def corr_lse(qn, kn, inv_temperature: float, planes: OperandPlanes | None = None):
    """(row_lse [B,Nq], col_lse [B,Nk]): the log-sum-exp of inv_temperature <qn_i, kn_j> over the keys and over the queries, with
    gradients for qn and kn (K49).  The forward is corr_match_mutual's sweep — the values are its row_lse / col_lse bit for bit; the
    backward is one sweep per operand that needs a gradient (cocos_corr_lse_bwd_f16x3: S recomputed, W . Kn on the MFMA), with a null g
    for an output nobody differentiated.  Nothing Nq x Nk is allocated, forward or backward; no atomics: bitwise reproducible.
    Operands as corr_match_mutual; shapes outside corr_match_mutual_ok raise ValueError."""
    name = "corr_lse"
    _lse_operands(name, qn, kn)
    _lse_device(name, qn, kn)
    qn, kn, pl = _fetch_planes(name, qn, kn, planes, False)
    return _CorrLse.apply(qn, kn, float(inv_temperature), *pl)


def corr_pair_nll(qn, kn, target, inv_temperature: float, planes: OperandPlanes | None = None, return_lse: bool = False,
                  check_target: bool = True):
    """The correspondence negative log-likelihood in both softmax directions (K49) -> (row_nll, col_nll), both [B,Nq] fp32:
        row_nll[b,i] = row_lse[b,i] - s,   col_nll[b,i] = col_lse[b,t] - s,   s = inv_temperature <qn_i, kn_t>,   t = target[b,i]
    — minus the log of the probability that query i picks key t among all keys, and that key t picks query i among all queries.
    target [B,Nq] int32 / int64: the key every query should match; negative = unsupervised (both terms 0, no gradient); a target >= Nk
    raises ValueError.  One autograd.Function, differentiable in qn and kn: it saves the operand planes, the two lse vectors and the
    table, nothing with an Nq x Nk extent (`check_target` False: the caller has checked the range already — the check reads the
    table's maximum back from the device, once per call is enough); the pair logit is sparse_softmax_warp's logit of the pair bit for bit; the key side of the
    pair terms and the gradient the gather col_lse[t] sends to col_lse walk the inverse table of the targets in a fixed order (no
    framework scatter, no atomics).  `return_lse`: also return (row_lse [B,Nq], col_lse [B,Nk]) without gradient.  Operands and refusals
    as corr_lse."""
    name = "corr_pair_nll"
    B, Nq, Nk = _lse_operands(name, qn, kn)
    table = _int_table(name, "target", target, (B, Nq))
    if check_target and target.numel() and int(target.max()) >= Nk:
        raise ValueError(f"{name}: target holds {int(target.max())}, expected values below Nk={Nk} (negative: unsupervised)")
    _lse_device(name, qn, kn, ((target, "target"),))
    qn, kn, pl = _fetch_planes(name, qn, kn, planes, False)
    row_nll, col_nll, row_lse, col_lse = _CorrPairNll.apply(qn, kn, table, float(inv_temperature), *pl)
    return (row_nll, col_nll, row_lse, col_lse) if return_lse else (row_nll, col_nll)


def match_round_trip(row_idx, col_idx, qgrid, kgrid):
    """The round trip of two index maps (K48, one launch) -> (q_back, q_dist, k_back, k_dist), all int32: row_idx [B,hq*wq] holds per
    position of the qgrid = (hq, wq) grid a position of the kgrid = (hk, wk) grid, col_idx [B,hk*wk] the other way round;
    q_back[b,i] = col_idx[b,row_idx[b,i]], q_dist[b,i] the Chebyshev distance in cells between q_back[b,i] and i on the qgrid, k_back /
    k_dist the same for the key side.  Any integer dtype (narrowed to int32 after a clamp); indices outside their range are clamped."""
    name = "match_round_trip"
    row_idx, col_idx = _int_table(name, "row_idx", row_idx, any_int=True), _int_table(name, "col_idx", col_idx, any_int=True)
    (hq, wq), (hk, wk) = _grid_pair(name, "qgrid", qgrid), _grid_pair(name, "kgrid", kgrid)
    if row_idx.dim() != 2 or col_idx.dim() != 2 or row_idx.shape[0] != col_idx.shape[0] or row_idx.shape[1] != hq * wq or col_idx.shape[1] != hk * wk:
        raise ValueError(f"{name}: row_idx {tuple(row_idx.shape)}, col_idx {tuple(col_idx.shape)} do not fit the grids {hq}x{wq} and {hk}x{wk}")
    _gate(name, ((row_idx, "row_idx"), (col_idx, "col_idx")), False)
    B = row_idx.shape[0]
    q_back, q_dist = torch.empty_like(row_idx), torch.empty_like(row_idx)
    k_back, k_dist = torch.empty_like(col_idx), torch.empty_like(col_idx)
    _call("match_round_trip", "cocos_match_round_trip", row_idx.data_ptr(), col_idx.data_ptr(), q_back.data_ptr(), q_dist.data_ptr(),
          k_back.data_ptr(), k_dist.data_ptr(), B, hq, wq, hk, wk, _stream())
    return q_back, q_dist, k_back, k_dist


def row_topk_lse(f: torch.Tensor, k: int):
    """(idx int32 [..., k], val [..., k], lse [...]) of the rows of a materialised logit matrix f [..., Nk] in one sweep (K39b):
    torch.topk(f, k, -1) with the lower index first among equal values, and torch.logsumexp(f, -1).  Rank 0 and lse are
    row_argmax_lse's outputs bit for bit.  Any Nk >= k, 1 <= k <= MATCH_TOPK_MAX (ValueError).  Forward only."""
    f, lead, B, Nq, Nk = _readout_rows("row_topk_lse", f)
    k = _check_topk("row_topk_lse", k, Nk)
    idx, val, lse = _readout_outputs(lead, k, f.device)
    _call("row_topk_lse", "cocos_row_topk_lse", f.data_ptr(), idx.data_ptr(), val.data_ptr(), lse.data_ptr(), B, Nq, Nk, k, _stream())
    return idx, val, lse


def gather_blend_patches(img: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, h: int, w_grid: int, down: int):
    """The k-sparse warp (K39c): out [B,C,H,W] whose cell (y, x) of the h x w_grid grid is sum_r w[b,r,y,x] * (the down x down patch of
    img at the cell idx[b,r,y,x]), accumulated in fp32 in the order r = 0, 1, ... — with k = 1 and w = 1 gather_patches bit for bit.
    img [Be,C,H,W] fp32 with H == h*down, W == w_grid*down and Be == B or 1; idx [B,k,h,w_grid] (or [B,k,h*w_grid]), any integer
    type (values outside [0, h*w_grid) are clamped into it); w fp32 of idx's shape; 1 <= k <= MATCH_TOPK_MAX."""
    img = _gather_gate("gather_blend_patches", img, idx)
    w = _chk(w.detach(), "gather_blend_patches: w")
    Be, C, H, W = img.shape
    B = idx.shape[0]
    k = idx.shape[1] if idx.dim() >= 3 else 0
    if ((H, W) != (h * down, w_grid * down) or not 1 <= k <= MATCH_TOPK_MAX or idx.numel() != B * k * h * w_grid
            or w.numel() != idx.numel() or w.shape[:2] != idx.shape[:2] or Be not in (B, 1)):
        raise ValueError(f"gather_blend_patches: img{tuple(img.shape)} idx{tuple(idx.shape)} w{tuple(w.shape)} do not fit k <= "
                         f"{MATCH_TOPK_MAX} candidates on a {h}x{w_grid} grid with down={down}")
    idx = idx.reshape(B, k, h * w_grid).to(torch.int32).contiguous()
    out = torch.empty((B, C, H, W), device=img.device, dtype=torch.float32)
    _call("gather_blend_patches", "cocos_gather_blend_patches", img.data_ptr(), idx.data_ptr(), w.data_ptr(), out.data_ptr(), B, C, H, W,
          int(down), k, C * H * W if Be == B else 0, _stream())
    return out


# ------------------------------------------------------------------------------------------
# K42  k-sparse correspondence warp with gradients: attention over the k selected keys of every query
# ------------------------------------------------------------------------------------------
def _transpose(x: torch.Tensor) -> torch.Tensor:
    """x [B,R,C] fp32 -> [B,C,R], a copy (cocos_transpose_f32): between the channel-major tensors of the ops and the position-major
    rows the K42 kernels gather"""
    B, R, C = x.shape
    out = torch.empty((B, C, R), device=x.device, dtype=torch.float32)
    _call("transpose", "cocos_transpose_f32", x.data_ptr(), out.data_ptr(), B, R, C, _stream())
    return out


def _inverse_index_table(idx: torch.Tensor, Nk: int):
    """idx [B,Nq,k] int32 with values in [0, Nk) -> (entries [B*Nq*k] int32, offsets [B*Nk+1] int32): the flat positions of idx grouped
    by the key b * Nk + j they name, ascending inside a group (a STABLE sort of the keys), and the group boundaries — what turns the
    key-side scatter into a gather in a fixed order.  Index plumbing on B*Nq*k integers; the arithmetic stays in the kernel."""
    B = idx.shape[0]
    key = (idx.long() + (torch.arange(B, device=idx.device) * Nk).view(B, 1, 1)).reshape(-1)
    entries = torch.sort(key, stable=True).indices.to(torch.int32)
    offsets = torch.zeros(B * Nk + 1, device=idx.device, dtype=torch.int32)
    offsets[1:] = torch.cumsum(torch.bincount(key, minlength=B * Nk), 0)
    return entries, offsets


def _plane_pair_backward(needs, qh, Nk, table, width, launch_query, launch_key, Cv=0):
    """The backward of K42 and K46 (plane_pair.hip); needs = (qn, kn, v), `table` [B,Nq,k] what the key side inverts, `width` the ds entries
    per query.  Every gradient comes from the same launch whichever others are asked for (the same bits); a launch that serves no needed
    gradient is skipped -> (dqn [B,K,Nq], dkn [B,K,Nk], dv [B,Cv,Nk]), None where not needed"""
    need_q, need_k, need_v = needs
    B, Nq, K = qh.shape
    new = lambda *shape: torch.empty(shape, device=qh.device, dtype=torch.float32)
    dqn = dkn = dv = ds = None
    if need_q or need_k:
        ds = new(B, Nq, width)
        dq_t = new(B, Nq, K) if need_q else None
        launch_query(ds.data_ptr(), _ptr(dq_t))
        if need_q:
            dqn = _transpose(dq_t)
            del dq_t
    if need_k or need_v:
        entries, offsets = _inverse_index_table(table, Nk)
        dk_t = new(B, Nk, K) if need_k else None
        dv_t = new(B, Nk, Cv) if need_v else None
        launch_key(_ptr(ds), entries.data_ptr(), offsets.data_ptr(), _ptr(dk_t), _ptr(dv_t))
        if need_k:
            dkn = _transpose(dk_t)
            del dk_t
        if need_v:
            dv = _transpose(dv_t)
    return dqn, dkn, dv


class _SparseSoftmaxWarp(torch.autograd.Function):
    """K42.  qn / kn are only the autograd inputs (fp32 tensors or producer handles): the kernels read their position-major operand
    planes qh, ql, kh, kl.  Saved for the backward: the four planes, v^T, idx and w [B,Nq,k] — nothing with an Nq x Nk extent."""

    @staticmethod
    def forward(ctx, qn, kn, v, idx, inv_t: float, qh, ql, kh, kl, k_bias=None):
        B, Nq, K = qh.shape
        Nk, Cv, k = kh.shape[1], v.shape[1], idx.shape[2]
        vt = _transpose(v)
        out_t = torch.empty((B, Nq, Cv), device=v.device, dtype=torch.float32)
        w = torch.empty((B, Nq, k), device=v.device, dtype=torch.float32)
        if k_bias is None:
            _call("sparse_softmax_warp_fwd", "cocos_sparse_softmax_warp_fwd_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(),
                  vt.data_ptr(), idx.data_ptr(), out_t.data_ptr(), w.data_ptr(), B, K, Nq, Nk, Cv, k, float(inv_t), SPLIT_OPERAND_SCALE, _stream())
        else:      # K50: the bias is a constant — the backward below consumes the saved w and never sees it
            _call("sparse_softmax_warp_bias_fwd", "cocos_sparse_softmax_warp_bias_fwd_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(),
                  kl.data_ptr(), vt.data_ptr(), idx.data_ptr(), k_bias.data_ptr(), out_t.data_ptr(), w.data_ptr(), B, K, Nq, Nk, Cv, k,
                  float(inv_t), SPLIT_OPERAND_SCALE, Nk, _stream())
        ctx.save_for_backward(qh, ql, kh, kl, vt, idx, w)
        ctx.inv_t = float(inv_t)
        ctx.mark_non_differentiable(w)
        return _transpose(out_t), w

    @staticmethod
    def backward(ctx, dout, _dw):
        qh, ql, kh, kl, vt, idx, w = ctx.saved_tensors
        B, Nq, K = qh.shape
        Nk, Cv, k = kh.shape[1], vt.shape[2], idx.shape[2]
        dout_t = _transpose(_chk(dout, "sparse_softmax_warp: dout"))
        name, dims = "sparse_softmax_warp_bwd_", (B, K, Nq, Nk, Cv, k, ctx.inv_t, SPLIT_OPERAND_SCALE, _stream())
        query = lambda *out: _call(name + "query", f"cocos_{name}query_f16x3", kh.data_ptr(), kl.data_ptr(), vt.data_ptr(), dout_t.data_ptr(),
                                   idx.data_ptr(), w.data_ptr(), *out, *dims)
        key = lambda ds, entries, offsets, *out: _call(name + "key", f"cocos_{name}key_f16x3", qh.data_ptr(), ql.data_ptr(), dout_t.data_ptr(),
                                                       ds, w.data_ptr(), entries, offsets, *out, *dims)
        return _plane_pair_backward(ctx.needs_input_grad[:3], qh, Nk, idx, k, query, key, Cv) + (None,) * 7


def sparse_softmax_warp(qn, kn, v, idx, inv_temperature: float, planes: OperandPlanes | None = None, return_weights: bool = False,
                        k_bias=None):
    """out [B,Cv,Nq] = sum_r w[b,i,r] * v[b,:,idx[b,i,r]] with w = softmax over r of inv_temperature * <qn[b,:,i], kn[b,:,idx[b,i,r]]>:
    attention over the k keys per query that a top-k readout selected (K42) — the k-sparse softmax of match(blend="topk"), with
    gradients for qn, kn and v (each computed only when needed; idx is data).  qn [B,256,Nq], kn [B,256,Nk] fp32 with unit-norm
    columns, or the handles of producer-made planes registered in `planes`, as corr_topk takes them (the logits come from the same
    operand planes that chose the candidates); v [B,Cv,Nk] fp32; idx [B,Nq,k] int32 / int64 with 1 <= k <= MATCH_TOPK_MAX, k <= Nk —
    any values: repeats inside a row are legal, values outside [0, Nk) are clamped into it.  Nothing Nq x Nk is allocated, forward or
    backward; dkn and dv are gathered over the inverse table of idx in a fixed order (no atomics: bitwise reproducible).
    `return_weights`: also return w [B,Nq,k] (no gradient).
    `k_bias` (K50; None, the default, is the code path above, untouched): float32 [B,Nk], finite or -inf — w = softmax over r of
    s_r + k_bias[b, idx[b,i,r]], the row-conditional transport plan on the k candidates when the bias is corr_sinkhorn's g.  The bias
    is NOT differentiable (one that requires a gradient raises ValueError): the gradients to qn, kn and v are those of the blend with
    the bias held constant.  A row whose candidates all carry -inf blends them uniformly."""
    if idx.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"sparse_softmax_warp: idx must be int32 or int64, got {idx.dtype}")
    if qn.dim() != 3 or kn.dim() != 3 or v.dim() != 3 or idx.dim() != 3:
        raise ValueError(f"sparse_softmax_warp: expected qn [B,256,Nq], kn [B,256,Nk], v [B,Cv,Nk], idx [B,Nq,k]; got {tuple(qn.shape)}, "
                         f"{tuple(kn.shape)}, {tuple(v.shape)}, {tuple(idx.shape)}")
    B, K, Nq = qn.shape
    Nk = kn.shape[2]
    if kn.shape[:2] != (B, K) or v.shape[0] != B or v.shape[2] != Nk or v.shape[1] < 1 or idx.shape[:2] != (B, Nq):
        raise ValueError(f"sparse_softmax_warp: shape mismatch qn{tuple(qn.shape)} kn{tuple(kn.shape)} v{tuple(v.shape)} idx{tuple(idx.shape)}")
    if K != FUSED_K:
        raise ValueError(f"sparse_softmax_warp: needs {FUSED_K} channels, got {K}")
    _check_topk("sparse_softmax_warp", int(idx.shape[2]), Nk)
    if k_bias is not None:
        k_bias = _bias_table("sparse_softmax_warp", k_bias, (B, Nk))
    _gate("sparse_softmax_warp", ((qn, "qn"), (kn, "kn"), (v, "v"), (idx, "idx")) + (((k_bias, "k_bias"),) if k_bias is not None else ()), True)
    qn, kn, pl = _fetch_planes("sparse_softmax_warp", qn, kn, planes, False)
    v = _chk(v, "sparse_softmax_warp: v")
    with torch.no_grad():
        idx = idx.clamp(0, Nk - 1).to(torch.int32).contiguous()
    out, w = _SparseSoftmaxWarp.apply(qn, kn, v, idx, float(inv_temperature), *pl, k_bias)
    return (out, w) if return_weights else out


# ------------------------------------------------------------------------------------------
# K43  PatchMatch candidate search: the selector of the k-sparse warp whose work does not grow with the number of keys
# ------------------------------------------------------------------------------------------
#: the largest number of search radii per iteration (COCOS_PATCHMATCH_MAX_RADII of cocos_hip.h)
PATCHMATCH_MAX_RADII = _lib.CONSTANTS["COCOS_PATCHMATCH_MAX_RADII"]
#: the schedule hot_path.correspondence_sparse(search="patchmatch") runs when search_opts names none: one launch per stride, `radii`
#: search radii per launch starting at `radius0` (DESIGN.md 3.27 holds the measurements behind it)
PATCHMATCH_DEFAULTS = dict(strides=(1, 2, 1, 1), radii=3, radius0=4, seed=0)


def _patchmatch_operands(name: str, qn, kn, grids, k):
    """the shape checks patchmatch_step / patchmatch_topk share -> (hq, wq, hk, wk); ValueError before the library is called"""
    try:
        qgrid, kgrid = grids
    except (TypeError, ValueError):
        raise ValueError(f"{name}: grids={grids!r}: expected ((hq, wq), (hk, wk))") from None
    (hq, wq), (hk, wk) = _grid_pair(name, "grids", qgrid), _grid_pair(name, "grids", kgrid)
    _operand_shapes(name, qn, kn, hq * wq, hk * wk, f" on a {hq}x{wq} query grid and a {hk}x{wk} key grid")
    _check_topk(name, k, hk * wk)
    return hq, wq, hk, wk


def _patchmatch_search(name: str, stride, radii, radius0, seed, iteration=0):
    if not _is_int(stride) or stride < 1:
        raise ValueError(f"{name}: stride={stride!r}: expected an integer >= 1")
    if not _is_int(radii) or not 0 <= radii <= PATCHMATCH_MAX_RADII:
        raise ValueError(f"{name}: radii={radii!r}: expected an integer in 0..{PATCHMATCH_MAX_RADII}")
    if not _is_int(radius0) or radius0 < 0:
        raise ValueError(f"{name}: radius0={radius0!r}: expected an integer >= 0")
    if not _is_int(seed) or not _is_int(iteration) or not (-2 ** 31 <= seed < 2 ** 31 and 0 <= iteration < 2 ** 31):
        raise ValueError(f"{name}: seed={seed!r} iteration={iteration!r}: expected 32-bit integers (iteration >= 0)")


def _patchmatch_launch(planes4, idx, hq, wq, hk, wk, inv_t, k, stride, radii, radius0, seed, iteration):
    """one K43 launch on ready planes; idx int32 [B,Nq,k] contiguous or None -> (idx_out, val_out), fresh buffers"""
    qh, ql, kh, kl = planes4
    B, Nq, K = qh.shape
    idx_out = torch.empty((B, Nq, k), device=qh.device, dtype=torch.int32)
    val_out = torch.empty((B, Nq, k), device=qh.device, dtype=torch.float32)
    _call("patchmatch_step", "cocos_patchmatch_step_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(), _ptr(idx),
          idx_out.data_ptr(), val_out.data_ptr(), B, K, hq, wq, hk, wk, k, stride, radii, radius0, seed, iteration, float(inv_t),
          SPLIT_OPERAND_SCALE, _stream())
    return idx_out, val_out


def _patchmatch_table(name: str, idx, B, Nq, k):
    idx = _int_table(name, "the index table", idx, (B, Nq, k))
    _gate(name, ((idx, "idx"),), False)
    return idx


def patchmatch_step(qn, kn, idx, grids, inv_t: float, k: int, stride: int, radii: int, radius0: int, seed: int, iteration: int,
                    planes: OperandPlanes | None = None):
    """One PatchMatch iteration (K43; forward only) -> (idx int32 [B,Nq,k], val [B,Nq,k]): per query the k best distinct keys, logit
    descending (equal bits: lower key first), of the pool {its own candidates idx[b,i,:]} U {the candidates of its four neighbours at
    distance `stride` on the query grid, shifted back by that offset} U {`radii` random offsets around each own candidate, the s-th
    within max(1, radius0 >> s)}.  qn [B,256,hq*wq], kn [B,256,hk*wk] as corr_topk takes them (fp32 unit-norm columns, or handles
    registered in `planes`); grids = ((hq, wq), (hk, wk)); idx [B,Nq,k] int32 / int64 (values outside the key grid are clamped into
    it) or None: a random initialisation hashed from (seed, iteration).  val holds the logits sparse_softmax_warp forms for the same
    pairs.  The draw is a pure function of (seed, iteration, query, rank), so a call is bitwise reproducible.  A pool with fewer than k
    distinct keys repeats its last pair.  Bad k, grids, stride, radii: ValueError before the library is called."""
    name = "patchmatch_step"
    hq, wq, hk, wk = _patchmatch_operands(name, qn, kn, grids, k)
    _patchmatch_search(name, stride, radii, radius0, seed, iteration)
    _gate(name, ((qn, "qn"), (kn, "kn")), True)
    with torch.no_grad():
        if idx is not None:
            idx = _patchmatch_table(name, idx, qn.shape[0], hq * wq, k)
        return _patchmatch_launch(_fetch_planes(name, qn, kn, planes, True, same_batch=True)[2], idx, hq, wq, hk, wk, inv_t, k, stride,
                                  radii, radius0, seed, iteration)


def patchmatch_topk(qn, kn, inv_t: float, k: int, grids, init="random", strides=PATCHMATCH_DEFAULTS["strides"],
                    radii=PATCHMATCH_DEFAULTS["radii"], seed: int = 0, planes: OperandPlanes | None = None):
    """PatchMatch top-k selection (K43; forward only) -> (idx int32 [B,Nq,k], val [B,Nq,k]) for sparse_softmax_warp: one
    patchmatch_step per entry of `strides` (iteration t = 0, 1, ...: launch t reads the table launch t - 1 wrote, two buffers alive at a
    time).  `init`: "random" or an integer tensor [B,Nq,k] of starting candidates.  `radii`: the number of search radii per iteration,
    starting at half the longer side of the key grid, or a pair (radii, radius0).  Operands, grids and errors as patchmatch_step; an
    empty `strides` is a ValueError (a selection needs scores)."""
    name = "patchmatch_topk"
    hq, wq, hk, wk = _patchmatch_operands(name, qn, kn, grids, k)
    if isinstance(init, str) and init != "random" or not (isinstance(init, str) or torch.is_tensor(init)):
        raise ValueError(f"{name}: init={init!r}: expected 'random' or an integer tensor [B,Nq,k]")
    try:
        strides = tuple(strides)
    except TypeError:
        raise ValueError(f"{name}: strides={strides!r}: expected a non-empty sequence of integers >= 1") from None
    if not strides:
        raise ValueError(f"{name}: strides is empty: expected a non-empty sequence of integers >= 1")
    n_radii, radius0 = radii if isinstance(radii, (tuple, list)) and len(radii) == 2 else (radii, max(hk, wk) // 2)
    for t, stride in enumerate(strides):
        _patchmatch_search(name, stride, n_radii, radius0, seed, t)
    _gate(name, ((qn, "qn"), (kn, "kn")), True)
    with torch.no_grad():
        idx = None if isinstance(init, str) else _patchmatch_table(name, init, qn.shape[0], hq * wq, k)
        planes4 = _fetch_planes(name, qn, kn, planes, True, same_batch=True)[2]
        val = None
        for t, stride in enumerate(strides):
            idx, val = _patchmatch_launch(planes4, idx, hq, wq, hk, wk, inv_t, k, stride, n_radii, radius0, seed, t)
        return idx, val


# ------------------------------------------------------------------------------------------
# K44  sub-cell match refinement: a soft-argmax over the window around a hard match, and the warp sampled there
# ------------------------------------------------------------------------------------------
#: the largest window radius of match_refine (COCOS_MATCH_REFINE_MAX_RADIUS of cocos_hip.h)
MATCH_REFINE_MAX_RADIUS = _lib.CONSTANTS["COCOS_MATCH_REFINE_MAX_RADIUS"]


def _refine_table(name: str, idx, B, Nq):
    """the centre table of K44, [B,Nq] or [B,h,w] -> int32 [B,Nq] contiguous (TypeError / ValueError first, then the device)"""
    idx = _int_table(name, "idx", idx)
    if idx.dim() < 1 or idx.shape[0] != B or idx.numel() != B * Nq:
        raise ValueError(f"{name}: idx is {tuple(idx.shape)}, expected {B} x {Nq} entries")
    _gate(name, ((idx, "idx"),), False)
    return idx.reshape(B, Nq)


def _refine_operands(name: str, qn, kn, kgrid, inv_t, radius):
    """the checks of the window soft-argmax's arguments (K44, K46) -> (hk, wk); ValueError before the library is called"""
    hk, wk = _grid_pair(name, "kgrid", kgrid)
    if not _is_int(radius) or not 1 <= radius <= MATCH_REFINE_MAX_RADIUS:
        raise ValueError(f"{name}: radius={radius!r}: expected an integer in 1..{MATCH_REFINE_MAX_RADIUS}")
    if not inv_t > 0:
        raise ValueError(f"{name}: inv_t={inv_t!r}: expected a positive number")
    _operand_shapes(name, qn, kn, None, hk * wk, f" on a {hk}x{wk} key grid")
    return hk, wk


def _match_refine_planes(qh, ql, kh, kl, idx, hk: int, wk: int, radius: int, inv_t: float):
    """K44 on operand planes and an int32 contiguous centre table [B,Nq] -> (off [B,Nq,2], lse_win [B,Nq])"""
    B, Nq, K = qh.shape
    off = torch.empty((B, Nq, 2), device=qh.device, dtype=torch.float32)
    lse_win = torch.empty((B, Nq), device=qh.device, dtype=torch.float32)
    _call("match_refine", "cocos_match_refine_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(), idx.data_ptr(),
          off.data_ptr(), lse_win.data_ptr(), B, K, Nq, hk * wk, hk, wk, radius, float(inv_t), SPLIT_OPERAND_SCALE, _stream())
    return off, lse_win


def match_refine(qn, kn, idx, kgrid, inv_t: float, radius: int, planes: OperandPlanes | None = None):
    """Sub-cell refinement of a hard match (K44; forward only) -> (off [B,Nq,2] fp32, x first; lse_win [B,Nq]): per query a softmax
    over the logits <qn[b,:,i], kn[b,:,j]> * inv_t of the keys j in the (2 radius + 1)^2 window around idx[b,i] on the `kgrid` =
    (hk, wk) key grid — positions outside the grid are left out — and its expected offset (sum p dx, sum p dy), in cells; lse_win is
    the window's log-sum-exp.  qn [B,256,Nq], kn [B,256,hk*wk] as corr_match takes them (fp32 unit-norm columns, or handles
    registered in `planes`); idx [B,Nq] (or [B,h,w]) int32 / int64, values outside the key grid are clamped into it.  The logits are
    sparse_softmax_warp's for the same pairs, bit for bit.  radius in 1..MATCH_REFINE_MAX_RADIUS, inv_t > 0: ValueError before the
    library is called."""
    name = "match_refine"
    hk, wk = _refine_operands(name, qn, kn, kgrid, inv_t, radius)
    B, _, Nq = qn.shape
    _gate(name, ((qn, "qn"), (kn, "kn")), True)
    with torch.no_grad():
        idx = _refine_table(name, idx, B, Nq)
        return _match_refine_planes(*_fetch_planes(name, qn, kn, planes, True, same_batch=True)[2], idx, hk, wk, radius, inv_t)


def _subcell_shapes(name: str, img, off, grid, kgrid, down):
    """the checks of the sub-cell gather's arguments (K44, K46) -> (fh, fw, hk, wk, B); TypeError / ValueError before the library is called"""
    fh, fw = _grid_pair(name, "grid", grid)
    hk, wk = _grid_pair(name, "kgrid", kgrid)
    if not _is_int(down) or down < 1:
        raise ValueError(f"{name}: down={down!r}: expected an integer >= 1")
    if not torch.is_tensor(off) or off.dtype != torch.float32:
        raise TypeError(f"{name}: off must be a float32 tensor")
    if img.dim() != 4 or tuple(img.shape[2:]) != (hk * down, wk * down):
        raise ValueError(f"{name}: img{tuple(img.shape)} is not a [Be,C,{hk * down},{wk * down}] image (a {hk}x{wk} grid with down={down})")
    B = off.shape[0]
    if tuple(off.shape) != (B, fh * fw, 2) or img.shape[0] not in (B, 1):
        raise ValueError(f"{name}: off{tuple(off.shape)} img{tuple(img.shape)}: expected off [B,{fh * fw},2] and an image batch of B or 1")
    return fh, fw, hk, wk, B


def gather_patches_subcell(img: torch.Tensor, idx: torch.Tensor, off: torch.Tensor, grid, kgrid, down: int):
    """gather_patches at a sub-cell position (K44; forward only): out [B,C,fh*down,fw*down] whose cell (y, x) of the `grid` = (fh, fw)
    samples img bilinearly where its match idx[b, y*fw+x] on the `kgrid` = (hk, wk) grid, moved by off[b, y*fw+x] = (off_x, off_y)
    cells, puts it (sample positions are clamped into the image).  img [Be,C,hk*down,wk*down] fp32, Be == B or 1; idx [B,fh*fw] or
    [B,fh,fw] int32 / int64 (values outside the key grid are clamped into it); off [B,fh*fw,2] fp32, x first, as match_refine returns
    it.  With off == 0 the output is gather_patches' copy, bit for bit."""
    name = "gather_patches_subcell"
    fh, fw, hk, wk, B = _subcell_shapes(name, img, off, grid, kgrid, down)
    img = _chk(img.detach(), f"{name}: img")
    with torch.no_grad():
        idx = _refine_table(name, idx, B, fh * fw)
        off = _chk(off.detach(), f"{name}: off")
        Be, C = img.shape[:2]
        out = torch.empty((B, C, fh * down, fw * down), device=img.device, dtype=torch.float32)
        _call("gather_patches_subcell", "cocos_gather_patches_subcell", img.data_ptr(), idx.data_ptr(), off.data_ptr(), out.data_ptr(), B,
              C, fh, fw, hk, wk, down, C * hk * down * wk * down if Be == B else 0, _stream())
    return out


# ------------------------------------------------------------------------------------------
# K46  trainable sub-cell correspondence: gradients of the window soft-argmax (to qn, kn) and of the bilinear warp (to the offset)
# ------------------------------------------------------------------------------------------
class _SoftMatchOffset(torch.autograd.Function):
    """K44's readout with K46's backward.  qn / kn are only the autograd inputs (fp32 tensors or producer handles): the kernels read
    their position-major operand planes.  Saved for the backward: the four planes and idx [B,Nq] — nothing with an Nq x Nk extent (the
    window's logits are recomputed)."""

    @staticmethod
    def forward(ctx, qn, kn, idx, inv_t: float, radius: int, hk: int, wk: int, qh, ql, kh, kl):
        off, lse_win = _match_refine_planes(qh, ql, kh, kl, idx, hk, wk, radius, inv_t)
        ctx.save_for_backward(qh, ql, kh, kl, idx)
        ctx.cfg = (float(inv_t), radius, hk, wk)
        ctx.mark_non_differentiable(lse_win)
        return off, lse_win

    @staticmethod
    def backward(ctx, doff, _dlse):
        qh, ql, kh, kl, idx = ctx.saved_tensors
        inv_t, radius, hk, wk = ctx.cfg
        B, Nq, K = qh.shape
        doff = _chk(doff, "soft_match_offset: doff")
        name, dims = "match_refine_bwd_", (B, K, Nq, hk * wk, hk, wk, radius, inv_t, SPLIT_OPERAND_SCALE, _stream())
        query = lambda *out: _call(name + "query", f"cocos_{name}query_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(),
                                   idx.data_ptr(), doff.data_ptr(), *out, *dims)
        key = lambda ds, entries, offsets, dk_t, _dv_t: _call(name + "key", f"cocos_{name}key_f16x3", qh.data_ptr(), ql.data_ptr(), ds, entries,
                                                              offsets, dk_t, *dims)
        # the key side gathers over the inverse table of the (clamped) centres: K42's, with k = 1
        needs = ctx.needs_input_grad[:2] + (False,)
        return _plane_pair_backward(needs, qh, hk * wk, idx.view(B, Nq, 1), (2 * radius + 1) ** 2, query, key)[:2] + (None,) * 9


def soft_match_offset(qn, kn, idx, kgrid, inv_t: float, radius: int, planes: OperandPlanes | None = None):
    """match_refine with gradients (K46) -> (off [B,Nq,2], lse_win [B,Nq]), both match_refine's bit for bit: the expected offset of the
    softmax over the (2 radius + 1)^2 window of keys around idx[b,i], differentiable in qn and kn (each gradient computed only when
    needed; idx is data, lse_win carries no gradient).  The forward's limit of off to [-radius, radius] only absorbs an ulp of rounding:
    the backward treats it as the identity.  Nothing Nq x Nk is allocated, forward or backward; dkn is gathered over the inverse table
    of the centres in a fixed order (no atomics: bitwise reproducible; a centre all queries share is one serial list per key around it).
    Arguments and errors as match_refine."""
    name = "soft_match_offset"
    hk, wk = _refine_operands(name, qn, kn, kgrid, inv_t, radius)
    B, _, Nq = qn.shape
    _gate(name, ((qn, "qn"), (kn, "kn")), True)
    with torch.no_grad():
        idx = _refine_table(name, idx, B, Nq).clamp(0, hk * wk - 1)      # the kernels clamp as well: the table the key side inverts
    qn, kn, pl = _fetch_planes(name, qn, kn, planes, False, same_batch=True)
    return _SoftMatchOffset.apply(qn, kn, idx, float(inv_t), radius, hk, wk, *pl)


class _SubcellWarp(torch.autograd.Function):
    """K44's sub-cell gather with K46's gradient to the offset (none to the image: subcell_warp refuses one that asks)."""

    @staticmethod
    def forward(ctx, off, img, idx, fh: int, fw: int, hk: int, wk: int, down: int):
        B, (Be, C) = off.shape[0], img.shape[:2]
        out = torch.empty((B, C, fh * down, fw * down), device=img.device, dtype=torch.float32)
        ctx.dims = (B, C, fh, fw, hk, wk, down, C * hk * down * wk * down if Be == B else 0)
        _call("gather_patches_subcell", "cocos_gather_patches_subcell", img.data_ptr(), idx.data_ptr(), off.data_ptr(), out.data_ptr(),
              *ctx.dims, _stream())
        ctx.save_for_backward(img, idx, off)
        return out

    @staticmethod
    def backward(ctx, dout):
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        img, idx, off = ctx.saved_tensors
        dout = _chk(dout, "subcell_warp: dout")
        doff = torch.empty_like(off)
        _call("gather_patches_subcell_bwd_off", "cocos_gather_patches_subcell_bwd_off", img.data_ptr(), idx.data_ptr(), off.data_ptr(),
              dout.data_ptr(), doff.data_ptr(), *ctx.dims, _stream())
        return (doff,) + (None,) * 7


def subcell_warp(img: torch.Tensor, idx: torch.Tensor, off: torch.Tensor, grid, kgrid, down: int):
    """gather_patches_subcell with a gradient to the offset (K46): out [B,C,fh*down,fw*down], gather_patches_subcell's bit for bit;
    d out / d off is the slope of the bilinear sample along each axis, 0 where the sample is clamped at the image border (at an exact
    pixel position: the right derivative).  The gradient to the image is not built: an `img` that requires one raises ValueError
    (detach it) — nothing drops a gradient silently.  Arguments and errors as gather_patches_subcell."""
    name = "subcell_warp"
    fh, fw, hk, wk, B = _subcell_shapes(name, img, off, grid, kgrid, down)
    if img.requires_grad:
        raise ValueError(f"{name}: img requires a gradient, and the gradient to the exemplar image is not built (pass img.detach())")
    img, off = _chk(img, f"{name}: img"), _chk(off, f"{name}: off")
    with torch.no_grad():
        idx = _refine_table(name, idx, B, fh * fw)
    return _SubcellWarp.apply(off, img, idx, fh, fw, hk, wk, down)


# ------------------------------------------------------------------------------------------
# K3  materialised correlation        (correspondence.py:291 + :304; return_corr / WTA / mk != 1)
# ------------------------------------------------------------------------------------------
class _CorrMaterialize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qn, kn, scale: float):
        qn, kn = _chk(qn, "qn"), _chk(kn, "kn")
        B, K, Nq = qn.shape
        Nk = kn.shape[2]
        if kn.shape[:2] != (B, K):
            raise ValueError(f"corr_materialize: shape mismatch qn{tuple(qn.shape)} kn{tuple(kn.shape)}")
        f = torch.empty((B, Nq, Nk), device=qn.device, dtype=torch.float32)
        ctx.amax = None
        if PRECISION == "f16x3" and min(K * Nq, K * Nk) >= 4:
            ctx.amax = (absmax(qn), absmax(kn))
            if K % 8 == 0:
                # both operands are k-major [K][positions]: the split GEMM would transpose them through 2-byte LDS
                # writes; position-major planes + the planes GEMM do the same product in half the time
                qh, ql, qs = split_f16(qn, True, amax=ctx.amax[0])
                kh, kl, ks = split_f16(kn, True, amax=ctx.amax[1])
                _call("corr_materialize", "cocos_hgemm_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(),
                      f.data_ptr(), B, Nq, Nk, K, float(scale), qs.data_ptr(), ks.data_ptr(), 0, _stream())
            else:                                                   # split GEMM (sgemm_f16x3.hip)
                _call("corr_materialize", "cocos_corr_materialize_f16x3", qn.data_ptr(), kn.data_ptr(), f.data_ptr(), B,
                      K, Nq, Nk, float(scale), ctx.amax[0].data_ptr(), ctx.amax[1].data_ptr(), _stream())
        else:
            _call("corr_materialize", "cocos_corr_materialize", qn.data_ptr(), kn.data_ptr(), f.data_ptr(), B, K, Nq,
                  Nk, float(scale), _stream())
        ctx.save_for_backward(qn, kn)
        ctx.scale = float(scale)
        return f

    @staticmethod
    def backward(ctx, df):
        qn, kn = ctx.saved_tensors
        df = _chk(df, "df")
        B, K, Nq = qn.shape
        Nk = kn.shape[2]
        need_q, need_k = ctx.needs_input_grad[:2]
        dqn = torch.empty_like(qn) if need_q else None
        dkn = torch.empty_like(kn) if need_k else None
        if ctx.amax is not None and Nq * Nk >= 4:
            qa, ka = ctx.amax
            ga = _recall_amax(df)            # left by the kernel that wrote df (K6's backward), else one pass
            if ga is None:
                ga = absmax(df)
            _call("corr_materialize_bwd", "cocos_corr_materialize_bwd_f16x3", qn.data_ptr(), kn.data_ptr(),
                  df.data_ptr(), _ptr(dqn), _ptr(dkn), B, K, Nq, Nk, ctx.scale, qa.data_ptr(), ka.data_ptr(),
                  ga.data_ptr(), _stream())
        else:
            _call("corr_materialize_bwd", "cocos_corr_materialize_bwd", qn.data_ptr(), kn.data_ptr(), df.data_ptr(),
                  _ptr(dqn), _ptr(dkn), B, K, Nq, Nk, ctx.scale, _stream())
        return dqn, dkn, None


def corr_materialize(qn, kn, scale: float = 1.0):
    """f[b,i,j] = scale * <qn[b,:,i], kn[b,:,j]>   -> [B,Nq,Nk] (any K)."""
    return _CorrMaterialize.apply(qn, kn, scale)


# ------------------------------------------------------------------------------------------
# K4  row softmax on a materialised matrix   (correspondence.py:307)
# ------------------------------------------------------------------------------------------
class _RowSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s):
        s = _chk(s, "row_softmax: s")
        cols = s.shape[-1]
        rows = s.numel() // cols
        p = torch.empty_like(s)
        _call("row_softmax_fwd", "cocos_row_softmax_fwd", s.data_ptr(), p.data_ptr(), rows, cols, _stream())
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, dp):
        (p,) = ctx.saved_tensors
        dp = _chk(dp, "row_softmax: dp")
        cols = p.shape[-1]
        rows = p.numel() // cols
        ds = torch.empty_like(p)
        _call("row_softmax_bwd", "cocos_row_softmax_bwd", p.data_ptr(), dp.data_ptr(), ds.data_ptr(), rows, cols,
                  _stream())
        return ds


def row_softmax(s):
    """softmax over the last dimension of a materialised matrix."""
    return _RowSoftmax.apply(s)


# ------------------------------------------------------------------------------------------
# K5  P @ V on a materialised P            (correspondence.py:318 on the fallback path)
# ------------------------------------------------------------------------------------------
class _WarpMaterialized(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, v):
        p, v = _chk(p, "p"), _chk(v, "v")
        B, Nq, Nk = p.shape
        Cv = v.shape[1]
        if v.shape[0] != B or v.shape[2] != Nk:
            raise ValueError(f"warp_materialized: shape mismatch p{tuple(p.shape)} v{tuple(v.shape)}")
        out = torch.empty((B, Cv, Nq), device=p.device, dtype=torch.float32)
        _call("warp_materialized_fwd", "cocos_warp_materialized_fwd", p.data_ptr(), v.data_ptr(), out.data_ptr(), B, Nq,
                  Nk, Cv, _stream())
        ctx.save_for_backward(p, v)
        return out

    @staticmethod
    def backward(ctx, dout):
        p, v = ctx.saved_tensors
        dout = _chk(dout, "dout")
        B, Nq, Nk = p.shape
        Cv = v.shape[1]
        need_p, need_v = ctx.needs_input_grad
        dp = torch.empty_like(p) if need_p else None
        dv = torch.empty_like(v) if need_v else None
        _call("warp_materialized_bwd", "cocos_warp_materialized_bwd", p.data_ptr(), v.data_ptr(), dout.data_ptr(),
                  _ptr(dp), _ptr(dv), B, Nq, Nk, Cv, _stream())
        return dp, dv


def warp_materialized(p, v):
    """out[b,c,i] = sum_j p[b,i,j] v[b,c,j]   (p [B,Nq,Nk], v [B,Cv,Nk]) -> [B,Cv,Nq]."""
    return _WarpMaterialized.apply(p, v)


# ------------------------------------------------------------------------------------------
# K0  theta / phi 1x1 projections            (correspondence.py:272, :282)
# ------------------------------------------------------------------------------------------
class _ThreadState(threading.local):
    """Host-side scratch that must not be shared between threads (SURVEY.md §8b threading contract: under the
    reference's DataParallelWithCallback every replica's forward runs in its own Python thread, and autograd runs
    each device's backward in its own thread): the pool of pre-zeroed max|x| cells and the producer -> consumer
    max|x| table.  threading.local gives every thread its own instance; no locks on the hot path."""

    def __init__(self):
        self.zero_pool = {}      # (device, stream) -> [zeros tensor, next free cell]
        self.known_amax = {}     # (device, storage pointer) -> (the tensor, its version, amax cell)
        self.known_rowdot = None  # (weakref of dout, its version, data_ptr of out, D [B,N]) left by warp_head's backward


_tls = _ThreadState()
_KNOWN_AMAX_MAX = 8      # entries per thread that hold their tensor
_KNOWN_AMAX_WEAK_MAX = 48      # ... and entries that only watch theirs (see _remember_amax)


#: tensors at least this large are remembered through a weak reference only (see _remember_amax)
_AMAX_WEAK_BYTES = 32 << 20


def _remember_amax(t: torch.Tensor, cell: torch.Tensor, weak: bool = False):
    """A producer kernel computed max|t| while writing t: keep it for the consumer (autograd hands the gradient on
    as a view of the same storage; producer and consumer of one device's backward run in the same thread).  Small
    tensors are held by the entry itself, so their address cannot be recycled for other data while the entry exists;
    it is dropped when the consumer picks it up, or when younger ones arrive.  LARGE tensors (the HWxHW box-adjoint
    gradient of match_kernel 3: 0.5 GB at B = 8) are held through a WEAK reference: a strong one kept up to
    four of them alive across steps and, by raising the use count of a gradient, forced autograd's accumulation of
    several passes' gradients out of place.  A dead weak reference means the tensor was summed into another one or
    freed: the entry is void and the consumer takes its own max|.| pass — never a stale value."""
    table = _tls.known_amax
    # (weak = True: the entry must not keep `t` alive whatever its size — a convolution's INPUT remembered for a sibling convolution
    #  (ADVICE r5): a strong reference kept up to four dead activations alive across steps)
    big = weak or t.numel() * t.element_size() >= _AMAX_WEAK_BYTES
    # two quotas: entries that HOLD their tensor (small ones) stay few — they pin memory; weak entries pin nothing and may be many: the
    # label map that a SPADEResnetBlock's three SPADEs read is found by the third one although a dozen producer entries (K21's weights,
    # K9's outputs) came in between (with one quota of 8 it had been evicted: 24 max|.| passes per module step)
    n_strong = sum(1 for e in table.values() if not isinstance(e[0], weakref.ref))
    if big:
        for k in [k for k, e in table.items() if isinstance(e[0], weakref.ref) and e[0]() is None]:
            del table[k]                                     # (dead tensors first)
        while len(table) - n_strong >= _KNOWN_AMAX_WEAK_MAX:
            table.pop(next(k for k, e in table.items() if isinstance(e[0], weakref.ref)), None)
    else:
        while n_strong >= _KNOWN_AMAX_MAX:
            table.pop(next(k for k, e in table.items() if not isinstance(e[0], weakref.ref)), None)
            n_strong -= 1
    table[(t.device, t.untyped_storage().data_ptr())] = (weakref.ref(t) if big else t, t._version, cell)


def _recall_amax(t: torch.Tensor, consume: bool = True):
    table = _tls.known_amax
    key = (t.device, t.untyped_storage().data_ptr())
    ent = table.pop(key, None) if consume else table.get(key)
    if ent is None:
        return None
    src, version, cell = ent
    if isinstance(src, weakref.ref):
        src = src()
        if src is None:
            table.pop(key, None)
            return None
    if (t.numel() != src.numel() or t.storage_offset() != src.storage_offset() or not t.is_contiguous()
            or t._version != version or src._version != version):
        return None
    return cell


def _zero_cell(device) -> torch.Tensor:
    """A 1-element fp32 tensor holding 0, from a per-thread pool zeroed 4096 cells at a time on the current stream
    (one fill per ~500 steps instead of a 5 us memset in front of each of the max|x| passes of a step)."""
    pool = _tls.zero_pool
    key = (device, _stream())
    ent = pool.get(key)
    if ent is None or ent[1] >= ent[0].numel():
        ent = pool[key] = [torch.zeros(4096, device=device, dtype=torch.float32), 0]
    cell = ent[0][ent[1]:ent[1] + 1]
    ent[1] += 1
    return cell


def _zero_cells(device, n: int) -> torch.Tensor:
    """n CONSECUTIVE cells of the pool above (a kernel that leaves several maxima takes one pointer)."""
    pool = _tls.zero_pool
    key = (device, _stream())
    ent = pool.get(key)
    if ent is None or ent[1] + n > ent[0].numel():
        ent = pool[key] = [torch.zeros(4096, device=device, dtype=torch.float32), 0]
    cells = ent[0][ent[1]:ent[1] + n]
    ent[1] += n
    return cells


def absmax(x: torch.Tensor) -> torch.Tensor:
    """max|x| as a 1-element CUDA tensor (one pass, no host sync) — the scale source of the f16 splits."""
    x = _chk(x, "absmax: x")
    out = _zero_cell(x.device)
    _call("absmax", "cocos_absmax_accumulate", x.data_ptr(), x.numel(), out.data_ptr(), _stream())
    return out


def absmax_many(xs):
    """[max|x| cell for x in xs] with ONE launch per four tensors (cocos_absmax4) — the max|.| passes a step takes in a row (the two
    feature tensors and the two projection weights in front of K23 / K0) used to be a 5-14 us launch each."""
    xs = [_chk(x, "absmax_many: x") for x in xs]
    cells = [_zero_cell(x.device) for x in xs]
    for i in range(0, len(xs), 4):
        args = []
        for x, c in zip(xs[i:i + 4], cells[i:i + 4]):
            args += [x.data_ptr(), x.numel(), c.data_ptr()]
        args += [None, 0, None] * (4 - len(xs[i:i + 4]))
        _call("absmax", "cocos_absmax4", *args, _stream())
    return cells


def prefetch_amax(xs):
    """max|x| of the tensors in `xs` that no producer has left a value for, in ONE launch, remembered for their consumers (the two
    feature tensors and the two weights of a pair of projections: match_kernel 3's K0 calls picked them up one 5-14 us pass each)."""
    todo = [x for x in xs if x is not None and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
            and _recall_amax(x, consume=False) is None]
    if todo:
        for x, c in zip(todo, absmax_many(todo)):
            _remember_amax(x, c)


def sum_leading(x: torch.Tensor) -> torch.Tensor:
    """x.sum(0) for contiguous fp32 partial tiles [S, ...] (cocos_sum_leading)."""
    x = _chk(x, "sum_leading: x")
    out = torch.empty(x.shape[1:], device=x.device, dtype=torch.float32)
    _call("sum_leading", "cocos_sum_leading", x.data_ptr(), out.data_ptr(), x.shape[0], out.numel(), _stream())
    return out


def channel_sum(dy: torch.Tensor) -> torch.Tensor:
    """dy.sum((0, 2, 3)) of a contiguous fp32 [B,C,...] tensor: the bias gradient of a convolution (cocos_channel_sum)."""
    dy = _chk(dy, "channel_sum: dy")
    B, C = dy.shape[:2]
    N = dy.numel() // (B * C)
    S = _lib.load().cocos_channel_sum_slices(C, N)
    db = torch.empty(C, device=dy.device, dtype=torch.float32)
    part = torch.empty(S * C, device=dy.device, dtype=torch.float32) if S > 1 else None
    _call("channel_sum", "cocos_channel_sum", dy.data_ptr(), db.data_ptr(), part.data_ptr() if S > 1 else None, B, C, N, _stream())
    return db


def _proj1x1_forward(x, weight, bias, need_t: bool, prepared=None):
    """y = conv1x1(x, weight, bias) on K0 -> (y, x, w2, state): `state` = what the backward needs (split / stream flags, the max|.|
    cells, the transposed weight planes when `need_t`).  Shared by _Proj1x1 and _ProjUnfoldStats.  `prepared`: the layer's frozen
    record (inference.py) — its max|w| cell and, when no transposed planes are wanted, its k-padded planes replace the preparation."""
    x = _chk(x, "proj1x1: x")
    w2 = _chk(weight.reshape(weight.shape[0], -1), "proj1x1: weight")
    B, Cin, h, w = x.shape
    Cout = w2.shape[0]
    if w2.shape[1] != Cin:
        raise ValueError(f"proj1x1: weight {tuple(weight.shape)} does not match input {tuple(x.shape)}")
    bb = None if bias is None else _chk(bias, "proj1x1: bias")
    y = torch.empty((B, Cout, h, w), device=x.device, dtype=torch.float32)
    split = PROJ_PRECISION == "f16x3" and min(Cin * Cout, Cin * h * w, Cout * h * w) >= 4
    # the reference's shapes (<= 416 input channels, grid a multiple of 64 positions): weight planes resident in
    # the accumulator file, x and y streamed once (proj_stream_f16x3.hip)
    lib = _lib.load()
    stream = (split and PROJ_STREAM and (h * w) % 64 == 0 and lib.cocos_proj1x1_stream_kpad(Cin) != 0
              and lib.cocos_proj1x1_stream_kpad(Cout) != 0)
    st = dict(split=split, stream=stream, amax=None, t_planes=None, wshape=tuple(weight.shape), has_bias=bias is not None)
    if split:      # products on the f16 MFMA, operands split on the fly (sgemm_f16x3.hip)
        # left by K21 when the layer is spectral-normed (W / sigma) or by prefetch_amax, else one small pass
        wa = _recall_amax(w2) if prepared is None else prepared.amax
        xa = _recall_amax(x)
        xa, wa = (absmax(x) if xa is None else xa), (absmax(w2) if wa is None else wa)
        if stream:
            # A = W as planes [Cout][Kpad], rows zero-padded to whole MFMA k-steps
            kp = lib.cocos_proj1x1_stream_kpad(Cin)
            if prepared is not None and not need_t:
                wh, wl, ws = prepared.planes("rows", kp)
            else:
                wh = torch.empty((Cout, kp), device=x.device, dtype=torch.float16)
                wl = torch.empty((Cout, kp), device=x.device, dtype=torch.float16)
                ws = torch.empty(1, device=x.device, dtype=torch.float32)
                # ... and, when the input gradient will be wanted, the transposed planes [Cin][Kpad(Cout)] of dx = W^T dy
                # in the same launch (they used to be a second split in the backward)
                th = tl = None
                if need_t:
                    kpo = lib.cocos_proj1x1_stream_kpad(Cout)
                    th = torch.empty((Cin, kpo), device=x.device, dtype=torch.float16)
                    tl = torch.empty((Cin, kpo), device=x.device, dtype=torch.float16)
                _call("split_f16", "cocos_proj_weight_planes", w2.data_ptr(), wh.data_ptr(), wl.data_ptr(), _ptr(th), _ptr(tl),
                      Cout, Cin, kp, lib.cocos_proj1x1_stream_kpad(Cout), wa.data_ptr(), ws.data_ptr(), _stream())
                st["t_planes"] = (th, tl, ws) if th is not None else None
            _call("proj1x1_fwd", "cocos_proj1x1_stream_f16x3", x.data_ptr(), wh.data_ptr(), wl.data_ptr(),
                  ws.data_ptr(), _ptr(bb), y.data_ptr(), B, Cin, Cout, h * w, xa.data_ptr(), _stream())
        else:
            _call("proj1x1_fwd", "cocos_proj1x1_fwd_f16x3", x.data_ptr(), w2.data_ptr(), _ptr(bb), y.data_ptr(),
                  B, Cin, Cout, h * w, xa.data_ptr(), wa.data_ptr(), _stream())
        st["amax"] = (xa, wa)
    else:
        _call("proj1x1_fwd", "cocos_proj1x1_fwd", x.data_ptr(), w2.data_ptr(), _ptr(bb), y.data_ptr(), B, Cin,
              Cout, h * w, _stream())
    return y, x, w2, st


class _Proj1x1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, prepared=None):
        y, x, w2, st = _proj1x1_forward(x, weight, bias, ctx.needs_input_grad[0], prepared)
        ctx.split, ctx.stream, ctx.amax, ctx.t_planes = st["split"], st["stream"], st["amax"], st["t_planes"]
        ctx.save_for_backward(x, w2)
        ctx.wshape, ctx.has_bias = st["wshape"], st["has_bias"]
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w2 = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        return (*_proj1x1_backward(x, w2, dy, ctx.amax if ctx.split else None, getattr(ctx, "t_planes", None), ctx.split, ctx.stream,
                                   need_x, need_w, need_b and ctx.has_bias, ctx.wshape), None)


def _proj1x1_backward(x, w2, dy, amax, t_planes, split, stream, need_x, need_w, need_b, wshape):
    """Backward of y = conv1x1(x, w2) given dy: (dx, dw, db) — shared by _Proj1x1 and the fused projection + normalisation
    (_ProjCenterL2NormPlanesPair).  `amax` = (max|x|, max|w|) device cells of the split flavour; `t_planes` = the transposed weight
    planes (hi, lo, scale) when the forward already made them."""
    dy = _chk(dy, "proj1x1: dy")
    B, Cin, h, w = x.shape
    Cout = w2.shape[0]
    N = h * w
    lib = _lib.load()
    dx = torch.empty_like(x) if need_x else None
    dw = db = None
    if split:
        xa, wa = amax
        ga = _recall_amax(dy)            # left by the kernel that wrote dy (K1's backward), else one pass
        if ga is None:
            ga = absmax(dy)
        dx_gemm, dw_gemm = need_x, need_w
        if stream and need_x:     # dx = W^T dy, same streaming kernel with the transposed weight planes
            if t_planes is not None:
                th, tl, ts = t_planes
            else:
                th, tl, ts = split_f16(w2.unsqueeze(0), transpose=True, cpad=lib.cocos_proj1x1_stream_kpad(Cout),
                                       amax=wa)
            _call("proj1x1_bwd", "cocos_proj1x1_stream_f16x3", dy.data_ptr(), th.data_ptr(), tl.data_ptr(),
                  ts.data_ptr(), None, dx.data_ptr(), B, Cout, Cin, N, ga.data_ptr(), _stream())
            dx_gemm = False
        parts = lib.cocos_proj1x1_dw_partials_f16x3(B, Cin, Cout, N) if (need_w and PROJ_STREAM) else 0
        if parts:                     # dw (and db) in one pass over dy and x (proj_dw_f16x3.hip)
            ws = torch.empty((parts, Cout, (Cin + 31) // 32 * 32), device=x.device, dtype=torch.float32)
            wsb = torch.empty((parts, Cout), device=x.device, dtype=torch.float32) if need_b else None
            dw = torch.empty((Cout, Cin), device=x.device, dtype=torch.float32)
            db = torch.empty(Cout, device=x.device, dtype=torch.float32) if need_b else None
            _call("proj1x1_bwd", "cocos_proj1x1_dw_f16x3", dy.data_ptr(), x.data_ptr(), ws.data_ptr(), _ptr(wsb),
                  dw.data_ptr(), _ptr(db), B, Cin, Cout, N, ga.data_ptr(), xa.data_ptr(), _stream())
            dw_gemm = False
        if dx_gemm or dw_gemm:
            dwb = None
            if dw_gemm:
                dwb = torch.empty((lib.cocos_proj1x1_bwd_partials_f16x3(B, Cin, Cout, N), Cout, Cin),
                                  device=x.device, dtype=torch.float32)
            _call("proj1x1_bwd", "cocos_proj1x1_bwd_f16x3", x.data_ptr(), w2.data_ptr(), dy.data_ptr(),
                  dx.data_ptr() if dx_gemm else None, _ptr(dwb), B, Cin, Cout, N, xa.data_ptr(), wa.data_ptr(),
                  ga.data_ptr(), _stream())
            if dw_gemm:
                dw = sum_leading(dwb)                                   # [P,256,Cl] partials, small
    else:
        dwb = None
        if need_w:
            dwb = torch.empty((lib.cocos_proj1x1_bwd_partials(B, Cin, Cout, N), Cout, Cin), device=x.device,
                              dtype=torch.float32)
        _call("proj1x1_bwd", "cocos_proj1x1_bwd", x.data_ptr(), w2.data_ptr(), dy.data_ptr(), _ptr(dx),
              _ptr(dwb), B, Cin, Cout, N, _stream())
        if need_w:
            dw = sum_leading(dwb)
    if need_w:
        dw = dw.reshape(wshape)
    if need_b and db is None:
        db = channel_sum(dy)
    return dx, dw, db


def proj1x1(x, weight, bias=None, prepared=None):
    """nn.Conv2d(Cin, Cout, kernel_size=1): x [B,Cin,h,w], weight [Cout,Cin,1,1].  PROJ_PRECISION "f16x3" (default):
    the streaming split-precision kernels at the reference's shapes, else the split GEMM; "fp32": the fp32-MFMA GEMM.
    `prepared`: the layer's frozen record (cocosnet_amd.inference), or None — today's route, byte for byte."""
    return _Proj1x1.apply(x, weight, bias, prepared)


# ------------------------------------------------------------------------------------------
# K23  K0 fused with K1: projection -> centre -> L2-normalise -> operand planes   (correspondence.py:272-289; proj_norm_f16x3.hip)
# ------------------------------------------------------------------------------------------
#: False: the fused match_kernel-1 path projects with K0 and normalises with K1 in separate launches (the round-5 chain; A/B runs)
PROJ_NORM_FUSED = os.environ.get("COCOS_PROJ_NORM_FUSED", "1") != "0"
#: K30: the row pass's head (ops.warp_head) also on the --warp_bilinear / --warp_patch / --warp_cycle_w flag sets and on passes without
#: mask channels, and warp_values without a direct mask / in patch mode (hot_path.py).  False: the framework ops of round 6.
WARP_HEAD_MODES = os.environ.get("COCOS_WARP_HEAD_MODES", "1") != "0"
#: False: the projections' backward runs as round 5's chain (K1 backward / K12 backward + autograd's add -> max|.| -> input gradient ->
#: weight gradient); True: K24 (cocos_proj_bwd_input_f16x3) folds everything in front of the input gradient into it and the weight
#: gradient rebuilds its dy on the fly (A/B runs)
PROJ_BWD_FUSED = os.environ.get("COCOS_PROJ_BWD_FUSED", "1") != "0"
#: False: theta's and phi's weight gradients run as two launches of cocos_proj1x1_dw_affine_f16x3 (A/B runs); True: one pair launch
PROJ_DW_PAIR = os.environ.get("COCOS_PROJ_DW_PAIR", "1") != "0"


class LazyProj1x1:
    """`conv1x1(x, weight, bias)` of the theta / phi projections (correspondence.py:272,:282), not computed yet.  The hot path asks
    for what its back end needs: `raw()` — the fp32 projection through K0 (computed once, cached) — or, on the fused
    match_kernel-1 / PONO_C path, nothing at all: `proj_center_l2norm_planes_pair` then produces the correlation kernels' operand
    planes straight from `x` (K23) and the projection never exists in HBM.  Quacks like the tensor it stands for where
    `correspondence_hot_path` looks (shape, is_cuda, dtype, requires_grad, detach)."""

    def __init__(self, x, weight, bias=None, prepared=None):
        if x.dim() != 4 or weight.shape[1] != x.shape[1]:
            raise ValueError(f"LazyProj1x1: weight {tuple(weight.shape)} does not match input {tuple(x.shape)}")
        self.x, self.weight, self.bias = x, weight, bias
        self.prepared = prepared      # the projection's frozen record (cocosnet_amd.inference), or None
        self._raw = None

    @property
    def shape(self):
        return torch.Size((self.x.shape[0], self.weight.shape[0], self.x.shape[2], self.x.shape[3]))

    is_cuda = property(lambda self: self.x.is_cuda)
    dtype = property(lambda self: self.x.dtype)
    device = property(lambda self: self.x.device)

    @property
    def requires_grad(self):
        return any(t is not None and t.requires_grad for t in (self.x, self.weight, self.bias))

    def detach(self):
        return LazyProj1x1(self.x.detach(), self.weight.detach(), None if self.bias is None else self.bias.detach(), self.prepared)

    def raw(self):
        if self._raw is None:
            self._raw = proj1x1(self.x, self.weight, self.bias, self.prepared)
        return self._raw


def _prepared_pair(theta: LazyProj1x1, phi: LazyProj1x1):
    """(theta's record, phi's record) when BOTH projections carry a frozen record, else None (the pair kernels prepare both or neither)."""
    a, b = getattr(theta, "prepared", None), getattr(phi, "prepared", None)
    return (a, b) if a is not None and b is not None else None


def proj_norm_fused_ok(p: LazyProj1x1) -> bool:
    """Shapes K23 takes: 256 output channels, whole 128-position tiles, fp32 on the GPU, the split flavour."""
    B, Cout, h, w = p.shape
    return (PROJ_NORM_FUSED and PROJ_PRECISION == "f16x3" and PRECISION == "f16x3" and p.is_cuda and p.dtype == torch.float32
            and Cout == FUSED_K and (h * w) % 128 == 0 and p.x.shape[1] <= 4096 and p.x.shape[1] * h * w * 4 < 2 ** 31 - 1)


class _ProjCenterL2NormPlanesPair(torch.autograd.Function):
    """K23 for the two projections of a forward call (theta, phi): ONE launch -> operand planes (handed to the caller's
    OperandPlanes) + row norms.  Outputs are HANDLES as in _CenterL2NormPlanes: [B,256,N] tensors whose memory is never written
    or read (the split correlation kernels read the planes); their gradients (d qn / d kn from K2's backward) come back here and
    go through K1's backward (cocos_center_l2norm_bwd_planes) and K0's (_proj1x1_backward)."""

    @staticmethod
    def forward(ctx, x1, w1, b1, x2, w2, b2, center_over_channels: int, eps: float, planes, want_chan: bool, prepared=None):
        lib = _lib.load()
        xs = [_chk(x1, "proj_center_l2norm_planes: x (theta)"), _chk(x2, "proj_center_l2norm_planes: x (phi)")]
        ws = [_chk(w1.reshape(w1.shape[0], -1), "proj_center_l2norm_planes: weight"),
              _chk(w2.reshape(w2.shape[0], -1), "proj_center_l2norm_planes: weight")]
        bs = [None if b is None else _chk(b, "proj_center_l2norm_planes: bias") for b in (b1, b2)]
        B, Cin, h, w = xs[0].shape
        N = h * w
        if xs[1].shape != xs[0].shape or ws[0].shape != (FUSED_K, Cin) or ws[1].shape != (FUSED_K, Cin):
            raise ValueError("proj_center_l2norm_planes_pair: the two projections must have the same shapes "
                             f"(x {tuple(xs[0].shape)} / {tuple(xs[1].shape)}, weights {tuple(ws[0].shape)} / {tuple(ws[1].shape)})")
        dev = xs[0].device
        half = dict(device=dev, dtype=torch.float16)
        args, keep, tplanes, tfrags = [], [], [], []
        # max|.| of the two feature tensors and the two weights: the ones no producer left behind (K21 leaves a spectral-normed
        # weight's, K13 / K9 epilogues the features') share ONE launch
        if prepared is None:
            amax = [_recall_amax(xs[0], consume=False), _recall_amax(ws[0]), _recall_amax(xs[1], consume=False), _recall_amax(ws[1])]
        else:      # frozen records (inference.py): the weights' cells are theirs
            amax = [_recall_amax(xs[0], consume=False), prepared[0].amax, _recall_amax(xs[1], consume=False), prepared[1].amax]
        missing = [i for i, c in enumerate(amax) if c is None]
        if missing:
            for i, c in zip(missing, absmax_many([(xs[0], ws[0], xs[1], ws[1])[i] for i in missing])):
                amax[i] = c
        # ... and so are the fragment-ordered planes, unless an input gradient wants the transposed layouts made with them
        frozen = prepared is not None and not ((ctx.needs_input_grad[0] or ctx.needs_input_grad[3]) and torch.is_grad_enabled())
        wprep = []
        for pi, (x, w2d, bb) in enumerate(zip(xs, ws, bs)):
            xa, wa = amax[2 * pi], amax[2 * pi + 1]
            if frozen:
                wfrag, _, wsc = prepared[pi].planes("frag")
            else:
                wfrag = torch.empty(lib.cocos_proj_weight_frag_bytes(Cin), device=dev, dtype=torch.uint8)
                wsc = torch.empty(1, device=dev, dtype=torch.float32)
            # ... and, when the input gradient will be wanted, the transposed planes [Cin][256] of dx = W^T dy in the same launch
            th = tl = None
            if ctx.needs_input_grad[3 * len(keep)] and not frozen:
                th, tl = torch.empty((Cin, FUSED_K), **half), torch.empty((Cin, FUSED_K), **half)
            tplanes.append((th, tl, wsc) if th is not None else None)
            # ... and W^T in K24's fragment order when the fused backward will run
            wtf = None
            if th is not None and PROJ_BWD_FUSED and lib.cocos_proj_bwd_input_supported(Cin, FUSED_K, N):
                wtf = torch.empty(lib.cocos_proj_weight_tfrag_bytes(), device=dev, dtype=torch.uint8)
            tfrags.append(wtf)
            wprep += [w2d.data_ptr(), wa.data_ptr(), wfrag.data_ptr(), wsc.data_ptr(), _ptr(th), _ptr(tl), _ptr(wtf)]
            norm = torch.empty((B, N), device=dev, dtype=torch.float32)
            ph, pl = torch.empty((B, N, FUSED_K), **half), torch.empty((B, N, FUSED_K), **half)
            ch = cl = None
            if want_chan:
                ch, cl = torch.empty((B, FUSED_K, N), **half), torch.empty((B, FUSED_K, N), **half)
            args += [x.data_ptr(), wfrag.data_ptr(), wsc.data_ptr(), _ptr(bb), xa.data_ptr(), norm.data_ptr(), ph.data_ptr(),
                     pl.data_ptr(), _ptr(ch), _ptr(cl)]
            keep.append((xa, wa, wfrag, wsc, norm, ph, pl, ch, cl))
        # every weight layout of both projections in one launch (they were four)
        if not frozen:
            _call("split_f16", "cocos_proj_weight_prep_pair", 2, *wprep, FUSED_K, Cin, _stream())
        _call("proj_center_l2norm_fwd", "cocos_proj_center_l2norm_planes_f16x3", 2, *args, B, Cin, N, int(center_over_channels),
              float(eps), SPLIT_OPERAND_SCALE, _stream())
        handles = []
        for (_xa, _wa, _wf, _ws, norm, ph, pl, ch, cl) in keep:
            hd = torch.empty((B, FUSED_K, N), device=dev, dtype=torch.float32)      # never written, never read: an autograd handle
            planes.put(hd, True, SPLIT_OPERAND_SCALE, ph, pl)
            if want_chan:
                planes.put(hd, False, SPLIT_OPERAND_SCALE, ch, cl)
            handles.append(hd)
        ctx.save_for_backward(xs[0], ws[0], xs[1], ws[1], keep[0][4], keep[1][4])
        ctx.chan = [(k[7], k[8]) for k in keep]
        ctx.amax = [(k[0], k[1]) for k in keep]
        ctx.t_planes = tplanes
        ctx.tfrags = tfrags
        ctx.pos = [(k[5], k[6]) for k in keep]          # position-major planes: K24 reads y back from them
        ctx.wsc = [k[3] for k in keep]
        ctx.cfg = (int(center_over_channels), float(eps))
        ctx.wshapes = (tuple(w1.shape), tuple(w2.shape))
        ctx.has_bias = (b1 is not None, b2 is not None)
        return handles[0], handles[1]

    @staticmethod
    def backward(ctx, d1, d2):
        x1, w1, x2, w2, n1, n2 = ctx.saved_tensors
        mode, eps = ctx.cfg
        needs = ctx.needs_input_grad[:10]
        if (d1 is not None and d2 is not None and needs[0] and needs[3] and all(t is not None for t in ctx.tfrags)
                and (needs[1] or not needs[2]) and (needs[4] or not needs[5])):
            # K24: K1's backward + the input gradient of BOTH projections in one launch; the weight gradients rebuild d on the fly
            d = [_chk(d1, "proj_center_l2norm_planes: d qn"), _chk(d2, "proj_center_l2norm_planes: d kn")]
            xs, w2s, norms = (x1, x2), (w1, w2), (n1, n2)
            B, K, N = d[0].shape
            Cin = x1.shape[1]
            dev = d[0].device
            dxs = [torch.empty_like(x1), torch.empty_like(x2)]
            coefs = [torch.empty((B, 3, N), device=dev, dtype=torch.float32) for _ in range(2)]
            cells = [_zero_cell(dev), _zero_cell(dev)]
            args = []
            for i in range(2):
                ph, pl = ctx.pos[i]
                args += [d[i].data_ptr(), ph.data_ptr(), pl.data_ptr(), norms[i].data_ptr(), None, ctx.tfrags[i].data_ptr(),
                         ctx.wsc[i].data_ptr(), dxs[i].data_ptr(), coefs[i].data_ptr(), cells[i].data_ptr()]
            _call("proj_bwd_input", "cocos_proj_bwd_input_f16x3", 0, 2, *args, B, Cin, N, mode, eps, SPLIT_OPERAND_SCALE, _stream())
            out = []
            nb = [needs[3 * i + 2] and ctx.has_bias[i] for i in range(2)]
            if needs[1] and needs[4] and nb[0] == nb[1] and PROJ_DW_PAIR:
                # both weight gradients in ONE launch (+ one reduction): half the partial tiles, the chip filled by the pair
                res = _proj1x1_dw_affine_pair(2, [(d[i], ctx.chan[i][0], ctx.chan[i][1], coefs[i], xs[i], cells[i], ctx.amax[i][0])
                                                  for i in range(2)], SPLIT_OPERAND_SCALE, nb[0])
                for i in range(2):
                    out += [dxs[i], res[i][0].reshape(ctx.wshapes[i]), res[i][1]]
                return (*out, None, None, None, None, None)
            for i in range(2):
                need_w, need_b = needs[3 * i + 1], nb[i]
                dw = db = None
                if need_w:
                    ch, cl = ctx.chan[i]
                    dw, db = _proj1x1_dw_affine(2, d[i], ch, cl, coefs[i], SPLIT_OPERAND_SCALE, xs[i], cells[i], ctx.amax[i][0], need_b)
                    dw = dw.reshape(ctx.wshapes[i])
                out += [dxs[i], dw, db]
            return (*out, None, None, None, None, None)
        out = []
        for i, (x, w2d, norm, dy) in enumerate(((x1, w1, n1, d1), (x2, w2, n2, d2))):
            need_x, need_w, need_b = ctx.needs_input_grad[3 * i:3 * i + 3]
            if dy is None or not (need_x or need_w or need_b):
                out += [None, None, None]
                continue
            ch, cl = ctx.chan[i]
            if ch is None:
                raise _lib.CocosHipError("proj_center_l2norm_planes: backward without the channel-major planes (forward ran without grad)")
            dy = _chk(dy, "proj_center_l2norm_planes: d qn")
            B, K, N = dy.shape
            dth = torch.empty((B, K, x.shape[2], x.shape[3]), device=dy.device, dtype=torch.float32)
            cell = _zero_cell(dy.device)
            _call("center_l2norm_bwd", "cocos_center_l2norm_bwd_planes", ch.data_ptr(), cl.data_ptr(), norm.data_ptr(),
                  dy.data_ptr(), dth.data_ptr(), B, K, N, mode, eps, SPLIT_OPERAND_SCALE, cell.data_ptr(), _stream())
            _remember_amax(dth, cell)
            lib = _lib.load()
            Cin = x.shape[1]
            stream = PROJ_STREAM and N % 64 == 0 and lib.cocos_proj1x1_stream_kpad(Cin) != 0 and lib.cocos_proj1x1_stream_kpad(K) != 0
            out += list(_proj1x1_backward(x, w2d, dth, ctx.amax[i], ctx.t_planes[i], True, stream, need_x, need_w,
                                          need_b and ctx.has_bias[i], ctx.wshapes[i]))
        return (*out, None, None, None, None, None)


def _proj1x1_dw_affine(mode, in1, in2a, in2b, coef, plane_scale, x, d_amax, x_amax, need_b):
    """(dw [Cout,Cin], db | None) of a 1x1 projection whose output gradient is alpha in1 + beta in2 + gamma (coef [B,3,N] from K24),
    rebuilt inside the weight-gradient kernel (cocos_proj1x1_dw_affine_f16x3).  in1 [B,Cout,N] fp32; mode 1: in2a fp32 [B,Cout,N];
    mode 2: in2a / in2b channel-major f16 planes."""
    lib = _lib.load()
    B, Cin = x.shape[:2]
    Cout, N = in1.shape[1], in1.shape[2]
    parts = lib.cocos_proj1x1_dw_partials_f16x3(B, Cin, Cout, N)
    if not parts:
        raise _lib.CocosHipError(f"proj1x1_dw_affine: shape not supported (Cin={Cin} Cout={Cout} N={N})")
    ws = torch.empty((parts, Cout, (Cin + 31) // 32 * 32), device=x.device, dtype=torch.float32)
    wsb = torch.empty((parts, Cout), device=x.device, dtype=torch.float32) if need_b else None
    dw = torch.empty((Cout, Cin), device=x.device, dtype=torch.float32)
    db = torch.empty(Cout, device=x.device, dtype=torch.float32) if need_b else None
    _call("proj1x1_bwd", "cocos_proj1x1_dw_affine_f16x3", mode, in1.data_ptr(), in2a.data_ptr(), _ptr(in2b), coef.data_ptr(),
          float(plane_scale), x.data_ptr(), ws.data_ptr(), _ptr(wsb), dw.data_ptr(), _ptr(db), B, Cin, Cout, N, d_amax.data_ptr(),
          x_amax.data_ptr(), _stream())
    return dw, db


def _proj1x1_dw_affine_pair(mode, probs, plane_scale, need_b, scale_cells=(None, None)):
    """_proj1x1_dw_affine for two projections of one shape in one launch: probs = [(in1, in2a, in2b, coef, x, d_amax, x_amax)] * 2
    -> [(dw, db | None)] * 2 (cocos_proj1x1_dw_affine_pair_f16x3)."""
    lib = _lib.load()
    x0 = probs[0][4]
    B, Cin = x0.shape[:2]
    Cout, N = probs[0][0].shape[1], probs[0][0].shape[2]
    parts = lib.cocos_proj1x1_dw_partials_pair_f16x3(B, Cin, Cout, N)
    if not parts or probs[1][4].shape != x0.shape:
        if any(c is not None for c in scale_cells):
            raise _lib.CocosHipError(f"proj1x1_dw_affine_pair: shape not supported (Cin={Cin} Cout={Cout} N={N})")
        return [_proj1x1_dw_affine(mode, in1, a, b, coef, plane_scale, x, da, xa, need_b) for (in1, a, b, coef, x, da, xa) in probs]
    res, args, hold = [], [], []
    f32 = dict(device=x0.device, dtype=torch.float32)
    for (in1, in2a, in2b, coef, x, d_amax, x_amax) in probs:
        ws = torch.empty((parts, Cout, (Cin + 31) // 32 * 32), **f32)
        wsb = torch.empty((parts, Cout), **f32) if need_b else None
        dw = torch.empty((Cout, Cin), **f32)
        db = torch.empty(Cout, **f32) if need_b else None
        res.append((dw, db))
        # the FIRST problem's partial tiles must outlive the loop: rebinding `ws` / `wsb` for the second problem handed their blocks back
        # to the allocator before the launch, and the second problem's 1 KB `db` was carved out of the first one's bias partials — the
        # reduction then read a partial row that the other half of the same launch was overwriting (caught by the full GPU suite only:
        # it takes an allocator state in which that block is the best fit)
        hold.append((ws, wsb))
        args += [in1.data_ptr(), in2a.data_ptr(), _ptr(in2b), coef.data_ptr(), x.data_ptr(), ws.data_ptr(), _ptr(wsb), dw.data_ptr(),
                 _ptr(db), d_amax.data_ptr(), x_amax.data_ptr()]
    _call("proj1x1_bwd", "cocos_proj1x1_dw_affine_pair_f16x3", mode, float(plane_scale), *args, _ptr(scale_cells[0]), _ptr(scale_cells[1]),
          B, Cin, Cout, N, _stream())
    del hold          # (released after the launch: stream order makes the reuse safe)
    return res


class _ProjUnfoldStats(torch.autograd.Function):
    """match_kernel 3 (round 6): theta_raw = conv1x1(x, w, b) AND the statistics (mu, a) of its 3x3-unfolded vectors (K0 + K12) as ONE
    autograd node, so that its backward sees both gradients of theta_raw at once — the one through the statistics (K12's
    backward: g1 + 2 theta_raw g2 per position) and the one from the correlation GEMMs — and folds K12's apply pass, autograd's
    addition and the max|.| pass into the projection's input gradient (K24 mode 1); the weight gradient rebuilds d on the fly."""

    @staticmethod
    def forward(ctx, x, weight, bias, k_unfolded: float, eps: float, prepared=None):
        lib = _lib.load()
        ctx.set_materialize_grads(False)      # (nrm is not differentiable: autograd would hand its backward a zero-filled [B,N] tensor per call)
        y, x, w2, st = _proj1x1_forward(x, weight, bias, ctx.needs_input_grad[0], prepared)
        B, C, h, w = y.shape
        N = h * w
        mk = lambda: torch.empty((B, N), device=y.device, dtype=torch.float32)
        mu, a, nrm = mk(), mk(), mk()
        ws = torch.empty(2 * B * N, device=y.device, dtype=torch.float32)
        cell = _zero_cell(y.device)          # max|theta_raw| as a by-product: the correlation GEMM of the fused family splits it next
        _call("unfold3_stats_fwd", "cocos_unfold3_stats_fwd_amax", y.data_ptr(), mu.data_ptr(), a.data_ptr(), nrm.data_ptr(),
              ws.data_ptr(), B, C, h, w, float(k_unfolded), float(eps), cell.data_ptr(), _stream())
        _remember_amax(y, cell)
        ctx.wtf = None
        if (ctx.needs_input_grad[0] and st["split"] and PROJ_BWD_FUSED and C == FUSED_K
                and lib.cocos_proj_bwd_input_supported(x.shape[1], C, N)):
            ctx.wtf = torch.empty(lib.cocos_proj_weight_tfrag_bytes(), device=y.device, dtype=torch.uint8)
            ctx.wtf_scale = torch.empty(1, device=y.device, dtype=torch.float32)
            _call("split_f16", "cocos_proj_weight_tfrag_planes", w2.data_ptr(), st["amax"][1].data_ptr(), ctx.wtf.data_ptr(),
                  ctx.wtf_scale.data_ptr(), C, x.shape[1], _stream())
        ctx.st = st
        ctx.kc = float(k_unfolded)
        ctx.save_for_backward(x, w2, y, mu, a, nrm)
        ctx.mark_non_differentiable(nrm)
        return y, mu, a, nrm

    @staticmethod
    def backward(ctx, dy, dmu, da, _dnrm):
        x, w2, y, mu, a, nrm = ctx.saved_tensors
        st = ctx.st
        B, C, h, w = y.shape
        N = h * w
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and st["has_bias"]
        dmu = None if dmu is None else _chk(dmu, "proj_unfold3_stats: dmu")
        da = None if da is None else _chk(da, "proj_unfold3_stats: da")
        if dy is not None and ctx.wtf is not None and need_x and (need_w or not need_b):
            dy = _chk(dy, "proj_unfold3_stats: d theta")
            maps = torch.empty(2 * B * N, device=y.device, dtype=torch.float32)
            _call("unfold3_stats_bwd", "cocos_unfold3_stats_bwd_maps", mu.data_ptr(), a.data_ptr(), nrm.data_ptr(), _ptr(dmu), _ptr(da),
                  maps.data_ptr(), B, h, w, ctx.kc, _stream())
            g1, g2 = maps[:B * N], maps[B * N:]
            dx = torch.empty_like(x)
            coef = torch.empty((B, 3, N), device=y.device, dtype=torch.float32)
            cell = _zero_cell(y.device)
            _call("proj_bwd_input", "cocos_proj_bwd_input_f16x3", 1, 1, dy.data_ptr(), y.data_ptr(), None, g1.data_ptr(), g2.data_ptr(),
                  ctx.wtf.data_ptr(), ctx.wtf_scale.data_ptr(), dx.data_ptr(), coef.data_ptr(), cell.data_ptr(),
                  None, None, None, None, None, None, None, None, None, None, B, x.shape[1], N, 1, 0.0, 1.0, _stream())
            dw = db = None
            if need_w:
                dw, db = _proj1x1_dw_affine(1, dy.reshape(B, C, N), y, None, coef, 1.0, x, cell, st["amax"][0], need_b)
                dw = dw.reshape(st["wshape"])
            return dx, dw, db, None, None, None
        # round 5's chain: K12's backward as a tensor, autograd-style addition, then the projection's backward
        dth = torch.empty_like(y)
        ws = torch.empty(2 * B * N, device=y.device, dtype=torch.float32)
        _call("unfold3_stats_bwd", "cocos_unfold3_stats_bwd", y.data_ptr(), mu.data_ptr(), a.data_ptr(), nrm.data_ptr(),
              _ptr(dmu), _ptr(da), dth.data_ptr(), ws.data_ptr(), B, C, h, w, ctx.kc, _stream())
        if dy is not None:
            dth = dth + dy
        return (*_proj1x1_backward(x, w2, dth, st["amax"], st["t_planes"], st["split"], st["stream"], need_x, need_w, need_b,
                                   st["wshape"]), None, None, None)


#: False: match_kernel 3 projects with K0 and takes the statistics / operand planes in separate launches (A/B runs)
PROJ_RAW_FUSED = os.environ.get("COCOS_PROJ_RAW_FUSED", "1") != "0"


class Box3RawPlanes:
    """What K25 leaves for the match_kernel-3 family about theta and phi, keyed by the autograd HANDLE that stands for each raw
    projection: (position-major hi, lo, channel-major hi | None, lo | None, scale cell).  Owned by hot_path's _BoxedCorr: one
    forward call, one thread."""

    def __init__(self):
        self._ent = {}

    def put(self, handle, ph, pl, ch, cl, scale):
        self._ent[id(handle)] = (handle, handle._version, ph, pl, ch, cl, scale)

    def get(self, handle):
        ent = self._ent.get(id(handle))
        if ent is None or ent[0] is not handle:
            return None
        if ent[1] != handle._version:
            raise _lib.CocosHipError("Box3RawPlanes: the tensor behind producer-made operand planes was modified in place")
        return ent[2:]


def proj_raw_fused_ok(theta: LazyProj1x1, phi: LazyProj1x1) -> bool:
    """Shapes / gradient patterns K25 and its backward take: both projections 256 channels from <= 448 of one shape, whole
    128-position tiles, and either nothing or everything (features, weights) differentiated."""
    if not (PROJ_RAW_FUSED and PROJ_BWD_FUSED and PROJ_PRECISION == "f16x3" and PRECISION == "f16x3"):
        return False
    B, Cout, h, w = theta.shape
    N = h * w
    if not (theta.is_cuda and theta.dtype == torch.float32 and theta.x.shape == phi.x.shape and phi.shape == theta.shape
            and Cout == FUSED_K and N % 128 == 0 and _lib.load().cocos_proj_bwd_input_supported(theta.x.shape[1], FUSED_K, N)
            and theta.x.shape[1] * N * 4 < 2 ** 31 - 1 and phi.is_cuda and phi.dtype == torch.float32):
        return False
    if not torch.is_grad_enabled():
        return True
    req = [t.requires_grad for t in (theta.x, theta.weight, phi.x, phi.weight)]
    return all(req) or not (any(req) or any(b is not None and b.requires_grad for b in (theta.bias, phi.bias)))


class _ProjRawPlanesStatsPair(torch.autograd.Function):
    """K25 for the two projections of a match_kernel-3 forward call: ONE launch from the features to the operand planes of the raw
    theta / phi (position-major for the x-box GEMM, channel-major for the backward GEMMs and the weight gradient) and to the
    per-position sums K12's statistics are box sums of; one more launch finishes (mu, a) / (nu, b).  Outputs: two HANDLES
    [B,256,h,w] (never written, never read: _Box3CorrXbox takes the planes from `holder`) and the statistics.  Backward: the
    handles' gradients (the correlation GEMMs') and the statistics' (K19's) meet here — K12's maps for both tensors (one launch),
    K24 mode C for both input gradients (one launch), both weight gradients (one launch + one reduction)."""

    @staticmethod
    def forward(ctx, x1, w1, b1, x2, w2, b2, k_unfolded: float, eps: float, holder, prepared=None):
        lib = _lib.load()
        ctx.set_materialize_grads(False)
        xs = [_chk(x1, "proj_raw_planes_stats: x (theta)"), _chk(x2, "proj_raw_planes_stats: x (phi)")]
        ws = [_chk(w1.reshape(w1.shape[0], -1), "proj_raw_planes_stats: weight"), _chk(w2.reshape(w2.shape[0], -1), "proj_raw_planes_stats: weight")]
        bs = [None if b is None else _chk(b, "proj_raw_planes_stats: bias") for b in (b1, b2)]
        B, Cin, h, w = xs[0].shape
        N = h * w
        dev = xs[0].device
        half, f32 = dict(device=dev, dtype=torch.float16), dict(device=dev, dtype=torch.float32)
        want_grad = any(ctx.needs_input_grad[:6])
        if prepared is None:
            amax = [_recall_amax(xs[0], consume=False), _recall_amax(ws[0]), _recall_amax(xs[1], consume=False), _recall_amax(ws[1])]
        else:      # frozen records (inference.py): the weights' cells and, without a backward, their fragment-ordered planes
            amax = [_recall_amax(xs[0], consume=False), prepared[0].amax, _recall_amax(xs[1], consume=False), prepared[1].amax]
        # (needs_input_grad mirrors requires_grad even under no_grad: a backward can only follow with gradients enabled)
        frozen = prepared is not None and not (want_grad and torch.is_grad_enabled())
        missing = [i for i, c in enumerate(amax) if c is None]
        if missing:
            for i, c in zip(missing, absmax_many([(xs[0], ws[0], xs[1], ws[1])[i] for i in missing])):
                amax[i] = c
        wprep, args, keep = [], [], []
        for pi in range(2):
            if frozen:
                wfrag, _, wsc = prepared[pi].planes("frag")
            else:
                wfrag = torch.empty(lib.cocos_proj_weight_frag_bytes(Cin), device=dev, dtype=torch.uint8)
                wsc = torch.empty(1, **f32)
            wtf = torch.empty(lib.cocos_proj_weight_tfrag_bytes(), device=dev, dtype=torch.uint8) if want_grad and not frozen else None
            wprep += [ws[pi].data_ptr(), amax[2 * pi + 1].data_ptr(), wfrag.data_ptr(), wsc.data_ptr(), None, None, _ptr(wtf)]
            sums = torch.empty((2, B, N), **f32)
            ysc = torch.empty(1, **f32)
            ph, pl = torch.empty((B, N, FUSED_K), **half), torch.empty((B, N, FUSED_K), **half)
            ch = cl = None
            if want_grad:
                ch, cl = torch.empty((B, FUSED_K, N), **half), torch.empty((B, FUSED_K, N), **half)
            args += [xs[pi].data_ptr(), wfrag.data_ptr(), wsc.data_ptr(), _ptr(bs[pi]), amax[2 * pi].data_ptr(), sums[0].data_ptr(),
                     sums[1].data_ptr(), ysc.data_ptr(), ph.data_ptr(), pl.data_ptr(), _ptr(ch), _ptr(cl)]
            keep.append((wfrag, wsc, wtf, sums, ysc, ph, pl, ch, cl))
        if not frozen:
            _call("split_f16", "cocos_proj_weight_prep_pair", 2, *wprep, FUSED_K, Cin, _stream())
        _call("proj1x1_fwd", "cocos_proj_raw_planes_stats_f16x3", 2, *args, B, Cin, N, _stream())
        stats = [tuple(torch.empty((B, N), **f32) for _ in range(3)) for _ in range(2)]      # (mu, a, nrm) per tensor
        fa = []
        for pi in range(2):
            fa += [keep[pi][3][0].data_ptr(), keep[pi][3][1].data_ptr()] + [t.data_ptr() for t in stats[pi]]
        _call("unfold3_stats_fwd", "cocos_unfold3_stats_finish_pair", *fa, B, h, w, float(k_unfolded), float(eps), _stream())
        handles = []
        for pi in range(2):
            hd = torch.empty((B, FUSED_K, h, w), **f32)      # never written, never read: an autograd handle
            (_wf, _ws, _wt, _s, ysc, ph, pl, ch, cl) = keep[pi]
            holder.put(hd, ph, pl, ch, cl, ysc)
            handles.append(hd)
        ctx.save_for_backward(xs[0], ws[0], xs[1], ws[1], *stats[0], *stats[1])
        ctx.keep = keep
        ctx.x_amax = (amax[0], amax[2])
        ctx.kc = float(k_unfolded)
        ctx.dims = (B, Cin, h, w)
        ctx.wshapes = (tuple(w1.shape), tuple(w2.shape))
        ctx.has_bias = (b1 is not None, b2 is not None)
        ctx.mark_non_differentiable(stats[0][2], stats[1][2])
        return handles[0], stats[0][0], stats[0][1], handles[1], stats[1][0], stats[1][1], stats[0][2], stats[1][2]

    @staticmethod
    def backward(ctx, d1, dmu1, da1, d2, dmu2, da2, _n1, _n2):
        x1, w1, x2, w2, mu1, a1, nrm1, mu2, a2, nrm2 = ctx.saved_tensors
        B, Cin, h, w = ctx.dims
        N = h * w
        dev = x1.device
        f32 = dict(device=dev, dtype=torch.float32)
        needs = ctx.needs_input_grad
        if not (needs[0] and needs[1] and needs[3] and needs[4]):
            raise _lib.CocosHipError("proj_raw_planes_stats: backward needs the gradients of both feature tensors and both weights "
                                     "(proj_raw_fused_ok gates the forward)")
        ds = []
        for d in (d1, d2):      # (a projection whose correlation gradient is absent: only the statistics' path contributes)
            ds.append(torch.zeros((B, FUSED_K, N), **f32) if d is None else _chk(d, "proj_raw_planes_stats: d theta").reshape(B, FUSED_K, N))
        stats = ((mu1, a1, nrm1, dmu1, da1), (mu2, a2, nrm2, dmu2, da2))
        maps = [torch.empty(2 * B * N, **f32) for _ in range(2)]
        ma = []
        for pi in range(2):
            mu, a, nrm, dmu, da = stats[pi]
            ma += [mu.data_ptr(), a.data_ptr(), nrm.data_ptr(), _ptr(None if dmu is None else _chk(dmu, "dmu")),
                   _ptr(None if da is None else _chk(da, "da")), maps[pi].data_ptr()]
        _call("unfold3_stats_bwd", "cocos_unfold3_stats_bwd_maps_pair", *ma, B, h, w, ctx.kc, _stream())
        xs, dxs = (x1, x2), [torch.empty_like(x1), torch.empty_like(x2)]
        coefs = [torch.empty((B, 3, N), **f32) for _ in range(2)]
        cells = [_zero_cell(dev), _zero_cell(dev)]
        args = []
        for pi in range(2):
            (_wf, wsc, wtf, _s, ysc, ph, pl, _ch, _cl) = ctx.keep[pi]
            g1, g2 = maps[pi][:B * N], maps[pi][B * N:]
            args += [ds[pi].data_ptr(), ph.data_ptr(), pl.data_ptr(), ysc.data_ptr(), g1.data_ptr(), g2.data_ptr(), wtf.data_ptr(),
                     wsc.data_ptr(), dxs[pi].data_ptr(), coefs[pi].data_ptr(), cells[pi].data_ptr()]
        _call("proj_bwd_input", "cocos_proj_bwd_input_planes_f16x3", 2, *args, B, Cin, N, _stream())
        nb = [needs[2] and ctx.has_bias[0], needs[5] and ctx.has_bias[1]]
        probs = [(ds[pi], ctx.keep[pi][7], ctx.keep[pi][8], coefs[pi], xs[pi], cells[pi], ctx.x_amax[pi]) for pi in range(2)]
        scale_cells = (ctx.keep[0][4], ctx.keep[1][4])
        if nb[0] == nb[1]:
            res = _proj1x1_dw_affine_pair(2, probs, 1.0, nb[0], scale_cells)
        else:       # (a bias on one projection only: two pair-API launches of one problem each would need another entry point — both
            #  biases' gradients are computed and the unwanted one dropped)
            res = _proj1x1_dw_affine_pair(2, probs, 1.0, True, scale_cells)
            res = [(res[pi][0], res[pi][1] if nb[pi] else None) for pi in range(2)]
        return (dxs[0], res[0][0].reshape(ctx.wshapes[0]), res[0][1], dxs[1], res[1][0].reshape(ctx.wshapes[1]), res[1][1], None, None, None, None)


def proj_raw_planes_stats_pair(theta: LazyProj1x1, phi: LazyProj1x1, k_unfolded: float, holder: Box3RawPlanes, eps: float = NORM_EPS):
    """((theta handle, mu, a), (phi handle, nu, b)) of two lazy projections through K25: see _ProjRawPlanesStatsPair.  The handles go
    to box3_corr_xbox(..., raw_planes=holder).  Only for proj_raw_fused_ok() pairs."""
    th, mu, a, ph, nu, b, _, _ = _ProjRawPlanesStatsPair.apply(theta.x, theta.weight, theta.bias, phi.x, phi.weight, phi.bias,
                                                               float(k_unfolded), eps, holder, _prepared_pair(theta, phi))
    return (th, mu, a), (ph, nu, b)


def proj_unfold3_stats(p: LazyProj1x1, k_unfolded: float, eps: float = NORM_EPS):
    """(theta_raw [B,C,h,w], mu, a [B,h*w]) of a lazy projection: K0 + K12 as one autograd node (see _ProjUnfoldStats)."""
    y, mu, a, _ = _ProjUnfoldStats.apply(p.x, p.weight, p.bias, float(k_unfolded), eps, p.prepared)
    return y, mu, a


def proj_center_l2norm_planes_pair(theta: LazyProj1x1, phi: LazyProj1x1, center_over_channels, planes: OperandPlanes,
                                   eps: float = NORM_EPS, want_chan: bool = True):
    """(qn handle, kn handle) of the two lazy projections through K23: see _ProjCenterL2NormPlanesPair.  Pass the handles to
    corr_softmax_warp(..., planes=planes).  Only for proj_norm_fused_ok() shapes on the split path (corr_split_ok)."""
    return _ProjCenterL2NormPlanesPair.apply(theta.x, theta.weight, theta.bias, phi.x, phi.weight, phi.bias,
                                             int(center_over_channels), eps, planes, bool(want_chan), _prepared_pair(theta, phi))


def proj_center_l2norm_planes_one(p: LazyProj1x1, center_over_channels, eps: float = NORM_EPS):
    """K23 for ONE lazy projection, forward only (inference with a prepared exemplar: theta alone per call, phi alone when the
    record is made): (pos_hi, pos_lo [B,N,256], norm [B,N]).  The same kernel as the pair's, launched with one problem
    (cocos_proj_center_l2norm_planes_f16x3, nprob = 1).  Only for proj_norm_fused_ok() shapes; no autograd node."""
    lib = _lib.load()
    with torch.no_grad():
        x = _chk(p.x, "proj_center_l2norm_planes: x")
        w2d = _chk(p.weight.reshape(p.weight.shape[0], -1), "proj_center_l2norm_planes: weight")
        bias = None if p.bias is None else _chk(p.bias, "proj_center_l2norm_planes: bias")
        B, Cin, h, w = x.shape
        N = h * w
        if w2d.shape != (FUSED_K, Cin):
            raise ValueError(f"proj_center_l2norm_planes_one: weight {tuple(w2d.shape)} does not match x {tuple(x.shape)}")
        dev = x.device
        xa = absmax(x)      # (its own pass: the version-keyed max|x| table is the training routes')
        if p.prepared is not None:      # frozen record (inference.py): its cell and its fragment-ordered planes
            wfrag, _, wsc = p.prepared.planes("frag")
        else:
            wa = absmax(w2d)
            wfrag = torch.empty(lib.cocos_proj_weight_frag_bytes(Cin), device=dev, dtype=torch.uint8)
            wsc = torch.empty(1, device=dev, dtype=torch.float32)
            _call("split_f16", "cocos_proj_weight_prep_pair", 1, w2d.data_ptr(), wa.data_ptr(), wfrag.data_ptr(), wsc.data_ptr(),
                  None, None, None, None, None, None, None, None, None, None, FUSED_K, Cin, _stream())
        norm = torch.empty((B, N), device=dev, dtype=torch.float32)
        ph = torch.empty((B, N, FUSED_K), device=dev, dtype=torch.float16)
        pl = torch.empty((B, N, FUSED_K), device=dev, dtype=torch.float16)
        _call("proj_center_l2norm_fwd", "cocos_proj_center_l2norm_planes_f16x3", 1, x.data_ptr(), wfrag.data_ptr(), wsc.data_ptr(),
              _ptr(bias), xa.data_ptr(), norm.data_ptr(), ph.data_ptr(), pl.data_ptr(), None, None,
              None, None, None, None, None, None, None, None, None, None, B, Cin, N, int(center_over_channels), float(eps),
              SPLIT_OPERAND_SCALE, _stream())
    return ph, pl, norm


# ------------------------------------------------------------------------------------------
# K16  nn.Conv2d (groups 1, dilation 1, zero padding) as a split-precision implicit GEMM   (conv_f16x3.hip)
#      ResidualBlock (correspondence.py:13-36), adaptor convolutions (:150-173), PatchGAN (discriminator.py:92-115)
# ------------------------------------------------------------------------------------------
#: K16's arithmetic: "f16x3" = f16 hi/lo split, three MFMA terms (fp32-class accuracy: everything upstream of the correlation);
#: "bf16" = single bf16 planes, one MFMA term (BASELINE config 3's precision for the generator / discriminator stacks behind
#: InstanceNorm / SPADE — ~3x less matrix work, no max|x| passes).  Module attribute, read at call time.
#: "torch" (A/B runs): producers.Conv2d / ReflectionPad2d / the spectral-norm hook keep the framework's kernels; a DIRECT
#: ops.conv2d call is an error in that setting.  This is the only copy of the switch (producers.conv_backend() reads it).
CONV_PRECISION = os.environ.get("COCOS_CONV", "f16x3")


def _conv_bf16() -> bool:
    if CONV_PRECISION == "torch":
        raise ValueError("cocosnet_amd.ops.conv2d called with CONV_PRECISION = 'torch': that setting routes the producers' "
                         "convolutions to the framework (producers.Conv2d); the HIP entry point needs 'f16x3' or 'bf16'")
    if CONV_PRECISION not in ("f16x3", "bf16"):
        raise ValueError(f"cocosnet_amd.ops.CONV_PRECISION = {CONV_PRECISION!r}: expected 'f16x3', 'bf16' or 'torch'")
    return CONV_PRECISION == "bf16"


def _conv_weight_planes(weight, amax, mode: int, JH=None, JW=None, ry=0, rx=0, s=1):
    """weight [Cout,Cin,KH,KW] -> K16's f16 hi/lo planes in ONE launch (cocos_conv2d_weight_planes): mode 0 = forward,
    mode 1 = input gradient (flipped (sub-)kernel w[:, :, ry::s, rx::s], channel roles swapped)."""
    Cout, Cin, KH, KW = weight.shape
    JH, JW = (KH if JH is None else JH), (KW if JW is None else JW)
    M, C = (Cout, Cin) if mode == 0 else (Cin, Cout)
    nkb = JH * JW * ((C + 31) // 32)
    wh = torch.empty((nkb, M, 32), device=weight.device, dtype=torch.float16)
    if amax is None:          # one bf16 plane (the bits live in an f16-typed tensor), no scale
        _call("split_f16", "cocos_conv2d_weight_planes", weight.data_ptr(), wh.data_ptr(), None, Cout, Cin, KH, KW, mode | 2,
              JH, JW, ry, rx, s, None, None, _stream())
        return wh, None, None
    wl = torch.empty_like(wh)
    ws = torch.empty(1, device=weight.device, dtype=torch.float32)
    _call("split_f16", "cocos_conv2d_weight_planes", weight.data_ptr(), wh.data_ptr(), wl.data_ptr(), Cout, Cin, KH, KW, mode,
          JH, JW, ry, rx, s, amax.data_ptr(), ws.data_ptr(), _stream())
    return wh, wl, ws


def _conv_fwd_call(x, wh, wl, ws, xa, bias, Cout, KH, KW, stride, pad, dil):
    B, Cin, H, W = x.shape
    lib = _lib.load()
    OH, OW = lib.cocos_conv2d_out_size(H, KH, stride, pad, dil), lib.cocos_conv2d_out_size(W, KW, stride, pad, dil)
    if OH < 1 or OW < 1:
        raise ValueError(f"conv2d: kernel {KH}x{KW} (dilation {dil}) does not fit input {tuple(x.shape)} with padding {pad}")
    y = torch.empty((B, Cout, OH, OW), device=x.device, dtype=torch.float32)
    _call("conv2d_fwd", "cocos_conv2d_fwd_f16x3", x.data_ptr(), wh.data_ptr(), _ptr(wl), _ptr(ws),
          _ptr(xa), _ptr(bias), y.data_ptr(), B, Cin, H, W, Cout, KH, KW, stride, pad, dil, _stream())
    return y


#: "0": COCOS_CONV=bf16 keeps every layer on conv_f16x3.hip's one-term kernels (fp32 NCHW operands gathered per tap) — A/B runs
CONV_NHWC = True


def _conv_nhwc_ok(Cin, Cout, KH, KW, stride):
    return CONV_NHWC and bool(_lib.load().cocos_conv2d_nhwc_bf16_supported(Cin, Cout, KH, KW, stride))


#: "0": the fp32-accurate flavour keeps every layer on conv_f16x3.hip's gather kernels (A/B runs); default: K16c, the same
#: arithmetic on K16b's data path (f16 hi/lo planes NHWC in memory, LDS-DMA GEMMs)
CONV_NHWC_F16X3 = True


def conv_nhwc_prep_split(x: torch.Tensor, pad: int, reflect: bool, amax: torch.Tensor) -> torch.Tensor:
    """fp32 [B,C,H,W] -> f16 [2,B,H+2p,W+2p,Cp]: hi and lo plane of x * 2^k (k from the max|x| cell `amax`), NHWC, border zero or
    mirrored: the operand of K16c (cocos_conv2d_nhwc_prep_f16x3)."""
    x = _chk(x, "conv_nhwc_prep_split: x")
    B, C, H, W = x.shape
    xp = torch.empty((2, B, H + 2 * pad, W + 2 * pad, (C + 31) // 32 * 32), device=x.device, dtype=torch.float16)
    _call("conv2d_nhwc_prep", "cocos_conv2d_nhwc_prep_f16x3", x.data_ptr(), xp.data_ptr(), _ptr(amax), B, C, H, W, int(pad),
          int(bool(reflect)), _stream())
    return xp


def _nhwc_out(xp_shape, Cout, KH, KW, dil, stride, fold, device):
    """Output (and, in fold mode, the border ring) of a K16b / K16c GEMM: fold = the layer sits behind nn.ReflectionPad2d(1) and this
    is its input gradient — y is the UNPADDED dx, the mirrored border comes back through the ring."""
    B, Hp, Wp = xp_shape[-4], xp_shape[-3], xp_shape[-2]
    if Hp <= dil * (KH - 1) or Wp <= dil * (KW - 1):
        raise ValueError(f"conv2d: kernel {KH}x{KW} (dilation {dil}) does not fit the padded input {tuple(xp_shape)}")
    OH, OW = (Hp - dil * (KH - 1) - 1) // stride + 1, (Wp - dil * (KW - 1) - 1) // stride + 1
    if not fold:
        return torch.empty((B, Cout, OH, OW), device=device, dtype=torch.float32), None
    return (torch.empty((B, Cout, OH - 2, OW - 2), device=device, dtype=torch.float32),
            torch.empty((B, Cout, 2 * OW + 2 * (OH - 2)), device=device, dtype=torch.float32))


def _conv_nhwc_split_call(xp, wh, wl, ws, xa, bias, Cout, KH, KW, dil, stride=1, fold=False):
    _, B, Hp, Wp, Cp = xp.shape
    y, ring = _nhwc_out(xp.shape, Cout, KH, KW, dil, stride, fold, xp.device)
    wsp = _conv_nhwc_workspace(xp.device, split=True)
    _call("conv2d_fwd", "cocos_conv2d_nhwc_f16x3", xp.data_ptr(), wh.data_ptr(), wl.data_ptr(), ws.data_ptr(), _ptr(xa), _ptr(bias),
          y.data_ptr(), _ptr(ring), _ptr(wsp), wsp.numel() * 4 if wsp is not None else 0, B, Cp, Hp, Wp, Cout, KH, KW, dil, int(stride),
          _stream())
    return y


def conv_nhwc_prep(x: torch.Tensor, pad: int, reflect: bool = False) -> torch.Tensor:
    """fp32 [B,C,H,W] -> bf16 [B,H+2p,W+2p,Cp] (channels padded to 32, border zero or mirrored): the operand layout of K16b
    (cocos_conv2d_nhwc_prep_bf16)."""
    x = _chk(x, "conv_nhwc_prep: x")
    B, C, H, W = x.shape
    xp = torch.empty((B, H + 2 * pad, W + 2 * pad, (C + 31) // 32 * 32), device=x.device, dtype=torch.bfloat16)
    _call("conv2d_nhwc_prep", "cocos_conv2d_nhwc_prep_bf16", x.data_ptr(), xp.data_ptr(), B, C, H, W, int(pad), int(bool(reflect)),
          _stream())
    return xp


#: "1": stream-K launches for K16b layers whose tile count is just above a whole round of the CUs.  Off by default: once the
#: DMA pieces were interleaved with the MFMAs a tile got 20 % faster and the parked partials (nearly every tile is cut: 128 MB)
#: cost what the second round costs (407 -> 407 input gradient 0.191 vs 0.192 ms, 512 -> 512 0.224 vs 0.239).
CONV_NHWC_STREAMK = False
#: the three-term flavour (K16c) is the other way round: a tile takes 3x as long, the parked partials cost the same — stream-K on
#: (407 -> 407 input gradient on 66 x 66: two rounds of 0.3 ms against 1.07 rounds + 0.04 ms)
CONV_NHWC_STREAMK_SPLIT = True


def _conv_nhwc_workspace(device, split=False):
    """K16b / K16c's stream-K scratch: one zero-initialised buffer per (thread, device, stream), cleared when it is allocated (the
    kernel leaves its flags zero)."""
    if not (CONV_NHWC_STREAMK_SPLIT if split else CONV_NHWC_STREAMK):
        return None
    pool = getattr(_tls, "nhwc_ws", None)
    if pool is None:
        pool = _tls.nhwc_ws = {}
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream())
    ws = pool.get(key)
    if ws is None:
        ws = pool[key] = torch.zeros(_lib.load().cocos_conv2d_nhwc_bf16_workspace_bytes() // 4, device=device, dtype=torch.int32)
    return ws


def _conv_nhwc_call(xp, planes, bias, Cout, KH, KW, dil, stride=1, fold=False):
    B, Hp, Wp, Cp = xp.shape
    y, ring = _nhwc_out(xp.shape, Cout, KH, KW, dil, stride, fold, xp.device)
    ws = _conv_nhwc_workspace(xp.device)
    _call("conv2d_fwd", "cocos_conv2d_nhwc_bf16", xp.data_ptr(), planes.data_ptr(), _ptr(bias), y.data_ptr(), _ptr(ring), _ptr(ws),
          ws.numel() * 4 if ws is not None else 0, B, Cp, Hp, Wp, Cout, KH, KW, dil, int(stride), _stream())
    return y


def _conv_dgrad_strided(xshape, weight, dy, ga, wa, s: int, p: int):
    """Input gradient of a stride-s convolution (dilation 1) as s*s stride-1 convolutions of dy.
    dx[y, x] only sees the taps with ky = (y + p) mod s (mod s): with y + p = s*u + ry and ky = ry + s*jy,
        dx[s*u + ry - p, s*v + rx - p] = sum_{co, jy, jx} w[co, ci, ry + s*jy, rx + s*jx] * dy[co, u - jy, v - jx],
    a correlation of dy with the flipped sub-kernel, evaluated for the u, v whose pixel lies inside the input and written
    straight into dx with stride s (cocos_conv2d_fwd_scatter_f16x3).  Returns None when a class needs negative padding."""
    B, Cin, H, W = xshape
    Cout, _, KH, KW = weight.shape
    OH, OW = dy.shape[2:]
    classes = []
    for ry in range(s):
        JH = len(range(ry, KH, s))
        u0 = max(0, -((ry - p) // s))                      # ceil((p - ry) / s), first u with s*u + ry - p >= 0
        U = (H - 1 + p - ry) // s + 1 - u0 if H - 1 + p - ry >= 0 else 0
        for rx in range(s):
            JW = len(range(rx, KW, s))
            v0 = max(0, -((rx - p) // s))
            V = (W - 1 + p - rx) // s + 1 - v0 if W - 1 + p - rx >= 0 else 0
            if U <= 0 or V <= 0:
                continue
            if JH == 0 or JW == 0:
                classes.append(None)                         # pixels no tap reaches: zeros
                continue
            py, px = JH - 1 - u0, JW - 1 - v0
            if py < 0 or px < 0:
                return None
            classes.append((ry, rx, JH, JW, u0, v0, U, V, py, px))
    dx = (torch.zeros if any(c is None for c in classes) else torch.empty)(xshape, device=dy.device, dtype=torch.float32)
    for c in classes:
        if c is None:
            continue
        ry, rx, JH, JW, u0, v0, U, V, py, px = c
        th, tl, ts = _conv_weight_planes(weight, wa, 1, JH, JW, ry, rx, s)
        off = (s * u0 + ry - p) * W + (s * v0 + rx - p)
        _call("conv2d_fwd", "cocos_conv2d_fwd_scatter_f16x3", dy.data_ptr(), th.data_ptr(), _ptr(tl), _ptr(ts),
              _ptr(ga), dx.data_ptr(), B, Cout, OH, OW, Cin, JH, JW, py, px, U, V, H * W, s * W, s, off, _stream())
    return dx


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride: int, pad: int, dil: int, reflect: int = 0, prepared=None):
        x = _chk(x, "conv2d: x")
        weight = _chk(weight, "conv2d: weight")
        if x.dim() != 4 or weight.dim() != 4 or weight.shape[1] != x.shape[1]:
            raise ValueError(f"conv2d: weight {tuple(weight.shape)} does not match input {tuple(x.shape)}")
        if stride < 1 or pad < 0 or dil < 1:
            raise ValueError(f"conv2d: stride {stride} / padding {pad} / dilation {dil}")
        Cout, Cin, KH, KW = weight.shape
        bb = None if bias is None else _chk(bias, "conv2d: bias")
        if _conv_bf16():          # one-term flavour: no max|x| passes at all
            xa = wa = None
        else:
            xa = _recall_amax(x, consume=False)      # (not consumed: SPADE's gamma and beta convolutions read the SAME activation)
            if xa is None:
                xa = absmax(x)
                _remember_amax(x, xa, weak=True)     # ... and the second one finds what the first one measured
            if prepared is not None:           # the layer's frozen record (inference.py): its cell, its planes
                wa = prepared.amax
            else:
                wa = _recall_amax(weight)          # K21 leaves it for spectral-normed layers
                if wa is None:
                    wa = absmax(weight)
        if prepared is not None:
            wh, wl, ws = prepared.planes("conv_fwd" if wa is not None else "conv_fwd_bf16")
        else:
            wh, wl, ws = _conv_weight_planes(weight, wa, 0)
        xp = None
        if wa is not None and CONV_NHWC_F16X3 and _conv_nhwc_ok(Cin, Cout, KH, KW, stride):
            # K16c: the split arithmetic on K16b's data path — hi/lo planes NHWC in memory, LDS-DMA GEMM, three terms
            xp = conv_nhwc_prep_split(x, reflect if reflect else pad, bool(reflect), xa)
            y = _conv_nhwc_split_call(xp, wh, wl, ws, xa, bb, Cout, KH, KW, dil, stride)
            if y.shape[3] % 32 != 0:
                xp = None
        elif wa is None and _conv_nhwc_ok(Cin, Cout, KH, KW, stride):
            # K16b: operands bf16 in memory (NHWC, border included), LDS-DMA GEMM — conv_nhwc_bf16.hip
            xp = conv_nhwc_prep(x, reflect if reflect else pad, bool(reflect))    # the border: zeros, or the layer's ReflectionPad2d
            y = _conv_nhwc_call(xp, wh, bb, Cout, KH, KW, dil, stride)
            if y.shape[3] % 32 != 0:
                xp = None               # its weight gradient takes whole rows of 32 positions: this layer's stays on K16
        else:
            y = _conv_fwd_call(x, wh, wl, ws, xa, bb, Cout, KH, KW, stride, pad, dil)
        if reflect and xp is None:
            raise _lib.CocosHipError("conv2d: reflect padding is only fused on the K16b path (ops.conv2d checks the shape first)")
        keep_xp = xp is not None and (ctx.needs_input_grad[1] or reflect)
        ctx.save_for_backward(weight, *((xp,) if keep_xp else (x,)))
        ctx.x_shape, ctx.has_xp, ctx.reflect = tuple(x.shape), keep_xp, int(reflect)
        ctx.cfg = (int(stride), int(pad), int(dil), bias is not None)
        ctx.amax = (xa, wa)
        # the input-gradient planes come from the record only where freeze() asked for them (the fixed VGG of a training step)
        ctx.prepared = prepared if prepared is not None and prepared.keep_dgrad else None
        return y

    @staticmethod
    def backward(ctx, dy):
        weight, saved = ctx.saved_tensors
        x, xp = (None, saved) if ctx.has_xp else (saved, None)
        stride, pad, dil, has_bias = ctx.cfg
        xa, wa = ctx.amax
        dy = _chk(dy, "conv2d: dy")
        B, Cin, H, W = ctx.x_shape
        reflect = ctx.reflect
        if reflect:                 # the layer the kernels see: pad 0 on the mirrored (H + 2r) x (W + 2r) input
            H, W = H + 2 * reflect, W + 2 * reflect
        Cout, _, KH, KW = weight.shape
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dx = dw = db = None
        bf = wa is None           # the flavour the forward ran
        ga = None
        if not bf:
            ga = _recall_amax(dy)
            if ga is None:
                ga = absmax(dy)
        q = dil * (KH - 1) - pad
        nhwc = bf or CONV_NHWC_F16X3
        dx_nhwc = need_x and nhwc and stride == 1 and q >= 0 and KW == KH and _conv_nhwc_ok(Cout, Cin, KH, KW, 1)
        dyp = None
        if dx_nhwc or (need_w and xp is not None):
            # dy as the NHWC operand (bf16, or f16 hi/lo planes), with the border the input gradient needs
            dyp = conv_nhwc_prep(dy, q if dx_nhwc else 0) if bf else conv_nhwc_prep_split(dy, q if dx_nhwc else 0, False, ga)
        fold = bool(dx_nhwc and reflect == 1 and H - 2 >= 4 and W - 2 >= 4)     # the mirrored border folded back by the GEMM itself
        if need_x:
            if dx_nhwc and not bf:
                th, tl, ts = _conv_weight_planes(weight, wa, 1) if ctx.prepared is None else ctx.prepared.planes("conv_dgrad")
                dx = _conv_nhwc_split_call(dyp, th, tl, ts, ga, None, Cin, KH, KW, dil, fold=fold)
            elif dx_nhwc:
                th, _, _ = _conv_weight_planes(weight, None, 1) if ctx.prepared is None else ctx.prepared.planes("conv_dgrad_bf16")
                dx = _conv_nhwc_call(dyp, th, None, Cin, KH, KW, dil, fold=fold)
            elif stride == 1 and q >= 0 and KW == KH:
                # dx = conv(dy, flipped weights with the channel roles swapped, padding d(K-1)-p): the same kernel
                if ctx.prepared is None:
                    th, tl, ts = _conv_weight_planes(weight, wa, 1)
                else:
                    th, tl, ts = ctx.prepared.planes("conv_dgrad" if not bf else "conv_dgrad_bf16")
                dx = _conv_fwd_call(dy, th, tl, ts, ga, None, Cin, KH, KW, 1, dil * (KH - 1) - pad, dil)
            elif stride > 1 and dil == 1 and (dx := _conv_dgrad_strided((B, Cin, H, W), weight, dy, ga, wa, stride, pad)) is not None:
                pass    # stride^2 parity classes, each a stride-1 convolution of dy scattered into dx (K16)
            else:       # whatever is left (dilated + strided, rectangular kernels with odd paddings): the framework
                dx = torch.nn.grad.conv2d_input((B, Cin, H, W), weight, dy, stride=stride, padding=pad, dilation=dil)
        if need_w and xp is not None:
            lib = _lib.load()
            Hp, Wp, Cp = xp.shape[-3:]
            S = lib.cocos_conv2d_nhwc_wgrad_bf16_slices(B, dy.shape[2], dy.shape[3], Cp, Cout, KH, KW)
            part = torch.empty((S, Cout, lib.cocos_conv2d_kdim(Cin, KH, KW)), device=dy.device, dtype=torch.float32)
            if bf:
                _call("conv2d_wgrad", "cocos_conv2d_nhwc_wgrad_bf16", xp.data_ptr(), dyp.data_ptr(), part.data_ptr(), B, Cp, Hp, Wp,
                      Cout, q if dx_nhwc else 0, KH, KW, dil, stride, _stream())
            else:
                _call("conv2d_wgrad", "cocos_conv2d_nhwc_wgrad_f16x3", xp.data_ptr(), dyp.data_ptr(), xa.data_ptr(), ga.data_ptr(),
                      part.data_ptr(), B, Cp, Hp, Wp, Cout, q if dx_nhwc else 0, KH, KW, dil, stride, _stream())
            dw = torch.empty_like(weight)
            _call("conv2d_wgrad", "cocos_conv2d_wgrad_reduce", part.data_ptr(), dw.data_ptr(), S, Cout, Cin, KH, KW, _stream())
        elif need_w:
            lib = _lib.load()
            S = lib.cocos_conv2d_wgrad_slices(B, Cin, H, W, Cout, KH, KW, stride, pad, dil)
            kdim = lib.cocos_conv2d_kdim(Cin, KH, KW)
            part = torch.empty((S, Cout, kdim), device=x.device, dtype=torch.float32)
            if bf:
                _call("conv2d_wgrad", "cocos_conv2d_wgrad_bf16", x.data_ptr(), dy.data_ptr(), part.data_ptr(), B, Cin, H, W,
                      Cout, KH, KW, stride, pad, dil, _stream())
            else:
                _call("conv2d_wgrad", "cocos_conv2d_wgrad_f16x3", x.data_ptr(), dy.data_ptr(), xa.data_ptr(), ga.data_ptr(),
                      part.data_ptr(), B, Cin, H, W, Cout, KH, KW, stride, pad, dil, _stream())
            dw = torch.empty_like(weight)          # sum over the S slices + back to [Cout, Cin, KH, KW] in one pass
            _call("conv2d_wgrad", "cocos_conv2d_wgrad_reduce", part.data_ptr(), dw.data_ptr(), S, Cout, Cin, KH, KW, _stream())
        if need_b and has_bias:
            db = channel_sum(dy)
        if reflect and dx is not None and not fold:          # fold the mirrored border back (K18's backward gather)
            dxp, dx = dx, torch.empty(ctx.x_shape, device=dy.device, dtype=torch.float32)
            _call("reflect_pad2d_bwd", "cocos_reflect_pad2d_bwd", dxp.data_ptr(), dx.data_ptr(), B * Cin, ctx.x_shape[2], ctx.x_shape[3],
                  reflect, _stream())
        return dx, dw, db, None, None, None, None, None


def conv2d(x, weight, bias=None, stride: int = 1, padding: int = 0, dilation: int = 1, reflect: int = 0, prepared=None):
    """torch.nn.functional.conv2d(x, weight, bias, stride, padding, dilation) for groups = 1 and one stride / padding /
    dilation for both axes: fp32 in and out, products on the f16 MFMA with split operands (3 terms, fp32 accumulate) —
    conv_f16x3.hip — or, under COCOS_CONV=bf16, in one bf16 term (stride-1 layers with >= 128 output channels: conv_nhwc_bf16.hip).
    `reflect` = r > 0: the convolution of nn.ReflectionPad2d(r)(x) — on the K16b path the mirrored border is written by the
    operand preparation (no padded fp32 tensor), everywhere else it is ops.reflect_pad2d followed by the plain layer.
    `prepared`: the layer's frozen record (cocosnet_amd.inference) — max|w| cell and weight planes are taken from it instead of being
    derived again; None: today's route, byte for byte."""
    reflect = int(reflect)
    if reflect:
        Cout, Cin, KH, KW = weight.shape
        ow = x.shape[3] + 2 * reflect + 2 * int(padding) - int(dilation) * (KW - 1)
        fused = ((_conv_bf16() or CONV_NHWC_F16X3) and int(stride) == 1 and int(padding) == 0 and x.dim() == 4 and reflect < min(x.shape[2:])
                 and ow >= 32 and ow % 32 == 0 and _conv_nhwc_ok(Cin, Cout, KH, KW, 1))
        if not fused:
            x, reflect = reflect_pad2d(x, reflect), 0
    return _Conv2d.apply(x, weight, bias, int(stride), int(padding), int(dilation), reflect, prepared)


# ------------------------------------------------------------------------------------------
# K6  match_kernel = 3 logits from the K = 256 correlation (no unfold)   (correspondence.py:276-304)
# ------------------------------------------------------------------------------------------
class _Box3Logits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c_raw, mu, nu, a, b, h: int, w: int, k_unfolded: float, scale: float):
        c_raw = _chk(c_raw, "c_raw")
        mu, nu, a, b = (_chk(t, n) for t, n in ((mu, "mu"), (nu, "nu"), (a, "a"), (b, "b")))
        B, N, _ = c_raw.shape
        if N != h * w or any(t.shape != (B, N) for t in (mu, nu, a, b)):
            raise ValueError("box3_logits: shape mismatch")
        f = torch.empty_like(c_raw)
        _call("box3_logits_fwd", "cocos_box3_logits_fwd", c_raw.data_ptr(), mu.data_ptr(), nu.data_ptr(),
              a.data_ptr(), b.data_ptr(), f.data_ptr(), B, h, w, float(k_unfolded), float(scale), _stream())
        ctx.save_for_backward(f, mu, nu, a, b)
        ctx.cfg = (int(h), int(w), float(k_unfolded), float(scale))
        return f

    @staticmethod
    def backward(ctx, g):
        f, mu, nu, a, b = ctx.saved_tensors
        h, w, kc, scale = ctx.cfg
        g = _chk(g, "box3_logits: g")
        B, N, _ = f.shape
        dc = torch.empty_like(f)
        r1, r2, c1, c2 = (torch.empty((B, N), device=f.device, dtype=torch.float32) for _ in range(4))
        nbytes = _lib.load().cocos_box3_logits_bwd_workspace_bytes(B, h, w)
        ws = torch.empty((nbytes + 3) // 4, device=f.device, dtype=torch.float32)
        if PRECISION == "f16x3":          # max|dc| as a by-product: the K3 backward (the consumer) scales its split with it
            cell = _zero_cell(dc.device)
            _call("box3_logits_bwd", "cocos_box3_logits_bwd_amax", g.data_ptr(), f.data_ptr(), mu.data_ptr(),
                  nu.data_ptr(), a.data_ptr(), b.data_ptr(), dc.data_ptr(), r1.data_ptr(), r2.data_ptr(),
                  c1.data_ptr(), c2.data_ptr(), ws.data_ptr(), ws.numel() * 4, B, h, w, scale, cell.data_ptr(),
                  _stream())
            _remember_amax(dc, cell)
        else:
            _call("box3_logits_bwd", "cocos_box3_logits_bwd", g.data_ptr(), f.data_ptr(), mu.data_ptr(),
                  nu.data_ptr(), a.data_ptr(), b.data_ptr(), dc.data_ptr(), r1.data_ptr(), r2.data_ptr(),
                  c1.data_ptr(), c2.data_ptr(), ws.data_ptr(), ws.numel() * 4, B, h, w, scale, _stream())
        dmu, dnu, da, db = (torch.empty_like(r1) for _ in range(4))
        _call("box3_logits_bwd", "cocos_box3_stat_grads", r1.data_ptr(), r2.data_ptr(), c1.data_ptr(), c2.data_ptr(),
              a.data_ptr(), b.data_ptr(), dmu.data_ptr(), dnu.data_ptr(), da.data_ptr(), db.data_ptr(), r1.numel(), kc, scale,
              _stream())
        return dc, dmu, dnu, da, db, None, None, None, None


def box3_logits(c_raw, mu, nu, a, b, h, w, k_unfolded, scale):
    """scale * (diagonal 3x3 box filter of c_raw - k mu nu^T) * a b^T  -> [B,N,N]; see cocos_hip.h K6."""
    return _Box3Logits.apply(c_raw, mu, nu, a, b, h, w, k_unfolded, scale)


# ------------------------------------------------------------------------------------------
# K19 / K20  match_kernel = 3 fused: x-box in the correlation GEMM's epilogue, y-box + softmax + warp in one kernel,
#            nothing box-filtered and no logits in HBM   (correspondence.py:276-291, :304, :307, :318; box3_fused_f16x3.hip)
# ------------------------------------------------------------------------------------------
#: "0": match_kernel 3 keeps the round-2 chain (K3 -> K6 -> K7) everywhere (A/B runs, tests of that chain)
BOX3_FUSED = True
#: the column pass of the cycle terms reads the row pass's T transposed and all passes share one gradient buffer (round 4)
BOX3_SHARE_T = True


#: T tensors of at least this many bytes lend their storage to the dC planes in the backward (see _Box3CorrXbox.backward): the
#: BASELINE config 5 class (128 x 128 grid: 1 GiB per sample).  Smaller ones keep a T that a retained graph may read again.
BOX3_ALIAS_T_BYTES = int(os.environ.get("COCOS_BOX3_ALIAS_T_BYTES", 2 << 30))


def box3_fused_ok(B, C, h, w, Cv=1):
    """Shapes the fused match_kernel-3 family takes (64- or 128-wide grid, whole 256-position tiles) on the split flavour."""
    return (BOX3_FUSED and PRECISION == "f16x3" and C == FUSED_K
            and bool(_lib.load().cocos_box3_fused_supported(h * w, h * w, min(Cv, MAX_FUSED_CV), h, w)))


class _Box3CorrXbox(torch.autograd.Function):
    """T = xbox(C_raw) with KEYS in the rows, tile-blocked (include/cocos_hip.h, K19).  Private contract with
    _Box3SoftmaxWarp: the gradient this node RECEIVES is G = dloss / d ybox(T) (same blocked layout), not dloss / dT — the
    y box of the adjoint is applied here, together with the x box, by K20."""

    @staticmethod
    def forward(ctx, q_raw, k_raw, sink=None, raw_planes=None):
        ctx.sink = sink
        q_raw, k_raw = _chk(q_raw, "box3_corr_xbox: q"), _chk(k_raw, "box3_corr_xbox: k")
        B, K, h, w = q_raw.shape
        N = h * w
        qp = kp = None
        if raw_planes is not None:        # K25 wrote the planes itself: q_raw / k_raw are handles (their memory is never read)
            qp, kp = raw_planes.get(q_raw), raw_planes.get(k_raw)
        ctx.chan = None
        if qp is not None and kp is not None:
            (qh, ql, qch, qcl, qs), (kh, kl, kch, kcl, ks) = qp, kp
            ctx.chan = ((qch, qcl, qs), (kch, kcl, ks))
            qa = ka = None
        else:
            if qp is not None or kp is not None:
                raise _lib.CocosHipError("box3_corr_xbox: producer-made planes for one operand only")
            qf, kf = q_raw.reshape(B, K, N), k_raw.reshape(B, K, N)
            qa, ka = _recall_amax(qf, consume=False), _recall_amax(kf, consume=False)   # left by K12 (both orientations read them)
            qa = absmax(qf) if qa is None else qa
            ka = absmax(kf) if ka is None else ka
            qh, ql, qs = split_f16(qf, True, amax=qa)            # position-major planes [B,N,K]
            kh, kl, ks = split_f16(kf, True, amax=ka)
        t = torch.empty(B * N * N, device=q_raw.device, dtype=torch.float32)
        _call("box3_corr_xbox", "cocos_box3_corr_xbox_f16x3", kh.data_ptr(), kl.data_ptr(), qh.data_ptr(), ql.data_ptr(),
              t.data_ptr(), B, N, N, K, w, ks.data_ptr(), qs.data_ptr(), _stream())
        ctx.save_for_backward(q_raw, k_raw)
        ctx.amax = (qa, ka)
        return t

    @staticmethod
    def backward(ctx, g):
        q_raw, k_raw = ctx.saved_tensors
        qa, ka = ctx.amax
        g = _chk(g, "box3_corr_xbox: g")
        B, K, h, w = q_raw.shape
        N = h * w
        gmax = _recall_amax(g)              # left by K19's backward; a sum of several passes' gradients: one pass over it
        if gmax is None:
            gmax = absmax(g)
        half = dict(device=g.device, dtype=torch.float16)
        t_dead = getattr(ctx.sink, "t_dead", None) if ctx.sink is not None else None
        if (t_dead is not None and t_dead.numel() == B * N * N and t_dead.dtype == torch.float32
                and B * N * N * 4 >= BOX3_ALIAS_T_BYTES):
            # round 5: T's last reader was the last pass's backward, which ran before this node — the dC planes
            # (two f16 planes = T's bytes) take T's storage instead of another B N^2 x 4 bytes (cfg5, B = 2: 5.1 -> 4.1 GiB peak).
            # The kernel writes through raw pointers, which autograd cannot see: the version counter of T is bumped by hand, so that
            # a second backward over a retained graph — T is a saved input of every pass — raises ("modified by an inplace
            # operation") instead of reading planes as logits.  Only for the large shapes (BOX3_ALIAS_T_BYTES).
            torch.autograd.graph.increment_version(t_dead)
            planes = t_dead.view(torch.float16)
            dch, dcl = planes[:B * N * N], planes[B * N * N:]
        else:
            dch, dcl = torch.empty(B * N * N, **half), torch.empty(B * N * N, **half)
        sc = torch.empty(1, device=g.device, dtype=torch.float32)
        _call("box3_adjoint_planes", "cocos_box3_adjoint_planes_f16x3", g.data_ptr(), gmax.data_ptr(), dch.data_ptr(),
              dcl.data_ptr(), sc.data_ptr(), B, N, N, h, w, _stream())
        dq = dk = None
        chan = ctx.chan
        if chan is not None and any(p is None for p in (chan[0][0], chan[1][0])):
            raise _lib.CocosHipError("box3_corr_xbox: backward without the channel-major planes (forward ran without grad)")
        if ctx.needs_input_grad[0]:         # d q_raw[c,P] = sum_Q dC[P,Q] k_raw[c,Q]
            ch, cl, cs = chan[1] if chan is not None else split_f16(k_raw.reshape(B, K, N), False, amax=ka)
            dq = torch.empty_like(q_raw)
            _call("box3_corr_grad", "cocos_hgemm_f16x3", ch.data_ptr(), cl.data_ptr(), dch.data_ptr(), dcl.data_ptr(),
                  dq.data_ptr(), B, K, N, N, 1.0, cs.data_ptr(), sc.data_ptr(), 3, _stream())
        if ctx.needs_input_grad[1]:         # d k_raw[c,Q] = sum_P dC[P,Q] q_raw[c,P]
            ch, cl, cs = chan[0] if chan is not None else split_f16(q_raw.reshape(B, K, N), False, amax=qa)
            dk = torch.empty_like(k_raw)
            _call("box3_corr_grad", "cocos_hgemm_f16x3", ch.data_ptr(), cl.data_ptr(), dch.data_ptr(), dcl.data_ptr(),
                  dk.data_ptr(), B, K, N, N, 1.0, cs.data_ptr(), sc.data_ptr(), 2, _stream())
        if ctx.sink is not None:
            ctx.sink.reset()      # (a second backward through the same graph starts a new G)
        return dq, dk, None, None


class Box3GradSink:
    """The ONE gradient buffer G of a T = box3_corr_xbox(...) that several box3_softmax_warp passes read (row pass, the column
    pass on the transposed T, a second row pass): the first pass's backward allocates G, writes it and hands it to autograd as
    d loss / d T; every later pass ADDS its G into the same buffer inside its kernel (COCOS_BOX3_G_ACCUMULATE) and returns no
    gradient for T — autograd never sums HWxHW tensors, and T's node runs ONE box adjoint + ONE pair of GEMMs for all passes.
    (T's node runs after all of its consumers, so the buffer is complete by then.)"""

    def __init__(self):
        self.buf = None
        self.gmax = None
        self.t_dead = None      # T as the LAST pass's backward saw it: nothing reads it after that (see _Box3CorrXbox.backward)

    def reset(self):
        self.buf = None
        self.gmax = None
        self.t_dead = None

    @staticmethod
    def begin(sink, needs_t: bool, numel: int, device, flags: int):
        """Before a pass's backward kernel (_Box3SoftmaxWarp's, _Box3Lse's) -> (g, g_ret, gmax, flags): the buffer the kernel writes G
        into, what the node returns for T (None on an accumulating pass and when T needs no gradient), a fresh zero max|G| cell and
        the flag word, with COCOS_BOX3_G_ACCUMULATE on a pass that adds.  `sink`: the pass's Box3GradSink or None."""
        if not needs_t:
            sink = None          # nobody differentiates T through this pass (autograd.grad(..., inputs=[v])): its G is scratch and must
                                 # not become — or be added into — the shared buffer
        gmax = _zero_cell(device)
        if sink is not None and sink.buf is not None:      # another pass over this T has written its G: add ours to it
            sink.gmax = gmax                               # ... and max|G| becomes that of the sum (a fresh zero cell)
            return sink.buf, None, gmax, flags | _C["COCOS_BOX3_G_ACCUMULATE"]
        g = torch.empty(numel, device=device, dtype=torch.float32)
        if sink is not None:
            sink.buf, sink.gmax = g, gmax
            # the buffer belongs to THIS backward: whatever happens to T's node (not reached, an exception on the way), the
            # engine drops it when the pass ends, so a later backward over a retained graph starts a new G
            torch.autograd.Variable._execution_engine.queue_callback(sink.reset)
        return g, (g if needs_t else None), gmax, flags

    @staticmethod
    def end(sink, needs_t: bool, t, g, gmax, flags: int):
        """After that kernel: what autograd and the max|x| cache cannot see of a write through raw pointers"""
        if flags & _C["COCOS_BOX3_G_ACCUMULATE"]:
            # the kernel added into another pass's buffer through raw pointers: the version counter follows by hand, so that whatever
            # was derived from the buffer as it was (the first pass's max|G| cell among them) is void
            torch.autograd.graph.increment_version(g)
        _remember_amax(g, gmax)      # (an accumulating pass replaces the cell remembered for the shared buffer)
        if sink is not None and needs_t and t.numel() * 4 >= BOX3_ALIAS_T_BYTES:
            sink.t_dead = t          # (only when T's node will take the storage over: the reference keeps T alive until then)


def box3_corr_xbox(q_raw, k_raw, sink: Box3GradSink | None = None, raw_planes: Box3RawPlanes | None = None):
    """x-direction diagonal box filter of the K = 256 correlation of two raw [B,256,h,w] feature maps (64- or 128-wide grid),
    keys in the rows, in the tile-blocked layout of K19 (an opaque 1-D tensor of B*N*N floats).  `sink`: the gradient sink the
    box3_softmax_warp passes over this T share (see Box3GradSink)."""
    return _Box3CorrXbox.apply(q_raw, k_raw, sink, raw_planes)


class _Box3SoftmaxWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, mu, a, nu, b, v, h: int, w: int, kc: float, scale: float, transposed: bool = False, sink=None):
        ctx.transposed, ctx.sink = bool(transposed), sink
        t, v = _chk(t, "box3_softmax_warp: t"), _chk(v, "box3_softmax_warp: v")
        mu, a, nu, b = (_chk(x, n) for x, n in ((mu, "mu"), (a, "a"), (nu, "nu"), (b, "b")))
        B, N = mu.shape
        Cv = v.shape[1]
        if N != h * w or v.shape != (B, Cv, N) or t.numel() != B * N * N or any(x.shape != (B, N) for x in (a, nu, b)):
            raise ValueError("box3_softmax_warp: shape mismatch")
        v_amax = _recall_amax(v)
        if v_amax is None:
            v_amax = absmax(v)
        vh, vl, v_scale, v_lomask = split_f16_chan_mask(v, v_amax, VALUE_LO_SKIP and Cv > 32)
        out = torch.empty((B, Cv, N), device=v.device, dtype=torch.float32)
        lse = torch.empty((B, N), device=v.device, dtype=torch.float32)
        _call("box3_softmax_warp_fwd", "cocos_box3_softmax_warp_fwd_f16x3", t.data_ptr(), mu.data_ptr(), a.data_ptr(),
              nu.data_ptr(), b.data_ptr(), vh.data_ptr(), vl.data_ptr(), out.data_ptr(), lse.data_ptr(), v_scale.data_ptr(),
              _ptr(v_lomask), B, N, N, Cv, h, w, float(kc), float(scale), 1 if transposed else 0, _stream())
        ctx.v_lomask = v_lomask
        ctx.save_for_backward(t, mu, a, nu, b, v, out, lse)
        ctx.cfg = (int(h), int(w), float(kc), float(scale))
        ctx.v_amax = v_amax
        return out

    @staticmethod
    def backward(ctx, dout):
        t, mu, a, nu, b, v, out, lse = ctx.saved_tensors
        h, w, kc, scale = ctx.cfg
        dout = _chk(dout, "box3_softmax_warp: dout")
        B, N = mu.shape
        Cv = v.shape[1]
        cvp = (Cv + 31) // 32 * 32
        g_amax = _recall_amax(dout)          # left by the kernel that wrote dout (warp_head's backward, concat_channels_amax), else one pass
        if g_amax is None:
            g_amax = absmax(dout)
        d_pre = _rowdot_cached(dout, out) if BWD_D_PRECOMPUTED else None
        (gph, gpl, gs), (vph, vpl, v_scale) = _split_pair_transposed(dout, g_amax, v, ctx.v_amax, cvp)
        f32 = dict(device=v.device, dtype=torch.float32)
        needs_t = ctx.needs_input_grad[0]
        g, g_ret, gmax, flags = Box3GradSink.begin(ctx.sink, needs_t, B * N * N, v.device, _C["COCOS_BOX3_T_TRANSPOSED"] if ctx.transposed else 0)
        dmu, da, dnu, db = (torch.empty((B, N), **f32) for _ in range(4))
        colpart = torch.empty(_lib.load().cocos_box3_softmax_warp_bwd_colpart_bytes(B, N, N) // 4, **f32)
        need_v = ctx.needs_input_grad[5]
        psh = psl = None
        if need_v:        # cycle terms: V itself is differentiated -> the planes of 2^14 P for dv = dout . P
            psh = torch.empty(B * N * N, device=v.device, dtype=torch.float16)
            psl = torch.empty_like(psh)
        _call("box3_softmax_warp_bwd", "cocos_box3_softmax_warp_bwd_f16x3", t.data_ptr(), mu.data_ptr(), a.data_ptr(),
              nu.data_ptr(), b.data_ptr(), vph.data_ptr(), vpl.data_ptr(), gph.data_ptr(), gpl.data_ptr(), gs.data_ptr(),
              v_scale.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), g.data_ptr(), dmu.data_ptr(),
              da.data_ptr(), dnu.data_ptr(), db.data_ptr(), colpart.data_ptr(), gmax.data_ptr(), _ptr(psh), _ptr(psl),
              _ptr(ctx.v_lomask), B, N, N, Cv, cvp, h, w, kc, scale, _ptr(d_pre), flags, _stream())
        Box3GradSink.end(ctx.sink, needs_t, t, g, gmax, flags)
        dv = None
        if need_v:
            gch, gcl, _ = split_f16(dout, False, amax=g_amax)
            dv = torch.empty_like(v)
            _call("box3_softmax_warp_bwd_dv", "cocos_hgemm_f16x3", gch.data_ptr(), gcl.data_ptr(), psh.data_ptr(),
                  psl.data_ptr(), dv.data_ptr(), B, Cv, N, N, 1.0 / 16384.0, gs.data_ptr(), None, 2, _stream())
        return g_ret, dmu, da, dnu, db, dv, None, None, None, None, None, None


def box3_softmax_warp(t, mu, a, nu, b, v, h, w, k_unfolded, scale, transposed: bool = False, sink: Box3GradSink | None = None):
    """out[b,c,p] = sum_q softmax_q(scale * a_p b_q (ybox(T)[p,q] - k mu_p nu_q)) v[b,c,q] with T from box3_corr_xbox —
    the whole match_kernel-3 attention of one orientation; v [B,Cv,N] in chunks of 160 channels.  `transposed`: T is the
    OTHER orientation's (mu / a then belong to T's keys, nu / b to its queries): the column pass on the row pass's T.
    `sink`: the Box3GradSink given to box3_corr_xbox — the passes then accumulate ONE gradient of T inside their kernels."""
    Cv = v.shape[1]
    if Cv <= MAX_FUSED_CV:
        return _Box3SoftmaxWarp.apply(t, mu, a, nu, b, v, h, w, k_unfolded, scale, transposed, sink)
    return torch.cat([_Box3SoftmaxWarp.apply(t, mu, a, nu, b, v[:, c0:c0 + MAX_FUSED_CV], h, w, k_unfolded, scale, transposed, sink)
                      for c0 in range(0, Cv, MAX_FUSED_CV)], dim=1)


def box3_match(t, mu, a, nu, b, h, w, k_unfolded, scale, transposed: bool = False):
    """(idx int32, max, lse), each [B,N]: row maximum, its (lowest) key index and the row log-sum-exp of box3_softmax_warp's logits
    z[p,q] = scale * a_p b_q (ybox(T)[p,q] - k mu_p nu_q), with T from box3_corr_xbox — that pass without its value tensor (K37;
    forward only: the inputs are detached and no autograd node is made).  `transposed` as for box3_softmax_warp.  Shapes outside
    cocos_box3_fused_supported raise: materialise the logits and use row_argmax_lse."""
    with torch.no_grad():
        operands, _ = _box3_readout_gate("box3_match", t, mu, a, nu, b, h, w)
        return _box3_readout_launch("box3_match", "cocos_box3_match_f16x3", operands, (), h, w, k_unfolded, scale, 0, transposed)


def _box3_readout_gate(name, t, mu, a, nu, b, h, w, *, typed=None, own=None, detach: bool = True, f16x3: bool = False):
    """The one gate of the operands of a T readout (box3_match, box3_topk, box3_topk_biased, box3_topk_labelled, box3_sinkhorn,
    box3_lse) -> ((t, mu, a, nu, b) contiguous fp32, detached unless `detach` is False; what `own` returned).  Refusals in this order;
    what the ops differ in is an argument:
      `typed` "tensor" (K54, K55): TypeError for a non-tensor, then ValueError unless mu is [B,N];
              "float32" (K53): TypeError unless the five are float32 tensors, then mu and the shapes (h, w integers) at once;
      `own(B, N)`: the op's own argument errors (a bias, labels, k, a scale), which come before any device is looked at -> the
              tensors the launch takes besides the five, checked (the bias; the two label tables);
      CocosHipError for a tensor off the device, TypeError for another dtype, ValueError for mu and the shapes;
      `f16x3`: CocosHipError under COCOS_PRECISION=fp32."""
    operands = ((t, "t"), (mu, "mu"), (a, "a"), (nu, "nu"), (b, "b"))

    def shapes():
        if mu.dim() != 2:
            raise ValueError(f"{name}: mu is [B,N]")
        B, N = mu.shape
        if N != h * w or t.numel() != B * N * N or any(x.shape != (B, N) for x in (a, nu, b)):
            raise ValueError(f"{name}: shape mismatch")

    if typed is not None:
        for x, what in operands:
            if not torch.is_tensor(x):
                raise TypeError(f"{name}: {what}: expected a tensor, got {type(x).__name__}")
            if typed == "float32" and x.dtype != torch.float32:
                raise TypeError(f"{name}: {what}: expected float32, got {x.dtype}")
        if mu.dim() != 2:
            raise ValueError(f"{name}: mu is [B,N]")
        if typed == "float32":
            if not (_is_int(h) and _is_int(w)):
                raise ValueError(f"{name}: shape mismatch")
            shapes()
    extra = own(*mu.shape) if own is not None else ()
    _gate(name, operands, False)
    t, mu, a, nu, b = (_chk(x.detach() if detach else x, f"{name}: {what}") for x, what in operands)
    if typed != "float32":
        shapes()
    _gate(name, (), f16x3)
    return (t, mu, a, nu, b), extra


def _box3_readout_launch(tag, entry, operands, extra, h, w, k_unfolded, scale, k: int, transposed: bool):
    """One launch of a readout entry point of T — cocos_box3_match_f16x3 (k = 0: outputs [B,N], no k argument), cocos_box3_topk_f16x3,
    cocos_box3_topk_bias_f16x3 or cocos_box3_topk_labels_f16x3 (`extra`: the bias, or the two label tables) — on `operands` = (t, mu, a, nu, b),
    checked, contiguous fp32 tensors -> (idx int32 [B,N,k], val [B,N,k], lse [B,N]).  `tag`: the KernelTimer label."""
    B, N = operands[1].shape
    idx, val, lse = _readout_outputs((B, N), k, operands[0].device)
    _call(tag, entry, *(x.data_ptr() for x in operands), *(x.data_ptr() for x in extra), idx.data_ptr(), val.data_ptr(), lse.data_ptr(), B, N, N, int(h), int(w), float(k_unfolded), float(scale), *((k,) if k else ()),
          _C["COCOS_BOX3_T_TRANSPOSED"] if transposed else 0, _stream())
    return idx, val, lse


def box3_topk_ok(k: int) -> bool:
    """K41 ships an instantiation that serves k candidates (one ships only with zero scratch at two waves per SIMD and when the route
    beats materialise + row_topk_lse at both benchmark shapes: DESIGN.md 3.25); above it the readout materialises (K39b)."""
    return 1 <= k <= _lib.load().cocos_box3_topk_max_k()


def box3_topk(t, mu, a, nu, b, h, w, k_unfolded, scale, k: int, transposed: bool = False):
    """(idx int32 [B,N,k], val [B,N,k], lse [B,N]): per query the k largest of box3_match's logits z[p,q], their key indices and the
    row log-sum-exp (K41; forward only: the inputs are detached and no autograd node is made).  Order: by the logit without its
    per-query factor (z = tt * scale * a_p, scale * a_p > 0) descending and, among bitwise-equal tt, the lower index first — val is
    non-increasing, and two unequal tt that round to the same val keep their tt order.  Rank 0 and lse are box3_match's outputs bit
    for bit.  1 <= k <= MATCH_TOPK_MAX, k <= N (ValueError); a k that box3_topk_ok refuses and the shapes box3_match refuses
    raise: materialise the logits and use row_topk_lse."""
    with torch.no_grad():
        operands, _ = _box3_readout_gate("box3_topk", t, mu, a, nu, b, h, w)
        k = _check_topk("box3_topk", k, mu.shape[1])
        return _box3_readout_launch("box3_topk", "cocos_box3_topk_f16x3", operands, (), h, w, k_unfolded, scale, k, transposed)


# K54  transport on the match_kernel-3 route: the biased readout of T and the Sinkhorn iteration on top of it
def box3_topk_biased(t, mu, a, nu, b, k_bias, h, w, k_unfolded, scale, k: int, transposed: bool = False):
    """box3_topk over z'[p,q] = z[p,q] + k_bias[b,q] (K54; forward only: the inputs are detached and no autograd node is made) ->
    (idx int32 [B,N,k], val [B,N,k] = z', lse [B,N] = log sum_q exp z'[p,q]).  k_bias [B,N] float32: finite values of any sign, or -inf
    to exclude a key (a row with every key excluded has lse = val = -inf and indices in range; no NaN from finite or -inf input).  The
    bias is added inside the scan of T, before the candidate list and the sum; a bias of zeros gives box3_topk's outputs bit for bit.
    `transposed` as for box3_match: the bias then belongs to T's queries, the keys of the transposed problem.  Refusals in this order:
    a bias of another dtype (TypeError), of another shape or one that requires a gradient, a bad k (ValueError); tensors off the
    device; the shapes box3_topk refuses."""
    name = "box3_topk_biased"

    def own(B, N):
        bias = _bias_table(name, k_bias, (B, N))
        _box3_served_k(name, k, N)
        _gate(name, ((bias, "k_bias"),), False)
        return (bias,)
    with torch.no_grad():
        operands, bias = _box3_readout_gate(name, t, mu, a, nu, b, h, w, typed="tensor", own=own)
        return _box3_readout_launch(name, "cocos_box3_topk_bias_f16x3", operands, bias, h, w, k_unfolded, scale, k, transposed)


def _box3_served_k(name, k, N):
    """ValueError unless k is a candidate count (_check_topk) that an instantiation serves: cocos_box3_topk_max_k owns the limit of all
    three top-k entries, and every BIAS and LABELS instantiation up to it ships"""
    if not box3_topk_ok(_check_topk(name, k, N)):
        raise ValueError(f"{name}: k={k}: no instantiation serves it (box3_topk_ok)")


def box3_sinkhorn(t, mu, a, nu, b, h, w, k_unfolded, scale, iters: int, tau: float = 1.0):
    """corr_sinkhorn's iteration on the match_kernel-3 logits z[p,q] of box3_match, from ONE T = box3_corr_xbox (K54; forward only,
    under torch.no_grad()) -> (f [B,N], g [B,N], row_lse [B,N]).  Uniform marginals 1 / N; with g = 0, `iters` times
        f_p = tau (-log N - log sum_q exp(z[p,q] + g_q)),   g_q = tau (-log N - log sum_p exp(z[p,q] + f_p))
    and row_lse_p = log sum_q exp(z[p,q] + g_q) against the final g.  Every half-step is one K = 1 launch of the biased readout over the
    same T: the row half-step reads it as stored with g as the key bias, the column half-step reads it transposed with (mu, a) and
    (nu, b) exchanged and f as the key bias; the affine update runs in torch on [B,N] vectors.  2 iters + 1 launches, no second
    correlation GEMM and nothing N x N besides T.  iters an integer in 1..SINKHORN_MAX_ITERS, 0 < tau <= 1 (ValueError); then the
    refusals of box3_match."""
    f, g, _, _, row_lse = _box3_sinkhorn_readout(t, mu, a, nu, b, h, w, k_unfolded, scale, iters, tau)
    return f, g, row_lse


def _box3_sinkhorn_readout(t, mu, a, nu, b, h, w, k_unfolded, scale, iters, tau):
    """box3_sinkhorn with all three outputs of its last launch -> (f, g, idx [B,N,1], val [B,N,1], row_lse): the k = 1 readout of
    z + g is that launch, so a caller that wants the best match per row pays nothing for it"""
    name = "box3_sinkhorn"
    iters, tau = _sinkhorn_args(name, iters, tau)
    with torch.no_grad():
        (t, mu, a, nu, b), _ = _box3_readout_gate(name, t, mu, a, nu, b, h, w, typed="tensor")
        B, N = mu.shape
        log_m = -math.log(N)
        launch = lambda operands, bias, transposed: _box3_readout_launch(name, "cocos_box3_topk_bias_f16x3", operands, (bias,), h, w,
                                                                         k_unfolded, scale, 1, transposed)
        rows = lambda g: launch((t, mu, a, nu, b), g, False)
        cols = lambda f: launch((t, nu, b, mu, a), f, True)[2]
        g = torch.zeros((B, N), device=t.device, dtype=torch.float32)
        for _ in range(iters):
            f = tau * (log_m - rows(g)[2])
            g = tau * (log_m - cols(f))
        return (f, g, *rows(g))


# K55  label restriction on the match_kernel-3 route: the readout of T over the keys each query's label allows
def box3_topk_labelled(t, mu, a, nu, b, q_label, k_label, h, w, k_unfolded, scale, k: int, transposed: bool = False):
    """box3_topk over the keys each query's label allows (K55; forward only: the inputs are detached and no autograd node is made) ->
    (idx int32 [B,N,k], val [B,N,k], lse [B,N]).  q_label, k_label [B,N] int32 / int64: key q is allowed for query p when
    q_label[b,p] < 0 (unrestricted) or q_label[b,p] == k_label[b,q] (corr_topk_labelled's rule; int64 is narrowed after the clamp that
    keeps a negative label negative).  The mask is applied inside the scan of T, before the candidate list and the sum: lse is over
    the allowed keys, idx / val their k best in box3_topk's order.  A row with fewer than k allowed keys has val = -inf on the missing
    ranks (idx stays inside [0, N)); a row with none has lse = -inf; no NaN from finite input.  With nothing restricted the outputs
    are box3_topk's bit for bit.  `transposed` as for box3_match: the caller exchanges the two label arrays together with (mu, a) and
    (nu, b).  Refusals in this order: a non-tensor or labels of another dtype (TypeError), labels of another shape, a bad k or one
    that box3_topk_ok refuses (ValueError); tensors off the device; the shapes box3_topk refuses; COCOS_PRECISION=fp32.  There is no
    materialised fall-back."""
    name = "box3_topk_labelled"

    def own(B, N):
        labels = _int_table(name, "q_label", q_label, (B, N)), _int_table(name, "k_label", k_label, (B, N))
        _box3_served_k(name, k, N)
        _gate(name, ((labels[0], "q_label"), (labels[1], "k_label")), False)
        return labels
    with torch.no_grad():
        operands, labels = _box3_readout_gate(name, t, mu, a, nu, b, h, w, typed="tensor", own=own, f16x3=True)
        return _box3_readout_launch(name, "cocos_box3_topk_labels_f16x3", operands, labels, h, w, k_unfolded, scale, k, transposed)


class _Box3Lse(torch.autograd.Function):
    """K53.  Forward: box3_match's launch, its lse.  Backward: cocos_box3_lse_bwd_f16x3 writes G = g_lse softmax(z) scale a_p b_q
    in _Box3SoftmaxWarp's convention and under its Box3GradSink protocol, so T's node runs one K20 and one pair of GEMMs for every
    pass over T.  Saved: T, the statistics, lse."""

    @staticmethod
    def forward(ctx, t, mu, a, nu, b, h: int, w: int, kc: float, scale: float, transposed: bool = False, sink=None):
        ctx.transposed, ctx.sink = bool(transposed), sink
        lse = _box3_readout_launch("box3_match", "cocos_box3_match_f16x3", (t, mu, a, nu, b), (), h, w, kc, scale, 0, transposed)[2]
        ctx.save_for_backward(t, mu, a, nu, b, lse)
        ctx.cfg = (int(h), int(w), float(kc), float(scale))
        return lse

    @staticmethod
    def backward(ctx, g_lse):
        t, mu, a, nu, b, lse = ctx.saved_tensors
        h, w, kc, scale = ctx.cfg
        g_lse = _chk(g_lse, "box3_lse: g_lse")
        B, N = mu.shape
        f32 = dict(device=t.device, dtype=torch.float32)
        needs_t = ctx.needs_input_grad[0]
        g, g_ret, gmax, flags = Box3GradSink.begin(ctx.sink, needs_t, B * N * N, t.device, _C["COCOS_BOX3_T_TRANSPOSED"] if ctx.transposed else 0)
        dmu, da, dnu, db = (torch.empty((B, N), **f32) for _ in range(4))
        colpart = torch.empty(_lib.load().cocos_box3_lse_bwd_colpart_bytes(B, N, N) // 4, **f32)
        _call("box3_lse_bwd", "cocos_box3_lse_bwd_f16x3", t.data_ptr(), mu.data_ptr(), a.data_ptr(), nu.data_ptr(), b.data_ptr(),
              lse.data_ptr(), g_lse.data_ptr(), g.data_ptr(), dmu.data_ptr(), da.data_ptr(), dnu.data_ptr(), db.data_ptr(),
              colpart.data_ptr(), gmax.data_ptr(), B, N, N, h, w, kc, scale, flags, _stream())
        Box3GradSink.end(ctx.sink, needs_t, t, g, gmax, flags)
        return g_ret, dmu, da, dnu, db, None, None, None, None, None, None


def box3_lse(t, mu, a, nu, b, h, w, k_unfolded, scale, transposed: bool = False, sink: Box3GradSink | None = None):
    """lse [B,N] = log sum_q exp z[p,q] of box3_match's logits z[p,q] = scale * a_p b_q (ybox(T)[p,q] - k mu_p nu_q), with T from
    box3_corr_xbox — box3_match's launch and its third output bit for bit — WITH a gradient (K53): the backward writes
    g_lse[p] softmax(z)[p,q] scale a_p b_q into T's gradient buffer (cocos_box3_lse_bwd_f16x3) and returns the statistics' gradients.
    `transposed`, `sink` as for box3_softmax_warp: a row pass and a transposed pass over one T that share a Box3GradSink end in one
    box adjoint and one pair of GEMMs.  T is saved for the backward and G is allocated in it: two HWxHW tensors, the dense route's
    budget.  CPU tensors raise CocosHipError, the fp32 flavour too; shapes outside cocos_box3_fused_supported raise ValueError."""
    name = "box3_lse"

    def own(B, N):
        if not scale > 0:
            raise ValueError(f"{name}: scale={scale!r}: expected a positive number")
        return ()
    operands, _ = _box3_readout_gate(name, t, mu, a, nu, b, h, w, typed="float32", own=own, detach=False, f16x3=True)
    if not _lib.load().cocos_box3_fused_supported(h * w, h * w, 1, h, w):
        raise ValueError(f"{name}: the fused box route does not take a {h}x{w} grid (64- or 128-wide, positions a multiple of 256)")
    return _Box3Lse.apply(*operands, h, w, float(k_unfolded), float(scale), transposed, sink)


# ------------------------------------------------------------------------------------------
# K12 statistics of the 3x3-unfolded vectors without unfolding   (correspondence.py:276-280, match_kernel 3)
# ------------------------------------------------------------------------------------------
class _Unfold3Stats(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k_unfolded: float, eps: float):
        x = _chk(x, "unfold3_stats: x")
        B, C, h, w = x.shape
        mk = lambda: torch.empty((B, h * w), device=x.device, dtype=torch.float32)
        mu, a, nrm = mk(), mk(), mk()
        ws = torch.empty(2 * B * h * w, device=x.device, dtype=torch.float32)
        if PRECISION == "f16x3":      # max|x| as a by-product: the correlation GEMM of the fused family splits x next
            cell = _zero_cell(x.device)
            _call("unfold3_stats_fwd", "cocos_unfold3_stats_fwd_amax", x.data_ptr(), mu.data_ptr(), a.data_ptr(),
                  nrm.data_ptr(), ws.data_ptr(), B, C, h, w, float(k_unfolded), float(eps), cell.data_ptr(), _stream())
            _remember_amax(x, cell)
        else:
            _call("unfold3_stats_fwd", "cocos_unfold3_stats_fwd", x.data_ptr(), mu.data_ptr(), a.data_ptr(), nrm.data_ptr(),
                  ws.data_ptr(), B, C, h, w, float(k_unfolded), float(eps), _stream())
        ctx.save_for_backward(x, mu, a, nrm)
        ctx.kc = float(k_unfolded)
        ctx.mark_non_differentiable(nrm)
        return mu, a, nrm

    @staticmethod
    def backward(ctx, dmu, da, _dnrm):
        x, mu, a, nrm = ctx.saved_tensors
        B, C, h, w = x.shape
        dmu = None if dmu is None else _chk(dmu, "unfold3_stats: dmu")
        da = None if da is None else _chk(da, "unfold3_stats: da")
        dx = torch.empty_like(x)
        ws = torch.empty(2 * B * h * w, device=x.device, dtype=torch.float32)
        _call("unfold3_stats_bwd", "cocos_unfold3_stats_bwd", x.data_ptr(), mu.data_ptr(), a.data_ptr(), nrm.data_ptr(),
              _ptr(dmu), _ptr(da), dx.data_ptr(), ws.data_ptr(), B, C, h, w, ctx.kc, _stream())
        return dx, None, None


def unfold3_stats(x, k_unfolded: float, eps: float = NORM_EPS):
    """(mu, a) [B,h*w] of the zero-padded 3x3-unfolded, centred vectors of x [B,C,h,w]: mean over the 9*C entries and
    1 / (L2 norm of the centred vector + eps)."""
    mu, a, _ = _Unfold3Stats.apply(x, k_unfolded, eps)
    return mu, a


# ------------------------------------------------------------------------------------------
# K51 / K52  the pair kernels of the match_kernel-3 route (box3_pair.hip): a softmax over a few candidate keys per query on the box
# logit of single pairs.  K51's candidates are the k keys of idx[b,p,:], K52's the window around idx[b,p]; what follows is shared.
# ------------------------------------------------------------------------------------------
def _box3_stats(name, B, Nq, Nk, mu, a, nu, b):
    """ValueError unless (mu, a) are [B,Nq] and (nu, b) [B,Nk] -> ((tensor, what), ...) of the four"""
    for t, what, n in ((mu, "mu", Nq), (a, "a", Nq), (nu, "nu", Nk), (b, "b", Nk)):
        if tuple(t.shape) != (B, n):
            raise ValueError(f"{name}: {what} is {tuple(t.shape)}, expected {(B, n)} (ops.unfold3_stats of "
                             f"{'theta_raw' if what in ('mu', 'a') else 'phi_raw'})")
    return (mu, "mu"), (a, "a"), (nu, "nu"), (b, "b")


def _box3_pair_gate(name, heads, stats, idx, shape, Nk):
    """_gate, then _chk of the float operands — `heads` = theta_raw, phi_raw (and v), then the statistics — and the clamp of the index
    table into int32 `shape` (the kernels clamp as well: this is the table the key side inverts) -> (*heads, *stats, idx)"""
    _gate(name, heads[:2] + stats + heads[2:] + ((idx, "idx"),), False)
    floats = [_chk(t, f"{name}: {what}") for t, what in heads + stats]
    with torch.no_grad():
        return (*floats, idx.reshape(shape).clamp(0, Nk - 1).to(torch.int32).contiguous())


def _box3_pair_backward(needs, th_t, ph_t, table, width, launch_pair, launch_theta, launch_key, Cv=0):
    """The backward of both pair functions; needs = (theta, phi, mu, a, nu, b, v), `table` [B,Nq,k] what the key side inverts, `width`
    the g / hb entries per query.  Every gradient comes from the same launch whichever others are asked for (the same bits); a launch
    that serves no needed gradient is skipped -> (dth [B,K,Nq], dph [B,K,Nk], dmu, da, dnu, db, dv), None where not needed"""
    need_th, need_ph, need_mu, need_a, need_nu, need_b, need_v = needs
    B, Nq, K = th_t.shape
    Nk = ph_t.shape[1]
    new = lambda *shape: torch.empty(shape, device=th_t.device, dtype=torch.float32)
    dth = dph = dmu = da = dnu = db = dv = g = hb = None
    if need_th or need_ph or need_mu or need_a or need_nu or need_b:
        g = new(B, Nq, width)
        hb = new(B, Nq, width) if need_b else None
        dmu = new(B, Nq) if need_mu else None
        da = new(B, Nq) if need_a else None
        launch_pair(g.data_ptr(), _ptr(hb), _ptr(dmu), _ptr(da))
    if need_th:
        dth_t = new(B, Nq, K)
        launch_theta(g.data_ptr(), dth_t.data_ptr())
        dth = _transpose(dth_t)
        del dth_t
    if need_ph or need_v or need_nu or need_b:
        entries, offsets = _inverse_index_table(table, Nk)      # K42's table: one per backward, shared by the nine taps
        dph_t = new(B, Nk, K) if need_ph else None
        dv_t = new(B, Nk, Cv) if need_v else None
        dnu = new(B, Nk) if need_nu else None
        db = new(B, Nk) if need_b else None
        launch_key(_ptr(g), _ptr(hb), entries.data_ptr(), offsets.data_ptr(), _ptr(dph_t), _ptr(dv_t), _ptr(dnu), _ptr(db))
        if need_ph:
            dph = _transpose(dph_t)
            del dph_t
        if need_v:
            dv = _transpose(dv_t)
    return dth, dph, dmu, da, dnu, db, dv


class _Box3SparseSoftmaxWarp(torch.autograd.Function):
    """K51.  Saved for the backward: the position-major copies of theta and phi, v^T, idx, w, c [B,Nq,k] and the four statistics —
    nothing with an Nq x Nk extent."""

    @staticmethod
    def forward(ctx, theta_raw, phi_raw, mu, a, nu, b, v, idx, inv_t: float, k_bias=None):
        B, K, fh, fw = theta_raw.shape
        gh, gw = phi_raw.shape[2:]
        Nq, Nk, Cv, k = fh * fw, gh * gw, v.shape[1], idx.shape[2]
        th_t, ph_t, vt = _transpose(theta_raw.reshape(B, K, Nq)), _transpose(phi_raw.reshape(B, K, Nk)), _transpose(v)
        out_t = torch.empty((B, Nq, Cv), device=v.device, dtype=torch.float32)
        w, c = (torch.empty((B, Nq, k), device=v.device, dtype=torch.float32) for _ in range(2))
        if k_bias is None:
            _call("box3_sparse_softmax_warp_fwd", "cocos_box3_sparse_softmax_warp_fwd", th_t.data_ptr(), ph_t.data_ptr(), mu.data_ptr(),
                  a.data_ptr(), nu.data_ptr(), b.data_ptr(), vt.data_ptr(), idx.data_ptr(), out_t.data_ptr(), w.data_ptr(), c.data_ptr(), B, K,
                  fh, fw, gh, gw, Cv, k, float(inv_t), _stream())
        else:       # K54: w = softmax(pair logit + k_bias[key]); the bias is a constant — the backward below consumes the saved w
            _call("box3_sparse_softmax_warp_fwd", "cocos_box3_sparse_softmax_warp_bias_fwd", th_t.data_ptr(), ph_t.data_ptr(), mu.data_ptr(),
                  a.data_ptr(), nu.data_ptr(), b.data_ptr(), vt.data_ptr(), idx.data_ptr(), k_bias.data_ptr(), out_t.data_ptr(), w.data_ptr(),
                  c.data_ptr(), B, K, fh, fw, gh, gw, Cv, k, float(inv_t), _stream())
        ctx.save_for_backward(th_t, ph_t, vt, idx, w, c, mu, a, nu, b)
        ctx.cfg = (fh, fw, gh, gw, float(inv_t))
        ctx.mark_non_differentiable(w)
        return _transpose(out_t), w

    @staticmethod
    def backward(ctx, dout, _dw):
        th_t, ph_t, vt, idx, w, c, mu, a, nu, b = ctx.saved_tensors
        fh, fw, gh, gw, inv_t = ctx.cfg
        B, _, K = th_t.shape
        Cv, k = vt.shape[2], idx.shape[2]
        dout_t = _transpose(_chk(dout, "box3_sparse_softmax_warp: dout"))
        name, dims = "box3_sparse_softmax_warp_bwd_", (B, K, fh, fw, gh, gw)
        pair = lambda *out: _call(name + "pair", f"cocos_{name}pair", vt.data_ptr(), dout_t.data_ptr(), idx.data_ptr(), w.data_ptr(),
                                  c.data_ptr(), a.data_ptr(), nu.data_ptr(), b.data_ptr(), *out, *dims, Cv, k, inv_t, _stream())
        theta = lambda g, dth_t: _call(name + "theta", f"cocos_{name}theta", ph_t.data_ptr(), idx.data_ptr(), g, dth_t, *dims, k, _stream())
        key = lambda g, hb, entries, offsets, *out: _call(name + "key", f"cocos_{name}key", th_t.data_ptr(), dout_t.data_ptr(), g, hb,
                                                          w.data_ptr(), mu.data_ptr(), entries, offsets, *out, *dims, Cv, k, _stream())
        dth, dph, *rest = _box3_pair_backward(ctx.needs_input_grad[:7], th_t, ph_t, idx, k, pair, theta, key, Cv)
        return (None if dth is None else dth.reshape(B, K, fh, fw), None if dph is None else dph.reshape(B, K, gh, gw), *rest, None, None, None)


def box3_sparse_softmax_warp(theta_raw, phi_raw, mu, a, nu, b, v, idx, inv_temperature: float, return_weights: bool = False, k_bias=None):
    """out [B,Cv,fh*fw] = sum_r w[b,p,r] * v[b,:,idx[b,p,r]] with w = softmax over r of the match_kernel-3 logit of the pair
    (p, idx[b,p,r]): z[p,q] = inv_temperature * a_p * b_q * (R[p,q] - 9*256 * mu_p * nu_q), R the sum over the nine taps d of
    <theta_raw[:,p+d], phi_raw[:,q+d]> where both p+d and q+d lie inside their grids (box3_logits' value — F.unfold(3, padding=1),
    centre, normalise, dot — for one pair): attention over the k keys per query that box3_topk selected (K51), with gradients for
    theta_raw, phi_raw, mu, a, nu, b and v (each computed only when needed; idx is data).  theta_raw [B,256,fh,fw], phi_raw
    [B,256,gh,gw] fp32, any grids, equal or not; (mu, a) [B,fh*fw] and (nu, b) [B,gh*gw] as unfold3_stats returns them for theta_raw
    and phi_raw (made by it from tensors that require a gradient, they carry the statistics' share of the gradient back); v
    [B,Cv,gh*gw] fp32; idx [B,fh*fw,k] int32 / int64 with 1 <= k <= MATCH_TOPK_MAX, k <= gh*gw — any values: repeats inside a row are
    legal, values outside [0, gh*gw) are clamped into it.  Nothing Nq x Nk is allocated, forward or backward; the gradients are
    gathered in a fixed order (no atomics: bitwise reproducible).  `return_weights`: also return w [B,fh*fw,k] (no gradient).
    `k_bias` (K54; None is the call as it was, launch for launch): float32 [B,gh*gw] added to each of the k pair logits before their
    softmax — a constant (a Sinkhorn potential): one that requires a gradient raises ValueError, another dtype TypeError; the
    gradients are those of the biased softmax through the k pair logits, the statistics and v."""
    name = "box3_sparse_softmax_warp"
    if not torch.is_tensor(idx) or idx.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{name}: idx must be an int32 or int64 tensor, got {idx.dtype if torch.is_tensor(idx) else type(idx).__name__}")
    if theta_raw.dim() != 4 or phi_raw.dim() != 4 or v.dim() != 3 or idx.dim() != 3:
        raise ValueError(f"{name}: expected theta_raw [B,256,fh,fw], phi_raw [B,256,gh,gw], v [B,Cv,gh*gw], idx [B,fh*fw,k]; got "
                         f"{tuple(theta_raw.shape)}, {tuple(phi_raw.shape)}, {tuple(v.shape)}, {tuple(idx.shape)}")
    B, K, fh, fw = theta_raw.shape
    gh, gw = phi_raw.shape[2:]
    Nq, Nk = fh * fw, gh * gw
    if (phi_raw.shape[:2] != (B, K) or Nq < 1 or Nk < 1 or v.shape[0] != B or v.shape[2] != Nk or v.shape[1] < 1
            or idx.shape[:2] != (B, Nq)):
        raise ValueError(f"{name}: shape mismatch theta_raw{tuple(theta_raw.shape)} phi_raw{tuple(phi_raw.shape)} v{tuple(v.shape)} "
                         f"idx{tuple(idx.shape)}")
    if K != FUSED_K:
        raise ValueError(f"{name}: needs {FUSED_K} channels, got {K}")
    _check_topk(name, int(idx.shape[2]), Nk)
    stats = _box3_stats(name, B, Nq, Nk, mu, a, nu, b)
    if k_bias is not None:
        k_bias = _bias_table(name, k_bias, (B, Nk))
        if k_bias.device != v.device:
            raise _lib.CocosHipError(f"{name}: k_bias: expected a tensor on v's device; the correspondence hot path has no CPU fallback")
    theta_raw, phi_raw, v, mu, a, nu, b, idx = _box3_pair_gate(name, ((theta_raw, "theta_raw"), (phi_raw, "phi_raw"), (v, "v")), stats, idx,
                                                               idx.shape, Nk)
    if k_bias is None:
        out, w = _Box3SparseSoftmaxWarp.apply(theta_raw, phi_raw, mu, a, nu, b, v, idx, float(inv_temperature))
    else:
        out, w = _Box3SparseSoftmaxWarp.apply(theta_raw, phi_raw, mu, a, nu, b, v, idx, float(inv_temperature), k_bias)
    return (out, w) if return_weights else out


# K52  trainable sub-cell refinement on the match_kernel-3 route: K46's window soft-argmax on K51's box logit
class _Box3SoftMatchOffset(torch.autograd.Function):
    """K52.  Saved for the backward: the position-major copies of theta and phi, idx [B,Nq], c [B,Nq,W] and the four statistics —
    nothing with an Nq x Nk extent."""

    @staticmethod
    def forward(ctx, theta_raw, phi_raw, mu, a, nu, b, idx, inv_t: float, radius: int, fh: int, fw: int, gh: int, gw: int):
        B, K = theta_raw.shape[:2]
        Nq, Nk, slots = fh * fw, gh * gw, (2 * radius + 1) ** 2
        th_t, ph_t = _transpose(theta_raw.reshape(B, K, Nq)), _transpose(phi_raw.reshape(B, K, Nk))
        new = lambda *shape: torch.empty(shape, device=th_t.device, dtype=torch.float32)
        off, lse_win, c = new(B, Nq, 2), new(B, Nq), new(B, Nq, slots)
        _call("box3_match_refine_fwd", "cocos_box3_match_refine_fwd", th_t.data_ptr(), ph_t.data_ptr(), mu.data_ptr(), a.data_ptr(),
              nu.data_ptr(), b.data_ptr(), idx.data_ptr(), off.data_ptr(), lse_win.data_ptr(), c.data_ptr(), B, K, fh, fw, gh, gw, radius,
              float(inv_t), _stream())
        ctx.save_for_backward(th_t, ph_t, idx, c, mu, a, nu, b)
        ctx.cfg = (fh, fw, gh, gw, radius, float(inv_t), tuple(theta_raw.shape), tuple(phi_raw.shape))
        ctx.mark_non_differentiable(lse_win)
        return off, lse_win

    @staticmethod
    def backward(ctx, doff, _dlse):
        th_t, ph_t, idx, c, mu, a, nu, b = ctx.saved_tensors
        needs = ctx.needs_input_grad[:6]
        fh, fw, gh, gw, radius, inv_t, th_shape, ph_shape = ctx.cfg
        B, Nq, K = th_t.shape
        if not any(needs):
            return (None,) * 13
        doff = _chk(doff, "box3_soft_match_offset: doff")
        name, dims = "box3_match_refine_bwd_", (B, K, fh, fw, gh, gw, radius)
        pair = lambda *out: _call(name + "pair", f"cocos_{name}pair", idx.data_ptr(), c.data_ptr(), a.data_ptr(), nu.data_ptr(), b.data_ptr(),
                                  doff.data_ptr(), *out, *dims, inv_t, _stream())
        theta = lambda g, dth_t: _call(name + "theta", f"cocos_{name}theta", ph_t.data_ptr(), idx.data_ptr(), g, dth_t, *dims, _stream())
        key = lambda g, hb, entries, offsets, dph_t, _dv_t, dnu, db: _call(name + "key", f"cocos_{name}key", th_t.data_ptr(), g, hb,
                                                                           mu.data_ptr(), entries, offsets, dph_t, dnu, db, *dims, _stream())
        # the key side gathers over the inverse table of the (clamped) centres: K42's, with k = 1
        dth, dph, *rest = _box3_pair_backward(needs + (False,), th_t, ph_t, idx.view(B, Nq, 1), c.shape[2], pair, theta, key)
        return (None if dth is None else dth.reshape(th_shape), None if dph is None else dph.reshape(ph_shape), *rest[:4]) + (None,) * 7


def box3_soft_match_offset(theta_raw, phi_raw, mu, a, nu, b, idx, grid, kgrid, inv_rt: float, radius: int):
    """soft_match_offset on the match_kernel-3 logit (K52) -> (off [B,Nq,2] fp32, x first; lse_win [B,Nq]): per query p a softmax over
    z[p,q] = inv_rt * a_p * b_q * (R[p,q] - 9*256 * mu_p * nu_q) — box3_sparse_softmax_warp's logit of one pair — of the keys q in the
    (2 radius + 1)^2 window around idx[b,p] on the `kgrid` = (gh, gw) exemplar grid (positions outside the grid are left out), and its
    expected offset (sum p dx, sum p dy) in cells, limited to [-radius, radius]; lse_win is the window's log-sum-exp (no gradient).
    Differentiable in theta_raw, phi_raw, mu, a, nu and b (each gradient computed only when needed; idx is data; the backward treats
    the limit as the identity).  theta_raw [B,256,fh,fw] or [B,256,fh*fw] on the `grid` = (fh, fw) content grid, phi_raw likewise on
    `kgrid`, fp32, any grids >= 1, equal or not; (mu, a) [B,fh*fw] and (nu, b) [B,gh*gw] as unfold3_stats returns them for theta_raw
    and phi_raw (made by it from tensors that require a gradient, they carry the statistics' share of the gradient back); idx [B,fh*fw]
    (or [B,fh,fw]) int32 / int64, values outside [0, gh*gw) are clamped into it.  Nothing Nq x Nk is allocated, forward or backward;
    the gradients are gathered in a fixed order (no atomics: bitwise reproducible; a centre all queries share is one serial list per
    key around it and tap).  radius in 1..MATCH_REFINE_MAX_RADIUS, inv_rt > 0: ValueError before the library is called."""
    name = "box3_soft_match_offset"
    fh, fw = _grid_pair(name, "grid", grid)
    gh, gw = _grid_pair(name, "kgrid", kgrid)
    if not _is_int(radius) or not 1 <= radius <= MATCH_REFINE_MAX_RADIUS:
        raise ValueError(f"{name}: radius={radius!r}: expected an integer in 1..{MATCH_REFINE_MAX_RADIUS}")
    if not inv_rt > 0:
        raise ValueError(f"{name}: inv_rt={inv_rt!r}: expected a positive number")
    Nq, Nk = fh * fw, gh * gw
    if theta_raw.dim() not in (3, 4) or phi_raw.dim() not in (3, 4):
        raise ValueError(f"{name}: expected theta_raw [B,256,{fh},{fw}] and phi_raw [B,256,{gh},{gw}] (or flat positions); got "
                         f"{tuple(theta_raw.shape)}, {tuple(phi_raw.shape)}")
    B, K = theta_raw.shape[:2]
    if (tuple(theta_raw.shape[2:]) not in ((fh, fw), (Nq,)) or tuple(phi_raw.shape[2:]) not in ((gh, gw), (Nk,))
            or tuple(phi_raw.shape[:2]) != (B, K) or B < 1):
        raise ValueError(f"{name}: shape mismatch theta_raw{tuple(theta_raw.shape)} phi_raw{tuple(phi_raw.shape)} on a {fh}x{fw} content "
                         f"grid and a {gh}x{gw} exemplar grid")
    if K != FUSED_K:
        raise ValueError(f"{name}: needs {FUSED_K} channels, got {K}")
    stats = _box3_stats(name, B, Nq, Nk, mu, a, nu, b)
    idx = _int_table(name, "idx", idx)
    if idx.dim() < 1 or idx.shape[0] != B or idx.numel() != B * Nq:
        raise ValueError(f"{name}: idx is {tuple(idx.shape)}, expected {B} x {Nq} entries")
    operands = _box3_pair_gate(name, ((theta_raw, "theta_raw"), (phi_raw, "phi_raw")), stats, idx, (B, Nq), Nk)
    return _Box3SoftMatchOffset.apply(*operands, float(inv_rt), radius, fh, fw, gh, gw)


# K53  the pair unit at one candidate per query with the logit itself as the output: the target logit of the match loss
class _Box3PairLogits(torch.autograd.Function):
    """Saved for the backward: the position-major copies of theta and phi, idx [B,Nq], c [B,Nq] and the four statistics — nothing
    with an Nq x Nk extent."""

    @staticmethod
    def forward(ctx, theta_raw, phi_raw, mu, a, nu, b, idx, inv_t: float):
        B, K, fh, fw = theta_raw.shape
        gh, gw = phi_raw.shape[2:]
        Nq, Nk = fh * fw, gh * gw
        th_t, ph_t = _transpose(theta_raw.reshape(B, K, Nq)), _transpose(phi_raw.reshape(B, K, Nk))
        z, c = (torch.empty((B, Nq), device=th_t.device, dtype=torch.float32) for _ in range(2))
        _call("box3_pair_logit_fwd", "cocos_box3_pair_logit_fwd", th_t.data_ptr(), ph_t.data_ptr(), mu.data_ptr(), a.data_ptr(),
              nu.data_ptr(), b.data_ptr(), idx.data_ptr(), z.data_ptr(), c.data_ptr(), B, K, fh, fw, gh, gw, float(inv_t), _stream())
        ctx.save_for_backward(th_t, ph_t, idx, c, mu, a, nu, b)
        ctx.cfg = (fh, fw, gh, gw, float(inv_t))
        return z

    @staticmethod
    def backward(ctx, dz):
        th_t, ph_t, idx, c, mu, a, nu, b = ctx.saved_tensors
        needs = ctx.needs_input_grad[:6]
        fh, fw, gh, gw, inv_t = ctx.cfg
        B, Nq, K = th_t.shape
        Nk = ph_t.shape[1]
        if not any(needs):
            return (None,) * 8
        dz = _chk(dz, "box3_pair_logits: dz")
        dims = (B, K, fh, fw, gh, gw)
        with torch.no_grad():
            table = idx.clamp(0, Nk - 1)      # what the gathers see: a negative (unsupervised) entry rides along with g = 0
        sparse = "box3_sparse_softmax_warp_bwd_"
        pair = lambda *out: _call("box3_pair_logit_bwd_pair", "cocos_box3_pair_logit_bwd_pair", idx.data_ptr(), c.data_ptr(), a.data_ptr(),
                                  nu.data_ptr(), b.data_ptr(), dz.data_ptr(), *out, *dims, inv_t, _stream())
        theta = lambda g, dth_t: _call(sparse + "theta", f"cocos_{sparse}theta", ph_t.data_ptr(), table.data_ptr(), g, dth_t, *dims, 1,
                                       _stream())
        key = lambda g, hb, entries, offsets, dph_t, _dv_t, dnu, db: _call(sparse + "key", f"cocos_{sparse}key", th_t.data_ptr(), 0, g, hb, 0,
                                                                           mu.data_ptr(), entries, offsets, dph_t, 0, dnu, db, *dims, 1, 1,
                                                                           _stream())
        dth, dph, *rest = _box3_pair_backward(needs + (False,), th_t, ph_t, table.view(B, Nq, 1), 1, pair, theta, key)
        return (None if dth is None else dth.reshape(B, K, fh, fw), None if dph is None else dph.reshape(B, K, gh, gw), *rest[:4], None, None)


def box3_pair_logits(theta_raw, phi_raw, mu, a, nu, b, idx, inv_temperature: float):
    """z [B,fh*fw] fp32: z[b,p] = inv_temperature * a_p * b_j * (R[p,j] - 9*256 * mu_p * nu_j) for j = idx[b,p] —
    box3_sparse_softmax_warp's logit of one pair per query, itself the output (K53: the target logit of the match loss), with gradients
    for theta_raw, phi_raw, mu, a, nu and b (each computed only when needed; idx is data).  A NEGATIVE idx gives 0 with zero
    gradients; values at or above gh*gw are clamped into the grid.  theta_raw [B,256,fh,fw], phi_raw [B,256,gh,gw] fp32, any grids;
    (mu, a) [B,fh*fw], (nu, b) [B,gh*gw] as unfold3_stats returns them; idx [B,fh*fw] (or [B,fh,fw]) int32 / int64.  Nothing Nq x Nk
    is allocated; the gradients are gathered in a fixed order over the inverse table of idx (no atomics: bitwise reproducible)."""
    name = "box3_pair_logits"
    idx = _int_table(name, "idx", idx)
    if theta_raw.dim() != 4 or phi_raw.dim() != 4:
        raise ValueError(f"{name}: expected theta_raw [B,256,fh,fw] and phi_raw [B,256,gh,gw]; got {tuple(theta_raw.shape)}, "
                         f"{tuple(phi_raw.shape)}")
    B, K, fh, fw = theta_raw.shape
    gh, gw = phi_raw.shape[2:]
    Nq, Nk = fh * fw, gh * gw
    if phi_raw.shape[:2] != (B, K) or B < 1 or Nq < 1 or Nk < 1:
        raise ValueError(f"{name}: shape mismatch theta_raw{tuple(theta_raw.shape)} phi_raw{tuple(phi_raw.shape)}")
    if K != FUSED_K:
        raise ValueError(f"{name}: needs {FUSED_K} channels, got {K}")
    if not inv_temperature > 0:
        raise ValueError(f"{name}: inv_temperature={inv_temperature!r}: expected a positive number")
    stats = _box3_stats(name, B, Nq, Nk, mu, a, nu, b)
    if idx.dim() < 1 or idx.shape[0] != B or idx.numel() != B * Nq:
        raise ValueError(f"{name}: idx is {tuple(idx.shape)}, expected {B} x {Nq} entries")
    _gate(name, ((theta_raw, "theta_raw"), (phi_raw, "phi_raw")) + stats + ((idx, "idx"),), False)
    floats = [_chk(t, f"{name}: {what}") for t, what in ((theta_raw, "theta_raw"), (phi_raw, "phi_raw")) + stats]
    return _Box3PairLogits.apply(*floats, idx.reshape(B, Nq), float(inv_temperature))


# K57  PatchMatch candidate search on the match_kernel-3 route: K43's step with K51's box logit as the score
def _patchmatch_box3_operands(name: str, theta_raw, phi_raw, mu, a, nu, b, k):
    """the shape checks patchmatch_step_box3 / patchmatch_topk_box3 share -> (B, fh, fw, gh, gw, stats); ValueError before the library
    is called"""
    if not (torch.is_tensor(theta_raw) and torch.is_tensor(phi_raw)) or theta_raw.dim() != 4 or phi_raw.dim() != 4:
        got = tuple(tuple(t.shape) if torch.is_tensor(t) else type(t).__name__ for t in (theta_raw, phi_raw))
        raise ValueError(f"{name}: expected theta_raw [B,256,fh,fw] and phi_raw [B,256,gh,gw]; got {got[0]}, {got[1]}")
    B, K, fh, fw = theta_raw.shape
    gh, gw = phi_raw.shape[2:]
    if phi_raw.shape[:2] != (B, K) or B < 1 or fh * fw < 1 or gh * gw < 1:
        raise ValueError(f"{name}: shape mismatch theta_raw{tuple(theta_raw.shape)} phi_raw{tuple(phi_raw.shape)}")
    if K != FUSED_K:
        raise ValueError(f"{name}: needs {FUSED_K} channels, got {K}")
    _check_topk(name, k, gh * gw)
    return B, fh, fw, gh, gw, _box3_stats(name, B, fh * fw, gh * gw, mu, a, nu, b)


def _patchmatch_box3_temperature(name: str, inv_t):
    if isinstance(inv_t, bool) or not isinstance(inv_t, (int, float)) or not inv_t > 0:
        raise ValueError(f"{name}: inv_t={inv_t!r}: expected a positive number")


def _patchmatch_box3_rows(name: str, theta_raw, phi_raw, stats):
    """_gate, then the detached float operands -> (th_t [B,Nq,256], ph_t [B,Nk,256], mu, a, nu, b): the position-major rows are made
    here, ONCE per call of the op (cocos_transpose_f32), not per iteration"""
    _gate(name, ((theta_raw, "theta_raw"), (phi_raw, "phi_raw")) + stats, False)
    th, ph, *st = (_chk(t.detach(), f"{name}: {what}") for t, what in ((theta_raw, "theta_raw"), (phi_raw, "phi_raw")) + stats)
    B, K = th.shape[:2]
    return (_transpose(th.reshape(B, K, -1)), _transpose(ph.reshape(B, K, -1)), *st)


def _patchmatch_box3_launch(rows6, idx, fh, fw, gh, gw, inv_t, k, stride, radii, radius0, seed, iteration):
    """one K57 launch on ready rows; idx int32 [B,Nq,k] contiguous or None -> (idx_out, val_out), fresh buffers"""
    th_t, ph_t, mu, a, nu, b = rows6
    B, Nq, K = th_t.shape
    idx_out = torch.empty((B, Nq, k), device=th_t.device, dtype=torch.int32)
    val_out = torch.empty((B, Nq, k), device=th_t.device, dtype=torch.float32)
    _call("patchmatch_step_box3", "cocos_patchmatch_step_box3", th_t.data_ptr(), ph_t.data_ptr(), mu.data_ptr(), a.data_ptr(),
          nu.data_ptr(), b.data_ptr(), _ptr(idx), idx_out.data_ptr(), val_out.data_ptr(), B, K, fh, fw, gh, gw, k, stride, radii, radius0,
          seed, iteration, float(inv_t), _stream())
    return idx_out, val_out


def patchmatch_step_box3(theta_raw, phi_raw, mu, a, nu, b, idx, inv_t: float, k: int, stride: int, radii: int, radius0: int, seed: int,
                         iteration: int):
    """One PatchMatch iteration on the match_kernel-3 route (K57; forward only: the inputs are detached and no autograd node is made)
    -> (idx int32 [B,Nq,k], val [B,Nq,k]).  The pool, the draw, the order and the short-pool rule are patchmatch_step's, with the
    content grid fh x fw of theta_raw [B,256,fh,fw] as the query grid and the exemplar grid gh x gw of phi_raw [B,256,gh,gw] as the key
    grid (any sizes, equal or not); (mu, a) [B,fh*fw] and (nu, b) [B,gh*gw] as unfold3_stats returns them for theta_raw and phi_raw.
    idx [B,Nq,k] int32 / int64 (values outside the key grid are clamped into it) or None: the hashed initialisation.  val holds the
    logits box3_sparse_softmax_warp forms for the same pairs, z = inv_t a_p b_q (R[p,q] - 9*256 mu_p nu_q).  Nothing Nq x Nk is
    allocated.  Bad shapes, k, inv_t, stride, radii: ValueError before the library is called."""
    name = "patchmatch_step_box3"
    B, fh, fw, gh, gw, stats = _patchmatch_box3_operands(name, theta_raw, phi_raw, mu, a, nu, b, k)
    _patchmatch_box3_temperature(name, inv_t)
    _patchmatch_search(name, stride, radii, radius0, seed, iteration)
    if idx is not None:
        idx = _int_table(name, "the index table", idx, (B, fh * fw, k))
    with torch.no_grad():
        rows6 = _patchmatch_box3_rows(name, theta_raw, phi_raw, stats)
        if idx is not None:
            _gate(name, ((idx, "idx"),), False)
        return _patchmatch_box3_launch(rows6, idx, fh, fw, gh, gw, inv_t, k, stride, radii, radius0, seed, iteration)


def patchmatch_topk_box3(theta_raw, phi_raw, mu, a, nu, b, inv_t: float, k: int, init="random", strides=PATCHMATCH_DEFAULTS["strides"],
                         radii=PATCHMATCH_DEFAULTS["radii"], seed: int = 0):
    """PatchMatch top-k selection on the match_kernel-3 route (K57; forward only) -> (idx int32 [B,Nq,k], val [B,Nq,k]) for
    box3_sparse_softmax_warp: one patchmatch_step_box3 launch per entry of `strides` (iteration t = 0, 1, ...: launch t reads the table
    launch t - 1 wrote, two buffers alive at a time) on position-major rows made once.  `init`, `strides`, `radii` (a number, starting
    at half the longer side of the exemplar grid, or a pair (radii, radius0)) and `seed` as patchmatch_topk takes them; operands and
    errors as patchmatch_step_box3; an empty `strides` is a ValueError (a selection needs scores)."""
    name = "patchmatch_topk_box3"
    B, fh, fw, gh, gw, stats = _patchmatch_box3_operands(name, theta_raw, phi_raw, mu, a, nu, b, k)
    _patchmatch_box3_temperature(name, inv_t)
    if isinstance(init, str) and init != "random" or not (isinstance(init, str) or torch.is_tensor(init)):
        raise ValueError(f"{name}: init={init!r}: expected 'random' or an integer tensor [B,Nq,k]")
    try:
        strides = tuple(strides)
    except TypeError:
        raise ValueError(f"{name}: strides={strides!r}: expected a non-empty sequence of integers >= 1") from None
    if not strides:
        raise ValueError(f"{name}: strides is empty: expected a non-empty sequence of integers >= 1")
    n_radii, radius0 = radii if isinstance(radii, (tuple, list)) and len(radii) == 2 else (radii, max(gh, gw) // 2)
    for t, stride in enumerate(strides):
        _patchmatch_search(name, stride, n_radii, radius0, seed, t)
    idx = None if isinstance(init, str) else _int_table(name, "the index table", init, (B, fh * fw, k))
    with torch.no_grad():
        rows6 = _patchmatch_box3_rows(name, theta_raw, phi_raw, stats)
        if idx is not None:
            _gate(name, ((idx, "idx"),), False)
        val = None
        for t, stride in enumerate(strides):
            idx, val = _patchmatch_box3_launch(rows6, idx, fh, fw, gh, gw, inv_t, k, stride, n_radii, radius0, seed, t)
        return idx, val


class _GatherKeys(torch.autograd.Function):
    """x[b, idx[b,p]] with a backward that is a GATHER in a fixed order: the key kernel of the pair unit at one channel — its dv output
    sums w over the inverse table's list of every key, with w the upstream gradient and dout = 1 (exact products)."""

    @staticmethod
    def forward(ctx, x, idx):
        ctx.save_for_backward(idx)
        ctx.nk = x.shape[1]
        return torch.where(idx >= 0, torch.gather(x, 1, idx.clamp_min(0).long()), torch.zeros((), device=x.device, dtype=x.dtype))

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        B, Nq = idx.shape
        Nk = ctx.nk
        dy = _chk(dy, "box3_gather_keys: dy")
        w = torch.where(idx >= 0, dy, torch.zeros((), device=dy.device, dtype=dy.dtype)).contiguous()
        ones = torch.ones((B, Nq), device=dy.device, dtype=torch.float32)
        entries, offsets = _inverse_index_table(idx.clamp(0, Nk - 1).view(B, Nq, 1), Nk)
        dx = torch.empty((B, Nk), device=dy.device, dtype=torch.float32)
        name = "box3_sparse_softmax_warp_bwd_key"
        _call(name, f"cocos_{name}", 0, ones.data_ptr(), 0, 0, w.data_ptr(), 0, entries.data_ptr(), offsets.data_ptr(), 0, dx.data_ptr(), 0, 0,
              B, FUSED_K, 1, Nq, 1, Nk, 1, 1, _stream())
        return dx, None


def box3_gather_keys(x, idx):
    """y [B,Nq] = x[b, idx[b,p]] for x [B,Nk] fp32 on the GPU and idx [B,Nq] int32 / int64 below Nk (a negative entry gives 0 and no
    gradient).  The gradient of x is gathered over the inverse table of idx in table order — no index_add_, no atomics: bitwise
    reproducible (K53: the column lse at the target)."""
    name = "box3_gather_keys"
    idx = _int_table(name, "idx", idx)
    if x.dim() != 2 or idx.dim() != 2 or idx.shape[0] != x.shape[0]:
        raise ValueError(f"{name}: expected x [B,Nk] and idx [B,Nq]; got {tuple(x.shape)}, {tuple(idx.shape)}")
    _gate(name, ((x, "x"), (idx, "idx")), False)
    x = _chk(x, f"{name}: x")
    return _GatherKeys.apply(x, idx)


# ------------------------------------------------------------------------------------------
# K7  softmax + warp from materialised key-major logits   (correspondence.py:307 + :318 ...)
# ------------------------------------------------------------------------------------------
class _LogitsSoftmaxWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits_t, v):
        logits_t, v = _chk(logits_t, "logits_t"), _chk(v, "v")
        B, Nk, Nq = logits_t.shape
        Cv = v.shape[1]
        if v.shape[0] != B or v.shape[2] != Nk:
            raise ValueError(f"logits_softmax_warp: shape mismatch {tuple(logits_t.shape)} {tuple(v.shape)}")
        out = torch.empty((B, Cv, Nq), device=v.device, dtype=torch.float32)
        lse = torch.empty((B, Nq), device=v.device, dtype=torch.float32)
        split = PRECISION == "f16x3" and Nk % 4 == 0 and Cv <= MAX_FUSED_CV and Nq * Nk * 4 < 2 ** 31 - 1
        ctx.v_amax = None
        if split:      # P.V on the f16 MFMA (logits_softmax_warp_f16x3.hip); V planes normalised on the device
            ctx.v_amax = _recall_amax(v)
            if ctx.v_amax is None:
                ctx.v_amax = absmax(v)
            vh, vl, v_scale = split_f16(v, False, amax=ctx.v_amax)
            _call("logits_softmax_warp_fwd", "cocos_logits_softmax_warp_fwd_f16x3", logits_t.data_ptr(), vh.data_ptr(),
                  vl.data_ptr(), out.data_ptr(), lse.data_ptr(), v_scale.data_ptr(), B, Nq, Nk, Cv, _stream())
        else:
            _call("logits_softmax_warp_fwd", "cocos_logits_softmax_warp_fwd", logits_t.data_ptr(), v.data_ptr(),
                  out.data_ptr(), lse.data_ptr(), B, Nq, Nk, Cv, _stream())
        ctx.split = split
        ctx.save_for_backward(logits_t, v, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        logits_t, v, out, lse = ctx.saved_tensors
        dout = _chk(dout, "dout")
        B, Nk, Nq = logits_t.shape
        Cv = v.shape[1]
        dlg = dv = None
        if ctx.needs_input_grad[0]:
            dlg = torch.empty_like(logits_t)
            if ctx.split:
                cvp = (Cv + 31) // 32 * 32
                g_amax = _recall_amax(dout)          # left by warp_head's backward, else one pass
                gph, gpl, gs = split_f16(dout, True, cpad=cvp, amax=absmax(dout) if g_amax is None else g_amax)
                vph, vpl, v_scale = split_f16(v, True, cpad=cvp, amax=ctx.v_amax)
                _call("logits_softmax_warp_bwd", "cocos_logits_softmax_warp_bwd_f16x3", logits_t.data_ptr(),
                      vph.data_ptr(), vpl.data_ptr(), gph.data_ptr(), gpl.data_ptr(), gs.data_ptr(), v_scale.data_ptr(),
                      out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dlg.data_ptr(), B, Nq, Nk, Cv, cvp, _stream())
            else:
                _call("logits_softmax_warp_bwd", "cocos_logits_softmax_warp_bwd", logits_t.data_ptr(), v.data_ptr(),
                      out.data_ptr(), lse.data_ptr(), dout.data_ptr(), dlg.data_ptr(), B, Nq, Nk, Cv, _stream())
        if ctx.needs_input_grad[1]:
            # dv[c,j] = sum_i P[i,j] dout[c,i] (cycle terms only): P^T is rebuilt once and contracted with
            # the K5 GEMM; exp() here is the only non-HIP arithmetic, on a path no README command trains
            p_t = torch.exp(logits_t - lse[:, None, :])
            dv = torch.empty_like(v)
            _call("warp_materialized_fwd", "cocos_warp_materialized_fwd", p_t.data_ptr(), dout.data_ptr(),
                  dv.data_ptr(), B, Nk, Nq, Cv, _stream())
        return dlg, dv


def logits_softmax_warp(logits_t, v):
    """out[b,c,i] = sum_j softmax_j(logits_t[b,j,i]) v[b,c,j]; logits_t [B,Nk,Nq] key-major, v [B,Cv,Nk]."""
    Cv = v.shape[1]
    if Cv <= MAX_FUSED_CV:
        return _LogitsSoftmaxWarp.apply(logits_t, v)
    return torch.cat([_LogitsSoftmaxWarp.apply(logits_t, v[:, c0:c0 + MAX_FUSED_CV])
                      for c0 in range(0, Cv, MAX_FUSED_CV)], dim=1)


# ------------------------------------------------------------------------------------------
# K8  WTA_scale + /temperature on the materialised correlation   (correspondence.py:38-77, :300-304)
# ------------------------------------------------------------------------------------------
class _WTAScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, scale: float, post_scale: float):
        f = _chk(f, "wta_scale: f")
        cols = f.shape[-1]
        rows = f.numel() // cols
        nbytes = _lib.load().cocos_wta_scale_mask_bytes(rows, cols)
        if nbytes < 0:
            raise ValueError(f"wta_scale: bad shape {tuple(f.shape)}")
        mask = torch.empty(nbytes, device=f.device, dtype=torch.uint8)      # 1 bit per element
        y = torch.empty_like(f)
        _call("wta_scale_fwd", "cocos_wta_scale_fwd", f.data_ptr(), y.data_ptr(), mask.data_ptr(), rows, cols,
              float(scale), float(post_scale), _stream())
        ctx.save_for_backward(mask)
        ctx.post = float(post_scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        dy = _chk(dy, "wta_scale: dy")
        cols = dy.shape[-1]
        dx = torch.empty_like(dy)
        _call("wta_scale_bwd", "cocos_wta_scale_bwd", dy.data_ptr(), mask.data_ptr(), dx.data_ptr(),
              dy.numel() // cols, cols, ctx.post, _stream())
        return dx, None, None


def wta_scale(f, scale: float, post_scale: float = 1.0):
    """WTA_scale.apply(f, scale) * post_scale: each row's maxima kept, the rest multiplied by `scale`;
    backward = grad * post_scale * (1 at the maxima, the reference's fixed 1e-4 elsewhere)."""
    return _WTAScale.apply(f, scale, post_scale)


# ------------------------------------------------------------------------------------------
# K9  PONO + SPADE modulation + LeakyReLU   (normalization.py:63-68,:148-151; architecture.py:88-95)
# ------------------------------------------------------------------------------------------
PONO_EPS = 1e-5   # PositionalNorm2d's epsilon (normalization.py:63)


class _PonoSpade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, slope: float, eps: float):
        x, gamma, beta = _chk(x, "pono_spade: x"), _chk(gamma, "pono_spade: gamma"), _chk(beta, "pono_spade: beta")
        if gamma.shape != x.shape or beta.shape != x.shape:
            raise ValueError(f"pono_spade: x{tuple(x.shape)} gamma{tuple(gamma.shape)} beta{tuple(beta.shape)}")
        B, C = x.shape[:2]
        N = x.numel() // (B * C)
        y = torch.empty_like(x)
        if CONV_PRECISION == "f16x3":         # max|y| as a by-product: y is the input of the block's next convolution
            cell = _zero_cell(x.device)
            part = torch.empty(_lib.load().cocos_pono_spade_amax_partials(B, C, N), device=x.device, dtype=torch.float32)
            _call("pono_spade_fwd", "cocos_pono_spade_fwd_amax", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                  cell.data_ptr(), part.data_ptr(), B, C, N, float(eps), float(slope), _stream())
            _remember_amax(y, cell, weak=True)
        else:
            _call("pono_spade_fwd", "cocos_pono_spade_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                  y.data_ptr(), B, C, N, float(eps), float(slope), _stream())
        ctx.save_for_backward(x, gamma, beta)
        ctx.cfg = (float(slope), float(eps))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta = ctx.saved_tensors
        slope, eps = ctx.cfg
        dy = _chk(dy, "pono_spade: dy")
        B, C = x.shape[:2]
        N = x.numel() // (B * C)
        need_x, need_g, need_b = ctx.needs_input_grad[:3]
        dx = torch.empty_like(x) if need_x else None
        dg = torch.empty_like(x) if need_g else None
        db = torch.empty_like(x) if need_b else None
        if (dg is not None or db is not None) and CONV_PRECISION == "f16x3":
            # max|dgamma| / max|dbeta| as by-products: the output gradients of SPADE's mlp_gamma / mlp_beta convolutions
            cells = _zero_cells(x.device, 2)
            part = torch.empty(2 * _lib.load().cocos_pono_spade_amax_partials(B, C, N), device=x.device, dtype=torch.float32)
            _call("pono_spade_bwd", "cocos_pono_spade_bwd_amax", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dy.data_ptr(), _ptr(dx),
                  _ptr(dg), _ptr(db), cells.data_ptr(), part.data_ptr(), B, C, N, eps, slope, _stream())
            if dg is not None:
                _remember_amax(dg, cells[0:1], weak=True)
            if db is not None:
                _remember_amax(db, cells[1:2], weak=True)
        else:
            _call("pono_spade_bwd", "cocos_pono_spade_bwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                  dy.data_ptr(), _ptr(dx), _ptr(dg), _ptr(db), B, C, N, eps, slope, _stream())
        return dx, dg, db, None, None


def pono_spade(x, gamma, beta, slope: float = 1.0, eps: float = PONO_EPS):
    """leaky_relu(PositionalNorm2d(x) * (1 + gamma) + beta, slope) for x, gamma, beta [B,C,H,W]."""
    return _PonoSpade.apply(x, gamma, beta, slope, eps)


class _ReflectPad2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pad: int):
        x = _chk(x, "reflect_pad2d: x")
        if x.dim() != 4 or not (0 <= pad < min(x.shape[2:])):
            raise ValueError(f"reflect_pad2d: x{tuple(x.shape)} pad={pad} (pad must be smaller than H and W)")
        B, C, H, W = x.shape
        y = torch.empty((B, C, H + 2 * pad, W + 2 * pad), device=x.device, dtype=torch.float32)
        _call("reflect_pad2d_fwd", "cocos_reflect_pad2d_fwd", x.data_ptr(), y.data_ptr(), B * C, H, W, int(pad), _stream())
        ctx.cfg = (B, C, H, W, int(pad))
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W, pad = ctx.cfg
        dy = _chk(dy, "reflect_pad2d: dy")
        dx = torch.empty((B, C, H, W), device=dy.device, dtype=torch.float32)
        _call("reflect_pad2d_bwd", "cocos_reflect_pad2d_bwd", dy.data_ptr(), dx.data_ptr(), B * C, H, W, pad, _stream())
        return dx, None


def reflect_pad2d(x, pad: int):
    """nn.ReflectionPad2d(pad)(x) for x [B,C,H,W] (one padding for the four sides, pad < H, W): K18, backward as a gather."""
    return _ReflectPad2d.apply(x, int(pad))


class _SpadeModulate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xh, gamma, beta, slope: float):
        xh, gamma, beta = (_chk(t, f"spade_modulate: {n}") for t, n in ((xh, "xh"), (gamma, "gamma"), (beta, "beta")))
        if gamma.shape != xh.shape or beta.shape != xh.shape:
            raise ValueError(f"spade_modulate: xh{tuple(xh.shape)} gamma{tuple(gamma.shape)} beta{tuple(beta.shape)}")
        y = torch.empty_like(xh)
        _call("spade_modulate_fwd", "cocos_spade_modulate_fwd", xh.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
              y.data_ptr(), xh.numel(), float(slope), _stream())
        ctx.save_for_backward(xh, gamma, beta)
        ctx.slope = float(slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        xh, gamma, beta = ctx.saved_tensors
        dy = _chk(dy, "spade_modulate: dy")
        need = ctx.needs_input_grad[:3]
        outs = [torch.empty_like(xh) if w else None for w in need]
        _call("spade_modulate_bwd", "cocos_spade_modulate_bwd", xh.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
              dy.data_ptr(), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), xh.numel(), ctx.slope, _stream())
        return outs[0], outs[1], outs[2], None


def spade_modulate(xh, gamma, beta, slope: float = 1.0):
    """leaky_relu(xh * (1 + gamma) + beta, slope) where xh is ALREADY normalised (instance / batch / sync-batch norm):
    the non-PONO tail of SPADE.forward (normalization.py:148) + the block's activation, one pass each way (K17)."""
    return _SpadeModulate.apply(xh, gamma, beta, slope)


# ------------------------------------------------------------------------------------------
# K26 parameter-free batch / sync-batch / instance norm + SPADE modulation + LeakyReLU   (normalization.py:93-101, :148;
#     architecture.py:88-95) — the non-PONO counterpart of K9, four passes: stats, apply | bwd_stats, bwd_apply
# ------------------------------------------------------------------------------------------
NORM_SPADE_KINDS = ("batch", "syncbatch", "instance")


def _ns_dims(x: torch.Tensor):
    if x.dim() < 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"norm_spade: expected x [B, C, ...], got {tuple(x.shape)}")
    B, C = x.shape[:2]
    return B, C, x.numel() // (B * C)


def _ns_workspace(x: torch.Tensor) -> torch.Tensor:
    B, C, N = _ns_dims(x)
    return torch.empty(max(_lib.load().cocos_norm_spade_workspace_floats(B, C, N), 4), device=x.device, dtype=torch.float32)


def _ns_same_shape(x, *ts):
    for t in ts:
        if t.shape != x.shape:
            raise ValueError(f"norm_spade: x{tuple(x.shape)} and an operand of shape {tuple(t.shape)}")


def norm_spade_stats(x, per_sample: bool, eps: float = 1e-5) -> torch.Tensor:
    """One pass over x [B, C, ...]: [4, G] = (count, mean, M2, 1/sqrt(M2/count + eps)) per statistics group — the channel over
    (B, H, W) for the batch norms (G = C), the plane (b, c) for per_sample (G = B*C).  Bitwise reproducible."""
    x = _chk(x, "norm_spade_stats: x")
    B, C, N = _ns_dims(x)
    stats = torch.empty((4, B * C if per_sample else C), device=x.device, dtype=torch.float32)
    _call("norm_spade_fwd", "cocos_norm_spade_stats", x.data_ptr(), stats.data_ptr(), _ns_workspace(x).data_ptr(), B, C, N,
          int(bool(per_sample)), float(eps), _stream())
    return stats


def merge_norm_stats(stats: torch.Tensor, eps: float = 1e-5):
    """Combine the [R, 4, G] (count, mean, M2, .) of R parts of a batch (ranks) into the whole batch's (count, mean, M2, invstd),
    each [G]: in fp64, M2 = sum_r M2_r + n_r (mean_r - mean)^2 (exact, no sum x^2 - n mean^2 cancellation)."""
    s = stats.double()
    n_r, m_r, M_r = s[:, 0], s[:, 1], s[:, 2]
    n = n_r.sum(0)
    mean = (n_r * m_r).sum(0) / n
    M2 = (M_r + n_r * (m_r - mean) ** 2).sum(0)
    invstd = torch.rsqrt(M2 / n + eps)
    return torch.stack([n, mean, M2, invstd]).float()


def norm_spade_apply(x, gamma, beta, mean, invstd, per_sample: bool, slope: float = 1.0, amax_cell=None) -> torch.Tensor:
    """y = leaky_relu((x - mean_g) * invstd_g * (1 + gamma) + beta, slope) with per-group mean / invstd [G] (batch statistics or
    running buffers).  amax_cell (optional 1-element tensor): max(cell, max|y|) from the same pass."""
    x, gamma, beta = (_chk(t, f"norm_spade_apply: {n}") for t, n in ((x, "x"), (gamma, "gamma"), (beta, "beta")))
    mean, invstd = _chk(mean, "norm_spade_apply: mean"), _chk(invstd, "norm_spade_apply: invstd")
    _ns_same_shape(x, gamma, beta)
    B, C, N = _ns_dims(x)
    y = torch.empty_like(x)
    ws = _ns_workspace(x) if amax_cell is not None else None
    _call("norm_spade_fwd", "cocos_norm_spade_apply", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
          invstd.data_ptr(), y.data_ptr(), _ptr(amax_cell), _ptr(ws), B, C, N, int(bool(per_sample)), float(slope), _stream())
    return y


def norm_spade_bwd_stats(x, gamma, beta, dy, mean, invstd, per_sample: bool, slope: float = 1.0) -> torch.Tensor:
    """One pass over x, gamma, beta, dy: [2, G] = (sum dxhat, sum dxhat * xhat) per group, dxhat = dy * act'(z) * (1 + gamma)."""
    x, gamma, beta, dy = (_chk(t, f"norm_spade_bwd_stats: {n}") for t, n in ((x, "x"), (gamma, "gamma"), (beta, "beta"), (dy, "dy")))
    mean, invstd = _chk(mean, "norm_spade_bwd_stats: mean"), _chk(invstd, "norm_spade_bwd_stats: invstd")
    _ns_same_shape(x, gamma, beta, dy)
    B, C, N = _ns_dims(x)
    sums = torch.empty((2, B * C if per_sample else C), device=x.device, dtype=torch.float32)
    _call("norm_spade_bwd", "cocos_norm_spade_bwd_stats", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dy.data_ptr(),
          mean.data_ptr(), invstd.data_ptr(), sums.data_ptr(), _ns_workspace(x).data_ptr(), B, C, N, int(bool(per_sample)), float(slope),
          _stream())
    return sums


def norm_spade_bwd_apply(x, gamma, beta, dy, mean, invstd, sums, inv_count: float, per_sample: bool, slope: float = 1.0,
                         need=(True, True, True), amax_cells=None):
    """(dx, dgamma, dbeta), each None where `need` says so.  sums: norm_spade_bwd_stats of the whole group (all ranks), scaled
    by inv_count = 1 / group size; None = constant statistics (running buffers): dx = invstd * dxhat.  amax_cells (optional
    2-element tensor): max(cell, max|dgamma|), max(cell, max|dbeta|) from the same pass."""
    x, gamma, beta, dy = (_chk(t, f"norm_spade_bwd_apply: {n}") for t, n in ((x, "x"), (gamma, "gamma"), (beta, "beta"), (dy, "dy")))
    mean, invstd = _chk(mean, "norm_spade_bwd_apply: mean"), _chk(invstd, "norm_spade_bwd_apply: invstd")
    sums = None if sums is None else _chk(sums, "norm_spade_bwd_apply: sums")
    _ns_same_shape(x, gamma, beta, dy)
    B, C, N = _ns_dims(x)
    outs = [torch.empty_like(x) if w else None for w in need]
    ws = _ns_workspace(x) if amax_cells is not None else None
    _call("norm_spade_bwd", "cocos_norm_spade_bwd_apply", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dy.data_ptr(),
          mean.data_ptr(), invstd.data_ptr(), _ptr(sums), float(inv_count), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
          _ptr(amax_cells), _ptr(ws), B, C, N, int(bool(per_sample)), float(slope), _stream())
    return tuple(outs)


class _NormSpade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, per_sample: bool, use_batch: bool, run_mean, run_var, eps: float, slope: float, sync: bool, group,
                holder: dict):
        x, gamma, beta = _chk(x, "norm_spade: x"), _chk(gamma, "norm_spade: gamma"), _chk(beta, "norm_spade: beta")
        _ns_same_shape(x, gamma, beta)
        B, C, N = _ns_dims(x)
        count = None
        if use_batch:
            stats = norm_spade_stats(x, per_sample, eps)
            if sync:            # every rank's (count, mean, M2): one small all-gather, merged in fp64
                import torch.distributed as dist
                parts = [torch.empty_like(stats) for _ in range(dist.get_world_size(group))]
                dist.all_gather(parts, stats.contiguous(), group=group)
                stats = merge_norm_stats(torch.stack(parts), eps)
                count = stats[0, :1]                   # (same for every channel; stays on the device)
            else:
                count = float(B * N if not per_sample else N)
            mean, invstd = stats[1].contiguous(), stats[3].contiguous()
            holder.update(mean=mean, m2=stats[2], count=count)
        else:
            mean = run_mean.detach().float().contiguous()
            invstd = torch.rsqrt(run_var.detach().float() + eps).contiguous()
        cell = _zero_cell(x.device) if CONV_PRECISION == "f16x3" else None   # y is the input of the block's next convolution
        y = norm_spade_apply(x, gamma, beta, mean, invstd, per_sample, slope, cell)
        if cell is not None:
            _remember_amax(y, cell, weak=True)
        ctx.save_for_backward(x, gamma, beta, mean, invstd)
        ctx.cfg = (bool(per_sample), bool(use_batch), float(slope), bool(sync), group, count)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mean, invstd = ctx.saved_tensors
        per_sample, use_batch, slope, sync, group, count = ctx.cfg
        dy = _chk(dy, "norm_spade: dy")
        need = tuple(ctx.needs_input_grad[:3])
        sums, inv_count = None, 1.0
        if use_batch and need[0]:
            sums = norm_spade_bwd_stats(x, gamma, beta, dy, mean, invstd, per_sample, slope)
            if sync:
                import torch.distributed as dist
                dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
                sums = (sums / count).contiguous()
            else:
                inv_count = 1.0 / count
        cells = _zero_cells(x.device, 2) if (need[1] or need[2]) and CONV_PRECISION == "f16x3" else None
        dx, dg, db = norm_spade_bwd_apply(x, gamma, beta, dy, mean, invstd, sums, inv_count, per_sample, slope, need, cells)
        if cells is not None:       # the output gradients of SPADE's mlp_gamma / mlp_beta convolutions
            if dg is not None:
                _remember_amax(dg, cells[0:1], weak=True)
            if db is not None:
                _remember_amax(db, cells[1:2], weak=True)
        return dx, dg, db, None, None, None, None, None, None, None, None, None


def norm_spade(x, gamma, beta, kind: str, running_mean=None, running_var=None, num_batches_tracked=None, training: bool = True,
               momentum=0.1, eps: float = 1e-5, slope: float = 1.0, group=None):
    """leaky_relu(norm(x) * (1 + gamma) + beta, slope) for x, gamma, beta [B, C, H, W], norm one of NORM_SPADE_KINDS without
    affine parameters: "batch" = nn.BatchNorm2d, "syncbatch" = dist.SyncBatchNorm2d (statistics over every rank of `group` when a
    process group is live), "instance" = nn.InstanceNorm2d (no running statistics).  The running buffers follow nn.BatchNorm2d:
    batch statistics when `training` or no buffers are given, updated with `momentum` (None: cumulative average), unbiased
    running_var, num_batches_tracked counted."""
    if kind not in NORM_SPADE_KINDS:
        raise ValueError(f"norm_spade: kind {kind!r} is not one of {NORM_SPADE_KINDS}")
    per_sample = kind == "instance"
    track = running_mean is not None and running_var is not None
    if per_sample and track:
        raise ValueError("norm_spade: instance norm with running statistics is not supported")
    use_batch = training or not track
    size = x.size()
    if use_batch:
        spatial = 1
        for d in size[2:]:
            spatial *= d
        if per_sample and spatial == 1:
            raise ValueError(f"Expected more than 1 spatial element when training, got input size {size}")
        if kind == "batch" and size[0] * spatial == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {size}")
    sync = False
    if kind == "syncbatch" and use_batch:
        from .dist import _live_world
        sync = _live_world(group) > 1
    holder = {}
    y = _NormSpade.apply(x, gamma, beta, per_sample, use_batch, running_mean, running_var, float(eps), float(slope), sync, group, holder)
    if training and track:
        with torch.no_grad():
            m = 0.0 if momentum is None else momentum
            if num_batches_tracked is not None:
                num_batches_tracked.add_(1)
                if momentum is None:
                    m = 1.0 / float(num_batches_tracked)
            n = holder["count"]
            if isinstance(n, torch.Tensor):
                unbiased = holder["m2"] / (n - 1).clamp_min(1.0)
            else:
                unbiased = holder["m2"] / max(n - 1.0, 1.0)
            running_mean.mul_(1 - m).add_(holder["mean"], alpha=m)
            running_var.mul_(1 - m).add_(unbiased, alpha=m)
    return y


# ------------------------------------------------------------------------------------------
# K11 nearest-neighbour up-sampling of the warped image   (correspondence.py:188, :327)
# ------------------------------------------------------------------------------------------
class _UpsampleNearest(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale: int):
        x = _chk(x, "upsample_nearest: x")
        B, C, h, w = x.shape
        y = torch.empty((B, C, h * scale, w * scale), device=x.device, dtype=torch.float32)
        _call("upsample_nearest_fwd", "cocos_upsample_nearest_fwd", x.data_ptr(), y.data_ptr(), B * C, h, w, int(scale),
              _stream())
        ctx.cfg = (B, C, h, w, int(scale))
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, h, w, scale = ctx.cfg
        dy = _chk(dy, "upsample_nearest: dy")
        dx = torch.empty((B, C, h, w), device=dy.device, dtype=torch.float32)
        _call("upsample_nearest_bwd", "cocos_upsample_nearest_bwd", dy.data_ptr(), dx.data_ptr(), B * C, h, w, scale,
              _stream())
        return dx, None


def upsample_nearest(x, scale: int):
    """F.interpolate(x, scale_factor=scale, mode='nearest') for integer scales (x [B,C,h,w] fp32, (w*scale) % 4 == 0)."""
    return _UpsampleNearest.apply(x, scale)



_HEAD_MODES = {m: _C["COCOS_WARP_HEAD_" + m.upper()] for m in ("nearest", "bilinear", "patch")}


class _WarpHeadModes(torch.autograd.Function):
    """The head of a row / column pass's output o [B,Ci+Cs,h*w] (correspondence.py:327, :334; K30: every flag set): warp_out by nearest /
    bilinear up-sampling of the Ci image channels or as the fold of non-overlapping patches, the Cs mask channels (if any) as a VIEW,
    optionally the image channels themselves as a view (`want_y`: the column pass's values under --warp_cycle_w) and the bilinear side
    output of inference --show_corr (`want_bi`, nearest mode).  Backward: ONE kernel (cocos_warp_head_bwd_ex) sums both gradients of
    the image channels — the adjoint of the up-sampling, as a fixed-order gather, and d y — next to d warp_mask (a gradient autograd
    did not deliver is NULL: zero), and leaves max|d o| and D = sum_c d o * o (fp64) for the K2 / K19 backward that consumes d o next —
    round 5 ran cocos_upsample_nearest_bwd, cocos_concat2_amax and cocos_rowdot_f64 for these."""

    @staticmethod
    def forward(ctx, o, n_img: int, h: int, w: int, down: int, mode: str, want_y: bool, want_bi: bool):
        o = _chk(o, "warp_head: o")
        B, C, N = o.shape
        m = _HEAD_MODES[mode]
        planes = n_img // (down * down) if mode == "patch" else n_img
        y = torch.empty((B, planes, h * down, w * down), device=o.device, dtype=torch.float32)
        y_bi = torch.empty_like(y) if want_bi else None
        _call("warp_head_fwd", "cocos_warp_head_fwd_ex", o.data_ptr(), y.data_ptr(), _ptr(y_bi), B, n_img, C, h, w, down, m, _stream())
        ctx.save_for_backward(o)
        ctx.cfg = (int(n_img), int(h), int(w), int(down), m)
        return (y, o[:, n_img:].view(B, C - n_img, h, w) if n_img < C else None, o[:, :n_img] if want_y else None, y_bi)

    @staticmethod
    def backward(ctx, g_img, g_mask, g_y, g_bi):
        o, = ctx.saved_tensors
        n_img, h, w, down, m = ctx.cfg
        B, C, N = o.shape
        g_img, g_mask, g_y, g_bi = (None if g is None else _chk(g, "warp_head: gradient") for g in (g_img, g_mask, g_y, g_bi))
        dout = torch.empty_like(o)
        drow = torch.empty((B, N), device=o.device, dtype=torch.float32)
        if g_bi is not None:        # (a loss on the inference side output: its adjoint first, then added like a second d y)
            t = torch.empty((B, n_img, N), device=o.device, dtype=torch.float32)
            o_img = o[:, :n_img].contiguous()
            _call("warp_head_bwd", "cocos_warp_head_bwd_ex", g_bi.data_ptr(), None, _ptr(g_y), o_img.data_ptr(),
                  t.data_ptr(), drow.data_ptr(), _zero_cell(o.device).data_ptr(), B, n_img, 0, h, w, down, _HEAD_MODES["bilinear"],
                  _stream())
            g_y = t
        cell = _zero_cell(o.device)
        _call("warp_head_bwd", "cocos_warp_head_bwd_ex", _ptr(g_img), _ptr(g_mask), _ptr(g_y), o.data_ptr(), dout.data_ptr(),
              drow.data_ptr(), cell.data_ptr(), B, n_img, C - n_img, h, w, down, m, _stream())
        if PRECISION == "f16x3":
            _remember_amax(dout, cell)
        _tls.known_rowdot = (weakref.ref(dout), dout._version, o.data_ptr(), drow)
        return dout, None, None, None, None, None, None, None


def warp_head_ok(o: torch.Tensor, n_img: int, h: int, w: int, down: int, mode: str = "nearest") -> bool:
    """Shapes cocos_warp_head_fwd_ex / _bwd_ex take: fp32 on the GPU, some image channels, grid width a multiple of 4; in patch mode the
    image channels are whole down x down patches.  (n_img == C: no mask channels.)"""
    return (mode in _HEAD_MODES and o.is_cuda and o.dtype == torch.float32 and o.dim() == 3 and 0 < n_img <= o.shape[1] and w % 4 == 0
            and o.shape[2] == h * w and o.shape[0] <= 65535 and down >= 1 and (mode != "patch" or n_img % (down * down) == 0)
            and (mode == "nearest" and n_img < o.shape[1] or o.is_contiguous()))


def warp_head(o, n_img: int, h: int, w: int, down: int, mode: str = "nearest", want_y: bool = False, want_bi: bool = False):
    """(warp_out, warp_mask or None[, y_view][, warp_out_bi]) of a row / column pass's output o [B,C,h*w]: see _WarpHeadModes.
    warp_out is [B,n_img,h*down,w*down] (mode 'nearest' | 'bilinear') or the fold [B,n_img/down^2,h*down,w*down]
    ('patch'); warp_mask [B,C-n_img,h,w] and y_view [B,n_img,h*w] are views of o."""
    if mode not in _HEAD_MODES:
        raise ValueError(f"warp_head: unknown mode {mode!r}")
    if want_bi and mode != "nearest":
        raise ValueError("warp_head: want_bi goes with mode='nearest' (the other modes' warp_out is the side output already)")
    res = _WarpHeadModes.apply(o, int(n_img), int(h), int(w), int(down), mode, bool(want_y), bool(want_bi))
    return res[:2] + ((res[2],) if want_y else ()) + ((res[3],) if want_bi else ())


def warp_values(img, seg_map, down: int, patch: bool = False):
    """torch.cat((F.avg_pool2d(img, down), F.interpolate(seg_map, scale_factor=1/down, mode='nearest')), 1) in one
    kernel (K14; correspondence.py:314, :318-319, :331-334): img [B,Ci,H,W], seg_map [B,Cs,H,W] or None -> [B,Ci+Cs,
    H/down,W/down].  patch=True (--warp_patch, :311): the image part is F.unfold(img, down, stride=down) instead, [B,Ci*down^2+Cs,
    H/down,W/down].  Forward only: the exemplar image and its label map are data (callers with gradients use torch)."""
    img = _chk(img, "warp_values: img")
    B, Ci, H, W = img.shape
    seg = None if seg_map is None else _chk(seg_map, "warp_values: seg_map")
    Cs = 0 if seg is None else seg.shape[1]
    if seg is not None and (seg.shape[0], seg.shape[2], seg.shape[3]) != (B, H, W):
        raise ValueError(f"warp_values: seg_map {tuple(seg.shape)} does not match img {tuple(img.shape)}")
    if patch:
        out = torch.empty((B, Ci * down * down + Cs, H // down, W // down), device=img.device, dtype=torch.float32)
        cell = _zero_cell(out.device) if PRECISION == "f16x3" else None
        _call("warp_values", "cocos_warp_values_patch_amax", img.data_ptr(), _ptr(seg), out.data_ptr(), B, Ci, Cs, H, W, int(down),
              _ptr(cell), _stream())
        if cell is not None:
            _remember_amax(out, cell)
        return out
    out = torch.empty((B, Ci + Cs, H // down, W // down), device=img.device, dtype=torch.float32)
    if PRECISION == "f16x3":      # max|V| as a by-product: the consumer (the K2 forward's f16 split of V) picks it up
        cell = _zero_cell(out.device)
        _call("warp_values", "cocos_warp_values_amax", img.data_ptr(), _ptr(seg), out.data_ptr(), B, Ci, Cs, H, W, int(down),
              cell.data_ptr(), _stream())
        _remember_amax(out, cell)
        return out
    _call("warp_values", "cocos_warp_values", img.data_ptr(), _ptr(seg), out.data_ptr(), B, Ci, Cs, H, W, int(down),
          _stream())
    return out


def concat_channels_amax(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """torch.cat((a, b), dim=1) of two fp32 CUDA tensors whose per-sample sizes are multiples of 4, with max|result| left for
    the consumer (the f16 split of the K2 backward's dout) — one kernel instead of a framework copy + a max pass."""
    a, b = _chk(a, "concat_channels_amax: a"), _chk(b, "concat_channels_amax: b")
    B = a.shape[0]
    na, nb = a.numel() // B, b.numel() // B
    if b.shape[0] != B or a.shape[2:] != b.shape[2:] or na % 4 or nb % 4 or a.data_ptr() % 16 or b.data_ptr() % 16:
        return torch.cat((a, b), dim=1)
    out = torch.empty((B, a.shape[1] + b.shape[1]) + tuple(a.shape[2:]), device=a.device, dtype=torch.float32)
    cell = _zero_cell(out.device) if PRECISION == "f16x3" else None
    _call("concat2_amax", "cocos_concat2_amax", a.data_ptr(), b.data_ptr(), out.data_ptr(), B, na, nb, _ptr(cell), _stream())
    if cell is not None:
        _remember_amax(out, cell)
    return out


# ------------------------------------------------------------------------------------------
# K13 InstanceNorm (+ residual) + PReLU of the ResidualBlocks   (correspondence.py:13-36)
# ------------------------------------------------------------------------------------------
INSTNORM_EPS = 1e-5   # nn.InstanceNorm2d default


#: planes above 128 x 128 (the adaptors' layer1 at the image size, the PatchGAN's first norm) take K34 (instnorm_prelu_split) in
#: producers.py / translation.py when True, the framework's InstanceNorm2d + leaky_relu when False.  Read at call time.  On by the
#: measurement of tools/instnorm_split_bench.py (0.19 against 0.31 ms forward + backward at [8, 64, 256, 256], ahead at
#: every shape).
INSTNORM_SPLIT = True


def _instnorm_split_workspace(x, planes: int, N: int) -> torch.Tensor:
    # (fp64 storage: the library wants the buffer 8-byte aligned whatever the allocator's granularity)
    return torch.empty((_lib.load().cocos_instnorm_prelu_split_workspace_floats(planes, N) + 1) // 2, device=x.device, dtype=torch.float64)


class _InstNormPReLU(torch.autograd.Function):
    """split = False: K13 (one workgroup per plane); True: K34 (instnorm_split.hip: a plane over several workgroups, the per-plane
    (mean, rstd) saved for the backward).  One Function: what leaves besides y and the gradients — the max|.| cells — is the same."""

    @staticmethod
    def forward(ctx, x, residual, weight, eps: float, split: bool = False):
        x = _chk(x, "instnorm_prelu: x")
        res = None if residual is None else _chk(residual, "instnorm_prelu: residual")
        w = _chk(weight, "instnorm_prelu: weight")
        if w.numel() != 1:
            raise ValueError("instnorm_prelu: nn.PReLU() with a single parameter expected")
        if res is not None and res.shape != x.shape:
            raise ValueError(f"instnorm_prelu: residual {tuple(res.shape)} vs x {tuple(x.shape)}")
        B, C = x.shape[:2]
        N = x.numel() // (B * C)
        y = torch.empty_like(x)
        stats = None
        # max|y| as a by-product: y is the next convolution's (or the projections') input, split with that scale
        cell = _zero_cell(x.device) if CONV_PRECISION == "f16x3" else None
        if split:
            stats = torch.empty(B * C, 2, device=x.device, dtype=torch.float32)       # (mean, rstd) per plane: the backward takes them
            ws = _instnorm_split_workspace(x, B * C, N)       # held by this name until the call below has launched what uses it
            _call("instnorm_prelu_split_fwd", "cocos_instnorm_prelu_split_fwd", x.data_ptr(), _ptr(res), w.data_ptr(), y.data_ptr(),
                  stats.data_ptr(), ws.data_ptr(), _ptr(cell), B * C, N, float(eps), _stream())
        elif cell is not None:
            part = torch.empty(B * C, device=x.device, dtype=torch.float32)       # one maximum per plane, reduced by the same call
            _call("instnorm_prelu_fwd", "cocos_instnorm_prelu_fwd_amax", x.data_ptr(), _ptr(res), w.data_ptr(), y.data_ptr(), cell.data_ptr(),
                  part.data_ptr(), B * C, N, float(eps), _stream())
        else:
            _call("instnorm_prelu_fwd", "cocos_instnorm_prelu_fwd", x.data_ptr(), _ptr(res), w.data_ptr(), y.data_ptr(),
                  B * C, N, float(eps), _stream())
        if cell is not None:
            _remember_amax(y, cell, weak=True)
        ctx.save_for_backward(x, res, w, stats)
        ctx.eps = float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, res, w, stats = ctx.saved_tensors
        dy = _chk(dy, "instnorm_prelu: dy")
        B, C = x.shape[:2]
        N = x.numel() // (B * C)
        need_x, need_r, need_w = ctx.needs_input_grad[:3]
        dx = torch.empty_like(x) if need_x else None
        dr = torch.empty_like(x) if (need_r and res is not None) else None
        dap = dw = None
        if need_w:
            # the weight's gradient is ONE number summed over every element of the layer, with cancelling terms: fp64 from the
            # products to the last addition (cocos_instnorm_prelu_bwd_f64; in fp32 it was up to 90x further from fp64 than the framework's)
            dw = torch.empty(1, device=x.device, dtype=torch.float32)
        # max|dx| as a by-product: dx is the output gradient of the convolution in front of the norm, whose backward splits it next
        cell = _zero_cell(x.device) if (dx is not None and CONV_PRECISION == "f16x3") else None
        if stats is not None:
            if dx is not None or dr is not None or dw is not None:
                ws = _instnorm_split_workspace(x, B * C, N)   # (the fp64 partials of d weight live in it)
                _call("instnorm_prelu_split_bwd", "cocos_instnorm_prelu_split_bwd", x.data_ptr(), _ptr(res), w.data_ptr(), dy.data_ptr(),
                      stats.data_ptr(), _ptr(dx), _ptr(dr), _ptr(dw), ws.data_ptr(), _ptr(cell), B * C, N, ctx.eps, _stream())
        else:
            if need_w:
                dap = torch.empty(B * C, device=x.device, dtype=torch.float64)
            if cell is not None:
                part = torch.empty(B * C, device=x.device, dtype=torch.float32)
                _call("instnorm_prelu_bwd", "cocos_instnorm_prelu_bwd_amax", x.data_ptr(), _ptr(res), w.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                      _ptr(dr), _ptr(dap), _ptr(dw), cell.data_ptr(), part.data_ptr(), B * C, N, ctx.eps, _stream())
            elif need_w:
                _call("instnorm_prelu_bwd", "cocos_instnorm_prelu_bwd_f64", x.data_ptr(), _ptr(res), w.data_ptr(), dy.data_ptr(),
                      _ptr(dx), _ptr(dr), dap.data_ptr(), dw.data_ptr(), B * C, N, ctx.eps, _stream())
            else:
                _call("instnorm_prelu_bwd", "cocos_instnorm_prelu_bwd", x.data_ptr(), _ptr(res), w.data_ptr(), dy.data_ptr(),
                      _ptr(dx), _ptr(dr), None, B * C, N, ctx.eps, _stream())
        if cell is not None:
            _remember_amax(dx, cell, weak=True)
        return dx, dr, (dw.reshape(w.shape) if need_w else None), None, None


def instnorm_prelu(x, residual, weight, eps: float = INSTNORM_EPS):
    """prelu(InstanceNorm2d(x) [+ residual], weight) for x [B,C,h,w]: nn.InstanceNorm2d(affine=False) statistics per
    (sample, channel) plane, nn.PReLU() with one parameter."""
    return _InstNormPReLU.apply(x, residual, weight, eps, False)


def instnorm_prelu_split(x, residual, weight, eps: float = INSTNORM_EPS):
    """K34 (instnorm_split.hip): `instnorm_prelu` for planes of any size — every (sample, channel) plane is cut into slices of 16384
    positions, one workgroup each, so a [B, 64, 256, 256] activation fills the device instead of running one workgroup per plane.
    Saves x, the residual, the weight and the per-plane (mean, rstd)."""
    return _InstNormPReLU.apply(x, residual, weight, eps, True)


# ------------------------------------------------------------------------------------------
# K35  3x3 convolution of a one-hot label map as table look-ups   (label_conv.hip; pix2pix_model.py:177-187 builds the map)
# ------------------------------------------------------------------------------------------
def labels_one_hot(label_map: torch.Tensor, nc: int):
    """(one-hot fp32 [B,nc,H,W], index int32 [B,H,W]) of an integer label map [B,1,H,W] on the GPU: `zeros.scatter_(1, label_map, 1.0)`
    with every element written by one kernel, and the compact index map the label route reads.  A label outside [0, nc) gives an
    all-zero column and index -1 (scatter_ raises there)."""
    if not label_map.is_cuda:
        raise _lib.CocosHipError("labels_one_hot: expected a CUDA/HIP tensor; cocosnet_amd.labels.one_hot handles host tensors")
    if label_map.dim() != 4 or label_map.shape[1] != 1 or label_map.dtype != torch.int64:
        raise ValueError(f"labels_one_hot: int64 [B,1,H,W] expected, got {label_map.dtype} {tuple(label_map.shape)}")
    lab = label_map.contiguous()
    B, _, H, W = lab.shape
    seg = torch.empty((B, int(nc), H, W), device=lab.device, dtype=torch.float32)
    index = torch.empty((B, H, W), device=lab.device, dtype=torch.int32)
    _call("labels_one_hot", "cocos_labels_one_hot", lab.data_ptr(), seg.data_ptr(), index.data_ptr(), B, int(nc), H, W, _stream())
    return seg, index


def label_conv_ok(weight, index, sample: int = 1, reflect: int = 0, stride=1, padding=1, dilation=1, nc=None) -> bool:
    """The ONE predicate of the label route: weight fp32 [Cout, nc, 3, 3] on the GPU with Cout % 16 == 0 and 1 <= nc <= 32767;
    stride 1, dilation 1; padding 1 (zeros) or ReflectionPad2d(1) in front of padding 0 with an output grid of 2x2 or more; the
    index map [B, Hs, Ws] int32 on the same device with Hs % sample == 0 and Ws % sample == 0.  Anything else: the dense route."""
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if not (torch.is_tensor(weight) and weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 4):
        return False
    Cout, Cin, KH, KW = weight.shape
    if (KH, KW) != (3, 3) or Cout % 16 != 0 or not 1 <= Cin <= 32767 or (nc is not None and int(nc) != Cin):
        return False
    if pair(stride) != (1, 1) or pair(dilation) != (1, 1) or isinstance(padding, str):
        return False
    if not (torch.is_tensor(index) and index.is_cuda and index.device == weight.device and index.dtype == torch.int32 and index.dim() == 3):
        return False
    sample, reflect = int(sample), int(reflect)
    Hs, Ws = index.shape[1:]
    if sample < 1 or Hs < 1 or Ws < 1 or Hs % sample or Ws % sample:
        return False
    if reflect == 0:
        return pair(padding) == (1, 1)
    return reflect == 1 and pair(padding) == (0, 0) and Hs // sample >= 2 and Ws // sample >= 2


def label_conv_table(weight: torch.Tensor) -> torch.Tensor:
    """W [Cout, nc, 3, 3] -> the tap-major table Wt [9, nc, Cout] of K35"""
    w = _chk(weight, "label_conv_table: weight")
    Cout, nc = w.shape[:2]
    table = torch.empty((9, nc, Cout), device=w.device, dtype=torch.float32)
    _call("label_conv_table", "cocos_label_conv_table", w.data_ptr(), table.data_ptr(), Cout, nc, _stream())
    return table


class _LabelConv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, index, weight, bias, nc: int, sample: int, reflect: int, relu: bool, prepared=None):
        weight = _chk(weight, "label_conv3x3: weight")
        bb = None if bias is None else _chk(bias, "label_conv3x3: bias")
        if not label_conv_ok(weight, index, sample, reflect, 1, 0 if reflect else 1, 1, nc):
            raise ValueError(f"label_conv3x3: weight {tuple(weight.shape)} / index {tuple(index.shape)} {index.dtype} / nc {nc} / sample "
                             f"{sample} / reflect {reflect} is outside ops.label_conv_ok")
        index = index.contiguous()
        Cout = weight.shape[0]
        B, Hs, Ws = index.shape
        table = prepared.label_table() if prepared is not None else label_conv_table(weight)
        y = torch.empty((B, Cout, Hs // sample, Ws // sample), device=weight.device, dtype=torch.float32)
        # max|y| as a by-product, as the other producer kernels leave it: a convolution that reads y directly finds the cell
        cell = _zero_cell(y.device) if CONV_PRECISION == "f16x3" else None
        _call("label_conv3x3_fwd", "cocos_label_conv3x3_fwd", index.data_ptr(), table.data_ptr(), _ptr(bb), y.data_ptr(), _ptr(cell),
              B, Hs, Ws, int(sample), int(reflect), int(bool(relu)), int(nc), Cout, _stream())
        _glue_remember(y, cell)           # (weak: the entry must not keep the activation alive)
        ctx.save_for_backward(index, *((y,) if relu else ()))
        ctx.cfg = (int(nc), int(sample), int(reflect), bool(relu), tuple(weight.shape), bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        index, *rest = ctx.saved_tensors
        nc, sample, reflect, relu, wshape, has_bias = ctx.cfg
        ysaved = rest[0] if relu else None
        need_w, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2] and has_bias
        dw = db = None
        if need_w or need_b:
            dy = _chk(dy, "label_conv3x3: dy")
            B, Hs, Ws = index.shape
            Cout = wshape[0]
            dw = torch.empty(wshape, device=dy.device, dtype=torch.float32)
            db = torch.empty(Cout, device=dy.device, dtype=torch.float32) if need_b else None
            n = _lib.load().cocos_label_conv3x3_bwd_workspace_floats(B, Hs // sample, Ws // sample, nc, Cout)
            ws = torch.empty(n, device=dy.device, dtype=torch.float32)      # held by this name until the call below has launched
            _call("label_conv3x3_bwd", "cocos_label_conv3x3_bwd", index.data_ptr(), dy.data_ptr(), _ptr(ysaved), dw.data_ptr(), _ptr(db),
                  ws.data_ptr(), B, Hs, Ws, sample, reflect, nc, Cout, _stream())
            if not need_w:
                dw = None
        return None, dw, db, None, None, None, None, None


def label_conv3x3(index, weight, bias, nc: int, sample: int = 1, reflect: int = 0, relu: bool = False, prepared=None):
    """conv2d(one_hot(index), weight, bias) for a 3x3 kernel as nine table look-ups per output pixel (K35):
    `index` int32 [B, Hs, Ws] (-1: no class) is read at every `sample`-th pixel of both axes — the nearest resize to
    (Hs / sample) x (Ws / sample) — with zero padding 1 (`reflect` = 0) or ReflectionPad2d(1) (`reflect` = 1), optionally followed by
    ReLU.  Exact fp32 sums of at most ten numbers.  Gradients reach weight and bias only (bit-reproducible: fixed order, no atomics).
    Saves the index map and, with relu, the output.  `prepared`: the layer's frozen record (its tap table is made once)."""
    return _LabelConv3x3.apply(index, weight, bias, int(nc), int(sample), int(reflect), bool(relu), prepared)


# ------------------------------------------------------------------------------------------
# K21  torch.nn.utils.spectral_norm's weight: power iteration + W / sigma, and its backward   (spectral_norm.hip)
# ------------------------------------------------------------------------------------------
class _SpectralWeight(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, u, v, power_iteration: bool, eps: float):
        w = _chk(weight, "spectral_weight: weight")
        R = w.shape[0]
        K = w.numel() // R
        if u.shape != (R,) or v.shape != (K,) or not (u.is_contiguous() and v.is_contiguous()):
            raise ValueError(f"spectral_weight: weight {tuple(w.shape)} with u {tuple(u.shape)} / v {tuple(v.shape)}")
        lib = _lib.load()
        wsn = torch.empty_like(w)
        sigma = torch.empty(1, device=w.device, dtype=torch.float32)
        ws = torch.empty(lib.cocos_spectral_weight_workspace_floats(R, K), device=w.device, dtype=torch.float32)
        # max|W / sigma| as a by-product: the convolution that consumes the weight splits it with it — only the f16x3
        # flavour does (bf16 planes carry no scale: the entries would pile up in the table and evict useful ones)
        cell = _zero_cell(w.device) if CONV_PRECISION != "bf16" else None
        _call("spectral_weight_fwd", "cocos_spectral_weight_fwd", w.data_ptr(), u.data_ptr(), v.data_ptr(), wsn.data_ptr(), sigma.data_ptr(),
              _ptr(cell), ws.data_ptr(), R, K, float(eps), int(bool(power_iteration)), _stream())
        if power_iteration:
            # the kernel wrote u and v through raw pointers, which autograd cannot see: whatever watches (data_ptr, _version) of the
            # buffers — a frozen record's signature (inference.py), a max|.| cell, operand planes — must find them changed
            torch.autograd.graph.increment_version([u, v])
        if cell is not None:
            _remember_amax(wsn, cell)
        # the vectors sigma was taken with: copies, because the next forward (GAN training: D(real), D(fake)) updates the buffers in place
        ctx.save_for_backward(w, u.clone(), v.clone(), sigma)
        return wsn

    @staticmethod
    def backward(ctx, g):
        w, u, v, sigma = ctx.saved_tensors
        g = _chk(g, "spectral_weight: grad")
        R = w.shape[0]
        K = w.numel() // R
        dw = torch.empty_like(w)
        ws = torch.empty(1024, device=w.device, dtype=torch.float32)
        _call("spectral_weight_bwd", "cocos_spectral_weight_bwd", g.data_ptr(), w.data_ptr(), u.data_ptr(), v.data_ptr(), sigma.data_ptr(),
              dw.data_ptr(), ws.data_ptr(), R, K, _stream())
        return dw, None, None, None, None


def spectral_weight(weight, u, v, power_iteration: bool, eps: float = 1e-12):
    """`SpectralNorm.compute_weight` of torch.nn.utils.spectral_norm (dim 0, one power iteration): u, v updated in place when
    `power_iteration`, returns weight / (u . W v) with the framework's gradient (through sigma as well) — K21."""
    return _SpectralWeight.apply(weight, u, v, bool(power_iteration), float(eps))


#: softmax_attention on the fused kernels for K < 256 as well (channels zero-padded to 256); "0": the materialised family
ATTENTION_FUSED = True


def softmax_attention(q, k, v, scale: float = 1.0):
    """out[b,c,i] = sum_j softmax_j(scale * <q[b,:,i], k[b,:,j]>) v[b,c,j] for any channel count K — the QK^T ->
    softmax -> PV op class of the path (`Attention.forward`, architecture.py:114-127, has K =
    ch/8 = 32..64, HW/4 keys and ch/2 value channels).

    K <= 256 on the split flavour: the FUSED kernels (K2) — nothing HWxHW is materialised in inference, training keeps the
    saved logits like the correspondence itself.  q / k are raw 1x1-conv outputs here, not unit-norm columns: their operand
    planes get device-side power-of-two scales from max|q|, max|k| (no fixed 2^4: ADVICE r2) and the kernels run in their
    magnitude-free flavour (exact exponent differences at any |logit|).  K < 256 sits zero-padded in the 256-channel planes
    the kernels are built for, and their K = 32 / K = 64 instantiations leave out the matrix steps, fragment reads and
    fetches of the padding; the two backward GEMMs (M = K resp. Cv rows: too few tiles for 256 CUs) split their reduction.
    netG's shape (B=4, K=32, 128x128 queries, 64x64 keys, Cv=128): 2.2 ms fwd+bwd against 6.3 ms materialised (round 3: 3.0;
    tools/attention_bench.py).  Everything else: the materialised family on the same MFMA GEMMs (K3 -> K4 -> K5)."""
    B, K, Nq = q.shape
    Nk = k.shape[2]
    keep = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)
    if (ATTENTION_FUSED and K <= FUSED_K and q.is_cuda and q.dtype == torch.float32
            and corr_split_ok(B, FUSED_K, Nq, Nk, v.shape[1], keep)):
        return corr_softmax_warp(q, k, v, scale, operand_amax=True)
    if K == FUSED_K and q.is_cuda and q.dtype == torch.float32:
        # the split path is not available (COCOS_PRECISION=fp32, odd Nq / Nk): K = 256 still takes the FUSED exact-fp32
        # kernels, which materialise nothing either (this branch had been lost — a B x Nq x Nk matrix at 4096^2)
        return corr_softmax_warp(q, k, v, scale, precision="fp32")
    return warp_materialized(row_softmax(corr_materialize(q, k, scale)), v)


# ------------------------------------------------------------------------------------------
# K15 row reductions of the contextual loss   (ContextualLoss.py:121-133)
# ------------------------------------------------------------------------------------------
class _ContextualRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cosm, h: float, eps: float):
        cosm = _chk(cosm, "contextual_rows: cos")
        cols = cosm.shape[-1]
        rows = cosm.numel() // cols
        cx = torch.empty(cosm.shape[:-1], device=cosm.device, dtype=torch.float32)
        _call("contextual_rows_fwd", "cocos_contextual_rows_fwd", cosm.data_ptr(), cx.data_ptr(), rows, cols, float(h),
              float(eps), _stream())
        ctx.save_for_backward(cosm)
        ctx.cfg = (float(h), float(eps))
        return cx

    @staticmethod
    def backward(ctx, dcx):
        (cosm,) = ctx.saved_tensors
        h, eps = ctx.cfg
        dcx = _chk(dcx, "contextual_rows: dcx")
        cols = cosm.shape[-1]
        dcos = torch.empty_like(cosm)
        _call("contextual_rows_bwd", "cocos_contextual_rows_bwd", cosm.data_ptr(), dcx.data_ptr(), dcos.data_ptr(),
              cosm.numel() // cols, cols, h, eps, _stream())
        return dcos, None, None


def contextual_rows(cosm, h: float = 0.1, eps: float = 1e-3):
    """cx[..., i] = max_j A[..., i, j] of the contextual affinity A built from the cosine matrix cosm [..., N, M <= 4096]
    (d = 1 - cos, d / (min_j d + eps), exp((1 - .) / h), row-normalised): ContextualLoss.py:121-132 in one pass."""
    return _ContextualRows.apply(cosm, h, eps)


# ------------------------------------------------------------------------------------------
# K22 the contextual loss without its [N, N] matrices   (ContextualLoss.py:121-133; contextual_fused_f16x3.hip)
# ------------------------------------------------------------------------------------------
CX_TILE = 128     # positions per workgroup / inner tile of K22: the planes are padded to whole tiles


def _cx_pad_positions(x: torch.Tensor) -> torch.Tensor:
    n = x.shape[2]
    npad = (n + CX_TILE - 1) // CX_TILE * CX_TILE
    return x if npad == n else torch.nn.functional.pad(x, (0, npad - n))


class _ContextualCx(torch.autograd.Function):
    """cx[b,i] = max_j A_ij of the contextual affinity of two sets of normalised features xn [B,C,Nq], yn [B,C,Nk]:
    1 / sum_j exp((cos_ij - m_i) tau_i).  Forward: one launch of K22 (two sweeps over the keys).  Backward: one launch per side
    (the cosine tiles are recomputed) + the argmax column's term as a gather (d xn) / scatter-add (d yn).  Nothing [Nq, Nk]
    exists at any point; saved for the backward: the operand planes (the size of the features) and four numbers per query."""

    @staticmethod
    def forward(ctx, xn, yn, h: float, eps: float):
        xn, yn = _chk(xn, "contextual_cx: xn"), _chk(yn, "contextual_cx: yn")
        B, C, Nq = xn.shape
        if yn.dim() != 3 or yn.shape[:2] != (B, C):
            raise ValueError(f"contextual_cx: shape mismatch xn{tuple(xn.shape)} yn{tuple(yn.shape)}")
        Nk = yn.shape[2]
        kp = (C + 31) // 32 * 32
        xp, yp = _cx_pad_positions(xn), _cx_pad_positions(yn)
        xa, ya = absmax(xn), absmax(yn)
        xh, xl, xs = split_f16(xp, True, cpad=kp, amax=xa)          # [B, Nqp, Kp]
        yh, yl, ys = split_f16(yp, True, cpad=kp, amax=ya)
        f32 = dict(device=xn.device, dtype=torch.float32)
        m, S, U = (torch.empty((B, Nq), **f32) for _ in range(3))
        jstar = torch.empty((B, Nq), device=xn.device, dtype=torch.int32)
        _call("contextual_cx_fwd", "cocos_contextual_cx_fwd_f16x3", xh.data_ptr(), xl.data_ptr(), yh.data_ptr(), yl.data_ptr(),
              xs.data_ptr(), ys.data_ptr(), m.data_ptr(), S.data_ptr(), U.data_ptr(), jstar.data_ptr(), B, Nq, Nk, xp.shape[2],
              yp.shape[2], kp, float(h), float(eps), _stream())
        ctx.save_for_backward(xn, yn, m, S, U, jstar)
        ctx.planes = (xh, xl, xs, xa, yh, yl, ys, ya)
        ctx.cfg = (float(h), float(eps))
        return 1.0 / S

    @staticmethod
    def backward(ctx, dcx):
        xn, yn, m, S, U, jstar = ctx.saved_tensors
        xh, xl, xs, xa, yh, yl, ys, ya = ctx.planes
        h, eps = ctx.cfg
        dcx = _chk(dcx, "contextual_cx: dcx")
        B, C, Nq = xn.shape
        Nk = yn.shape[2]
        kp, nqp, nkp = xh.shape[2], xh.shape[1], yh.shape[1]
        need_x, need_y = ctx.needs_input_grad[:2]
        # per query: the coefficient of e_ij, the temperature and the argmax column's extra term — one small launch
        f32 = dict(device=xn.device, dtype=torch.float32)
        a, t2, extra = (torch.empty((B, Nq), **f32) for _ in range(3))
        a_amax = _zero_cell(xn.device)
        st = _stream()
        _call("contextual_cx_coeffs", "cocos_contextual_cx_coeffs", dcx.data_ptr(), S.data_ptr(), U.data_ptr(), m.data_ptr(), a.data_ptr(),
              t2.data_ptr(), extra.data_ptr(), a_amax.data_ptr(), B * Nq, h, eps, st)
        dx = dy = None
        if need_x:     # rows = queries, inner = keys, values = yn (channel-major), (m, t) and beta = a per row; the argmax column's
            vh, vl, vs = split_f16(_cx_pad_positions(yn), False, amax=ya)          # term is gathered from yn in the epilogue
            dx = torch.empty_like(xn)
            _call("contextual_cx_bwd", "cocos_contextual_cx_bwd_f16x3", xh.data_ptr(), xl.data_ptr(), yh.data_ptr(), yl.data_ptr(),
                  vh.data_ptr(), vl.data_ptr(), xs.data_ptr(), ys.data_ptr(), vs.data_ptr(), None, m.data_ptr(), t2.data_ptr(), None, None,
                  a.data_ptr(), yn.data_ptr(), jstar.data_ptr(), extra.data_ptr(), dx.data_ptr(), B, Nq, Nk, nqp, nkp, kp, C, 1, 1.0, st)
        if need_y:     # rows = keys, inner = queries, values = xn, (m, t) and alpha = a / max|a| per inner position
            vh, vl, vs = split_f16(_cx_pad_positions(xn), False, amax=xa)
            dy = torch.empty_like(yn)
            _call("contextual_cx_bwd", "cocos_contextual_cx_bwd_f16x3", yh.data_ptr(), yl.data_ptr(), xh.data_ptr(), xl.data_ptr(),
                  vh.data_ptr(), vl.data_ptr(), ys.data_ptr(), xs.data_ptr(), vs.data_ptr(), a_amax.data_ptr(), m.data_ptr(),
                  t2.data_ptr(), a.data_ptr(), a_amax.data_ptr(), None, None, None, None, dy.data_ptr(), B, Nk, Nq, nkp, nqp, kp, C, 0, 1.0, st)
            # the argmax column's term lands on key j*_i: a scatter-add over the queries (the exemplar side is detached by the
            # reference's caller, pix2pix_model.py:197-201: this branch is for completeness)
            dy.scatter_add_(2, jstar.long().unsqueeze(1).expand(B, C, Nq), extra.unsqueeze(1) * xn)
        return dx, dy, None, None


def contextual_cx(xn, yn, h: float = 0.1, eps: float = 1e-3):
    """cx [B,Nq] = max_j A_ij of the contextual affinity (ContextualLoss.py:121-132) of normalised features xn [B,C,Nq],
    yn [B,C,Nk] — any Nq, Nk, C; no [Nq, Nk] tensor in HBM, forward or backward (K22)."""
    return _ContextualCx.apply(xn, yn, float(h), float(eps))


# ------------------------------------------------------------------------------------------
# K27  the glue of the fixed VGG19: preprocess, ReLU, ReLU + 2x2 pool   (correspondence.py:79-146, util/util.py:45-54)
# ------------------------------------------------------------------------------------------
def _glue_cell(device):
    """A max|.| cell for a K27 output that a K16 layer splits next, or None where nothing reads it (COCOS_CONV=bf16 splits nothing,
    'torch' runs the framework's convolutions)."""
    return _zero_cell(device) if CONV_PRECISION == "f16x3" else None


def _glue_remember(t, cell):
    if cell is not None:
        _remember_amax(t, cell, weak=True)


class _VggPreprocess(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, normal_correct: bool):
        x = _chk(x, "vgg_preprocess: x")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"vgg_preprocess: expected an RGB batch [B, 3, H, W], got {tuple(x.shape)}")
        B, _, H, W = x.shape
        y = torch.empty_like(x)
        cell = _glue_cell(x.device)
        _call("vgg_preprocess", "cocos_vgg_preprocess_fwd", x.data_ptr(), y.data_ptr(), _ptr(cell), B, H, W, int(normal_correct), _stream())
        _glue_remember(y, cell)
        ctx.cfg = (B, H, W, int(normal_correct))
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _chk(dy, "vgg_preprocess: dy")
        dx = torch.empty_like(dy)
        _call("vgg_preprocess", "cocos_vgg_preprocess_bwd", dy.data_ptr(), dx.data_ptr(), *ctx.cfg, _stream())
        return dx, None


def vgg_preprocess(x: torch.Tensor, normal_correct: bool = False) -> torch.Tensor:
    """util.vgg_preprocess (util/util.py:45-54) in one pass, bitwise: ((x + 1) / 2 when normal_correct), RGB -> BGR, minus the
    reference's mean, x 255.  Leaves max|y| for the first convolution."""
    return _VggPreprocess.apply(x, bool(normal_correct))


class _Relu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y):
        y = _chk(y, "relu: y")
        r = torch.empty_like(y)
        cell = _glue_cell(y.device)
        _call("relu", "cocos_relu_fwd", y.data_ptr(), r.data_ptr(), _ptr(cell), y.numel(), _stream())
        _glue_remember(r, cell)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(r)
        return r

    @staticmethod
    def backward(ctx, dr):
        r, = ctx.saved_tensors
        dr = _chk(dr, "relu: dr")
        dy = torch.empty_like(r)
        cell = _glue_cell(r.device)
        _call("relu", "cocos_relu_bwd", dr.data_ptr(), r.data_ptr(), dy.data_ptr(), _ptr(cell), r.numel(), _stream())
        _glue_remember(dy, cell)
        return dy


def relu(y: torch.Tensor) -> torch.Tensor:
    """F.relu(y), bitwise (NaN kept), out of place; leaves max|r| for the next convolution and, backward, max|dy| for its own."""
    return _Relu.apply(y)


class _ReluPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, mode: int, keep_r: bool):
        y = _chk(y, "relu_pool2: y")
        if y.dim() != 4:
            raise ValueError(f"relu_pool2: expected [B, C, H, W], got {tuple(y.shape)}")
        B, C, H, W = y.shape
        p = y.new_empty((B, C, H // 2, W // 2))
        r = torch.empty_like(y) if keep_r else None
        cell = _glue_cell(y.device)
        _call("relu_pool2", "cocos_relu_pool2_fwd", y.data_ptr(), _ptr(r), p.data_ptr(), _ptr(cell), B * C, H, W, mode, _stream())
        _glue_remember(p, cell)
        if ctx.needs_input_grad[0]:
            # the backward recomputes the mask and the arg-max from relu(src): r where it exists, else the pre-activation y
            ctx.save_for_backward(r if keep_r else y)
        ctx.cfg = (mode, keep_r)
        ctx.set_materialize_grads(False)     # an output the loss does not reach costs no zero-filled gradient
        return (r, p) if keep_r else p

    @staticmethod
    def backward(ctx, *grads):
        src, = ctx.saved_tensors
        mode, keep_r = ctx.cfg
        dr, dp = grads if keep_r else (None, grads[0])
        if dr is None and dp is None:
            return None, None, None
        dr = None if dr is None else _chk(dr, "relu_pool2: dr")
        dp = None if dp is None else _chk(dp, "relu_pool2: dp")
        B, C, H, W = src.shape
        dy = torch.empty_like(src)
        cell = _glue_cell(src.device)
        _call("relu_pool2", "cocos_relu_pool2_bwd", src.data_ptr(), _ptr(dr), _ptr(dp), dy.data_ptr(), _ptr(cell), B * C, H, W, mode,
              _stream())
        _glue_remember(dy, cell)
        return dy, None, None


def relu_pool2(y: torch.Tensor, mode: str = "max", keep_r: bool = False):
    """p = F.max_pool2d(F.relu(y), 2, 2) (mode "max") or F.avg_pool2d(F.relu(y), 2, 2) ("avg"), bitwise, from one read of y;
    returns (r, p) with r = F.relu(y) when keep_r, else p alone.  No index tensor: the backward recomputes the window's arg-max.
    Leaves max|p| for the next convolution and, backward, max|dy| for the one that produced y."""
    if mode not in ("max", "avg"):
        raise ValueError(f"relu_pool2: mode {mode!r}: expected 'max' or 'avg'")
    return _ReluPool2.apply(y, 0 if mode == "max" else 1, bool(keep_r))


# ------------------------------------------------------------------------------------------
# K28  the loss block: pair (L1 / MSE) groups, GANLoss over a prediction list, the warp-mask NLL
#      (pix2pix_model.py:205-296, util/util.py:36-43, networks/loss.py:15-97)
# ------------------------------------------------------------------------------------------
#: widest group one launch takes (COCOS_PAIR_LOSS_MAX_SEGMENTS / COCOS_GAN_LOSS_MAX_TENSORS of include/cocos_hip.h)
PAIR_LOSS_MAX_SEGMENTS = _C["COCOS_PAIR_LOSS_MAX_SEGMENTS"]
GAN_LOSS_MAX_TENSORS = _C["COCOS_GAN_LOSS_MAX_TENSORS"]
#: GANLoss.loss's cases -> the kernel's mode (COCOS_GAN_* of include/cocos_hip.h)
GAN_MODES = {m: _C["COCOS_GAN_" + m.upper()] for m in ("hinge_d_real", "hinge_d_fake", "neg_mean", "mean", "ls", "bce")}


def _loss_chk(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype:
        what = f"{t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise _lib.CocosHipError(f"{name}: expected a {dtype} CUDA/HIP tensor, got {what}; the loss kernels have no CPU fallback")
    return t.contiguous()


def _table(ctype, values):
    return (ctype * len(values))(*values)


def _pair_parse(spec, tensors, name="pair_loss"):
    """(a, b, w) lists of the contiguous tensors of a flat argument list; every one of them is referenced by the returned lists
    until the caller drops them — after the launch is queued."""
    A, Bs, Ws, it = [], [], [], 0
    for has_b, has_w, _, _ in spec:
        A.append(_loss_chk(tensors[it], f"{name}: a"))
        it += 1
        Bs.append(_loss_chk(tensors[it], f"{name}: b") if has_b else None)
        it += int(has_b)
        Ws.append(_loss_chk(tensors[it], f"{name}: w") if has_w else None)
        it += int(has_w)
    return A, Bs, Ws


class _PairLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, *tensors):
        A, Bs, Ws = _pair_parse(spec, tensors)
        nseg = len(spec)
        n = [a.numel() for a in A]
        inner = []
        for a, b, w in zip(A, Bs, Ws):
            if b is not None and b.shape != a.shape:
                raise ValueError(f"pair_loss: a {tuple(a.shape)} and b {tuple(b.shape)} differ")
            if w is not None and (a.dim() < 1 or a.shape[0] == 0 or w.numel() != a.shape[0]):
                raise ValueError(f"pair_loss: {w.numel()} sample weights for a {tuple(a.shape)}")
            inner.append(a.numel() // a.shape[0] if w is not None and a.numel() else a.numel())
        n_t, in_t = _table(ctypes.c_longlong, n), _table(ctypes.c_longlong, inner)
        c1_t, c2_t = _table(ctypes.c_float, [sp[2] for sp in spec]), _table(ctypes.c_float, [sp[3] for sp in spec])
        slots = _lib.load().cocos_loss_partials(nseg, n_t)
        dev = A[0].device
        partials = torch.empty(max(2 * slots, 2), device=dev, dtype=torch.float64)
        out = torch.empty((nseg + 1, 2), device=dev, dtype=torch.float32)
        _call("pair_loss", "cocos_pair_loss_fwd", nseg, _table(ctypes.c_void_p, [a.data_ptr() for a in A]),
              _table(ctypes.c_void_p, [_ptr(b) for b in Bs]), _table(ctypes.c_void_p, [_ptr(w) for w in Ws]), n_t, in_t, c1_t, c2_t,
              partials.data_ptr(), out.data_ptr(), _stream())
        ctx.save_for_backward(*A, *[b for b in Bs if b is not None], *[w for w in Ws if w is not None])
        ctx.spec = spec
        return out

    @staticmethod
    def backward(ctx, gout):
        spec, nseg = ctx.spec, len(ctx.spec)
        saved = list(ctx.saved_tensors)
        A, rest = saved[:nseg], saved[nseg:]
        Bs = [rest.pop(0) if sp[0] else None for sp in spec]
        Ws = [rest.pop(0) if sp[1] else None for sp in spec]
        gout = _loss_chk(gout, "pair_loss: gout")
        pos, it = [], 1                                   # position of every a among forward's arguments
        for has_b, has_w, _, _ in spec:
            pos.append(it)
            it += 1 + int(has_b) + int(has_w)
        dA = [torch.empty_like(a) if ctx.needs_input_grad[p] else None for a, p in zip(A, pos)]
        n = [a.numel() for a in A]
        inner = [a.numel() // a.shape[0] if w is not None else a.numel() for a, w in zip(A, Ws)]
        _call("pair_loss", "cocos_pair_loss_bwd", nseg, _table(ctypes.c_void_p, [a.data_ptr() for a in A]),
              _table(ctypes.c_void_p, [_ptr(b) for b in Bs]), _table(ctypes.c_void_p, [_ptr(w) for w in Ws]),
              _table(ctypes.c_void_p, [_ptr(d) for d in dA]), _table(ctypes.c_longlong, n), _table(ctypes.c_longlong, inner),
              _table(ctypes.c_float, [sp[2] for sp in spec]), _table(ctypes.c_float, [sp[3] for sp in spec]), gout.data_ptr(), _stream())
        grads = [None] * it
        for p, d in zip(pos, dA):
            grads[p] = d
        return tuple(grads)


def pair_loss(segments) -> torch.Tensor:
    """One launch over up to 16 segments `(a, b, w, c_l1, c_mse)`: segment s contributes c_l1 * mean(w[sample] * |a - b|) and
    c_mse * mean((a - b)^2); b None = 0, w None = 1 (w: one weight per sample of a's leading dimension).  Returns out
    [nseg + 1, 2] fp32: (L1 term, MSE term) per segment and their sums over the segments in the last row.  fp64 sums,
    bitwise reproducible, nothing tensor-sized saved; only the a's receive gradients (K28)."""
    segments = list(segments)
    if not 1 <= len(segments) <= PAIR_LOSS_MAX_SEGMENTS:
        raise ValueError(f"pair_loss: {len(segments)} segments (1 ... {PAIR_LOSS_MAX_SEGMENTS})")
    spec, flat = [], []
    for a, b, w, c1, c2 in segments:
        spec.append((b is not None, w is not None, float(c1), float(c2)))
        flat += [t.detach() if i else t for i, t in enumerate((a, b, w)) if t is not None]
    return _PairLoss.apply(tuple(spec), *flat)


class _GanLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mode, label, *xs):
        X = [_loss_chk(x, "gan_loss: x") for x in xs]
        n_t = _table(ctypes.c_longlong, [x.numel() for x in X])
        slots = _lib.load().cocos_loss_partials(len(X), n_t)
        partials = torch.empty(max(slots, 1), device=X[0].device, dtype=torch.float64)
        out = torch.empty(1, device=X[0].device, dtype=torch.float32)
        _call("gan_loss", "cocos_gan_loss_fwd", len(X), _table(ctypes.c_void_p, [x.data_ptr() for x in X]), n_t, mode, label,
              partials.data_ptr(), out.data_ptr(), _stream())
        ctx.save_for_backward(*X)
        ctx.cfg = (mode, label)
        return out

    @staticmethod
    def backward(ctx, g):
        X = list(ctx.saved_tensors)
        mode, label = ctx.cfg
        g = _loss_chk(g, "gan_loss: g")
        dX = [torch.empty_like(x) if ctx.needs_input_grad[2 + i] else None for i, x in enumerate(X)]
        _call("gan_loss", "cocos_gan_loss_bwd", len(X), _table(ctypes.c_void_p, [x.data_ptr() for x in X]),
              _table(ctypes.c_void_p, [_ptr(d) for d in dX]), _table(ctypes.c_longlong, [x.numel() for x in X]), mode, label,
              g.data_ptr(), _stream())
        return (None, None, *dX)


def gan_loss(xs, mode: str, label: float = 0.0) -> torch.Tensor:
    """GANLoss over a list of up to 8 prediction tensors in one launch: [1] = (sum_t m_t) / len(xs) with m_t the per-tensor mean
    of the mode's term — "hinge_d_real" -mean(min(x - 1, 0)), "hinge_d_fake" -mean(min(-x - 1, 0)), "neg_mean" -mean(x),
    "mean" mean(x), "ls" mean((x - label)^2), "bce" binary_cross_entropy_with_logits against the constant label (K28)."""
    xs = list(xs)
    if mode not in GAN_MODES:
        raise ValueError(f"gan_loss: mode {mode!r}: expected one of {sorted(GAN_MODES)}")
    if not 1 <= len(xs) <= GAN_LOSS_MAX_TENSORS:
        raise ValueError(f"gan_loss: {len(xs)} tensors (1 ... {GAN_LOSS_MAX_TENSORS})")
    return _GanLoss.apply(GAN_MODES[mode], float(label), *xs)


class _MaskNll(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, gt, ref):
        p = _loss_chk(p, "mask_nll_loss: p")
        gt = _loss_chk(gt, "mask_nll_loss: gt", torch.int64)
        ref = _loss_chk(ref, "mask_nll_loss: ref", torch.int64)
        if p.dim() != 4 or gt.numel() != p.shape[0] * gt.shape[-2] * gt.shape[-1] or ref.numel() != p.shape[0] * ref.shape[-2] * ref.shape[-1]:
            raise ValueError(f"mask_nll_loss: p {tuple(p.shape)}, gt {tuple(gt.shape)}, ref {tuple(ref.shape)}: expected [B, nc, h, w] and "
                             "one label per pixel")
        B, nc, h, w = p.shape
        H, W, Hr, Wr = gt.shape[-2], gt.shape[-1], ref.shape[-2], ref.shape[-1]
        if (h, w) != (H // 4, W // 4):
            raise ValueError(f"mask_nll_loss: p is {h}x{w}, the {H}x{W} label map gives {H // 4}x{W // 4} at scale 0.25")
        slots = _lib.load().cocos_mask_nll_partials(B, H, W)
        partials = torch.empty(max(2 * slots, 2), device=p.device, dtype=torch.float64)
        present = torch.empty((B, 8), device=p.device, dtype=torch.int32)
        out = torch.empty(2, device=p.device, dtype=torch.float32)
        _call("mask_nll", "cocos_mask_nll_fwd", p.data_ptr(), gt.data_ptr(), ref.data_ptr(), B, nc, H, W, Hr, Wr, partials.data_ptr(),
              present.data_ptr(), out.data_ptr(), _stream())
        ctx.save_for_backward(p, gt, present, out)
        ctx.cfg = (B, nc, H, W)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        p, gt, present, out = ctx.saved_tensors
        g = _loss_chk(g, "mask_nll_loss: g")
        dp = torch.empty_like(p)
        _call("mask_nll", "cocos_mask_nll_bwd", p.data_ptr(), gt.data_ptr(), present.data_ptr(), out.data_ptr() + 4, g.data_ptr(),
              dp.data_ptr(), *ctx.cfg, _stream())
        return dp, None, None


def mask_nll_loss(p: torch.Tensor, gt_label: torch.Tensor, ref_label: torch.Tensor) -> torch.Tensor:
    """The warp-mask loss of pix2pix_model.py:262-276 before `* weight_mask`, without a host read: p [B, nc, H // 4, W // 4] the
    warped mask, gt_label [B, (1,) H, W] and ref_label [B, (1,) Hr, Wr] int64, both sampled as F.interpolate(scale_factor=0.25,
    mode='nearest') samples them; weight 1 where the ground-truth class is not 0 and occurs in the sample's reference map;
    sum(weight * -log(p[gt] + 1e-10)) / (sum(weight) + 1e-5) as a 0-dim tensor.  The backward writes the dense gradient of p
    in one pass; nothing but the class sets (32 bytes per sample) and sum(weight) is saved (K28)."""
    return _MaskNll.apply(p, gt_label, ref_label)


# ------------------------------------------------------------------------------------------
# K29  the tail of the step: multi-tensor Adam and EMA (pix2pix_trainer.py:57,61-62,73; generator.py:268-274)
# ------------------------------------------------------------------------------------------
def optim_constants() -> dict:
    """COCOS_OPTIM_* as the loaded library was built with them: TABLE_ENTRIES (table entries per launch), TABLE_GROUPS (Adam group
    rows per launch), CHUNK_ELEMS (elements per workgroup), ENTRY_ELEMS (elements per table entry)."""
    f = _lib.load().cocos_optim_constant
    return {name: f(k) for k, name in enumerate(("TABLE_ENTRIES", "TABLE_GROUPS", "CHUNK_ELEMS", "ENTRY_ELEMS"))}


def _optim_chk(t, name: str) -> None:
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.layout == torch.strided and t.is_contiguous()
            and t.numel() > 0):
        what = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise _lib.CocosHipError(f"{name}: expected a dense contiguous non-empty float32 CUDA/HIP tensor, got {what}; the optimiser "
                                 "kernels have no CPU fallback")


def adam_multi_step(params, grads, exp_avgs, exp_avg_sqs, group_rows, group_index, validate: bool = True) -> int:
    """torch.optim.Adam's update (no amsgrad, no maximize) of every listed parameter, one launch per 64 table entries, in place:
    one read of p, g, m, v and one write of p, m, v per element.  `group_rows`: one (step_size, bc2_sqrt, beta1, 1 - beta1, beta2,
    1 - beta2, eps, weight_decay) per row — lr / (1 - beta1^t), sqrt(1 - beta2^t) formed in double by the caller;
    `group_index[i]`: the row of tensor i.  The tables are host arrays: no copy to the device, no allocation, no host
    synchronisation.  Bumps `_version` of every p, m, v.  `validate=False`: the caller has already checked that every tensor is a
    dense contiguous fp32 tensor of its parameter's size on one device.  Returns the number of kernel launches the call made,
    as counted by the library (K29)."""
    params, grads, exp_avgs, exp_avg_sqs = list(params), list(grads), list(exp_avgs), list(exp_avg_sqs)
    n = len(params)
    if not (n and n == len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(group_index)) or not len(group_rows):
        raise ValueError(f"adam_multi_step: {n} parameters, {len(grads)} gradients, {len(exp_avgs)} / {len(exp_avg_sqs)} moments, "
                         f"{len(group_index)} group indices, {len(group_rows)} group rows")
    words = []
    for p, g, m, v, k in zip(params, grads, exp_avgs, exp_avg_sqs, group_index):
        cnt = p.numel()
        if validate:
            for t, what in ((p, "p"), (g, "g"), (m, "exp_avg"), (v, "exp_avg_sq")):
                _optim_chk(t, "adam_multi_step: " + what)
        if validate and not (g.numel() == m.numel() == v.numel() == cnt and g.device == m.device == v.device == p.device):
            raise ValueError(f"adam_multi_step: p {tuple(p.shape)}, g {tuple(g.shape)}, exp_avg {tuple(m.shape)}, exp_avg_sq {tuple(v.shape)}")
        # cocos_adam_entry as six 8-byte words (little endian: group in the low half of the last one)
        words += (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), cnt, int(k) & 0xffffffff)
    entries = _table(ctypes.c_uint64, words)
    rows = _table(ctypes.c_float, [float(x) for row in group_rows for x in row])
    if len(rows) != 8 * len(group_rows):
        raise ValueError("adam_multi_step: a group row has 8 numbers")
    launches = ctypes.c_int(0)
    _call("adam_multi", "cocos_adam_multi_step", ctypes.addressof(entries), n, ctypes.addressof(rows), len(group_rows),
          ctypes.addressof(launches), _stream())
    torch.autograd.graph.increment_version(params + exp_avgs + exp_avg_sqs)
    return launches.value


def ema_multi_update(shadows, params, mu: float) -> int:
    """shadow = (1 - mu) * p + mu * shadow for every pair, in place, bitwise what the expression gives in torch ops (two rounded
    products, one rounded sum), one launch per 64 table entries.  Bumps `_version` of every shadow.  Returns the number of kernel
    launches the call made, as counted by the library (K29)."""
    shadows, params = list(shadows), list(params)
    if not shadows or len(shadows) != len(params):
        raise ValueError(f"ema_multi_update: {len(shadows)} shadows, {len(params)} parameters")
    words = []
    for s, p in zip(shadows, params):
        _optim_chk(s, "ema_multi_update: shadow")
        _optim_chk(p, "ema_multi_update: p")
        if s.numel() != p.numel() or s.device != p.device:
            raise ValueError(f"ema_multi_update: shadow {tuple(s.shape)} on {s.device}, p {tuple(p.shape)} on {p.device}")
        words += (s.data_ptr(), p.data_ptr(), s.numel())
    entries = _table(ctypes.c_uint64, words)
    launches = ctypes.c_int(0)
    _call("ema_multi", "cocos_ema_multi_update", ctypes.addressof(entries), len(shadows), float(mu), ctypes.addressof(launches), _stream())
    torch.autograd.graph.increment_version(shadows)
    return launches.value


# ------------------------------------------------------------------------------------------
# K32  weight preparation for frozen-weight inference: many weights per launch   (inference.py; weight_prepare_multi.hip)
# ------------------------------------------------------------------------------------------
#: layout name -> COCOS_WPREP_* (include/cocos_hip.h)
WPREP_LAYOUTS = {m: _C["COCOS_WPREP_" + m.upper()] for m in ("conv_fwd", "conv_dgrad", "conv_fwd_bf16", "conv_dgrad_bf16", "rows", "frag")}


def weight_prepare_constants() -> dict:
    """COCOS_WPREP_* as the loaded library was built with them: TABLE_ENTRIES (entries per launch), ABSMAX_CHUNK (elements per workgroup)."""
    f = _lib.load().cocos_weight_prepare_constant
    return {name: f(k) for k, name in enumerate(("TABLE_ENTRIES", "ABSMAX_CHUNK"))}


def weight_absmax_multi(weights):
    """([max|w| cell for w in weights], kernel launches): one pass over every listed weight, two launches per 64 of them
    (per-workgroup maxima, then one finishing workgroup per weight) — the bits `absmax(w)` leaves, without its launch per tensor."""
    weights = list(weights)
    if not weights:
        return [], 0
    for w in weights:
        _optim_chk(w, "weight_absmax_multi: weight")
    dev = weights[0].device
    if any(w.device != dev for w in weights):
        raise ValueError("weight_absmax_multi: the weights live on different devices")
    cells = torch.empty(len(weights), device=dev, dtype=torch.float32)
    words = []
    for i, w in enumerate(weights):
        words += (w.data_ptr(), w.numel(), cells.data_ptr() + 4 * i)
    entries = _table(ctypes.c_uint64, words)
    n_ws = _lib.load().cocos_weight_absmax_multi_workspace_floats(ctypes.addressof(entries), len(weights))
    ws = torch.empty(max(int(n_ws), 1), device=dev, dtype=torch.float32)
    launches = ctypes.c_int(0)
    _call("weight_prepare", "cocos_weight_absmax_multi", ctypes.addressof(entries), len(weights), ws.data_ptr(), ws.numel(),
          ctypes.addressof(launches), _stream())
    return [cells[i:i + 1] for i in range(len(weights))], launches.value


def weight_planes_shape(weight, layout: str, aux: int = 0):
    """(hi shape, dtype, has lo) of `layout` for a weight [Cout,Cin,KH,KW] (or [Cout,Cin])."""
    Cout, Cin = weight.shape[:2]
    KH, KW = (weight.shape[2], weight.shape[3]) if weight.dim() == 4 else (1, 1)
    if layout.startswith("conv_"):
        M, C = (Cout, Cin) if "fwd" in layout else (Cin, Cout)
        return (KH * KW * ((C + 31) // 32), M, 32), torch.float16, not layout.endswith("bf16")
    if layout == "rows":
        return (Cout, int(aux)), torch.float16, True
    if layout == "frag":
        return (int(_lib.load().cocos_proj_weight_frag_bytes(Cin * KH * KW)),), torch.uint8, False
    raise ValueError(f"weight_planes_multi: unknown layout {layout!r} (expected one of {sorted(WPREP_LAYOUTS)})")


def weight_planes_multi(requests):
    """requests: (weight, max|w| cell or None, layout, aux) each -> ([(hi, lo, scale)], kernel launches): the planes of ONE layout per
    request, one launch per 64 requests, byte for byte what the single-tensor routines write —
      "conv_fwd" / "conv_dgrad"            _conv_weight_planes(weight, cell, 0 / 1): K16 / K16c;
      "conv_fwd_bf16" / "conv_dgrad_bf16"  _conv_weight_planes(weight, None, 0 / 1): one bf16 plane, lo and scale None (K16b);
      "rows"                               cocos_split_f16_rows with rows of `aux` halfs (K0 stream, aux = cocos_proj1x1_stream_kpad(Cin));
      "frag"                               cocos_proj_weight_frag_planes (K23 / K25): hi = the fragment buffer, lo None."""
    requests = list(requests)
    if not requests:
        return [], 0
    out, words = [], []
    for weight, cell, layout, aux in requests:
        _optim_chk(weight, "weight_planes_multi: weight")
        if weight.dim() not in (2, 4):
            raise ValueError(f"weight_planes_multi: weight {tuple(weight.shape)}")
        shape, dtype, has_lo = weight_planes_shape(weight, layout, aux)
        bf = layout.endswith("bf16")
        if not bf and cell is None:
            raise ValueError(f"weight_planes_multi: layout {layout!r} needs the weight's max|w| cell")
        hi = torch.empty(shape, device=weight.device, dtype=dtype)
        lo = torch.empty_like(hi) if has_lo else None
        sc = None if bf else torch.empty(1, device=weight.device, dtype=torch.float32)
        Cout, Cin = weight.shape[:2]
        KH, KW = (weight.shape[2], weight.shape[3]) if weight.dim() == 4 else (1, 1)
        if layout == "frag":
            Cin, KH, KW = Cin * KH * KW, 1, 1
        words += (weight.data_ptr(), 0 if bf else cell.data_ptr(), hi.data_ptr(), _ptr(lo), _ptr(sc),
                  WPREP_LAYOUTS[layout] | (Cout << 32), Cin | (KH << 32), KW | (int(aux) << 32))
        out.append((hi, lo, sc))
    entries = _table(ctypes.c_uint64, words)
    launches = ctypes.c_int(0)
    _call("weight_prepare", "cocos_weight_planes_multi", ctypes.addressof(entries), len(requests), ctypes.addressof(launches), _stream())
    return out, launches.value


def mfma_probe() -> torch.Tensor:
    """Debug: the 64x16 accumulator image of one v_mfma_f32_32x32x2_f32 (see api_common.hip)."""
    out = torch.empty((64, 16), device="cuda", dtype=torch.float32)
    _lib.call("cocos_debug_mfma_probe", out.data_ptr(), _stream())
    return out
