/*
 * cocos_hip.h — C ABI of the MI355X-native (gfx950) correspondence hot path.
 *
 * The reference (microsoft/CoCosNet) has no FFI of its own: its hot path is a chain of
 * ATen calls inside NoVGGCorrespondence.forward (models/networks/correspondence.py:271-372).
 * This header is the boundary we introduce underneath that Python class contract; each entry
 * point names the reference lines it replaces.  See INTEGRATION.md for the ctypes binding.
 *
 * Conventions (all entry points):
 *   - plain C, no torch types; pointers are DEVICE pointers owned by the caller, fp32,
 *     contiguous, 16-byte aligned; the library never allocates or frees device memory;
 *   - "positions" are the flattened h*w feature grid; every feature tensor is CHANNEL-MAJOR
 *     [B, C, positions] — exactly what `tensor.view(B, C, -1)` gives in the reference;
 *   - asynchronous on `stream` (a hipStream_t passed as void*), no hidden device sync;
 *   - re-entrant / thread-safe (no global mutable state except a thread-local error string);
 *   - return 0 on success, a negative code on failure (never throws):
 *       -1 invalid argument, -2 unsupported shape, -3 HIP runtime error, -4 workspace too small.
 */
#ifndef COCOS_HIP_H
#define COCOS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COCOS_OK 0
#define COCOS_ERR_INVALID (-1)
#define COCOS_ERR_UNSUPPORTED (-2)
#define COCOS_ERR_HIP (-3)
#define COCOS_ERR_WORKSPACE (-4)

typedef void* cocos_stream_t; /* hipStream_t */

/* ABI version: major*10000 + minor*100 + patch. */
int cocos_version(void);
/* Message for the last failing call on this thread ("" if none). */
const char* cocos_last_error_string(void);

/* ---------------------------------------------------------------------------------------
 * K1  centre + L2-normalise  (correspondence.py:277-280 for theta, :287-289 for phi)
 *   x      [B,K,N]  raw theta/phi (after view or F.unfold)
 *   y      [B,K,N]  out: (x - mean) / (||x - mean||_2 over K + eps)
 *   norm   [B,N]    out: ||x - mean||_2 per position (saved for backward)
 *   center_over_channels == 1  -> PONO_C: mean over K per position   (dim_mean = 1)
 *                        == 0  -> mean over N per channel            (dim_mean = -1);
 *                                 needs row_ws [B,K] floats of scratch.
 *                        == 2  -> no centring: y = x / (||x||_2 over K + eps), i.e.
 *                                 util.feature_normalize (util/util.py:31-34) as applied to the adaptor
 *                                 outputs at correspondence.py:247-248 (and :245 for the feature-pair loss)
 *   eps = sys.float_info.epsilon (2.220446049250313e-16) in the reference.
 * ------------------------------------------------------------------------------------- */
#define COCOS_CENTER_POSITIONS 0
#define COCOS_CENTER_CHANNELS 1
#define COCOS_CENTER_NONE 2
int cocos_center_l2norm_fwd(const float* x, float* y, float* norm, float* row_ws,
                            int B, int K, int N, int center_over_channels, float eps,
                            cocos_stream_t stream);
/* Backward of K1 (autograd of :277-280).  dy [B,K,N] -> dx [B,K,N].
 * col_ws [B,N] and row_ws [B,K] floats of scratch are required when center_over_channels == 0
 * (may be NULL otherwise). */
int cocos_center_l2norm_bwd(const float* y, const float* norm, const float* dy, float* dx,
                            float* col_ws, float* row_ws,
                            int B, int K, int N, int center_over_channels, float eps,
                            cocos_stream_t stream);
/* Same as cocos_center_l2norm_bwd, and on return *dx_amax_inout = max(*dx_amax_inout, max|dx|) (the cell must hold
 * a finite value >= 0, e.g. 0): the consumer of dx on the hot path — the backward of the theta/phi projection,
 * correspondence.py:272,:282 — needs it for the scale of its f16 split; produced while dx is written. */
int cocos_center_l2norm_bwd_amax(const float* y, const float* norm, const float* dy, float* dx, float* col_ws,
                                 float* row_ws, int B, int K, int N, int center_over_channels, float eps,
                                 float* dx_amax_inout, cocos_stream_t stream);

/* K1 for the split-precision correlation kernels (round 3): the forward writes the f16 hi/lo OPERAND PLANES of
 * plane_scale * y itself — position-major [B,N,256] (always) and channel-major [B,256,N] (nullable pair; the backward wants
 * them) — and no fp32 y: 12 B/element instead of 24 for K1 + two cocos_split_f16 launches per tensor.  K == 256,
 * N % 4 == 0, center_over_channels 1 (PONO_C) or 2 (none).  The planes are bit-identical to cocos_split_f16(y, scale).
 * The backward reads y back from the channel-major planes. */
int cocos_center_l2norm_fwd_planes(const float* x, float* norm, void* pos_hi, void* pos_lo, void* chan_hi /* nullable */,
                                   void* chan_lo /* nullable */, int B, int K, int N, int center_over_channels, float eps,
                                   float plane_scale, cocos_stream_t stream);
int cocos_center_l2norm_bwd_planes(const void* chan_hi, const void* chan_lo, const float* norm, const float* dy, float* dx,
                                   int B, int K, int N, int center_over_channels, float eps, float plane_scale,
                                   float* dx_amax_inout /* nullable */, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K2  fused correlation -> /temperature -> softmax over key positions -> warp
 *     (correspondence.py:281,291,304,307,318 and the extra P@V products at :334,:343-344,
 *      :351-372; the HWxHW matrix never reaches HBM)
 *   qn   [B,K,Nq]   normalised theta (query / content positions)
 *   kn   [B,K,Nk]   normalised phi   (key / exemplar positions)
 *   v    [B,Cv,Nk]  channels to warp (avg-pooled exemplar RGB, label maps, ... concatenated)
 *   out  [B,Cv,Nq]  out[b,c,i] = sum_j softmax_j(qn[:,i].kn[:,j] * inv_temperature) * v[b,c,j]
 *   lse  [B,Nq]     row log-sum-exp of the scaled logits (natural log), saved for backward
 *   logits_t [B,Nk,Nq] or NULL: when given (training), the scaled logits * log2(e) are also
 *                   written, key-major, for cocos_corr_softmax_warp_bwd_query to read back instead
 *                   of recomputing them (inference passes NULL: nothing HWxHW reaches HBM)
 * The column softmax `softmax(f^T)` of :338/:351 is this same call with qn/kn swapped.
 * Supported: K == 256 (match_kernel 1), 1 <= Cv <= 160, any Nq, Nk >= 1.
 * ------------------------------------------------------------------------------------- */
int cocos_corr_softmax_warp_fwd(const float* qn, const float* kn, const float* v,
                                float* out, float* lse, float* logits_t /* nullable */,
                                int B, int K, int Nq, int Nk, int Cv, float inv_temperature,
                                cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K2 forward, split-precision flavour (same reference lines, same outputs as the call above): the
 * matrix products run on v_mfma_f32_32x32x16_f16 with every fp32 operand carried as two f16 planes,
 * x*scale ~= hi + lo (22 mantissa bits), three MFMA terms per product, fp32 accumulation — fp32-class
 * accuracy at ~1/5 of the fp32-MFMA pipe time on gfx950.
 *   cocos_split_f16:  x [B,C,N] fp32 -> hi, lo (f16); transpose = 0: [B,C,N]; 1: [B,N,C]; `scale` must be
 *                     a power of two (exact).
 *   qh,ql [B,Nq,256]  kh,kl [B,Nk,256]  position-major planes of qn*operand_scale, kn*operand_scale
 *   vh,vl [B,Cv,Nk]   channel-major planes of v * s_v, s_v = *v_scale_dev (a power of two, e.g. the one
 *                     cocos_split_f16_ex derives from max|v|; NULL = 1): V has no a-priori magnitude in a general
 *                     forward() call, so its planes are normalised like every other operand and the epilogue
 *                     undoes the scale
 *   saved_logits      NULL (inference: nothing HWxHW reaches HBM) or cocos_corr_softmax_warp_saved_logits_bytes()
 *                     bytes, 16-byte aligned (training): the raw logits accumulator of every 32x32 tile in a
 *                     PRIVATE tile-blocked layout ([key tile][32-query block][k][lane][4]: four contiguous 1 KB
 *                     stores per wave and tile), read back only by cocos_corr_softmax_warp_bwd_query_f16x3
 *   Supported: K == 256, 1 <= Cv <= 159 (one padding channel of the V tile carries the row sums), Nk % 4 == 0
 *   (otherwise COCOS_ERR_UNSUPPORTED: use the fp32 call).
 * ------------------------------------------------------------------------------------- */
int cocos_split_f16(const float* x, void* hi, void* lo, int B, int C, int N, int transpose, float scale,
                    cocos_stream_t stream);
size_t cocos_corr_softmax_warp_saved_logits_bytes(int B, int Nq, int Nk);
int cocos_corr_softmax_warp_fwd_f16x3(const void* qh, const void* ql, const void* kh, const void* kl,
                                      const void* vh, const void* vl,
                                      float* out, float* lse, void* saved_logits /* nullable */,
                                      const float* v_scale_dev /* nullable */,
                                      const unsigned* v_lo_mask_dev /* nullable */,
                                      int B, int K, int Nq, int Nk, int Cv, float inv_temperature,
                                      float operand_scale,
                                      const float* q_scale_dev /* nullable */, const float* k_scale_dev /* nullable: operands
                                      without an a-priori magnitude (ops.softmax_attention) — planes scaled by device-side
                                      powers of two (cocos_split_f16_ex); given as a pair they replace operand_scale */,
                                      cocos_stream_t stream);
/* The same with one more output for the MAGNITUDE-FREE flavour (q_scale_dev / k_scale_dev given, v_lo_mask_dev NULL: operands that
 * are not unit-norm columns — Attention.forward, architecture.py:114-127, feeds raw 1x1-conv outputs; a randomly initialised SPADE
 * generator reaches |logit| ~ 1e10 there): in that flavour the running maximum is kept in the units of the raw accumulator and the
 * exponent is formed from an EXACT difference (round 4; with the maximum in the log2 domain one ulp of m was ~700 in the exponent
 * and the output NaN).  rowstat_out (nullable) [B][3][Nq]: per query (m as an unevaluated fp32 sum hi + lo in raw units, log2 l - bias) — what the backward of this
 * flavour takes instead of the row LSE (cocos_corr_softmax_warp_bwd_query_f16x3_ex).  In this flavour saved_logits holds RELATIVE
 * raw accumulators, s - m_tile, and mtile_out [B][ceil(Nk/32)][2][Nq] (required with saved_logits) the m_tile (hi, lo) they are relative to:
 * absolute logits of 1e9 would be rounded to +-70 in the exponent, differences of fp32 maxima are exact. */
int cocos_corr_softmax_warp_fwd_f16x3_ex(const void* qh, const void* ql, const void* kh, const void* kl,
                                         const void* vh, const void* vl, float* out, float* lse, void* saved_logits,
                                         const float* v_scale_dev, const unsigned* v_lo_mask_dev, int B, int K, int Nq, int Nk, int Cv,
                                         float inv_temperature, float operand_scale, const float* q_scale_dev,
                                         const float* k_scale_dev, float* rowstat_out /* nullable */, float* mtile_out /* nullable */,
                                         int k_active /* 0 = K; else: channels >= k_active of q and k are zero padding (the Attention
                                         block's C/8 channels in 256-channel planes): k_active <= 32 / <= 64 / <= 128 run instantiations without
                                         the QK steps, fragment reads and key fetches of the padding */,
                                         cocos_stream_t stream);
/* The inference forward with key and value planes that several query batches may SHARE (a prepared exemplar, inference.py:
 * one style image against B label maps).  Same kernels, same arithmetic in the same order as cocos_corr_softmax_warp_fwd_f16x3
 * on the unit-norm flavour (no q_scale_dev / k_scale_dev, no k_active); the only difference is where sample b's key / value planes
 * start: kh, kl at b * k_batch_stride halfs, vh, vl at b * v_batch_stride halfs.  (k_batch_stride, v_batch_stride) is (0, 0) — kh,kl
 * [Nk,256] and vh,vl [Cv,Nk] hold ONE set that all B samples read — or the dense (Nk * 256, Cv * Nk); anything else is
 * COCOS_ERR_INVALID.  *v_scale_dev (required) and *v_lo_mask_dev (nullable) describe the value planes as a whole, as above.
 * saved_logits must be NULL (COCOS_ERR_INVALID otherwise: this entry point has no backward).  Supported shapes as above
 * (K != 256, Cv > 159, Nk % 4 != 0: COCOS_ERR_UNSUPPORTED).  Nothing is launched when an error is returned. */
int cocos_corr_softmax_warp_fwd_f16x3_shared(const void* qh, const void* ql, const void* kh, const void* kl,
                                             const void* vh, const void* vl, float* out, float* lse,
                                             void* saved_logits /* must be NULL */, const float* v_scale_dev,
                                             const unsigned* v_lo_mask_dev /* nullable */, int B, int K, int Nq, int Nk, int Cv,
                                             float inv_temperature, float operand_scale, long long k_batch_stride,
                                             long long v_batch_stride, cocos_stream_t stream);
/* The schedule of the split-precision forward's key-tile loop, process-wide, for the three entry points above.  1 = "QK ahead": the
 * QK MFMAs of tile t+1 are issued under the softmax arithmetic of tile t (second accumulator set); 0 = QK(t), softmax(t), P.V(t) in
 * turn.  Same arithmetic in the same order: out, lse and saved_logits are bit-identical.  Only whole-tile key counts (Nk % 32 == 0)
 * of the unit-norm flavour have the skewed form; every other call runs schedule 0 whatever is selected.  mode 0 / 1 selects and
 * returns the previous selection; any other mode only returns the current one.  Launches no kernel, touches no device memory. */
#define COCOS_FWD_QK_AHEAD_DEFAULT 1
int cocos_corr_fwd_f16x3_qk_ahead(int mode);
/* bit (c >> 5) of *mask_inout_dev |= (channel c of the channel-major f16 plane [B,C,N] has a non-zero element); the
 * cell must hold 0 (or an earlier partial mask) on entry; C <= 1024.  Run on the LO plane of V: value channels that
 * are exact in f16 (one-hot labels, masks) have an all-zero lo plane, and when every 32-channel block but the first
 * reports zero the K2 split kernels skip that plane's staging, fragment reads and MFMA term for those blocks
 * (v_lo_mask_dev of the two calls; NULL = no information, the general path). */
int cocos_f16_plane_block_mask(const void* plane, int B, int C, int N, unsigned* mask_inout_dev, cocos_stream_t stream);

/* Split-precision backward of K2 (same reference lines as cocos_corr_softmax_warp_bwd_query / _bwd_key_from_ds):
 *   cocos_split_f16_ex: as cocos_split_f16, plus (a) transposed rows padded with zero channels to Cpad halfs,
 *       (b) when amax_dev != NULL the scale is chosen on the device as the power of two that brings
 *       *amax_dev (= max|x|, e.g. torch's x.abs().amax()) into [2^9, 2^10), and written to *scale_out_dev.
 *   cocos_corr_softmax_warp_bwd_query_f16x3:
 *       kch,kcl [B,256,Nk]  channel-major planes of k_scale*kn
 *       vph,vpl [B,Nk,CvPad] position-major planes of s_v*v, s_v = *v_scale_dev (NULL = 1);
 *       gph,gpl [B,Nq,CvPad] of s_o*dout, s_o = *g_scale_dev
 *       out, dout [B,Cv,Nq] fp32 (for D = sum_c dout*out, fp64);  lse, saved_logits as left by the f16x3 forward
 *       -> dqn [B,256,Nq] fp32;  dsh,dsl [B,Nk,Nq] planes of dS'' = s_o*s_v*ds_shift * dS^T/T (both NULL: skipped);
 *          *ds_scale_out_dev = s_o*s_v*ds_shift (ds_shift is derived on the device from *v_amax_dev = max|v|);
 *          psh,psl [B,Nk,Nq] planes of 2^14 * P (both NULL: skipped) for the V gradient of the cycle terms:
 *          dv = hgemm(A = channel-major planes of s_o*dout [Cv][Nq], B = P planes, host_scale = 2^-14,
 *          dev_scale = g_scale_dev)
 *       Supported: K == 256, Cv <= 160, CvPad = Cv rounded up to 32, Nk % 8 == 0.
 *   planes_blocked != 0 (query kernel) <-> b_blocked = 2 (GEMM): the dS'' / P planes are stored in the orientation
 *       the accumulators of the query kernel have — [query][key] — as [Nq/32][Nk/32] blocks of 2 x [32 queries][16 keys]
 *       halfs (2 KB each, contiguous; the two halves are keys 0..15 and 16..31 of the tile): a wave's tile leaves its registers as two 16-byte stores per plane (no transposition),
 *       the GEMM stages four consecutive blocks per k-step and reads its B fragments with the transposing LDS read
 *       (needs Nk % 128 == 0, Nq % 32 == 0; both sides must agree).  planes_blocked = 0 <-> b_blocked = 0: row-major
 *       [Nk][Nq].  b_blocked = 1 (GEMM only): [N/128][K/32] blocks of [128 n][32 k] halfs, k contiguous.
 *   cocos_hgemm_f16x3: C[b][m][n] = host_scale / (*dev_scale * *dev_scale2) * sum_k A[b][m][k] B[b][n][k] on hi/lo planes
 *       (k contiguous, K % 8 == 0); the key side is  dkn = hgemm(A = planes of k_scale*qn [256][Nq],
 *       B = dS'' planes [Nk][Nq], host_scale = 1/k_scale, dev_scale = ds_scale_out_dev). */
int cocos_split_f16_ex(const float* x, void* hi, void* lo, int B, int C, int N, int Cpad, int transpose,
                       float scale, const float* amax_dev /* nullable */, float* scale_out_dev /* nullable */,
                       cocos_stream_t stream);
/* 2-D form with padded rows: x [rows][cols] -> hi, lo [rows][cols_pad], zero beyond cols (scale as in _ex): the
 * weight planes [M][Kpad] of cocos_proj1x1_stream_f16x3 straight from the weight matrix. */
int cocos_split_f16_rows(const float* x, void* hi, void* lo, int rows, int cols, int cols_pad, float scale,
                         const float* amax_dev, float* scale_out_dev, cocos_stream_t stream);
/* cocos_split_f16_ex(transpose = 1, device-side scales) for two tensors of one shape [B,C,N] in one launch (the K2 / K19 backward
 * splits d out and v back to back). */
int cocos_split_f16_transpose_pair(const float* x0, void* hi0, void* lo0, const float* amax0_dev, float* scale0_out_dev,
                                   const float* x1, void* hi1, void* lo1, const float* amax1_dev, float* scale1_out_dev, int B, int C,
                                   int N, int Cpad, cocos_stream_t stream);
int cocos_corr_softmax_warp_bwd_query_f16x3(
    const void* kch, const void* kcl, const void* vph, const void* vpl, const void* gph, const void* gpl,
    const float* g_scale_dev, const float* out, const float* dout, const float* lse, const void* saved_logits,
    float* dqn, void* dsh /* nullable */, void* dsl /* nullable */, void* psh /* nullable */,
    void* psl /* nullable */, const float* v_amax_dev, const float* v_scale_dev /* nullable */,
    float* ds_scale_out_dev, const unsigned* v_lo_mask_dev /* nullable: as in the forward call */,
    int B, int K, int Nq, int Nk, int Cv, int CvPad, float inv_temperature, float k_scale,
    const float* q_scale_dev /* nullable */, const float* k_scale_dev /* nullable: as in the forward call */,
    int planes_blocked, cocos_stream_t stream);
/* ... with `rowstat` [B][3][Nq] and `mtile` [B][ceil(Nk/32)][2][Nq] (both or neither) as written by
 * cocos_corr_softmax_warp_fwd_f16x3_ex: the magnitude-free flavour's backward (P from exact differences; `lse` is then not read for P). */
int cocos_corr_softmax_warp_bwd_query_f16x3_ex(
    const void* kch, const void* kcl, const void* vph, const void* vpl, const void* gph, const void* gpl,
    const float* g_scale_dev, const float* out, const float* dout, const float* lse, const void* saved_logits,
    float* dqn, void* dsh, void* dsl, void* psh, void* psl, const float* v_amax_dev, const float* v_scale_dev,
    float* ds_scale_out_dev, const unsigned* v_lo_mask_dev, int B, int K, int Nq, int Nk, int Cv, int CvPad,
    float inv_temperature, float k_scale, const float* q_scale_dev, const float* k_scale_dev, int planes_blocked,
    const float* rowstat /* nullable */, const float* mtile /* nullable */,
    const float* d_pre /* nullable: D[b][i] = sum_c dout * out from cocos_rowdot_f64 — the kernel then skips its own serial fp64 loop */,
    int k_active /* 0 = K; as in the forward call: the dqn MFMAs of all-padding channel blocks do not exist in the K <= 32 / 64 / 128
    instantiations, and the dqn rows of those blocks (channels >= 32 / 64 / 128) are NOT written */,
    cocos_stream_t stream);
/* d[b][i] = sum_c a[b][c][i] * b[b][c][i], fp64 accumulation, fp32 result: D of the softmax backward (autograd of
 * correspondence.py:307/:318: dS = P * (dP - D)) as a streaming kernel. */
int cocos_rowdot_f64(const float* a, const float* b, float* d, int B, int C, int N, cocos_stream_t stream);
int cocos_hgemm_f16x3(const void* a_hi, const void* a_lo, const void* b_hi, const void* b_lo, float* c,
                      int batch, int M, int N, int K, float host_scale, const float* dev_scale /* nullable */,
                      const float* dev_scale2 /* nullable */, int b_blocked, cocos_stream_t stream);

/* Backward of K2 (autograd of :291-318), flash-style: the logits are recomputed from qn/kn and `lse`.
 *   dout [B,Cv,Nq] -> dqn [B,K,Nq], dkn [B,K,Nk], dv [B,Cv,Nk]
 * It is exposed in stages so that the caller picks the strategy for the key side:
 *   prepare        dvec[b,i] = sum_c dout[b,c,i] * out[b,c,i]      (needed by `key`, and by `query`
 *                  when it has no saved logits; the saved-logits query kernel computes it itself)
 *   query          dqn; reads the forward's logits_t if given (else recomputes the logits);
 *                  optionally also writes ds_t [B,Nk,Nq] = (dS)^T / T
 *   key            dkn (and dv if non-NULL) with a SECOND recomputation of the logits
 *   key_from_ds    dkn = qn . dS as a plain fp32-MFMA GEMM over the ds_t written by `query`
 * `query(ds_t) + key_from_ds` executes 2*HW^2*(K+Cv) fewer MFMA FLOPs per sample than `query + key`
 * for 8 bytes of HBM traffic per logit — the faster choice on MI355X (fp32 MFMA is only ~25 FLOP per
 * HBM byte) whenever B*Nq*Nk*4 bytes of scratch are available and dv is not needed.
 * cocos_corr_softmax_warp_bwd is the all-in-one convenience (prepare + query + key; ws holds dvec:
 * cocos_corr_softmax_warp_bwd_workspace_bytes() = B*Nq*4 bytes; dqn / dkn / dv may be NULL). */
size_t cocos_corr_softmax_warp_bwd_workspace_bytes(int B, int K, int Nq, int Nk, int Cv);
int cocos_corr_softmax_warp_bwd_prepare(const float* out, const float* dout, float* dvec,
                                        int B, int Nq, int Cv, cocos_stream_t stream);
int cocos_corr_softmax_warp_bwd_query(const float* qn, const float* kn, const float* v,
                                      const float* out, const float* lse, const float* dout,
                                      const float* dvec /* nullable when logits_t is given */,
                                      const float* logits_t /* nullable: from the forward */,
                                      float* dqn, float* ds_t /* nullable */,
                                      int B, int K, int Nq, int Nk, int Cv, float inv_temperature,
                                      cocos_stream_t stream);
int cocos_corr_softmax_warp_bwd_key(const float* qn, const float* kn, const float* v,
                                    const float* lse, const float* dout, const float* dvec,
                                    float* dkn, float* dv /* nullable */,
                                    int B, int K, int Nq, int Nk, int Cv, float inv_temperature,
                                    cocos_stream_t stream);
int cocos_corr_softmax_warp_bwd_key_from_ds(const float* qn, const float* ds_t, float* dkn,
                                            int B, int K, int Nq, int Nk, cocos_stream_t stream);
int cocos_corr_softmax_warp_bwd(const float* qn, const float* kn, const float* v,
                                const float* out, const float* lse, const float* dout,
                                float* dqn, float* dkn, float* dv,
                                void* ws, size_t ws_bytes,
                                int B, int K, int Nq, int Nk, int Cv, float inv_temperature,
                                cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K3  materialised correlation  f[b,i,j] = scale * sum_k qn[b,k,i] * kn[b,k,j]
 *     (correspondence.py:291 + :304; needed by return_corr=True (:305-306), WTA_scale (:300-303)
 *      and match_kernel != 1 where K = 256*mk^2)
 *   f [B,Nq,Nk]; any K >= 1.
 * ------------------------------------------------------------------------------------- */
int cocos_corr_materialize(const float* qn, const float* kn, float* f,
                           int B, int K, int Nq, int Nk, float scale, cocos_stream_t stream);

/* K3b  gradients of K3 w.r.t. its operands (autograd of :291):
 *   dqn[b,k,i] = scale * sum_j df[b,i,j] kn[b,k,j] ;  dkn[b,k,j] = scale * sum_i df[b,i,j] qn[b,k,i]
 *   Either output may be NULL. */
int cocos_corr_materialize_bwd(const float* qn, const float* kn, const float* df,
                               float* dqn, float* dkn,
                               int B, int K, int Nq, int Nk, float scale, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K4  row softmax over the last dimension of a materialised matrix (correspondence.py:307)
 *     and its backward  ds = p * (dp - sum(p*dp)).  In-place (p == s, ds == dp) allowed.
 * ------------------------------------------------------------------------------------- */
int cocos_row_softmax_fwd(const float* s, float* p, int64_t rows, int cols, cocos_stream_t stream);
int cocos_row_softmax_bwd(const float* p, const float* dp, float* ds, int64_t rows, int cols,
                          cocos_stream_t stream);

/* K5  P @ V on a materialised P  (correspondence.py:318 on the fallback path)
 *   p [B,Nq,Nk], v [B,Cv,Nk] -> out [B,Cv,Nq];  and its two gradients:
 *   dp[b,i,j] = sum_c dout[b,c,i] v[b,c,j] ;  dv[b,c,j] = sum_i p[b,i,j] dout[b,c,i]. */
int cocos_warp_materialized_fwd(const float* p, const float* v, float* out,
                                int B, int Nq, int Nk, int Cv, cocos_stream_t stream);
int cocos_warp_materialized_bwd(const float* p, const float* v, const float* dout,
                                float* dp, float* dv,
                                int B, int Nq, int Nk, int Cv, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K0  theta / phi 1x1 projections (correspondence.py:272, :282: nn.Conv2d(Cl, 256, kernel_size=1))
 *   fwd: y[b,co,n] = sum_ci w[co,ci] x[b,ci,n] + bias[co]      x [B,Cin,N], w [Cout,Cin], bias [Cout] or NULL
 *   bwd: dx[b,ci,n] = sum_co w[co,ci] dy[b,co,n]  (dx may be NULL);
 *        dw_p[p,co,ci] = sum_{n in slice p} dy[b,co,n] x[b,ci,n]  partial sums (may be NULL):
 *        P = cocos_proj1x1_bwd_partials(B,Cin,Cout,N) slabs of [Cout,Cin] (sample x split-K slice, so the
 *        launch fills the chip); the caller adds the P slabs, and sums dy over (b,n) for the bias gradient.
 * ------------------------------------------------------------------------------------- */
int cocos_proj1x1_fwd(const float* x, const float* w, const float* bias, float* y,
                      int B, int Cin, int Cout, int N, cocos_stream_t stream);
int cocos_proj1x1_bwd_partials(int B, int Cin, int Cout, int N);   /* 0 on bad dims */
int cocos_proj1x1_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw_p,
                      int B, int Cin, int Cout, int N, cocos_stream_t stream);

/* K0 on the split-precision GEMM (sgemm_f16x3.hip): same contract, fp32 tensors in and out; the operands are
 * split into f16 hi/lo on the fly inside the kernel (3 MFMA terms per product, fp32 accumulate).  Each operand
 * is pre-scaled by a power of two derived from a device-side max|.| (x_amax, w_amax, dy_amax: 1-element device
 * arrays, e.g. from cocos_absmax; NULL = the operand is already O(1)).
 *   cocos_absmax: *out_dev = max|x[0..n)| (one pass; cleared by the call). */
int cocos_absmax(const float* x, long long n, float* out_dev, cocos_stream_t stream);
/* *inout_dev = max(*inout_dev, max|x|) without the memset cocos_absmax puts in front: the cell must hold a finite
 * value >= 0 (pre-zeroed pool; or the running maximum over the parts of a virtually concatenated tensor). */
int cocos_absmax_accumulate(const float* x, long long n, float* inout_dev, cocos_stream_t stream);
/* The same for up to four tensors in ONE launch (x_i == NULL: slot unused): the max|.| passes a step takes in a row — the two
 * feature tensors and the two projection weights in front of K23 / K0 — share a launch (csrc/sgemm_f16x3.hip). */
int cocos_absmax4(const float* x0, long long n0, float* c0, const float* x1, long long n1, float* c1, const float* x2,
                  long long n2, float* c2, const float* x3, long long n3, float* c3, cocos_stream_t stream);
int cocos_proj1x1_fwd_f16x3(const float* x, const float* w, const float* bias, float* y,
                            int B, int Cin, int Cout, int N, const float* x_amax, const float* w_amax,
                            cocos_stream_t stream);
int cocos_proj1x1_bwd_partials_f16x3(int B, int Cin, int Cout, int N);   /* 0 on bad dims */
/* K3 (cocos_corr_materialize / _bwd: correspondence.py:291 (+:304) and its autograd) on the same split GEMM;
 * q_amax, k_amax, df_amax: device-side max|.| of the operands (NULL = O(1)). */
int cocos_corr_materialize_f16x3(const float* qn, const float* kn, float* f, int B, int K, int Nq, int Nk,
                                 float scale, const float* q_amax, const float* k_amax, cocos_stream_t stream);
int cocos_corr_materialize_bwd_f16x3(const float* qn, const float* kn, const float* df, float* dqn, float* dkn,
                                     int B, int K, int Nq, int Nk, float scale, const float* q_amax,
                                     const float* k_amax, const float* df_amax, cocos_stream_t stream);
int cocos_proj1x1_bwd_f16x3(const float* x, const float* w, const float* dy, float* dx, float* dw_p,
                            int B, int Cin, int Cout, int N, const float* x_amax, const float* w_amax,
                            const float* dy_amax, cocos_stream_t stream);
/* K0 streaming form (correspondence.py:272,:282 at the reference's shapes: 256 or 256+151 channels -> 256):
 *     y[b,m,n] = (sum_k A[m,k] x[b,k,n]) / (*a_scale_dev * x_scale) + bias[m]
 * A = the weight (forward) or its transpose (input gradient) as f16 hi/lo planes [M][Kpad], zero beyond K, from
 * cocos_split_f16_ex(transpose = 1, Cpad = Kpad) of the k-major matrix [K][M] (its scale goes to a_scale_dev);
 * Kpad = cocos_proj1x1_stream_kpad(K) (0: K not supported).  x fp32 [B,K,N] is split in flight with the
 * power-of-two scale from x_amax (NULL = 1).  A stays in registers, x and y are touched once (HBM-bound).
 * COCOS_ERR_UNSUPPORTED unless K <= 416 and N % 64 == 0 (callers then use cocos_proj1x1_fwd_f16x3 / _bwd_f16x3). */
int cocos_proj1x1_stream_kpad(int K);
int cocos_proj1x1_stream_f16x3(const float* x, const void* a_hi, const void* a_lo, const float* a_scale_dev,
                               const float* bias, float* y, int B, int K, int M, int N, const float* x_amax,
                               cocos_stream_t stream);
/* K23 (round 6): K0 FUSED with K1 — the theta / phi 1x1 projection, centring over the channels and the L2 normalisation in one
 * kernel whose only products are the operand planes of the split correlation kernels (correspondence.py:272 + :277-280,
 * :282 + :287-289; csrc/proj_norm_f16x3.hip).  The fp32 projection never reaches HBM.
 *   cocos_proj_weight_frag_planes: w [256][K] fp32 (+ device cell max|w|) -> the weight's f16 hi / lo planes in the kernel's
 *       fragment order (cocos_proj_weight_frag_bytes(K) bytes: one 16 KB stage per 16 input channels, zero beyond K) and
 *       *w_scale = the power of two they were multiplied with; t_hi / t_lo (nullable pair): the same scaled numbers as transposed
 *       row-major planes [K][256] = the A operand of dx = W^T dy in cocos_proj1x1_stream_f16x3 (scale: *w_scale).  Once per step
 *       and projection.
 *   cocos_proj_center_l2norm_planes_f16x3: up to two projections of the same shape in one launch (theta and phi of a
 *       forward call fill the chip together: two workgroups per CU).  Per projection: x [B,K,N] fp32 (N % 128 == 0),
 *       x_amax (device cell max|x|, NULL = 1), bias [256] (nullable) -> norm [B,N] (the L2 norm of the centred column) and the
 *       planes of plane_scale * y, y = (W x + bias - mean) / (norm + eps): position-major [B,N,256] (always) and
 *       channel-major [B,256,N] (chan_hi / chan_lo, nullable pair — the backward's operands), same layouts and rounding
 *       as cocos_center_l2norm_fwd_planes.  center_over_channels: 1 (PONO_C) or 2 (no centring).
 *       The backward is cocos_center_l2norm_bwd_planes followed by K0's (cocos_proj1x1_stream_f16x3 with the transposed
 *       planes, cocos_proj1x1_dw_f16x3). */
size_t cocos_proj_weight_frag_bytes(int K);
int cocos_proj_weight_frag_planes(const float* w, const float* w_amax_dev, void* wfrag, float* w_scale_dev,
                                  void* t_hi /* nullable */, void* t_lo /* nullable */, int M, int K, cocos_stream_t stream);
int cocos_proj_center_l2norm_planes_f16x3(
    int nprob, const float* x0, const void* wfrag0, const float* w_scale0, const float* bias0, const float* x_amax0, float* norm0,
    void* pos_hi0, void* pos_lo0, void* chan_hi0, void* chan_lo0, const float* x1, const void* wfrag1, const float* w_scale1,
    const float* bias1, const float* x_amax1, float* norm1, void* pos_hi1, void* pos_lo1, void* chan_hi1, void* chan_lo1, int B,
    int K, int N, int center_over_channels, float eps, float plane_scale, cocos_stream_t stream);
/* K24 (round 6): the projection's INPUT gradient fused with what autograd puts between it and the correlation's gradient
 * (csrc/proj_bwd_f16x3.hip; autograd of correspondence.py:272-289 / :272 + :276-280):
 *     d[b,ch,n] = alpha[b,n] in1[b,ch,n] + beta[b,n] in2[b,ch,n] + gamma[b,n],      dx[b,ci,n] = sum_ch W[ch,ci] d[b,ch,n]
 *   mode 0 (match_kernel 1, K1's backward folded in): in1 = d qn [B,256,N], in2a / in2b = the position-major f16 hi / lo planes
 *       [B,N,256] of plane_scale * y (K23's / K1's), c1 = nrm [B,N]; alpha, beta, gamma are computed by a first sweep over the
 *       channels exactly as cocos_center_l2norm_bwd_planes does (center_over_channels 1 or 2);
 *   mode 1 (match_kernel 3, K12's backward and autograd's sum folded in): in1 = d theta from the correlation GEMMs, in2a = the
 *       fp32 projection [B,256,N], c1 = g1, c2 = g2 [B,N] (cocos_unfold3_stats_bwd's maps): alpha = 1, beta = 2 g2, gamma = g1.
 * Outputs per projection: dx [B,Cin,N] fp32; coef [B,3,N] = (alpha, beta, gamma); *amax = max(*amax, max|d|) (mode 0: an upper
 * bound; the cell must hold a finite value >= 0) — the inputs of cocos_proj1x1_dw_affine_f16x3, which rebuilds d while it
 * stages in1 / in2: the fp32 d is neither written nor read.  Up to two projections of one shape per launch; N % 128 == 0,
 * Cin <= 448 (cocos_proj_bwd_input_supported).  wtfrag: cocos_proj_weight_tfrag_planes (cocos_proj_weight_tfrag_bytes() bytes). */
size_t cocos_proj_weight_tfrag_bytes(void);
int cocos_proj_weight_tfrag_planes(const float* w, const float* w_amax_dev, void* wtfrag, float* w_scale_dev /* nullable */, int M,
                                   int Cin, cocos_stream_t stream);
/* cocos_proj_weight_frag_planes + cocos_proj_weight_tfrag_planes for up to two projections of one shape (theta and phi of a
 * forward call) in ONE launch: per projection w [256][K], its max|w| cell, wfrag + w_scale, t_hi / t_lo (nullable pair) and
 * wtfrag (nullable; needs K <= 448).  Same bytes as the single entry points write. */
int cocos_proj_weight_prep_pair(int nprob, const float* w0, const float* w_amax0, void* wfrag0, float* w_scale0, void* t_hi0,
                                void* t_lo0, void* wtfrag0, const float* w1, const float* w_amax1, void* wfrag1, float* w_scale1,
                                void* t_hi1, void* t_lo1, void* wtfrag1, int M, int K, cocos_stream_t stream);
int cocos_proj_bwd_input_supported(int Cin, int M, int N);
int cocos_proj_bwd_input_f16x3(
    int mode, int nprob, const float* in1_0, const void* in2a_0, const void* in2b_0, const float* c1_0, const float* c2_0,
    const void* wtfrag0, const float* w_scale0, float* dx0, float* coef0, float* amax0, const float* in1_1, const void* in2a_1,
    const void* in2b_1, const float* c1_1, const float* c2_1, const void* wtfrag1, const float* w_scale1, float* dx1, float* coef1,
    float* amax1, int B, int Cin, int N, int center_over_channels, float eps, float plane_scale, cocos_stream_t stream);
/* cocos_proj1x1_dw_f16x3 (below) with dy rebuilt on the fly: dy = coef[:,0] in1 + coef[:,1] in2 + coef[:,2].  mode 1: in2a = fp32
 * [B,M,N]; mode 2: in2a / in2b = CHANNEL-major f16 hi / lo planes [B,M,N] of plane_scale * in2.  dy_amax: max|dy| or a bound. */
int cocos_proj1x1_dw_affine_f16x3(int mode, const float* in1, const void* in2a, const void* in2b, const float* coef,
                                  float plane_scale, const float* x, float* ws_dw, float* ws_db, float* dw, float* db, int B,
                                  int C, int M, int N, const float* dy_amax, const float* x_amax, cocos_stream_t stream);
/* The same for TWO projections of one shape (theta and phi of a step) in one launch: half as many, twice as long position chunks
 * per projection (cocos_proj1x1_dw_partials_pair_f16x3 partial tiles each), one reduction launch for both. */
int cocos_proj1x1_dw_partials_pair_f16x3(int B, int C, int M, int N);   /* 0 on bad dims */
int cocos_proj1x1_dw_affine_pair_f16x3(
    int mode, float plane_scale, const float* in1_0, const void* in2a_0, const void* in2b_0, const float* coef0, const float* x0,
    float* ws_dw0, float* ws_db0, float* dw0, float* db0, const float* dy_amax0, const float* x_amax0, const float* in1_1,
    const void* in2a_1, const void* in2b_1, const float* coef1, const float* x1, float* ws_dw1, float* ws_db1, float* dw1, float* db1,
    const float* dy_amax1, const float* x_amax1, const float* plane_scale_dev0 /* nullable */, const float* plane_scale_dev1 /* nullable */,
    int B, int C, int M, int N, cocos_stream_t stream);   /* plane_scale_dev_i (mode 2): device cell with the planes' scale, overrides plane_scale */
/* K25 (round 6, match_kernel 3; csrc/proj_norm_f16x3.hip): the theta / phi projection with NO normalisation, straight to what the
 * match_kernel-3 family reads (correspondence.py:272, :282 + :276-280 / :286-289 without the unfold): per projection x [B,K,N] ->
 *   sum1 = sum_c y, sum2 = sum_c y^2 [B,N] (y = W x + bias) — cocos_unfold3_stats_finish_pair makes mu / a / nrm of both tensors from
 *       them in one launch (cocos_unfold3_stats_fwd's second half);
 *   the f16 hi / lo planes of s * y, position-major [B,N,256] (the x-box GEMM's operands) and channel-major [B,256,N] (nullable pair:
 *       the backward GEMMs' and the weight gradient's operands), *y_scale = s: a power of two from the a-priori bound
 *       K max|w| max|x| + max|bias| (no pass over y; the bound lands in [2^13, 2^14)).  The fp32 projection is never written.
 * Backward: cocos_unfold3_stats_bwd_maps_pair (g1, g2 of both tensors), cocos_proj_bwd_input_planes_f16x3 (K24 mode C: d = in1 +
 * 2 g2 y + g1 with y read back from the position-major planes, dx = W^T d), cocos_proj1x1_dw_affine_pair_f16x3 (mode 2, plane_scale_dev). */
int cocos_proj_raw_planes_stats_f16x3(
    int nprob, const float* x0, const void* wfrag0, const float* w_scale0, const float* bias0, const float* x_amax0, float* sum1_0,
    float* sum2_0, float* y_scale0, void* pos_hi0, void* pos_lo0, void* chan_hi0, void* chan_lo0, const float* x1, const void* wfrag1,
    const float* w_scale1, const float* bias1, const float* x_amax1, float* sum1_1, float* sum2_1, float* y_scale1, void* pos_hi1,
    void* pos_lo1, void* chan_hi1, void* chan_lo1, int B, int K, int N, cocos_stream_t stream);
int cocos_unfold3_stats_finish_pair(const float* s1_0, const float* s2_0, float* mu0, float* a0, float* nrm0, const float* s1_1,
                                    const float* s2_1, float* mu1, float* a1, float* nrm1, int B, int h, int w, float k_unfolded,
                                    float eps, cocos_stream_t stream);
int cocos_unfold3_stats_bwd_maps_pair(const float* mu0, const float* a0, const float* nrm0, const float* dmu0 /* nullable */,
                                      const float* da0 /* nullable */, float* ws0 /* 2*B*h*w */, const float* mu1, const float* a1,
                                      const float* nrm1, const float* dmu1 /* nullable */, const float* da1 /* nullable */,
                                      float* ws1, int B, int h, int w, float k_unfolded, cocos_stream_t stream);
int cocos_proj_bwd_input_planes_f16x3(
    int nprob, const float* in1_0, const void* y_hi0, const void* y_lo0, const float* y_scale0, const float* g1_0, const float* g2_0,
    const void* wtfrag0, const float* w_scale0, float* dx0, float* coef0, float* amax0, const float* in1_1, const void* y_hi1,
    const void* y_lo1, const float* y_scale1, const float* g1_1, const float* g2_1, const void* wtfrag1, const float* w_scale1, float* dx1,
    float* coef1, float* amax1, int B, int Cin, int N, cocos_stream_t stream);
/* K0 weight and bias gradient as one streaming reduction (autograd of correspondence.py:272,:282):
 *     dw[m,c] = sum_{b,n} dy[b,m,n] x[b,c,n]      db[m] = sum_{b,n} dy[b,m,n]   (db, ws_db: both or neither NULL)
 * dy [B,M,N], x [B,C,N] fp32, read once; f16x3 products with the power-of-two scales from dy_amax / x_amax.
 * S = cocos_proj1x1_dw_partials_f16x3(B, C, M, N) partial tiles go through the caller's workspace
 * (ws_dw: S*M*roundup(C,32) floats, ws_db: S*M floats) and are summed on the device; S = 0: shape not supported
 * (needs M <= 256, C <= 448, N % 4 == 0) -> cocos_proj1x1_bwd_f16x3. */
int cocos_proj1x1_dw_partials_f16x3(int B, int C, int M, int N);
int cocos_proj1x1_dw_f16x3(const float* dy, const float* x, float* ws_dw, float* ws_db, float* dw, float* db,
                           int B, int C, int M, int N, const float* dy_amax, const float* x_amax,
                           cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K6  match_kernel = 3 without unfolding (correspondence.py:276-280,:286-289 + :291 + :304, PONO_C):
 *     f[b,p,q] = scale * ( sum_{d in 3x3, p+d and q+d inside} c_raw[b,p+d,q+d] - k_unfolded*mu[b,p]*nu[b,q] )
 *                      * a[b,p] * b[b,q]
 *   c_raw [B,N,N] = theta_b^T phi_b (K = 256, cocos_corr_materialize), N = h*w;
 *   mu, a / nu, b [B,N]: mean and 1/(norm+eps) of the unfolded, centred theta / phi vectors
 *   (3x3 box sums of per-position channel sums — computed by the caller); k_unfolded = 256*9.
 *   bwd: g = dL/df ->  dc_raw = boxdiag(g * a_p * b_q * scale)  and the four reductions
 *        r1[p] = sum_q g b_q nu_q, r2[p] = sum_q g f, c1[q] = sum_p g a_p mu_p, c2[q] = sum_p g f
 *        from which dmu = -k*scale*a*r1, da = r2/a, dnu = -k*scale*b*c1, db = c2/b.
 * ------------------------------------------------------------------------------------- */
int cocos_box3_logits_fwd(const float* c_raw, const float* mu, const float* nu, const float* a,
                          const float* b, float* f, int B, int h, int w, float k_unfolded,
                          float scale, cocos_stream_t stream);
size_t cocos_box3_logits_bwd_workspace_bytes(int B, int h, int w);
int cocos_box3_logits_bwd(const float* g, const float* f, const float* mu, const float* nu,
                          const float* a, const float* b, float* dc_raw, float* r1, float* r2,
                          float* c1, float* c2, void* ws, size_t ws_bytes, int B, int h, int w,
                          float scale, cocos_stream_t stream);
/* Same, and on return *dc_amax_inout = max(*dc_amax_inout, max|dc_raw|) (the cell must hold a finite value >= 0): the
 * scale source of the K3 backward that consumes dc_raw, produced while it is written. */
int cocos_box3_logits_bwd_amax(const float* g, const float* f, const float* mu, const float* nu,
                               const float* a, const float* b, float* dc_raw, float* r1, float* r2,
                               float* c1, float* c2, void* ws, size_t ws_bytes, int B, int h, int w,
                               float scale, float* dc_amax_inout, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K7  softmax + warp from MATERIALISED, KEY-MAJOR logits (correspondence.py:307 + :318/:334/... and
 *     their autograd in one streaming kernel each; P never reaches HBM).  Used by match_kernel = 3.
 *   logits_t [B,Nk,Nq]: logits_t[b,j,i] = f[b,i,j] / temperature
 *   fwd: out[b,c,i] = sum_j softmax_j(logits_t[b,j,i]) v[b,c,j];  lse [B,Nq]
 *   bwd: dlogits_t[b,j,i] = P[i,j] * (sum_c dout[b,c,i] v[b,c,j] - sum_c dout[b,c,i] out[b,c,i])
 * ------------------------------------------------------------------------------------- */
int cocos_logits_softmax_warp_fwd(const float* logits_t, const float* v, float* out, float* lse,
                                  int B, int Nq, int Nk, int Cv, cocos_stream_t stream);
int cocos_logits_softmax_warp_bwd(const float* logits_t, const float* v, const float* out,
                                  const float* lse, const float* dout, float* dlogits_t,
                                  int B, int Nq, int Nk, int Cv, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K8  WTA_scale (correspondence.py:38-77, applied :300-303) fused with the /temperature of :304,
 *     on a materialised [rows, cols] correlation (rows = B*Nq):
 *   fwd: y = (x == rowmax(x) ? x : x*scale) * post_scale;  mask = one BIT per element (x == rowmax),
 *        64 columns per 64-bit word, cocos_wta_scale_mask_bytes(rows, cols) bytes (-1 on bad dims)
 *   bwd: dx = dy * post_scale * (mask ? 1 : 1e-4)   — the reference's hard-coded 1e-4 (:72)
 * ------------------------------------------------------------------------------------- */
long long cocos_wta_scale_mask_bytes(long long rows, int cols);
int cocos_wta_scale_fwd(const float* x, float* y, void* mask, long long rows, int cols,
                        float scale, float post_scale, cocos_stream_t stream);
int cocos_wta_scale_bwd(const float* dy, const void* mask, float* dx, long long rows, int cols,
                        float post_scale, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K9  PONO + SPADE modulation + LeakyReLU, fused (`--PONO` networks):
 *     PositionalNorm2d (normalization.py:63-68) -> SPADE.forward's `normalized * (1 + gamma) + beta`
 *     (normalization.py:148-151) -> the LeakyReLU(0.2) of SPADEResnetBlock.actvn (architecture.py:88-95)
 *   x, gamma, beta, y [B,C,N] fp32 (N = H*W);  C >= 2 (unbiased variance over channels)
 *   fwd: xn = (x - mean_C) / sqrt(var_C + eps);  z = xn*(1+gamma) + beta;  y = z > 0 ? z : slope*z
 *        (slope = 1: no activation, as for norm_s)
 *   bwd: dx, dgamma, dbeta from dy (any of the three may be NULL); statistics are recomputed from x.
 * ------------------------------------------------------------------------------------- */
int cocos_pono_spade_fwd(const float* x, const float* gamma, const float* beta, float* y,
                         int B, int C, int N, float eps, float slope, cocos_stream_t stream);
int cocos_pono_spade_bwd(const float* x, const float* gamma, const float* beta, const float* dy,
                         float* dx, float* dgamma, float* dbeta,
                         int B, int C, int N, float eps, float slope, cocos_stream_t stream);
/* Round 6: the same passes also leaving max|.| of the tensors the next convolutions split (*cell = max(*cell, max|.|); cells holding
 * finite values >= 0): the forward's y — the input of conv_0 / conv_1 / conv_s (architecture.py:88-95) — and the backward's dgamma /
 * dbeta — the output gradients of SPADE's mlp_gamma / mlp_beta (normalization.py:121-127): amax2 = [max|dgamma|, max|dbeta|].
 * amax_partials = workspace of cocos_pono_spade_amax_partials(B, C, N) floats (forward) resp. twice that (backward). */
int cocos_pono_spade_amax_partials(int B, int C, int N);
int cocos_pono_spade_fwd_amax(const float* x, const float* gamma, const float* beta, float* y, float* y_amax_inout_dev,
                              float* amax_partials, int B, int C, int N, float eps, float slope, cocos_stream_t stream);
int cocos_pono_spade_bwd_amax(const float* x, const float* gamma, const float* beta, const float* dy,
                              float* dx, float* dgamma, float* dbeta, float* amax2_inout_dev, float* amax_partials,
                              int B, int C, int N, float eps, float slope, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K11 nearest-neighbour up-sampling of the warped image (self.upsampling = nn.Upsample(scale_factor=down),
 *     correspondence.py:188, applied at :327) and its backward.  x [planes,h,w] -> y [planes,h*scale,w*scale]
 *     (planes = B*C);  bwd: dx[p,y,x] = sum of the scale x scale block of dy.  (w*scale) % 4 == 0.
 * ------------------------------------------------------------------------------------- */
int cocos_upsample_nearest_fwd(const float* x, float* y, int planes, int h, int w, int scale, cocos_stream_t stream);
int cocos_upsample_nearest_bwd(const float* dy, float* dx, int planes, int h, int w, int scale, cocos_stream_t stream);
/* The head of a row / column pass (csrc/warp_head.hip; correspondence.py:327, :334 and their autograd; K30: also --warp_bilinear and
 * --warp_patch, :184-186, :321, :357, and passes without mask channels).
 *   mode = COCOS_WARP_HEAD_NEAREST   y [B,Ci,h*down,w*down] = nearest up-sampling of channels [0,Ci) of o [B,C,h,w]
 *          COCOS_WARP_HEAD_BILINEAR  y = F.interpolate(o[:, :Ci], scale_factor=down, mode="bilinear", align_corners=False); the
 *                                    backward is its adjoint as a gather in a fixed order (no atomics: reproducible bit for bit)
 *          COCOS_WARP_HEAD_PATCH     y [B,Ci/down^2,h*down,w*down] = F.fold(o[:, :Ci], (h*down, w*down), down, stride=down), a copy:
 *                                    y[b,c,yy*down+i,xx*down+j] = o[b, c*down^2 + i*down + j, yy*w + xx]; Ci % down^2 == 0
 *   cocos_warp_head_fwd_ex: y_bi (optional, nearest mode only) receives the bilinear up-sampling from the same launch (the inference
 *       --show_corr pair).  Ci <= C, (w*down) % 4 == 0, outputs 16-byte aligned.
 *   cocos_warp_head_bwd_ex: g_img [B,Ci,h*down,w*down] = d loss / d warp_out, g_mask [B,Cs,h,w] = d loss / d warp_mask,
 *       o [B,Ci+Cs,h,w] -> dout [B,Ci+Cs,h,w] (the adjoint of y | copy), drow [B,h*w] = sum_c dout * o accumulated in fp64 (the D of
 *       the softmax backward), *amax_inout = max(*amax_inout, max|dout|) — one pass instead of cocos_upsample_nearest_bwd +
 *       cocos_concat2_amax + cocos_rowdot_f64.  g_y [B,Ci,h*w] (optional) is added to rows [0,Ci) of dout before drow and max|dout|
 *       are taken — the image channels' second gradient when they are also the column pass's values (:353-362).  g_img, g_mask and
 *       g_y may each be NULL (a zero gradient), Cs may be 0.  w % 4 == 0, tensors 16-byte aligned. */
#define COCOS_WARP_HEAD_NEAREST 0
#define COCOS_WARP_HEAD_BILINEAR 1
#define COCOS_WARP_HEAD_PATCH 2
int cocos_warp_head_fwd_ex(const float* o, float* y, float* y_bi, int B, int Ci, int C, int h, int w, int down, int mode,
                           cocos_stream_t stream);
int cocos_warp_head_bwd_ex(const float* g_img, const float* g_mask, const float* g_y, const float* o, float* dout, float* drow,
                           float* amax_inout_dev, int B, int Ci, int Cs, int h, int w, int down, int mode, cocos_stream_t stream);
/* Host-side: the bilinear backward's compile-time tap table (down = 2, 4): weight of output index down*x - down/2 + idx, idx in
 * [0, 2*down), on source index x; first / last = x is the first / last source index (clamped taps).  -1: no table for this scale. */
float cocos_warp_head_bilinear_tap(int down, int idx, int first, int last);

/* ---------------------------------------------------------------------------------------
 * K14  value tensor of the first row pass in one kernel (correspondence.py:314, :318-319, :331-334):
 *     out[b, 0:Ci]     = F.avg_pool2d(img, down)                          img [B,Ci,H,W]
 *     out[b, Ci:Ci+Cs] = F.interpolate(seg, scale_factor=1/down, 'nearest') = seg[.., y*down, x*down]
 *   out [B, Ci+Cs, H/down, W/down] (= torch.cat of the two); either part may be absent (count 0, NULL pointer).
 *   Forward only (the exemplar image and its label map are data).  H, W multiples of down. */
int cocos_warp_values(const float* img, const float* seg, float* out, int B, int Ci, int Cs, int H, int W,
                      int down, cocos_stream_t stream);
/* Same, and *amax_inout_dev = max(*amax_inout_dev, max|out|): the scale source of the K2 forward's f16 split of V comes out
 * of the kernel that writes V. */
int cocos_warp_values_amax(const float* img, const float* seg, float* out, int B, int Ci, int Cs, int H, int W,
                           int down, float* amax_inout_dev, cocos_stream_t stream);
/* --warp_patch (:311): out[b, 0:Ci*down^2] = F.unfold(img, down, stride=down) — out[b, c*down^2 + i*down + j, y, x] =
 * img[b, c, y*down + i, x*down + j], a copy — followed by the Cs nearest-sampled label channels as above;
 * out [B, Ci*down^2 + Cs, H/down, W/down].  amax_inout_dev may be NULL (no maximum wanted). */
int cocos_warp_values_patch_amax(const float* img, const float* seg, float* out, int B, int Ci, int Cs, int H, int W,
                                 int down, float* amax_inout_dev, cocos_stream_t stream);

/* Plane preparation folded into kernels that already touch the data (csrc/plane_prep.hip):
 *   cocos_concat2_amax: out[b] = [a[b] | b[b]] (torch.cat of two [B, *] fp32 tensors along dim 1; na, nb = elements per
 *       sample, multiples of 4) and *amax_inout_dev = max(., max|out|) — the backward of the row pass's output split, whose
 *       result is the `dout` of the K2 backward.
 *   cocos_split_f16_chan_mask: cocos_split_f16_ex(transpose = 0, amax_dev) + cocos_f16_plane_block_mask(lo) in one launch.
 *   cocos_proj_weight_planes: the f16 hi/lo planes of a 1x1-projection weight w [Cout][Cin] in both orientations —
 *       rows [Cout][KpadIn] (= cocos_split_f16_rows) and, when t_hi/t_lo are given, transposed [Cin][KpadOut]
 *       (= cocos_split_f16_ex(transpose = 1, Cpad = KpadOut)) — scaled by the power of two from *amax_dev. */
int cocos_concat2_amax(const float* a, const float* b, float* out, int B, long long na, long long nb,
                       float* amax_inout_dev /* nullable */, cocos_stream_t stream);
int cocos_split_f16_chan_mask(const float* x, void* hi, void* lo, int B, int C, int N, const float* amax_dev,
                              float* scale_out_dev /* nullable */, unsigned* mask_inout_dev /* nullable */,
                              cocos_stream_t stream);
int cocos_proj_weight_planes(const float* w, void* rows_hi, void* rows_lo, void* t_hi /* nullable */,
                             void* t_lo /* nullable */, int Cout, int Cin, int KpadIn, int KpadOut, const float* amax_dev,
                             float* scale_out_dev /* nullable */, cocos_stream_t stream);

/* Small reductions that used to be framework calls inside the autograd Functions:
 *   cocos_sum_leading: out[i] = sum_s x[s][i] over [S][n] partial tiles (weight-gradient partials of the general GEMMs);
 *   cocos_channel_sum: db[c] = sum_{b,n} dy[b][c][n] (the bias gradient of a convolution, dy.sum((0,2,3)));
 *   cocos_box3_stat_grads: dmu = -k s a r1, dnu = -k s b c1, da = r2 / a, db = c2 / b from K6's row / column sums. */
int cocos_sum_leading(const float* x, float* out, int S, long long n, cocos_stream_t stream);
int cocos_channel_sum_slices(int C, long long N);   /* S: `partials` of cocos_channel_sum holds S * C floats */
int cocos_channel_sum(const float* dy, float* db, float* partials, int B, int C, long long N, cocos_stream_t stream);
int cocos_box3_stat_grads(const float* r1, const float* r2, const float* c1, const float* c2, const float* a, const float* b,
                          float* dmu, float* dnu, float* da, float* db, long long n, float k_unfolded, float scale,
                          cocos_stream_t stream);

/* K7 on the f16 MFMA (same contract as cocos_logits_softmax_warp_fwd / _bwd; operand planes as for K2's split flavour):
 *   fwd: vh,vl [B,Cv,Nk] channel-major planes of s_v*v, s_v = *v_scale_dev (NULL = 1; undone in the epilogue); Nk % 4 == 0
 *   bwd: vph,vpl [B,Nk,CvPad] and gph,gpl [B,Nq,CvPad] position-major planes of s_v*v and of (*g_scale_dev)*dout
 *        (cocos_split_f16_ex), out/dout fp32 for D; writes dlogits_t fp32. */
int cocos_logits_softmax_warp_fwd_f16x3(const float* logits_t, const void* vh, const void* vl, float* out, float* lse,
                                        const float* v_scale_dev /* nullable */, int B, int Nq, int Nk, int Cv,
                                        cocos_stream_t stream);
int cocos_logits_softmax_warp_bwd_f16x3(const float* logits_t, const void* vph, const void* vpl, const void* gph,
                                        const void* gpl, const float* g_scale_dev, const float* v_scale_dev /* nullable */,
                                        const float* out, const float* dout, const float* lse, float* dlogits_t, int B,
                                        int Nq, int Nk, int Cv, int CvPad, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K15 row reductions of the contextual loss (ContextualLoss_forward.forward,
 *     models/networks/ContextualLoss.py:121-133, after its cosine-similarity matmul = cocos_corr_materialize):
 *       d = 1 - cos;  d_norm = d / (min_j d + eps);  w = exp((1 - d_norm) / h);  A = w / sum_j w;  cx[i] = max_j A[i,j]
 *     = 1 / sum_j exp((cos[i,j] - m_i) s_i),  m_i = max_j cos[i,j],  s_i = 1 / (h (1 - m_i + eps)).
 *   cosm [rows, cols] fp32 (rows = B * positions of X), 1 <= cols <= 4096; one read of the matrix forward, one read +
 *   one write backward (row statistics recomputed).  bwd: dcos[i,j] = dcx[i] * d cx[i] / d cos[i,j], including the
 *   path through the row maximum (first index on ties, like torch.min's gradient).
 * ------------------------------------------------------------------------------------- */
int cocos_contextual_rows_fwd(const float* cosm, float* cx, long long rows, int cols, float h, float eps,
                              cocos_stream_t stream);
int cocos_contextual_rows_bwd(const float* cosm, const float* dcx, float* dcos, long long rows, int cols, float h,
                              float eps, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K22 the contextual loss WITHOUT its [N, N] matrices (round 5; replaces cocos_corr_materialize + K15 inside
 *     ContextualLoss_forward.forward, models/networks/ContextualLoss.py:93-137, for any N and C):
 *       cx[i] = 1 / S_i,  S_i = sum_j exp((cos_ij - m_i) tau_i),  m_i = max_j cos_ij,  tau_i = 1 / (h (1 - m_i + eps))
 *     forward: one launch, a workgroup owns 128 queries and sweeps the keys twice (maximum, then sums); each sweep is a K = C
 *     GEMM on the f16 MFMA with split operands (three terms, fp32 accumulate), the cosine tile never leaves the registers.
 *     backward: G_ij = a_i e_ij (+ a term on column argmax_j only, which the caller applies as a gather / scatter-add):
 *       d Xn[:, i] = sum_j G_ij Yn[:, j],   d Yn[:, j] = sum_i G_ij Xn[:, i]
 *     — one launch per side; per 128 x 128 tile the cosines are recomputed, exponentiated, written to LDS as f16 hi / lo planes
 *     and multiplied with the other side's channel-major planes (256 output channels per workgroup).
 *   Planes: position-major [B][Np][Kp] f16 hi / lo of the normalised features times a power-of-two device scale
 *   (cocos_split_f16_ex), Np % 128 == 0, Kp % 32 == 0, zero beyond the real positions / channels; channel-major value planes
 *   [B][Cv][Nip].  All statistics fp32 [B][N].
 * ------------------------------------------------------------------------------------- */
int cocos_contextual_cx_fwd_f16x3(const void* xh, const void* xl, const void* yh, const void* yl, const float* x_scale_dev,
                                  const float* y_scale_dev, float* m_out /* max_j cos */, float* s_out /* S */,
                                  float* u_out /* sum_j e_ij (cos_ij - m_i) */, int* j_out /* argmax_j, first */, int B, int Nq,
                                  int Nk, int Nqp, int Nkp, int Kp, float h, float eps, cocos_stream_t stream);
/* out[b][ch][r] = host_scale * (*mul_dev) * beta[r] * sum_c (alpha[c] / *alpha_div_dev) exp2((cos_rc - m) t) V[ch][c]
 *                 (+ gather_coef[r] * gather_src[b][ch][gather_idx[r]]: the argmax column's term of d Xn, from the fp32 values);
 * (m, t = tau log2 e) per QUERY: indexed by r when stats_on_rows (rows = queries, inner = keys: d Xn), by c otherwise (rows = keys,
 * inner = queries: d Yn).  |alpha / alpha_div| <= 1.  alpha, alpha_div_dev, beta, mul_dev, gather_* nullable. */
int cocos_contextual_cx_bwd_f16x3(const void* rh, const void* rl, const void* ih, const void* il, const void* vh, const void* vl,
                                  const float* r_scale_dev, const float* i_scale_dev, const float* v_scale_dev,
                                  const float* mul_dev /* nullable */, const float* m, const float* t,
                                  const float* alpha /* nullable */, const float* alpha_div_dev /* nullable */,
                                  const float* beta /* nullable */, const float* gather_src /* nullable: [B][Cv][Ni] */,
                                  const int* gather_idx, const float* gather_coef, float* out, int B, int Nr, int Ni, int Nrp,
                                  int Nip, int Kp, int Cv, int stats_on_rows, float host_scale, cocos_stream_t stream);
/* The backward's per-query coefficients (n = B * Nq) from the forward's statistics and d loss / d cx:  a = dS tau with
 * dS = -dcx / S^2, tau = 1 / (h (1 - m + eps));  t2 = tau log2 e;  extra = dS (h tau^2 U - tau S);  *a_amax_dev = max |a| (zero on entry). */
int cocos_contextual_cx_coeffs(const float* dcx, const float* S, const float* U, const float* m, float* a_out, float* t2_out,
                               float* extra_out, float* a_amax_dev, long long n, float h, float eps, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K18 nn.ReflectionPad2d(pad) and its backward: the pad in front of the 3x3 convolutions of ResidualBlock
 *     (correspondence.py:19,:23), SPADE (normalization.py:118,:146) and SPADEResnetBlock (architecture.py:30).
 *   fwd: x [planes,H,W] -> y [planes,H+2pad,W+2pad];  bwd: dy -> dx as a gather (no atomics).  pad < H, W.
 * ------------------------------------------------------------------------------------- */
int cocos_reflect_pad2d_fwd(const float* x, float* y, long long planes, int H, int W, int pad, cocos_stream_t stream);
int cocos_reflect_pad2d_bwd(const float* dy, float* dx, long long planes, int H, int W, int pad, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K17 SPADE modulation + LeakyReLU behind any parameter-free norm (the non-PONO branch of SPADE, normalization.py
 *     :93-101 instance | syncbatch | batch, then :148 and architecture.py:88-95): xh = the normalised activations,
 *     gamma, beta, y and the gradients all hold n fp32 elements (same shape).
 *   fwd: y = leaky_relu(xh*(1+gamma) + beta, slope)       bwd: dxh, dgamma, dbeta (any may be NULL), z recomputed
 * ------------------------------------------------------------------------------------- */
int cocos_spade_modulate_fwd(const float* xh, const float* gamma, const float* beta, float* y, long long n, float slope,
                             cocos_stream_t stream);
int cocos_spade_modulate_bwd(const float* xh, const float* gamma, const float* beta, const float* dy, float* dxh,
                             float* dgamma, float* dbeta, long long n, float slope, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K26 parameter-free batch / sync-batch / instance norm + SPADE modulation + LeakyReLU, fused (the non-PONO branch of SPADE,
 *     normalization.py:93-101 and :148, architecture.py:88-95) — K9's counterpart for the norms whose statistics span the batch:
 *   x, gamma, beta, y, dy and the gradients [B,C,N] fp32 (N = H*W).  Statistics group g: channel c over (B, N) for
 *   per_sample = 0 (batch / sync-batch), plane (b, c) over N for per_sample = 1 (instance); G = C resp. B*C.
 *   xhat = (x - mean_g) * invstd_g;  z = xhat*(1+gamma) + beta;  y = z > 0 ? z : slope*z   (slope = 1: no activation)
 *   workspace: cocos_norm_spade_workspace_floats(B, C, N) floats, 16-byte aligned (partials of the passes below).
 *   stats:     one pass over x -> stats [4][G] = count, mean, M2 (sum of squared deviations), 1/sqrt(M2/count + eps).
 *              Per-workgroup partials merged (Chan) by a finishing kernel of the same call: bitwise reproducible, no atomics.
 *   apply:     y from x, gamma, beta and per-group mean / invstd (batch statistics, or the running buffers in eval mode);
 *              y_amax_inout_dev (nullable) = max(*cell, max|y|), the workspace then holds the per-workgroup maxima.
 *   bwd_stats: one pass over x, gamma, beta, dy (z recomputed) -> sums [2][G] = sum dxhat, sum dxhat * xhat,
 *              dxhat = dy * act'(z) * (1 + gamma).
 *   bwd_apply: any of dx, dgamma, dbeta (NULL = not wanted):  dgamma = dz * xhat, dbeta = dz = dy * act'(z),
 *              dx = invstd * (dxhat - sums[0]*inv_count - xhat * sums[1]*inv_count);  sums NULL = constant statistics (eval):
 *              dx = invstd * dxhat.  amax2_inout_dev (nullable) = [max|dgamma|, max|dbeta|] as for cocos_pono_spade_bwd_amax.
 * ------------------------------------------------------------------------------------- */
int cocos_norm_spade_workspace_floats(int B, int C, int N);
int cocos_norm_spade_stats(const float* x, float* stats, float* workspace, int B, int C, int N, int per_sample, float eps,
                           cocos_stream_t stream);
int cocos_norm_spade_apply(const float* x, const float* gamma, const float* beta, const float* mean, const float* invstd, float* y,
                           float* y_amax_inout_dev, float* workspace, int B, int C, int N, int per_sample, float slope,
                           cocos_stream_t stream);
int cocos_norm_spade_bwd_stats(const float* x, const float* gamma, const float* beta, const float* dy, const float* mean,
                               const float* invstd, float* sums, float* workspace, int B, int C, int N, int per_sample, float slope,
                               cocos_stream_t stream);
int cocos_norm_spade_bwd_apply(const float* x, const float* gamma, const float* beta, const float* dy, const float* mean,
                               const float* invstd, const float* sums, float inv_count, float* dx, float* dgamma, float* dbeta,
                               float* amax2_inout_dev, float* workspace, int B, int C, int N, int per_sample, float slope,
                               cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K27 the glue between the convolutions of the fixed VGG19 feature extractor (VGG19_feature_color_torchversion,
 *     correspondence.py:79-146; vgg_preprocess, util/util.py:45-54) — every result BITWISE equal to the framework's fp32 ops on
 *     the same input (same operations in the same order, no contraction).  Out-of-place: no output may alias an input.
 *   amax_inout_dev (nullable, every entry that has it): *cell = max(*cell, max|out|) for the tensor named below, as uint bits
 *   (the cell must hold a finite value >= 0, e.g. 0; a NaN in the output leaves a NaN) — the scale of the next K16 layer's split.
 *   preprocess_fwd: x, y [B,3,H,W]: y[:, c] = (x'[:, 2-c] - mean_bgr[c]) * 255, x' = (x + 1) / 2 if normal_correct else x,
 *                   mean_bgr = (0.40760392, 0.45795686, 0.48501961).  Cell: max|y|.
 *   preprocess_bwd: dx[:, c] = dy[:, 2-c] * 255 (then / 2 if normal_correct).
 *   relu_fwd:       r = relu(y) over n elements, a NaN kept (torch.relu).  Cell: max|r|.
 *   relu_bwd:       dy = src <= 0 ? 0 : dr (threshold_backward: a select, NaN passes; src = r or the pre-activation y).
 *                   Cell: max|dy|.
 *   relu_pool2_fwd: y [BC,H,W] -> p [BC,H/2,W/2] = pool2x2(relu(y)) (floor), and r [BC,H,W] = relu(y) when r is non-NULL, from
 *                   one read of y.  mode 0 = max (first maximum in scan order, NaN wins: max_pool2d), 1 = avg (sum in scan order,
 *                   / 4: avg_pool2d).  Cell: max|p|.
 *   relu_pool2_bwd: dy [BC,H,W] = (dr + route(dp)) where !(src <= 0), else 0; route = dp to the window's arg-max (recomputed from
 *                   relu(src): no index tensor) or dp / 4 to each of its four elements (avg); rows / columns cut by the floor get
 *                   dr only.  dr [BC,H,W] and dp [BC,H/2,W/2] are each nullable (= zero).  src = r or y.  Cell: max|dy|.
 *   H < 2 or W < 2 (no 2x2 window) -> COCOS_ERR_UNSUPPORTED.  Element indices are 64-bit.
 * ------------------------------------------------------------------------------------- */
int cocos_vgg_preprocess_fwd(const float* x, float* y, float* amax_inout_dev, int B, int H, int W, int normal_correct,
                             cocos_stream_t stream);
int cocos_vgg_preprocess_bwd(const float* dy, float* dx, int B, int H, int W, int normal_correct, cocos_stream_t stream);
int cocos_relu_fwd(const float* y, float* r, float* amax_inout_dev, long long n, cocos_stream_t stream);
int cocos_relu_bwd(const float* dr, const float* src, float* dy, float* amax_inout_dev, long long n, cocos_stream_t stream);
int cocos_relu_pool2_fwd(const float* y, float* r /* nullable */, float* p, float* amax_inout_dev, int BC, int H, int W, int mode,
                         cocos_stream_t stream);
int cocos_relu_pool2_bwd(const float* src, const float* dr /* nullable */, const float* dp /* nullable */, float* dy,
                         float* amax_inout_dev, int BC, int H, int W, int mode, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K28 the loss block of Pix2PixModel.compute_generator_loss / compute_discriminator_loss (pix2pix_model.py:205-296,
 *     util/util.py:36-43, networks/loss.py:15-97) as reductions: one launch per GROUP of tensors + a one-workgroup finishing
 *     kernel in the same call.  Per-element arithmetic fp32 in the framework's order, sums fp64 (lane -> wave -> workgroup ->
 *     one partial per workgroup, added in a fixed order: bitwise reproducible, no atomics on a value), one rounding at the end.
 *     Nothing tensor-sized is saved: the backward entries recompute and write each gradient once; the upstream gradient is
 *     read from device memory.  The tables (a, b, w, da, n, inner, c_l1, c_mse, x, dx) are HOST arrays of nseg entries, copied
 *     into the kernel arguments; the tensors they name are device memory.
 *   loss_partials(nseg, n): workgroups (= fp64 partial slots; pair_loss needs 2 doubles per slot, gan_loss 1) of a launch over
 *                   segments of n[s] elements; 0 for invalid arguments.
 *   pair_loss_fwd:  segment s contributes L1_s = c_l1[s] * mean(w[s][i / inner[s]] * |a - b|) and
 *                   L2_s = c_mse[s] * mean((a - b)^2) over its n[s] elements; w (table or entry) nullable = 1, b (table or
 *                   entry) nullable = 0, inner (table) nullable = n; inner[s] must divide n[s].  A coefficient of 0 switches
 *                   its term off.  out [nseg + 1][2]: (L1_s, L2_s) per segment, then (sum_s L1_s, sum_s L2_s).
 *                   1 <= nseg <= COCOS_PAIR_LOSS_MAX_SEGMENTS.  16-byte loads when a, b are 16-byte aligned (and inner % 4 == 0
 *                   where there are weights), a scalar route otherwise.
 *   pair_loss_bwd:  da[s] = g1 * c_l1 * w * sign(a - b) / n + g2 * c_mse * 2 (a - b) / n (sign(0) = 0), with
 *                   g1 = gout[s][0] + gout[nseg][0], g2 = gout[s][1] + gout[nseg][1]; gout [nseg + 1][2] on the device.  A NULL
 *                   da[s] skips the segment.  b and w get no gradient.
 *   gan_loss_fwd:   out[0] = (sum_t m_t) / nt over nt <= COCOS_GAN_LOSS_MAX_TENSORS tensors x[t] of n[t] elements, m_t by mode:
 *                   HINGE_D_REAL -mean(min(x - 1, 0)), HINGE_D_FAKE -mean(min(-x - 1, 0)), NEG_MEAN -mean(x), MEAN mean(x),
 *                   LS mean((x - label)^2), BCE mean((1 - label) x - log_sigmoid(x)) (binary_cross_entropy_with_logits against
 *                   the constant label).
 *   gan_loss_bwd:   dx[t] = g[0] * d m_t / d x / nt; a hinge argument exactly at the kink gets half (torch.min's rule).
 *   mask_nll_fwd:   p [B,nc,h,w] (h = H / 4, w = W / 4, floor), gt [B,H,W] and ref [B,Hr,Wr] int64 label maps, both sampled as
 *                   F.interpolate(scale_factor = 0.25, mode = 'nearest') samples them (source index min(4 * dst, size - 1)).
 *                   weight = 1 where the ground-truth class is not 0 and occurs in the sample's downsampled reference map;
 *                   out[0] = sum(weight * -log(p[gt] + 1e-10)) / (sum(weight) + 1e-5), out[1] = sum(weight);
 *                   present [B][COCOS_MASK_NLL_MAX_CLASSES / 32]: the reference's class sets, kept for the backward.  A label
 *                   outside [0, nc) has weight 0 and is never used as an index.  partials: 2 doubles per slot of
 *                   mask_nll_partials(B, H, W).  nc > COCOS_MASK_NLL_MAX_CLASSES or a label map (either one) smaller than 4x4 ->
 *                   COCOS_ERR_UNSUPPORTED.
 *   mask_nll_bwd:   dp (dense, every element written) = -g[0] / (sum_w[0] + 1e-5) / (p + 1e-10) on the ground-truth channel of
 *                   a weighted pixel, else 0.
 * ------------------------------------------------------------------------------------- */
#define COCOS_PAIR_LOSS_MAX_SEGMENTS 16
#define COCOS_GAN_LOSS_MAX_TENSORS 8
#define COCOS_MASK_NLL_MAX_CLASSES 256
#define COCOS_GAN_HINGE_D_REAL 0
#define COCOS_GAN_HINGE_D_FAKE 1
#define COCOS_GAN_NEG_MEAN 2
#define COCOS_GAN_MEAN 3
#define COCOS_GAN_LS 4
#define COCOS_GAN_BCE 5
int cocos_loss_partials(int nseg, const long long* n);
int cocos_pair_loss_fwd(int nseg, const float* const* a, const float* const* b /* nullable */, const float* const* w /* nullable */,
                        const long long* n, const long long* inner /* nullable */, const float* c_l1, const float* c_mse,
                        double* partials, float* out, cocos_stream_t stream);
int cocos_pair_loss_bwd(int nseg, const float* const* a, const float* const* b /* nullable */, const float* const* w /* nullable */,
                        float* const* da, const long long* n, const long long* inner /* nullable */, const float* c_l1,
                        const float* c_mse, const float* gout, cocos_stream_t stream);
int cocos_gan_loss_fwd(int nt, const float* const* x, const long long* n, int mode, float label, double* partials, float* out,
                       cocos_stream_t stream);
int cocos_gan_loss_bwd(int nt, const float* const* x, float* const* dx, const long long* n, int mode, float label, const float* g,
                       cocos_stream_t stream);
int cocos_mask_nll_partials(int B, int H, int W);
int cocos_mask_nll_fwd(const float* p, const long long* gt, const long long* ref, int B, int nc, int H, int W, int Hr, int Wr,
                       double* partials, unsigned* present, float* out, cocos_stream_t stream);
int cocos_mask_nll_bwd(const float* p, const long long* gt, const unsigned* present, const float* sum_w, const float* g, float* dp,
                       int B, int nc, int H, int W, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K29 the tail of the training step (trainers/pix2pix_trainer.py:57,61-62,73): torch.optim.Adam over a parameter list and the
 *     reference's EMA update (models/networks/generator.py:268-274) as multi-tensor launches (csrc/optim_step.hip).  `entries` and
 *     `groups` are HOST arrays; the function copies them, COCOS_OPTIM_TABLE_ENTRIES at a time, into the kernel arguments of one
 *     launch each — no copy to the device, no allocation, no synchronisation.  A tensor of more than COCOS_OPTIM_ENTRY_ELEMS
 *     elements takes ceil(n / COCOS_OPTIM_ENTRY_ELEMS) table entries; launches = ceil(table entries / COCOS_OPTIM_TABLE_ENTRIES)
 *     (an Adam launch also ends when its entries name more than COCOS_OPTIM_TABLE_GROUPS different groups); both calls leave
 *     the number of kernel launches they made in *launches_out (host, nullable).  cocos_optim_constant(which) returns the
 *     COCOS_OPTIM_* macro selected by COCOS_OPTIM_CONST_* as the library was built with it (0 for an unknown selector).  A workgroup owns COCOS_OPTIM_CHUNK_ELEMS contiguous elements; 16-byte loads and stores when the
 *     entry's pointers are 16-byte aligned (a gradient that is only 4-byte aligned is read dword by dword, the rest stays
 *     16-byte), dword accesses otherwise.  Every tensor fp32, dense, contiguous.
 *   adam_multi_step:  per element, fp32, each operation rounded on its own, correctly rounded sqrt and division (Adam without
 *                   amsgrad / maximize, torch's single-tensor operation order):
 *                     g' = g + weight_decay * p                              (only if weight_decay != 0)
 *                     m  = m + one_minus_beta1 * (g' - m)                    (beta1 == 0: m = g', m is not read)
 *                     v  = beta2 * v + (one_minus_beta2 * g') * g'
 *                     p  = p - (step_size * m) / (sqrt(v) / bc2_sqrt + eps)
 *                   p, m, v are updated in place, g is only read.  beta outside [0, 1), eps < 0 or bc2_sqrt <= 0 (a step
 *                   count of 0) -> COCOS_ERR_UNSUPPORTED.
 *   ema_multi_update: shadow = fl(fl((float)(1.0 - mu) * p) + fl((float)mu * shadow)) in place: bitwise what
 *                   `(1.0 - mu) * p + mu * shadow` gives in torch for a Python float mu (hence the double).
 * ------------------------------------------------------------------------------------- */
#define COCOS_OPTIM_TABLE_ENTRIES 64          /* table entries (tensors or pieces of one) per launch */
#define COCOS_OPTIM_TABLE_GROUPS 8            /* different cocos_adam_group rows per launch */
#define COCOS_OPTIM_CHUNK_ELEMS 4096          /* elements per workgroup */
#define COCOS_OPTIM_ENTRY_ELEMS (1 << 24)     /* elements per table entry (a multiple of the chunk) */
typedef struct cocos_adam_entry {
    float* p;          /* parameter (device), updated in place */
    const float* g;    /* gradient (device), read only; may be 4-byte aligned */
    float* m;          /* exp_avg (device), updated in place */
    float* v;          /* exp_avg_sq (device), updated in place */
    long long n;       /* elements, >= 1 */
    int group;         /* index into groups */
    int reserved;      /* pads the entry to 48 bytes; ignored */
} cocos_adam_entry;
typedef struct cocos_adam_group {          /* every field formed in double on the host and rounded once to fp32 */
    float step_size;                       /* lr / (1 - beta1^t) */
    float bc2_sqrt;                        /* sqrt(1 - beta2^t) */
    float beta1, one_minus_beta1;
    float beta2, one_minus_beta2;
    float eps;
    float weight_decay;                    /* L2 (added to the gradient), not decoupled */
} cocos_adam_group;
typedef struct cocos_ema_entry {
    float* shadow;     /* running average (device), updated in place */
    const float* p;    /* parameter (device), read only */
    long long n;       /* elements, >= 1 */
} cocos_ema_entry;
#define COCOS_OPTIM_CONST_TABLE_ENTRIES 0
#define COCOS_OPTIM_CONST_TABLE_GROUPS 1
#define COCOS_OPTIM_CONST_CHUNK_ELEMS 2
#define COCOS_OPTIM_CONST_ENTRY_ELEMS 3
int cocos_optim_constant(int which);
int cocos_adam_multi_step(const cocos_adam_entry* entries, int n_entries, const cocos_adam_group* groups, int n_groups,
                          int* launches_out /* host, nullable */, cocos_stream_t stream);
int cocos_ema_multi_update(const cocos_ema_entry* entries, int n_entries, double mu, int* launches_out /* host, nullable */,
                           cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K32 weight preparation for frozen-weight inference (cocosnet_amd/inference.py; csrc/weight_prepare_multi.hip): the max|w| cells
 *     and the operand planes of MANY weights per launch.  `entries` are HOST arrays, copied COCOS_WPREP_TABLE_ENTRIES at a time into
 *     the kernel arguments (as K29); *launches_out (host, nullable) receives the number of kernel launches made.
 *   weight_absmax_multi: *cell = max|w[0..n)| for every entry (the cell is WRITTEN, not accumulated): one workgroup per
 *       COCOS_WPREP_ABSMAX_CHUNK elements leaves its maximum in `workspace` (device, >= cocos_weight_absmax_multi_workspace_floats
 *       floats), one finishing workgroup per entry reduces them — two launches per table, no atomics.  Bitwise cocos_absmax.
 *   weight_planes_multi: per entry the planes of ONE layout of w [Cout][Cin][KH][KW], scaled by the power of two that brings *amax
 *       into [2^9, 2^10) (written to *scale_out), byte for byte what the single-tensor routine writes:
 *         COCOS_WPREP_CONV_FWD / _DGRAD            cocos_conv2d_weight_planes mode 0 / 1 (whole kernel: J = K, r = 0, s = 1); hi, lo
 *         COCOS_WPREP_CONV_FWD_BF16 / _DGRAD_BF16  ... mode 2 / 3: one bf16 plane in hi; lo, amax, scale_out unused
 *         COCOS_WPREP_ROWS                         cocos_split_f16_rows(rows = Cout, cols = Cin*KH*KW, cols_pad = aux, amax given);
 *                                                  aux a multiple of 8
 *         COCOS_WPREP_FRAG                         cocos_proj_weight_frag_planes (no transposed planes) of w [256][Cin]: hi = the
 *                                                  cocos_proj_weight_frag_bytes(Cin) buffer, lo unused
 *       Planes 16-byte aligned.
 * ------------------------------------------------------------------------------------- */
#define COCOS_WPREP_TABLE_ENTRIES 64          /* table entries per launch */
#define COCOS_WPREP_ABSMAX_CHUNK 8192         /* elements per workgroup of the max|w| pass */
#define COCOS_WPREP_CONV_FWD 0
#define COCOS_WPREP_CONV_DGRAD 1
#define COCOS_WPREP_CONV_FWD_BF16 2
#define COCOS_WPREP_CONV_DGRAD_BF16 3
#define COCOS_WPREP_ROWS 4
#define COCOS_WPREP_FRAG 5
typedef struct cocos_wprep_absmax_entry {
    const float* w;    /* weight (device) */
    long long n;       /* elements, >= 1 */
    float* cell;       /* max|w| (device), written */
} cocos_wprep_absmax_entry;
typedef struct cocos_wprep_planes_entry {
    const float* w;       /* weight (device) */
    const float* amax;    /* its max|w| cell (device); NULL for the bf16 layouts */
    void* hi;             /* hi plane / bf16 plane / fragment buffer (device) */
    void* lo;             /* lo plane (device); NULL where unused */
    float* scale_out;     /* the scale the planes carry (device); NULL for the bf16 layouts */
    int layout;           /* COCOS_WPREP_* */
    int Cout, Cin, KH, KW;
    int aux;              /* COCOS_WPREP_ROWS: padded row length */
} cocos_wprep_planes_entry;
#define COCOS_WPREP_CONST_TABLE_ENTRIES 0
#define COCOS_WPREP_CONST_ABSMAX_CHUNK 1
int cocos_weight_prepare_constant(int which);
long long cocos_weight_absmax_multi_workspace_floats(const cocos_wprep_absmax_entry* entries, int n_entries);
int cocos_weight_absmax_multi(const cocos_wprep_absmax_entry* entries, int n_entries, float* workspace, long long workspace_floats,
                              int* launches_out /* host, nullable */, cocos_stream_t stream);
int cocos_weight_planes_multi(const cocos_wprep_planes_entry* entries, int n_entries, int* launches_out /* host, nullable */,
                              cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K16 2-D convolution (cross-correlation, zero padding, like torch.nn.functional.conv2d with groups = 1, one stride /
 *     padding / dilation for both axes)
 *     as an implicit GEMM on the f16 MFMA with split operands (conv_f16x3.hip).  Replaces the nn.Conv2d calls of the
 *     networks in front of and behind the path: ResidualBlock (correspondence.py:13-36: ReflectionPad2d(1) stays a
 *     host-side pad, the 3x3 convolution is this kernel with pad = 0), the adaptor layers (correspondence.py:150-173)
 *     and the k4 s2 layers of the PatchGAN (discriminator.py:92-115).
 *   The contraction index runs over blocks of 32 channels, taps inside:  k = ((ci/32) * T + ky*KW + kx) * 32 + ci%32,
 *   T = KH*KW, channels zero-padded to Cp = 32*ceil(Cin/32), K = cocos_conv2d_kdim(Cin,KH,KW) = T*Cp (a k-block of 32
 *   is 32 channels at one tap; consecutive k-blocks re-read the same channels).
 *   fwd:   x [B,Cin,H,W] fp32, weight planes w_hi/w_lo [K/32][Cout][32] f16 (k-block major so that a tile's rows are
 *          contiguous; zero for ci >= Cin): cocos_split_f16_rows of the re-laid-out weight matrix, whose *scale_out
 *          goes to w_scale_dev (NULL = 1), x_amax_dev = max|x| (NULL: x is O(1)), bias [Cout] or NULL
 *          ->  y [B,Cout,OH,OW] fp32, OH = cocos_conv2d_out_size(H,KH,stride,pad,dilation) (0 when the kernel does not fit).
 *          The input gradient of a stride-1 convolution is the same call on dy with the planes of the flipped,
 *          transposed weight (roles of Cin and Cout swapped) and pad' = dilation*(K-1)-pad; of a strided one
 *          (dilation 1) stride^2 calls of cocos_conv2d_fwd_scatter_f16x3, one per parity class.
 *   wgrad: x, dy [B,Cout,OH,OW] (+ their max|.|, NULL = O(1))  ->  partials [S][Cout][K] fp32 (k as above; entries
 *          with ci >= Cin are written as zeros), S = cocos_conv2d_wgrad_slices(...) slices over the B*OH*OW
 *          positions; the caller sums them (and sums dy over (b,oy,ox) for the bias gradient).
 *   Every tensor (and Cout*K*4) must stay below 2 GiB (32-bit offsets).
 * ------------------------------------------------------------------------------------- */
int cocos_conv2d_out_size(int in, int k, int stride, int pad, int dilation);
int cocos_conv2d_kdim(int Cin, int KH, int KW);
int cocos_conv2d_fwd_f16x3(const float* x, const void* w_hi, const void* w_lo, const float* w_scale_dev /* nullable */,
                           const float* x_amax_dev /* nullable */, const float* bias /* nullable */, float* y,
                           int B, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad, int dilation,
                           cocos_stream_t stream);
/* One parity class of the input gradient of a STRIDED convolution.  For stride s, dx[y,x] only receives the taps with
 * ky = (y+p) mod s (mod s), kx likewise: the pixels of one class (ry,rx) form a grid on which the gradient is a
 * stride-1 convolution of dy with the JH x JW sub-kernel w[:, :, ry::s, rx::s] (flipped, channel roles swapped; planes
 * as for cocos_conv2d_fwd_f16x3).  This entry runs that convolution on x = dy [B,Cin,H,W] with separate row / column
 * padding, an explicit output grid OHo x OWo (reads beyond x are zero) and writes output pixel (oy,ox) of plane (b,m)
 * to y[(b*Cout + m)*y_plane + y_offset + oy*y_pitch + ox*y_col_stride]  (elements). */
int cocos_conv2d_fwd_scatter_f16x3(const float* x, const void* w_hi, const void* w_lo, const float* w_scale_dev,
                                   const float* x_amax_dev, float* y, int B, int Cin, int H, int W, int Cout, int JH, int JW,
                                   int pad_y, int pad_x, int OHo, int OWo, long long y_plane, int y_pitch, int y_col_stride,
                                   long long y_offset, cocos_stream_t stream);
/* The two pieces of host-side glue around the calls above as one launch each:
 *   cocos_conv2d_weight_planes: weight [Cout,Cin,KH,KW] fp32 -> the planes of cocos_conv2d_fwd_f16x3 (mode 0) or of the
 *       input-gradient calls (mode 1: channel roles swapped, sub-kernel w[:, :, ry::s, rx::s] of JH x JW taps, flipped;
 *       stride-1 layers: ry = rx = 0, s = 1, J = K), scaled by the power of two from *amax_dev (-> *scale_out_dev).
 *   cocos_conv2d_wgrad_reduce: partials [S][Cout][K] of cocos_conv2d_wgrad_f16x3 -> dw [Cout,Cin,KH,KW]. */
int cocos_conv2d_weight_planes(const float* w, void* hi, void* lo, int Cout, int Cin, int KH, int KW, int mode, int JH, int JW,
                               int ry, int rx, int s, const float* amax_dev /* nullable */,
                               float* scale_out_dev /* nullable */, cocos_stream_t stream);
int cocos_conv2d_wgrad_reduce(const float* partials, float* dw, int S, int Cout, int Cin, int KH, int KW,
                              cocos_stream_t stream);
int cocos_conv2d_wgrad_slices(int B, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad,
                              int dilation);   /* 0 on bad dims */
int cocos_conv2d_wgrad_f16x3(const float* x, const float* dy, const float* x_amax_dev /* nullable */,
                             const float* dy_amax_dev /* nullable */, float* partials, int B, int Cin, int H, int W,
                             int Cout, int KH, int KW, int stride, int pad, int dilation, cocos_stream_t stream);
/* One-term bf16 flavour of K16 (BASELINE config 3: "bf16 MFMA" for the SPADE generator / PatchGAN convolutions): single
 * bf16 operand planes, ONE v_mfma_f32_32x32x16_bf16 per product, fp32 accumulate, no scales (bf16 has fp32's range).
 *   forward / input gradient: cocos_conv2d_fwd_f16x3 / _fwd_scatter_f16x3 with w_lo = NULL and w_hi = the bf16 plane written
 *       by cocos_conv2d_weight_planes(mode | 2) (lo may be NULL there; scale pointers ignored);
 *   weight gradient: cocos_conv2d_wgrad_bf16 (partials as for the f16x3 entry point).
 * 8 mantissa bits per operand: measured error vs fp64 in tests/test_gpu_conv.py; never used upstream of the correlation. */
int cocos_conv2d_wgrad_bf16(const float* x, const float* dy, float* partials, int B, int Cin, int H, int W, int Cout, int KH,
                            int KW, int stride, int pad, int dilation, cocos_stream_t stream);

/* K19 / K20 — match_kernel = 3 (the reference's DEFAULT, options/base_options.py:70) fused, round 3: replaces
 * F.unfold(k=3) + centre + normalise (correspondence.py:276-280, :286-289), the K = 2304 matmul (:291), /temperature (:304),
 * softmax (:307) and the warp matmul (:318 / :334) — and their autograd — for --PONO_C on a 64- or 128-wide feature grid, without a
 * [B,2304,HW] tensor, without the box-filtered logits matrix and without saved logits.  Decomposition (csrc/box3_common.h):
 *     S[p,q] = sum over the 3x3 offsets d of C[p+d, q+d]   (C = the K = 256 correlation; zero outside the grid)
 *            = ybox(xbox(C)),   xbox along a row (both indices +-1), ybox across rows (both indices +-w)
 *     z[p,q] = scale * a_p * b_q * (S[p,q] - kc * mu_p * nu_q),  kc = 9*256,
 *   mu / a (queries), nu / b (keys): mean and 1 / (norm + eps) of the unfolded, centred vectors (cocos_unfold3_stats_*).
 *   cocos_box3_corr_xbox_f16x3: T = xbox(C) from POSITION-major f16 hi/lo planes of the raw theta / phi ([B][N][K],
 *       scaled by *k_scale_dev / *q_scale_dev as written by cocos_split_f16_ex), keys in the rows.  T is TILE-BLOCKED:
 *       [B][Nk/32][Nq/32] blocks of 4 KB = [g][lane][4] — the accumulator image of a 32x32 MFMA tile (registers 4g..4g+3 of a
 *       lane = keys 8g + 4*(lane>>5) + 0..3, lane & 31 = query), B*Nk*Nq floats in all.
 *   cocos_box3_softmax_warp_fwd_f16x3: out[b,c,p] = sum_q softmax_q(z[p,q]) v[b,c,q], lse [B,Nq]; reads three blocks of T per
 *       tile (the y box) and nothing else of size HWxHW.  v planes channel-major [B,Cv,Nk] (cocos_split_f16_ex).
 *   cocos_box3_softmax_warp_bwd_f16x3: with L = dloss/dz = P * (V.dout - sum_c dout*out) it writes
 *       g_blocked = L * scale * a_p * b_q (= dloss / d ybox(T)[p,q], blocked like T), dmu, da [B,Nq], dnu, db [B,Nk] (column
 *       sums: per-workgroup partials in `colpart`, cocos_box3_softmax_warp_bwd_colpart_bytes, folded by a second launch),
 *       max|g| into *gmax_dev (a zeroed cell on entry; atomic max), and — when psh/psl are given (V is differentiated: the
 *       cycle terms) — the planes of 2^14 P in the [Nq/32][Nk/32] blocked orientation of cocos_hgemm_f16x3 mode 2.
 *       vph/vpl [B,Nk,CvPad], gph/gpl [B,Nq,CvPad]: position-major planes of s_v*v and s_o*dout as for K2 / K7.
 *   cocos_box3_adjoint_planes_f16x3: dC = xbox(ybox(g)) (the filter is self-adjoint) as f16 hi/lo planes scaled by the power of
 *       two written to *scale_out_dev (from *gmax_dev), in [Nq/32][Nk/32] blocks of 2 x [32 queries][16 keys]; then
 *           d theta_raw [256][Nq] = hgemm(A = channel-major planes of phi_raw,  B = dC planes, b_blocked = 3)
 *           d phi_raw   [256][Nk] = hgemm(A = channel-major planes of theta_raw, B = dC planes, b_blocked = 2)
 *       (b_blocked = 3: the same blocks read with n = queries, k = keys).
 *   cocos_box3_fused_supported: 1 when this family takes the shape (64- or 128-wide grid — every BASELINE configuration: 256^2 at
 *       down 4; 512^2 at down 4 and 256^2 at --warp_stride 2 are 128 x 128 — Nq == Nk == h*w, Nq % 256 == 0, Cv <= 160, one sample's
 *       T below 2 GiB); every other match_kernel-3 shape keeps the K3 -> K6 -> K7 chain.  Round 4: on 128-wide grids the x box
 *       exchanges its halo between the two 64-position chunks of an image row (GEMM epilogue: within a wave for the keys,
 *       between neighbouring waves for the queries; K20: four waves per row pair), the y box spans grid_w / 32 tiles, and the
 *       per-key statistics of samples with more than 4096 keys pass through LDS in a ring of 2048-key chunks.
 *   `flags` (round 4): bit 0 (COCOS_BOX3_T_TRANSPOSED) — t_blocked holds T of the OTHER orientation (keys and queries exchanged:
 *       xbox(C)^T = xbox(C^T)); the kernels read block (qb, kt) for (kt, qb) and transpose it in LDS, so the column pass of
 *       the cycle terms (correspondence.py:338,:351) shares the row pass's T — no second correlation GEMM — and the backward
 *       writes g_blocked in the layout of that stored T.  Bit 1 (COCOS_BOX3_G_ACCUMULATE, backward) — g_blocked already holds
 *       another pass's G over the same T: this pass's G is ADDED to it and *gmax_dev (zeroed on entry) receives max|sum|: one
 *       g tensor, one cocos_box3_adjoint_planes_f16x3 and one pair of GEMMs for all passes over a T. */
#define COCOS_BOX3_T_TRANSPOSED 1
#define COCOS_BOX3_G_ACCUMULATE 2
int cocos_box3_fused_supported(int Nq, int Nk, int Cv, int grid_h, int grid_w);
int cocos_box3_corr_xbox_f16x3(const void* k_hi, const void* k_lo, const void* q_hi, const void* q_lo, float* t_blocked,
                               int batch, int Nk, int Nq, int K, int grid_w, const float* k_scale_dev /* nullable */,
                               const float* q_scale_dev /* nullable */, cocos_stream_t stream);
int cocos_box3_softmax_warp_fwd_f16x3(const float* t_blocked, const float* mu_q, const float* a_q, const float* nu_k,
                                      const float* b_k, const void* vh, const void* vl, float* out, float* lse,
                                      const float* v_scale_dev /* nullable */,
                                      const unsigned* v_lo_mask_dev /* nullable: as for cocos_corr_softmax_warp_fwd_f16x3 */,
                                      int B, int Nq, int Nk, int Cv, int grid_h, int grid_w, float k_unfolded, float scale,
                                      int flags, cocos_stream_t stream);
/* K37 — the match readout (K36) of these logits: from the T of cocos_box3_corr_xbox_f16x3 and the K12 statistics, per query p
 *         max_out[b,p] = max_q z[p,q]                  (natural units; z exactly as cocos_box3_softmax_warp_fwd_f16x3 forms it)
 *         idx_out[b,p] = the q of that maximum, the lowest one among equals; always in [0, Nk), also for non-finite input
 *         lse_out[b,p] = log sum_q exp z[p,q]
 *     The forward kernel's T / statistics path without a value tensor: three blocks of T per tile, nothing else of size HWxHW,
 *     no box-filtered logits.  Supported: exactly cocos_box3_fused_supported(Nq, Nk, 1, grid_h, grid_w) (else
 *     COCOS_ERR_UNSUPPORTED; nothing is launched).  flags: COCOS_BOX3_T_TRANSPOSED only (the column direction on the row pass's
 *     T: mu / a then belong to T's keys, nu / b to its queries); any other bit is COCOS_ERR_INVALID.  T, nu, b 16-byte aligned. */
int cocos_box3_match_f16x3(const float* t_blocked, const float* mu_q, const float* a_q, const float* nu_k, const float* b_k,
                           int* idx_out, float* max_out, float* lse_out, int B, int Nq, int Nk, int grid_h, int grid_w,
                           float k_unfolded, float scale, int flags, cocos_stream_t stream);
/* K41 — the top-k match readout (K39) of these logits, from the same T and statistics: per query p the k largest z[p,q]
 *         idx[b,p,r], val[b,p,r] = the key index and the logit (natural units) of rank r = 0 .. k-1;  lse[b,p] = log sum_q exp z[p,q]
 *     (idx [B,Nq,k] int32, val [B,Nq,k], lse [B,Nq]).  One kernel template with cocos_box3_match_f16x3 (K = 1, 2, 4, 8 candidates per
 *     lane; a request for k runs the next one up): idx[..,0], val[..,0] and lse are cocos_box3_match_f16x3's three outputs bit for bit,
 *     and k = 1 IS that call.  Nothing of size HWxHW besides T.
 *     Order: a query's logit is z = tt * a_n with a_n = scale * a_p > 0 its own factor; the candidates are ordered by tt descending and,
 *     among bitwise-equal tt, the lower key index first.  val is therefore non-increasing; two unequal tt whose products round to the
 *     same val keep their tt order.  The k indices of a row are pairwise distinct for finite input; for non-finite input they are
 *     clamped into [0, Nk) as K36 / K37 do and may repeat.
 *     Arguments, supported shapes, flags and alignment as cocos_box3_match_f16x3; k outside 1..COCOS_MATCH_TOPK_MAX or above Nk is
 *     COCOS_ERR_INVALID before any launch; k above cocos_box3_topk_max_k() (the largest instantiation that ships) is
 *     COCOS_ERR_UNSUPPORTED (materialise and use cocos_row_topk_lse). */
int cocos_box3_topk_max_k(void);
int cocos_box3_topk_f16x3(const float* t_blocked, const float* mu_q, const float* a_q, const float* nu_k, const float* b_k,
                          int* idx, float* val, float* lse, int B, int Nq, int Nk, int grid_h, int grid_w, float k_unfolded,
                          float scale, int k, int flags, cocos_stream_t stream);
/* K54 — the biased readout of these logits (the BIAS instantiations of the same kernel template): cocos_box3_topk_f16x3 over
 *         z'[p,q] = z[p,q] + k_bias[b,q]
 *     k_bias fp32 [B,Nk], 16-byte aligned (it is staged into LDS beside the key statistics).  val holds z' (natural units), lse = log
 *     sum_q exp z'[p,q], idx / val the k best z' in K41's order.  The kernel's state lives in the tt domain (z = tt * a_n with a_n =
 *     scale * a_p the query's factor): the bias enters as tt += k_bias / a_n, one fma per element before the tile maximum, the list and
 *     the sum, so a bias of zeros gives cocos_box3_topk_f16x3's three outputs bit for bit.  A finite bias of any sign is legal; -inf
 *     excludes the key; a row with every key excluded has lse = -inf, val = -inf and indices in [0, Nk); finite or -inf input never
 *     produces a NaN.  +inf and NaN are not sanitised; idx stays in [0, Nk).  One launch at k = 1 is one half-step of a log-domain
 *     Sinkhorn iteration over ONE T: f_p = tau (log mu_p - lse_p) with the other side's potential g as the bias; the column half-step is
 *     the same entry with COCOS_BOX3_T_TRANSPOSED, (mu, a) and (nu, b) exchanged and f as the bias.
 *     Arguments, supported shapes, flags, k and error codes of cocos_box3_topk_f16x3; a null k_bias or one that is not 16-byte aligned
 *     is COCOS_ERR_INVALID; all checked before any HIP call. */
int cocos_box3_topk_bias_f16x3(const float* t_blocked, const float* mu_q, const float* a_q, const float* nu_k, const float* b_k,
                               const float* k_bias, int* idx, float* val, float* lse, int B, int Nq, int Nk, int grid_h, int grid_w,
                               float k_unfolded, float scale, int k, int flags, cocos_stream_t stream);
/* K55 — the label-restricted readout of these logits (the LABELS instantiations of the same kernel template): cocos_box3_topk_f16x3
 *     over the allowed pairs only, K47's rule word for word:
 *         allowed(p, q) = q_label[b,p] < 0  ||  q_label[b,p] == k_label[b,q]
 *     q_label int32 [B,Nq], k_label int32 [B,Nk], any values, both 4-byte aligned.  idx / val are the k best allowed keys in K41's
 *     order (tt descending, the lower index first among bitwise-equal tt), lse the log-sum-exp over the allowed keys.  A row with
 *     fewer than k allowed keys has val = -inf on the missing ranks with idx clamped into [0, Nk); a row with none has lse = -inf;
 *     finite input never produces a NaN.  The key labels are staged into LDS beside the key statistics as integer bits and compared
 *     as integers; a disallowed element becomes -inf before the tile maximum, the list and the sum, so with every query label
 *     negative the three outputs are cocos_box3_topk_f16x3's bit for bit.  With COCOS_BOX3_T_TRANSPOSED the labels belong to the
 *     problem's queries and keys after the exchange: the caller swaps the two label arrays together with (mu, a) and (nu, b).
 *     Restriction together with a bias is not built.
 *     Arguments, supported shapes, flags, k and error codes of cocos_box3_topk_f16x3; a null label pointer or one that is not
 *     4-byte aligned is COCOS_ERR_INVALID; all checked before any HIP call. */
int cocos_box3_topk_labels_f16x3(const float* t_blocked, const float* mu_q, const float* a_q, const float* nu_k, const float* b_k,
                                 const int* q_label, const int* k_label, int* idx, float* val, float* lse, int B, int Nq, int Nk,
                                 int grid_h, int grid_w, float k_unfolded, float scale, int k, int flags, cocos_stream_t stream);
size_t cocos_box3_softmax_warp_bwd_colpart_bytes(int B, int Nq, int Nk);
int cocos_box3_softmax_warp_bwd_f16x3(const float* t_blocked, const float* mu_q, const float* a_q, const float* nu_k,
                                      const float* b_k, const void* vph, const void* vpl, const void* gph, const void* gpl,
                                      const float* g_scale_dev, const float* v_scale_dev /* nullable */, const float* out,
                                      const float* dout, const float* lse, float* g_blocked, float* dmu, float* da, float* dnu,
                                      float* db, void* colpart, float* gmax_dev, void* psh /* nullable */,
                                      void* psl /* nullable */, const unsigned* v_lo_mask_dev /* nullable */, int B, int Nq,
                                      int Nk, int Cv, int CvPad, int grid_h, int grid_w, float k_unfolded, float scale,
                                      const float* d_pre /* nullable: D = sum_c dout * out [B][Nq] (cocos_rowdot_f64) */,
                                      int flags, cocos_stream_t stream);
int cocos_box3_adjoint_planes_f16x3(const float* g_blocked, const float* gmax_dev, void* dc_hi, void* dc_lo,
                                    float* scale_out_dev, int B, int Nq, int Nk, int grid_h, int grid_w,
                                    cocos_stream_t stream);
/* K53 — the adjoint of cocos_box3_match_f16x3's log-sum-exp (box3_lse_bwd_f16x3.hip): with lse [B,Nq] that kernel's third output on
 *     the same arguments and g_lse [B,Nq] the upstream gradient on it (any magnitude; null = all zero),
 *         w[p,q] = g_lse[p] exp(z[p,q] - lse[p])        (z formed from T as cocos_box3_match_f16x3 forms it, bit for bit; the
 *                                                        difference is rounded once and clamped at 0 from above: |w| <= |g_lse|)
 *     and the outputs are those of cocos_box3_softmax_warp_bwd_f16x3 with w in the place of its L, in the same convention:
 *         g_blocked = w scale a_p b_q = dloss / d ybox(T)[p,q], fp32, unscaled, tile-blocked like the STORED T (so that
 *                     cocos_box3_adjoint_planes_f16x3 and the two cocos_hgemm_f16x3 launches follow unchanged),
 *         dmu, da [B,Nq] (row sums), dnu, db [B,Nk] (column sums: per-workgroup partials in `colpart`, folded in workgroup order by a
 *         second launch), *gmax_dev = max|g_blocked| (written, not accumulated: the cell need not be zeroed).
 *     colpart: cocos_box3_lse_bwd_colpart_bytes(B, Nq, Nk) bytes (the column partials and one maximum per wave), 16-byte aligned.
 *     flags: COCOS_BOX3_T_TRANSPOSED (the column direction on the row pass's T; g_blocked in the layout of the stored T) and
 *     COCOS_BOX3_G_ACCUMULATE (g_blocked holds another pass's G: this one is added, *gmax_dev receives max|sum|), as for
 *     cocos_box3_softmax_warp_bwd_f16x3; any other bit is COCOS_ERR_INVALID.  Supported: exactly
 *     cocos_box3_fused_supported(Nq, Nk, 1, grid_h, grid_w), else COCOS_ERR_UNSUPPORTED with nothing launched.  T, G, nu, b, colpart
 *     16-byte aligned.  No atomics, every sum in a fixed order: bitwise reproducible. */
size_t cocos_box3_lse_bwd_colpart_bytes(int B, int Nq, int Nk);
int cocos_box3_lse_bwd_f16x3(const float* t_blocked, const float* mu_q, const float* a_q, const float* nu_k, const float* b_k,
                             const float* lse, const float* g_lse /* nullable */, float* g_blocked, float* dmu, float* da, float* dnu,
                             float* db, void* colpart, float* gmax_dev, int B, int Nq, int Nk, int grid_h, int grid_w,
                             float k_unfolded, float scale, int flags, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K12 statistics of the zero-padded 3x3-unfolded, centred feature vectors without unfolding (match_kernel 3 with
 *     PONO_C: correspondence.py:276-280 / :286-289), feeding K6:
 *   fwd: x [B,C,h,w] -> mu[b,p] = mean of the 9*C unfolded entries at p, nrm[b,p] = ||U_p - mu||_2,
 *        a[b,p] = 1/(nrm + eps);  k_unfolded = 9*C;  ws: 2*B*h*w floats of scratch
 *   bwd: dmu, da (either may be NULL) -> dx [B,C,h,w] (written, not accumulated);  ws: 2*B*h*w floats
 * ------------------------------------------------------------------------------------- */
int cocos_unfold3_stats_fwd(const float* x, float* mu, float* a, float* nrm, float* ws,
                            int B, int C, int h, int w, float k_unfolded, float eps, cocos_stream_t stream);
/* Same, and *amax_inout_dev = max(*amax_inout_dev, max|x|): the scale source of the f16 split of x (K19's correlation GEMM). */
int cocos_unfold3_stats_fwd_amax(const float* x, float* mu, float* a, float* nrm, float* ws, int B, int C, int h, int w,
                                 float k_unfolded, float eps, float* amax_inout_dev, cocos_stream_t stream);
int cocos_unfold3_stats_bwd(const float* x, const float* mu, const float* a, const float* nrm,
                            const float* dmu, const float* da, float* dx, float* ws,
                            int B, int C, int h, int w, float k_unfolded, cocos_stream_t stream);
/* ... only its two per-position maps (ws = [g1 | g2]): the consumer applies dx[c,p] = g1[p] + 2 x[c,p] g2[p]
 * (cocos_proj_bwd_input_f16x3 mode 1). */
int cocos_unfold3_stats_bwd_maps(const float* mu, const float* a, const float* nrm, const float* dmu /* nullable */,
                                 const float* da /* nullable */, float* ws /* 2*B*h*w */, int B, int h, int w, float k_unfolded,
                                 cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K13 InstanceNorm2d(affine=False) (+ residual) + PReLU of the ResidualBlocks in front of theta/phi
 *     (correspondence.py:13-36: `prelu(bn1(conv1(..)))` at :29 and `prelu(bn2(conv2(..)) + x)` at :31-33):
 *   x, residual (nullable), y: [planes, N] with planes = B*C, N = h*w;  prelu_weight: 1 float (nn.PReLU())
 *   fwd: z = (x - mean)/sqrt(biased var + eps) (+ residual);  y = z > 0 ? z : a*z
 *   bwd: dx, dresidual (nullable, = dz), da_partials [planes] (nullable; the caller sums them)
 * ------------------------------------------------------------------------------------- */
int cocos_instnorm_prelu_fwd(const float* x, const float* residual, const float* prelu_weight, float* y,
                             int planes, int N, float eps, cocos_stream_t stream);
int cocos_instnorm_prelu_bwd(const float* x, const float* residual, const float* prelu_weight, const float* dy,
                             float* dx, float* dresidual, float* da_partials, int planes, int N, float eps,
                             cocos_stream_t stream);
/* The same with the PReLU weight's gradient accumulated in fp64 from the products to the last addition (round 6: da is one number
 * summed over every element of the layer with cancelling terms): da_partials_f64 = workspace of `planes` doubles, *da_out = the sum. */
int cocos_instnorm_prelu_bwd_f64(const float* x, const float* residual, const float* prelu_weight, const float* dy, float* dx,
                                 float* dresidual, double* da_partials_f64, float* da_out, int planes, int N, float eps,
                                 cocos_stream_t stream);
/* Round 6: the same two passes also leaving max|out| in a device cell (*cell = max(*cell, max|.|); the cell must hold a finite value
 * >= 0) — y is the input of the next convolution / projection (correspondence.py:21, :25, :272, :282) and dx the output gradient of the
 * convolution in front of the norm (:20, :24): both are split into f16 hi / lo planes scaled by that maximum, which used to cost a
 * pass over the tensor each (cocos_absmax).  amax_partials = workspace of `planes` floats: one maximum per plane, reduced into the cell
 * by a one-workgroup kernel of the same call (same-address atomics from 13 k waves serialise at ~10 ns each: measured 5x slower).
 * _bwd_amax: da_partials_f64 / da_out both NULL = no PReLU-weight gradient. */
int cocos_instnorm_prelu_fwd_amax(const float* x, const float* residual, const float* prelu_weight, float* y, float* y_amax_inout_dev,
                                  float* amax_partials, int planes, int N, float eps, cocos_stream_t stream);
int cocos_instnorm_prelu_bwd_amax(const float* x, const float* residual, const float* prelu_weight, const float* dy, float* dx,
                                  float* dresidual, double* da_partials_f64, float* da_out, float* dx_amax_inout_dev, float* amax_partials,
                                  int planes, int N, float eps, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K34 the same InstanceNorm2d(affine=False) (+ residual) + PReLU for planes of ANY size: a plane is cut into
 *     S = ceil(N / 16384) slices, one workgroup each, and every direction is two launches (per-slice partials, then
 *     the apply pass that combines them in a fixed order) — the adaptors' layer1 at the full image size
 *     (correspondence.py:150-173) and the PatchGAN's first norm (discriminator.py:92-115).  No workgroup waits for
 *     another, no atomics: results are bitwise reproducible.  Any planes >= 1, N >= 1 (N % 4 != 0 or tensors that are
 *     not 16-byte aligned take 4-byte accesses).
 *   cocos_instnorm_prelu_split_workspace_floats: floats of `workspace` for either call (host arithmetic, no GPU needed;
 *       0 for planes < 1 or N < 1) = 7 * planes * S: the forward's (mean, M2) and the backward's (sum dz, sum dz xn) per
 *       slice, the fp64 da partials (two floats each) and one maximum per slice.  8-byte aligned.  The same buffer may
 *       serve both calls; its contents need not survive between them.
 *   _fwd: y as K13's; stats [planes][2] = (mean, 1/sqrt(biased var + eps)) of every plane, which _bwd takes instead of
 *       recomputing them (per-slice mean and centred squares, combined by Chan's formula in fp64).
 *       y_amax_inout_dev (nullable): *cell = max(*cell, max|y|), the cell holding a finite value >= 0.
 *   _bwd: dx (nullable), dresidual (nullable, = dz), da_out (nullable): 1 float = sum over the layer of dy z where
 *       z <= 0, accumulated in fp64 from the products to the last addition as cocos_instnorm_prelu_bwd_f64 does.
 *       dx_amax_inout_dev (nullable, needs dx): *cell = max(*cell, max|dx|).  eps is not read (the statistics are given).
 * ------------------------------------------------------------------------------------- */
size_t cocos_instnorm_prelu_split_workspace_floats(int planes, int N);
int cocos_instnorm_prelu_split_fwd(const float* x, const float* residual, const float* prelu_weight, float* y, float* stats,
                                   float* workspace, float* y_amax_inout_dev, int planes, int N, float eps, cocos_stream_t stream);
int cocos_instnorm_prelu_split_bwd(const float* x, const float* residual, const float* prelu_weight, const float* dy,
                                   const float* stats, float* dx, float* dresidual, float* da_out, float* workspace,
                                   float* dx_amax_inout_dev, int planes, int N, float eps, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K35 3x3 convolution of a ONE-HOT label map as nine table look-ups per output pixel (label_conv.hip):
 *       y[b, :, p] = bias + sum_tap W[:, label(p + tap), tap]
 *     exact fp32 sums of at most ten numbers; 4 bytes read per pixel instead of 4 nc; no operand preparation.
 *   cocos_labels_one_hot: label_map int64 [B,1,H,W] -> onehot fp32 [B,nc,H,W] (EVERY element written) and index int32
 *       [B,H,W].  A label outside [0, nc) gives an all-zero column and index -1.  1 <= nc <= 32767.
 *   cocos_label_conv_table: weight [Cout,nc,3,3] -> table [9][nc][Cout] (tap-major; tap = 3 ky + kx).
 *   cocos_label_conv3x3_fwd: index [B,Hs,Ws] on its source grid; the output grid is (Hs/sample) x (Ws/sample) and output
 *       pixel (y, x) stands on source pixel (y sample, x sample) — F.interpolate(mode="nearest") for whole ratios
 *       (Hs, Ws multiples of sample, else COCOS_ERR_UNSUPPORTED).  reflect 0: zero padding 1; 1: ReflectionPad2d(1) of
 *       the sampled grid (needs a 2x2 grid or more).  bias nullable; relu != 0: y = max(y, 0).  An index of -1 (or any
 *       value outside [0, nc)) contributes nothing.  y fp32 [B,Cout,H,W], Cout % 16 == 0; table and bias 16-byte aligned.
 *       y_amax_inout_dev (nullable): *cell = max(*cell, max|y|), the cell holding a finite value >= 0.
 *   cocos_label_conv3x3_bwd_workspace_floats: floats of `workspace` for _bwd at an OUTPUT grid of H x W (host arithmetic;
 *       0 for bad dims): per-slice partial sums, at most 64 MiB + the slices of dbias.
 *   cocos_label_conv3x3_bwd: dweight [Cout,nc,3,3] (every element written: classes that never occur get exact zeros) and
 *       dbias [Cout] (nullable) from dy [B,Cout,H,W].  y_saved (nullable) = the forward's output when it ran with relu:
 *       dy is masked where y_saved <= 0.  No atomics; the order of every sum is fixed by the shapes alone: two calls on
 *       the same inputs give the same bits.  No input gradient exists.
 * ------------------------------------------------------------------------------------- */
int cocos_labels_one_hot(const long long* label_map, float* onehot, int* index, int B, int nc, int H, int W, cocos_stream_t stream);
int cocos_label_conv_table(const float* weight, float* table, int Cout, int nc, cocos_stream_t stream);
int cocos_label_conv3x3_fwd(const int* index, const float* table, const float* bias, float* y, float* y_amax_inout_dev, int B,
                            int Hs, int Ws, int sample, int reflect, int relu, int nc, int Cout, cocos_stream_t stream);
size_t cocos_label_conv3x3_bwd_workspace_floats(int B, int H, int W, int nc, int Cout);
int cocos_label_conv3x3_bwd(const int* index, const float* dy, const float* y_saved, float* dweight, float* dbias,
                            float* workspace, int B, int Hs, int Ws, int sample, int reflect, int nc, int Cout,
                            cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K36 match readout: where each content position matched in the exemplar, and how sure the match is — what a caller of the
 *     reference's forward(return_corr=True) takes with max / argmax over the returned [B,HW,HW] matrix
 *     (correspondence.py:291, :304-307).
 *   cocos_corr_match_f16x3 (K36a, corr_topk_f16x3.hip at K = 1): from the operand planes of cocos_corr_softmax_warp_fwd_f16x3
 *       (qh,ql [B,Nq,256], kh,kl [B,Nk,256]: position-major f16 hi / lo planes of unit-norm columns x operand_scale) and with
 *       that kernel's QK arithmetic (three f16 MFMA terms, fp32 accumulate, same order: the same logits), per query i
 *         max_out[b,i] = max_j inv_temperature <q_i, k_j>            (natural units)
 *         idx_out[b,i] = the j of that maximum, the lowest one among equals; always in [0, Nk), also for non-finite input
 *         lse_out[b,i] = log sum_j exp(inv_temperature <q_i, k_j>)   (confidence of the match: exp(max - lse))
 *       Nothing Nq x Nk reaches memory.  k_batch_stride (halfs): Nk * 256, or 0 = every sample reads the ONE key set at kh, kl
 *       (a prepared exemplar); anything else is COCOS_ERR_INVALID.  Supported: K == 256, Nk % 4 == 0, any Nq >= 1
 *       (otherwise COCOS_ERR_UNSUPPORTED; nothing is launched).  Planes 16-byte aligned.
 *   cocos_row_argmax_lse (K36b, row_topk_lse.hip at K = 1): the same three results from a materialised matrix logits [B,Nq,Nk] in one
 *       sweep (16-byte loads when Nk % 4 == 0 and the base is 16-byte aligned): max is an element of the row, bit for bit;
 *       same tie and range rules.  Any Nq, Nk >= 1.  For every route that holds its logits in memory anyway.
 *   cocos_gather_patches (K36c, gather_warp.hip): the hard warp at full resolution, a bitwise copy:
 *         out[b,c,y down+dy,x down+dx] = img[b_e,c,(j / w) down+dy,(j % w) down+dx],  j = idx[b, y w + x],  h = H / down, w = W / down
 *       img [Be,C,H,W] with img_batch_stride = C H W (b_e = b) or 0 (Be = 1: b_e = 0; anything else is COCOS_ERR_INVALID),
 *       idx [B,h w] int32, out [B,C,H,W].  An index outside [0, h w) is clamped into it.  H, W multiples of down
 *       (else COCOS_ERR_UNSUPPORTED).
 * ------------------------------------------------------------------------------------- */
int cocos_corr_match_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, int* idx_out, float* max_out,
                           float* lse_out, int B, int K, int Nq, int Nk, float inv_temperature, float operand_scale,
                           long long k_batch_stride, cocos_stream_t stream);
int cocos_row_argmax_lse(const float* logits, int* idx, float* max, float* lse, int B, int Nq, int Nk, cocos_stream_t stream);
int cocos_gather_patches(const float* img, const int* idx, float* out, int B, int C, int H, int W, int down,
                         long long img_batch_stride, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K39 top-k match readout: per position the k best candidates instead of the one — what a caller of the reference's
 *     forward(return_corr=True) takes with topk / logsumexp over the returned [B,HW,HW] matrix (correspondence.py:291, :304-307).
 *     Order (all three): logit descending and, among bitwise-equal logits, key index ascending.  The k indices of a row are
 *     pairwise distinct for finite input; for non-finite input they are clamped into [0, Nk) as K36 does and may repeat.
 *     1 <= k <= COCOS_MATCH_TOPK_MAX and k <= Nk, else COCOS_ERR_INVALID before any launch.
 *   cocos_corr_topk_f16x3 (K39a, corr_topk_f16x3.hip, K = 1, 2, 4, 8): operands, arithmetic and limits of cocos_corr_match_f16x3;
 *         idx [B,Nq,k] int32, val [B,Nq,k] (the logits, natural units), lse [B,Nq].
 *       idx[..,0], val[..,0] and lse are cocos_corr_match_f16x3's three outputs bit for bit.  Nothing Nq x Nk reaches memory.
 *       k above cocos_corr_topk_max_k() (the largest fused instantiation that ships), K != 256, Nk % 4 != 0: COCOS_ERR_UNSUPPORTED
 *       (use cocos_row_topk_lse).
 *   cocos_row_topk_lse (K39b, row_topk_lse.hip, K = 1, 2, 4, 8): the same from a materialised matrix logits [B,Nq,Nk] in one sweep; val holds
 *       elements of the row, bit for bit; idx[..,0], val[..,0], lse are cocos_row_argmax_lse's outputs bit for bit.  Any Nq >= 1,
 *       any Nk >= k.
 *   cocos_gather_blend_patches (K39c, gather_warp.hip): the k-sparse warp at full resolution,
 *         out[b,c,y down+dy,x down+dx] = sum_r w[b,r,y,x] img[b_e,c,(j_r / wg) down+dy,(j_r % wg) down+dx],  j_r = idx[b,r,y,x],
 *       hg = H / down, wg = W / down; idx [B,k,hg,wg] int32 (clamped into [0, hg wg)), w [B,k,hg,wg] fp32, img / out /
 *       img_batch_stride as cocos_gather_patches.  fp32, fixed order: acc = w_0 p_0, then acc = fma(w_r, p_r, acc), r = 1 .. k-1;
 *       k = 1 with w = 1 is cocos_gather_patches bit for bit.
 * ------------------------------------------------------------------------------------- */
#define COCOS_MATCH_TOPK_MAX 8
int cocos_corr_topk_max_k(void);
int cocos_corr_topk_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, int* idx_out, float* val_out,
                          float* lse_out, int B, int K, int Nq, int Nk, int k, float inv_temperature, float operand_scale,
                          long long k_batch_stride, cocos_stream_t stream);
int cocos_row_topk_lse(const float* logits, int* idx, float* val, float* lse, int B, int Nq, int Nk, int k, cocos_stream_t stream);
/* K47 label-restricted readout (corr_topk_f16x3.hip, the LABELS instantiations): cocos_corr_topk_f16x3 over the keys a query's label
 *     allows.  q_label [B,Nq], k_label [B,Nk] int32 (k_batch_stride == 0: k_label is the one [Nk] row of the shared key set), 4-byte
 *     aligned, any values;  allowed(i, j) = q_label[i] < 0 || q_label[i] == k_label[j]  (a negative query label: unrestricted; a
 *     negative key label is matched by unrestricted queries only).  A disallowed logit is -inf before the candidate list and the
 *     log-sum-exp: lse is over the allowed keys, idx / val are the k best allowed keys in K39's order.  A row with fewer than k
 *     allowed keys has val = -inf on the missing ranks (idx clamped into [0, Nk)); a row with none has lse = -inf.  No NaN from
 *     finite input.  With every query unrestricted, or one label everywhere, the three outputs are cocos_corr_topk_f16x3's bit for
 *     bit.  Arguments, limits and error codes of cocos_corr_topk_f16x3; a null label pointer is COCOS_ERR_INVALID. */
int cocos_corr_topk_labels_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const int* q_label, const int* k_label,
                                 int* idx_out, float* val_out, float* lse_out, int B, int K, int Nq, int Nk, int k,
                                 float inv_temperature, float operand_scale, long long k_batch_stride, cocos_stream_t stream);
/* K50 biased readout (corr_topk_bias_f16x3.hip, the BIAS instantiations): cocos_corr_topk_f16x3 over z_ij = s_ij + k_bias[b,j].
 *     k_bias fp32 [B,Nk] (k_batch_stride == 0: the one [Nk] row of the shared key set), 4-byte aligned, read through a bounds-checked
 *     descriptor.  val holds z (natural units), lse = log sum_j exp z_ij, idx / val the k best z in K39's order (z descending, the lower
 *     key among bitwise-equal z).  The bias meets the raw accumulator in one fma (raw += bias * operand_scale^2 / inv_temperature), so a
 *     bias of zeros gives cocos_corr_topk_f16x3's three outputs bit for bit.  A finite bias of any sign is legal; -inf excludes the key
 *     (K47's mask is the bias 0 / -inf); a row with every key excluded has lse = -inf, val = -inf and indices in [0, Nk); finite or -inf
 *     input never produces a NaN.  +inf and NaN are not sanitised; idx stays in [0, Nk).  One launch is one half-step of a log-domain
 *     Sinkhorn iteration: f_i = tau (log mu_i - lse_i) with the other side's potential g as the bias; the column half-step is the same
 *     entry with the operand planes exchanged.  Arguments, limits and error codes of cocos_corr_topk_f16x3; a null k_bias is
 *     COCOS_ERR_INVALID; all checked before any HIP call. */
int cocos_corr_topk_bias_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const float* k_bias, int* idx_out,
                               float* val_out, float* lse_out, int B, int K, int Nq, int Nk, int k, float inv_temperature,
                               float operand_scale, long long k_batch_stride, cocos_stream_t stream);
int cocos_gather_blend_patches(const float* img, const int* idx, const float* w, float* out, int B, int C, int H, int W, int down,
                               int k, long long img_batch_stride, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K48 mutual match (corr_match_mutual_f16x3.hip): both softmax directions of the correlation from ONE sweep of Q.K^T, and the round
 *     trip i -> j -> i' on top — the validity signal of a dense correspondence (i' == i, or within a cell of it), the hard-readout
 *     counterpart of the cycle terms the reference trains with (warp_cycle_w, correspondence.py:350-372).
 *   cocos_corr_match_mutual_f16x3: operands, staging, QK arithmetic and row state of cocos_corr_match_f16x3 (the MUTUAL instantiation
 *       of the same kernel template, dense keys only);  row_idx / row_max / row_lse [B,Nq] are that entry's outputs bit for bit.  Per key j
 *         col_max[b,j] = max_i inv_temperature <q_i, k_j>  over the queries i < Nq — an ELEMENT of the tile, the register value the row
 *                        side saw: where row_idx[b,i] == j and col_idx[b,j] == i, row_max[b,i] and col_max[b,j] are equal bitwise
 *         col_idx[b,j] = the i of that maximum, the lowest one among bitwise-equal logits; always in [0, Nq), also for non-finite input
 *         col_lse[b,j] = log sum_i exp(inv_temperature <q_i, k_j>), with a running maximum as the reference of the sum
 *       Queries past Nq in the last block of 128 are -inf for the column state.  The queries of a key are reduced across the lanes of
 *       a wave, across the four waves of a workgroup through LDS, and one partial (max, sum, index) per (query block, key) is written to
 *       `workspace`; a finishing kernel (second launch of this entry) merges a key's partials in ascending block order, comparing
 *       (logit, index).  No atomics: two calls on the same inputs give the same bits.  Nothing Nq x Nk reaches memory.
 *       workspace_bytes >= cocos_corr_match_mutual_workspace_bytes(B, Nq, Nk) = 12 B ceil(Nq / 128) Nk (host arithmetic; 0 for bad
 *       dims), 4-byte aligned, contents undefined before and after.
 *       Supported: K == 256, Nq % 4 == 0, Nk % 4 == 0 (otherwise COCOS_ERR_UNSUPPORTED); null / misaligned pointers (planes 16 bytes,
 *       outputs and workspace 4), bad dims and a short workspace are COCOS_ERR_INVALID; all checked before any HIP call.
 *   cocos_match_round_trip: from row_idx [B,hq wq] (values are positions of the hk x wk grid) and col_idx [B,hk wk] (positions of the
 *       hq x wq grid), one launch writes, all int32,
 *         q_back[b,i] = col_idx[b,row_idx[b,i]],   q_dist[b,i] = max(|x(q_back) - x(i)|, |y(q_back) - y(i)|) on the hq x wq grid (cells),
 *         k_back[b,j] = row_idx[b,col_idx[b,j]],   k_dist[b,j] = the same on the hk x wk grid.
 *       Indices outside their range are clamped into it.  Integer code; serves every route that made the two index maps.
 * ------------------------------------------------------------------------------------- */
size_t cocos_corr_match_mutual_workspace_bytes(int B, int Nq, int Nk);
int cocos_corr_match_mutual_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, int* row_idx, float* row_max,
                                  float* row_lse, int* col_idx, float* col_max, float* col_lse, void* workspace, size_t workspace_bytes,
                                  int B, int K, int Nq, int Nk, float inv_temperature, float operand_scale, cocos_stream_t stream);
int cocos_match_round_trip(const int* row_idx, const int* col_idx, int* q_back, int* q_dist, int* k_back, int* k_dist, int B, int hq,
                           int wq, int hk, int wk, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K49 trainable match readout (corr_lse_bwd_f16x3.hip): the backward of K48's row_lse / col_lse and the pair terms of the
 *     correspondence negative log-likelihood  row_nll_i = row_lse_i - s_{i,t(i)},  col_nll_i = col_lse_{t(i)} - s_{i,t(i)}.
 *     Nothing Nq x Nk reaches memory.  qh,ql [B,Nq,256], kh,kl [B,Nk,256]: the position-major f16 hi / lo operand planes of
 *     cocos_corr_match_mutual_f16x3 (value = (hi + lo) / operand_scale), 16-byte aligned.
 *   cocos_corr_lse_bwd_f16x3: one dense sweep with S recomputed tile by tile in the readout kernels' arithmetic; writes
 *         out_t[b,i,:] = inv_temperature sum_j w_ij kn[b,j,:]      (fp32 [B,Nq,256], position-major, 16-byte aligned)
 *         w_ij = g_row[b,i] exp(s_ij - row_lse[b,i]) + g_col[b,j] exp(s_ij - col_lse[b,j])
 *       — d qn of  sum_i g_row[i] row_lse[i] + sum_j g_col[j] col_lse[j].  The key side is the SAME entry with (qh, ql) <-> (kh, kl),
 *       (row_lse, g_row) <-> (col_lse, g_col) and Nq <-> Nk exchanged.  g_row [B,Nq] / g_col [B,Nk] are each nullable (that term and
 *       its exp are skipped; a null g is bitwise the same as a g of zeros), not both; the lse of a non-null g must be given.  The
 *       exponent's argument is fma(s, scale, -lse) — one rounding, of the difference — clamped at 0 from above.  Keys past Nk and
 *       queries past Nq of partial tiles contribute nothing.  The
 *       second product runs on the MFMA with W split hi / lo at a per-sample power-of-two scale taken from max|g_row| + max|g_col|.
 *       No atomics: bitwise reproducible.
 *       Supported: K == 256, Nq % 4 == 0, Nk % 4 == 0 (otherwise COCOS_ERR_UNSUPPORTED); null / misaligned pointers (planes and out_t
 *       16 bytes, vectors 4) and bad dims are COCOS_ERR_INVALID; all checked before any HIP call.
 *   cocos_pair_logits_f16x3: s[b,i] = inv_temperature <qn_i, kn_t>, t = target[b,i] (int32 [B,Nq]; clamped into [0, Nk) from above),
 *       formed as cocos_sparse_softmax_warp_fwd_f16x3 forms the logit of the same pair, bit for bit; t < 0: s = 0.
 *   cocos_pair_logits_bwd_query_f16x3: dq_t[b,i,:] (+)= inv_temperature g[b,i] kn[b,t,:]  (zeros for t < 0); accumulate != 0 adds to
 *       what dq_t holds (the sweep's output).  The key side is cocos_sparse_softmax_warp_bwd_key_f16x3 with k = 1 over the inverse
 *       table of the targets.  Null pointers and bad dims: COCOS_ERR_INVALID; K != 256, or B Nq / B Nk at or above 2^31:
 *       COCOS_ERR_UNSUPPORTED — before any HIP call.
 * ------------------------------------------------------------------------------------- */
int cocos_corr_lse_bwd_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const float* row_lse, const float* col_lse,
                             const float* g_row, const float* g_col, float* out_t, int B, int K, int Nq, int Nk, float inv_temperature,
                             float operand_scale, cocos_stream_t stream);
int cocos_pair_logits_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const int* target, float* s, int B, int K,
                            int Nq, int Nk, float inv_temperature, float operand_scale, cocos_stream_t stream);
int cocos_pair_logits_bwd_query_f16x3(const void* kh, const void* kl, const int* target, const float* g, float* dq_t, int B, int K,
                                      int Nq, int Nk, float inv_temperature, float operand_scale, int accumulate, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K42 k-sparse correspondence warp with gradients (plane_pair.hip): attention over the k keys per query that the top-k match
 *     readout selected (selection itself carries no gradient),
 *         s[b,i,r] = inv_temperature <qn[b,:,i], kn[b,:,j_r]>,  j_r = idx[b,i,r],  w = softmax over r of s,
 *         out[b,:,i] = sum_r w[b,i,r] v[b,:,j_r]
 *     — the weights of the k-sparse blend of cocos_gather_blend_patches, now differentiable in qn, kn and v.  Nothing Nq x Nk exists:
 *     the state is idx, w and ds, each [B,Nq,k].
 *     Common to the three kernels: qh,ql [B,Nq,256], kh,kl [B,Nk,256] are the position-major f16 hi / lo operand planes of
 *     cocos_corr_topk_f16x3 (value = (hi + lo) / operand_scale), 16-byte aligned; idx [B,Nq,k] int32, ANY values (repeats inside a row
 *     are legal, values outside [0, Nk) are clamped into it); every fp32 tensor is POSITION-major: v_t [B,Nk,Cv], out_t / dout_t
 *     [B,Nq,Cv], dq_t [B,Nq,256], dk_t [B,Nk,256], dv_t [B,Nk,Cv] (cocos_transpose_f32 makes them from / turns them into the
 *     channel-major tensors, once per tensor).  fp32 arithmetic in a fixed order, no atomics: results are bitwise reproducible.
 *     Null pointers, dims < 1, k outside 1..COCOS_MATCH_TOPK_MAX or above Nk: COCOS_ERR_INVALID; K != 256, or B Nq k / B Nk at or
 *     above 2^31: COCOS_ERR_UNSUPPORTED — all before any HIP call.
 *   cocos_sparse_softmax_warp_fwd_f16x3: one wave per query; writes out_t and w [B,Nq,k].
 *   cocos_sparse_softmax_warp_bwd_query_f16x3: one wave per query; dw_r = <dout_t[i], v_t[j_r]>, ds_r = w_r (dw_r - sum_r' w_r' dw_r');
 *       writes ds [B,Nq,k] and, unless dq_t is null, dq_t[i] = inv_temperature sum_r ds_r kn[j_r].
 *   cocos_sparse_softmax_warp_bwd_key_f16x3: one wave per key, a gather over the INVERSE table of idx: entries [B Nq k] int32 holds the
 *       flat positions p = (b Nq + i) k + r of idx grouped by the key b Nk + j they name (clamped), ascending inside a group;
 *       offsets [B Nk + 1] int32 the group boundaries.  dk_t[j] = inv_temperature sum ds[p] qn[i], dv_t[j] = sum w[p] dout_t[i], summed
 *       serially in table order; either output may be null (not both; dk_t null: qh, ql, ds may be null too).  A key nobody names gets
 *       zeros, written by the kernel.  A key all queries name is one serial list of Nq entries for one wave.  Positions and offsets
 *       are clamped into the tables.
 *   cocos_transpose_f32: in [B,R,C] -> out [B,C,R] (B <= 65535, R <= 65535 * 32, else COCOS_ERR_UNSUPPORTED).
 * ------------------------------------------------------------------------------------- */
int cocos_sparse_softmax_warp_fwd_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const float* v_t,
                                        const int* idx, float* out_t, float* w, int B, int K, int Nq, int Nk, int Cv, int k,
                                        float inv_temperature, float operand_scale, cocos_stream_t stream);
/* K50: the forward above with s_r += k_bias[b, j_r] (the clamped j_r) before the softmax over r — the row-conditional transport plan
 *     softmax_j(s_ij + g_j) on the k candidates.  k_bias fp32, 4-byte aligned, [B,Nk] with bias_batch_stride == Nk or one [Nk] row with
 *     bias_batch_stride == 0 (anything else, and a null bias, is COCOS_ERR_INVALID); finite or -inf.  A row whose k candidates all
 *     carry -inf gets the uniform w = 1 / k.  The two backward entries are unchanged: they consume the saved w, the bias is a constant. */
int cocos_sparse_softmax_warp_bias_fwd_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const float* v_t,
                                             const int* idx, const float* k_bias, float* out_t, float* w, int B, int K, int Nq, int Nk,
                                             int Cv, int k, float inv_temperature, float operand_scale, long long bias_batch_stride,
                                             cocos_stream_t stream);
int cocos_sparse_softmax_warp_bwd_query_f16x3(const void* kh, const void* kl, const float* v_t, const float* dout_t, const int* idx,
                                              const float* w, float* ds, float* dq_t /* nullable */, int B, int K, int Nq, int Nk,
                                              int Cv, int k, float inv_temperature, float operand_scale, cocos_stream_t stream);
int cocos_sparse_softmax_warp_bwd_key_f16x3(const void* qh, const void* ql, const float* dout_t, const float* ds, const float* w,
                                            const int* entries, const int* offsets, float* dk_t /* nullable */,
                                            float* dv_t /* nullable */, int B, int K, int Nq, int Nk, int Cv, int k,
                                            float inv_temperature, float operand_scale, cocos_stream_t stream);
int cocos_transpose_f32(const float* in, float* out, int B, int R, int C, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K51 k-sparse correspondence warp with gradients on the match_kernel-3 route (box3_pair.hip, the TopkSet candidate policy): K42's blend on the logit of the
 *     3x3-unfolded, centred, normalised vectors, taken for one pair.  Content grid fh x fw (Nq = fh fw, position p = py fw + px),
 *     exemplar grid gh x gw (Nk = gh gw), any sizes >= 1, equal or not; taps d in {-1,0,1}^2:
 *         R[p,q] = sum_d [p+d inside the content grid] [q+d inside the exemplar grid] <theta[:,p+d], phi[:,q+d]>
 *         z[p,q] = inv_temperature a_p b_q (R[p,q] - kc mu_p nu_q),  kc = 9 * 256,
 *         w = softmax over r of z[p, j_r],  j_r = idx[b,p,r],  out[b,:,p] = sum_r w_r v[b,:,j_r]
 *     with (mu, a) [B,Nq] and (nu, b) [B,Nk] the statistics cocos_unfold3_stats_fwd returns for theta and phi (cocos_box3_logits_fwd's
 *     logit).  "Inside" is decided on the 2-D coordinates, never on the flat index.  Nothing Nq x Nk exists.
 *     Common to the four kernels: th_t [B,Nq,256], ph_t [B,Nk,256] are theta / phi as fp32 POSITION-major rows, 16-byte aligned, and so
 *     is every other fp32 tensor with channels: v_t [B,Nk,Cv], out_t / dout_t [B,Nq,Cv], dth_t [B,Nq,256], dph_t [B,Nk,256], dv_t
 *     [B,Nk,Cv] (cocos_transpose_f32 makes them from / turns them into the channel-major tensors); idx [B,Nq,k] int32, ANY values
 *     (repeats inside a row are legal, values outside [0, Nk) are clamped into it).  fp32 arithmetic in a fixed order, no atomics:
 *     results are bitwise reproducible.  Null pointers, dims < 1 (an empty grid), k outside 1..COCOS_MATCH_TOPK_MAX or above Nk:
 *     COCOS_ERR_INVALID; K != 256, or B Nq k / B Nk at or above 2^31: COCOS_ERR_UNSUPPORTED — all before any HIP call.
 *   cocos_box3_sparse_softmax_warp_fwd: one wave per query; writes out_t, w [B,Nq,k] and c [B,Nq,k] = R - kc mu_p nu_j.
 *   cocos_box3_sparse_softmax_warp_bwd_pair: one wave per query; dw_r = <dout_t[p], v_t[j_r]>, dz_r = w_r (dw_r - sum_r' w_r' dw_r');
 *       writes g [B,Nq,k] = dz inv_temperature a_p b_j (the coefficient on R) and, each unless null, hb [B,Nq,k] = dz inv_temperature
 *       a_p c (the pair's share of db_j), dmu [B,Nq] = -kc sum_r g_r nu_j, da [B,Nq] = sum_r dz_r inv_temperature b_j c_r.
 *   cocos_box3_sparse_softmax_warp_bwd_theta: one wave per content position m, a gather:
 *       dth_t[m] = sum over d (raster order) with p = m - d in the content grid, over r ascending, of
 *                  g[p,r] [j_{p,r} + d in the exemplar grid] phi[j_{p,r} + d];  a position nobody reaches gets zeros, written here.
 *   cocos_box3_sparse_softmax_warp_bwd_key: one wave per exemplar position n, a gather over the INVERSE table of idx (entries, offsets:
 *       as cocos_sparse_softmax_warp_bwd_key_f16x3 takes them):
 *       dph_t[n] = sum over d (raster order) with q = n - d in the exemplar grid, over list(q) in table order, of
 *                  g[p,r] [p + d in the content grid] theta[p + d];
 *       and from list(n) alone dv_t[n] = sum w dout_t[p], dnu [B,Nk] = -kc sum g mu_p, db [B,Nk] = sum hb.  Each output may be null
 *       (not all four), with the inputs only it reads: dph_t reads th_t, g; dv_t reads dout_t, w; dnu reads g, mu; db reads hb.  A key
 *       nobody names gets zeros.  A key all queries name is one serial list of Nq entries, walked for up to nine taps.  Positions and
 *       offsets are clamped into the tables.
 * ------------------------------------------------------------------------------------- */
int cocos_box3_sparse_softmax_warp_fwd(const float* th_t, const float* ph_t, const float* mu, const float* a, const float* nu,
                                       const float* b, const float* v_t, const int* idx, float* out_t, float* w, float* c, int B, int K,
                                       int fh, int fw, int gh, int gw, int Cv, int k, float inv_temperature, cocos_stream_t stream);
/* K54: cocos_box3_sparse_softmax_warp_fwd with w = softmax over r of z[p, j_r] + k_bias[b, j_r]; k_bias fp32 [B,Nk] (finite, or -inf on
 *     keys no row names alone), a constant of the softmax: c, w and the three backward entries are the unbiased ones.  A bias of zeros
 *     gives the unbiased forward's out_t, w and c bit for bit.  A null k_bias is COCOS_ERR_INVALID; otherwise its refusals. */
int cocos_box3_sparse_softmax_warp_bias_fwd(const float* th_t, const float* ph_t, const float* mu, const float* a, const float* nu,
                                            const float* b, const float* v_t, const int* idx, const float* k_bias, float* out_t, float* w,
                                            float* c, int B, int K, int fh, int fw, int gh, int gw, int Cv, int k, float inv_temperature,
                                            cocos_stream_t stream);
int cocos_box3_sparse_softmax_warp_bwd_pair(const float* v_t, const float* dout_t, const int* idx, const float* w, const float* c,
                                            const float* a, const float* nu, const float* b, float* g, float* hb /* nullable */,
                                            float* dmu /* nullable */, float* da /* nullable */, int B, int K, int fh, int fw, int gh,
                                            int gw, int Cv, int k, float inv_temperature, cocos_stream_t stream);
int cocos_box3_sparse_softmax_warp_bwd_theta(const float* ph_t, const int* idx, const float* g, float* dth_t, int B, int K, int fh, int fw,
                                             int gh, int gw, int k, cocos_stream_t stream);
int cocos_box3_sparse_softmax_warp_bwd_key(const float* th_t, const float* dout_t, const float* g, const float* hb, const float* w,
                                           const float* mu, const int* entries, const int* offsets, float* dph_t /* nullable */,
                                           float* dv_t /* nullable */, float* dnu /* nullable */, float* db /* nullable */, int B, int K,
                                           int fh, int fw, int gh, int gw, int Cv, int k, cocos_stream_t stream);
/* K53 — the logit head of the same pair unit (TopkSet at k = 1): the pair's logit itself, for the supervised match loss.
 *   cocos_box3_pair_logit_fwd: one wave per query; idx [B,Nq] int32; z[b,p] = inv_temperature a_p b_j (R[p,j] - kc mu_p nu_j) and
 *       c[b,p] = R[p,j] - kc mu_p nu_j for j = idx[b,p] (values at or above Nk are clamped into the grid); a NEGATIVE idx gives
 *       z = c = 0 (an unsupervised cell).  z, c [B,Nq] fp32.
 *   cocos_box3_pair_logit_bwd_pair: one thread per query; from dz [B,Nq] writes g [B,Nq] = dz inv_temperature a_p b_j and, each
 *       unless null, hb = dz inv_temperature a_p c, dmu = -kc g nu_j, da = dz inv_temperature b_j c; all 0 where idx is negative.
 *       g / hb then go through cocos_box3_sparse_softmax_warp_bwd_theta and _bwd_key at k = 1 (the inverse table of the idx clamped
 *       into [0, Nk): a negative entry rides along with a zero coefficient).
 *   Refusals as the K51 entry points at k = 1. */
int cocos_box3_pair_logit_fwd(const float* th_t, const float* ph_t, const float* mu, const float* a, const float* nu, const float* b,
                              const int* idx, float* z, float* c, int B, int K, int fh, int fw, int gh, int gw, float inv_temperature,
                              cocos_stream_t stream);
int cocos_box3_pair_logit_bwd_pair(const int* idx, const float* c, const float* a, const float* nu, const float* b, const float* dz,
                                   float* g, float* hb /* nullable */, float* dmu /* nullable */, float* da /* nullable */, int B, int K,
                                   int fh, int fw, int gh, int gw, float inv_temperature, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K43 PatchMatch candidate search for the k-sparse warp (patchmatch_f16x3.hip): ONE Jacobi iteration per call — a second selector
 *     next to cocos_corr_topk_f16x3 whose work is O(Nq k (5 + radii)) dot products whatever Nk is (CoCosNet-v2's replacement of the
 *     dense scan).  Query grid hq x wq (Nq = hq wq, position i = y wq + x), key grid hk x wk (Nk = hk wk); operand planes, score
 *     arithmetic and output order as K42 / K39: val is the logit cocos_sparse_softmax_warp_fwd_f16x3 forms for the same pair, bit for
 *     bit; idx_out / val_out [B,Nq,k] hold the k best DISTINCT keys of the pool, score descending, equal bits: lower key first.
 *     The pool of query (b, y, x), idx_in [B,Nq,k] int32 clamped into [0, Nk) first:
 *       own          idx_in[b,i,r], r < k;
 *       propagation  neighbours n = (y -+ stride, x), (y, x -+ stride) inside the query grid, r < k: the key position of idx_in[b,n,r]
 *                    minus (n - i); skipped when it leaves the key grid;
 *       search       s < radii, r < k: own key position + (oy, ox), clamped into the key grid; rho = max(1, radius0 >> s),
 *                    oy = H(word) mod (2 rho + 1) - rho, ox = H(word | 1) mod (2 rho + 1) - rho, word = (r << 8) | (s << 1).
 *     H(word) = f(f(f(f(seed ^ 0x9e3779b9) ^ iteration) ^ (b Nq + i)) ^ word) on uint32, f the murmur3 finaliser
 *     (h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16).  idx_in null: every list (own and neighbours')
 *     is the random initialisation  p_r = H((r << 8) | 0xff) mod Nk, stepped by +1 mod Nk while it equals an earlier p_e, e < r.
 *     A pool with fewer than k distinct keys repeats its last (key, score) in the remaining slots (K42 accepts repeats).
 *     idx_in and idx_out must be different buffers; the result is a pure function of the arguments (no atomics, bitwise reproducible).
 *     Null planes / outputs, idx_in == idx_out, non-positive inv_temperature / operand_scale, misaligned planes: COCOS_ERR_INVALID;
 *     K != 256, k outside 1..COCOS_MATCH_TOPK_MAX or above Nk, an empty grid or batch, stride < 1, radii outside
 *     0..COCOS_PATCHMATCH_MAX_RADII, radius0 outside 0..2^20, B Nq k or B Nk at or above 2^31: COCOS_ERR_UNSUPPORTED — all before any
 *     HIP call.  Instantiated for 1, 2, 4, 8 candidates; a k between two runs the next larger one, truncated.
 * ------------------------------------------------------------------------------------- */
#define COCOS_PATCHMATCH_MAX_RADII 8
int cocos_patchmatch_step_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const int* idx_in /* nullable */,
                                int* idx_out, float* val_out, int B, int K, int hq, int wq, int hk, int wk, int k, int stride, int radii,
                                int radius0, int seed, int iteration, float inv_temperature, float operand_scale, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K57 PatchMatch candidate search on the match_kernel-3 route (patchmatch_box3.hip): ONE Jacobi iteration per call, K43's step with
 *     the box logit of K51 as the score — the selector of cocos_box3_sparse_softmax_warp_fwd that needs no HW x HW tensor.
 *     Content (query) grid fh x fw, exemplar (key) grid gh x gw, any sizes, equal or not.  The pool of a query, the hash, the random
 *     initialisation with idx_in null, the order of idx_out / val_out [B,Nq,k] (the k best DISTINCT keys, score descending, equal bits:
 *     lower key first), the repeat of the last pair in a short pool and the instantiations (1, 2, 4, 8; a k between two runs the next
 *     larger one, truncated) are cocos_patchmatch_step_f16x3's, word for word (patchmatch_pool.h is shared).
 *     val is the logit z = inv_temperature a_p b_q (R[p,q] - 9*256 mu_p nu_q) of cocos_box3_sparse_softmax_warp_fwd for the same pair,
 *     formed in the same expressions: th_t [B,Nq,256], ph_t [B,Nk,256] fp32 position-major rows, (mu, a) [B,Nq], (nu, b) [B,Nk] the
 *     K12 statistics.  A tap is inside a grid by its 2-D coordinates.
 *     Null rows / statistics / outputs, idx_in == idx_out, non-positive inv_temperature, misaligned rows: COCOS_ERR_INVALID; K != 256,
 *     an empty grid or batch, k outside 1..COCOS_MATCH_TOPK_MAX or above Nk, stride < 1, radii outside 0..COCOS_PATCHMATCH_MAX_RADII,
 *     radius0 outside 0..2^20, B Nq k or B Nk at or above 2^31: COCOS_ERR_UNSUPPORTED — in this order, all before any HIP call.
 * ------------------------------------------------------------------------------------- */
int cocos_patchmatch_step_box3(const float* th_t, const float* ph_t, const float* mu, const float* a, const float* nu, const float* b,
                               const int* idx_in /* nullable */, int* idx_out, float* val_out, int B, int K, int fh, int fw, int gh, int gw,
                               int k, int stride, int radii, int radius0, int seed, int iteration, float inv_temperature,
                               cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K44 Sub-cell match refinement (plane_pair.hip, gather_warp.hip): a soft-argmax over the window of keys around a hard
 *     match, and the full-resolution warp sampled at the refined position.
 *   cocos_match_refine_f16x3: qh, ql [B,Nq,256], kh, kl [B,Nk,256] operand planes and score arithmetic as K42 / K43 (the logit
 *     cocos_sparse_softmax_warp_fwd_f16x3 forms for the same pair, bit for bit); idx [B,Nq] int32 the centre key of every query,
 *     clamped into [0, Nk) first, at (yk, xk) of the hk x wk key grid (hk wk == Nk).  The window is the keys (yk + dy, xk + dx),
 *     |dy|, |dx| <= radius, INSIDE the grid (a position outside is left out: neither clamped nor wrapped), visited dy ascending
 *     outside, dx ascending inside.  With s the window's logits: m = max s, lse_win = m + log sum exp(s - m), p = exp(s - lse_win),
 *     off = (sum p dx, sum p dy) in visiting order, limited to [-radius, radius] (the rounded p may sum to an ulp above 1).
 *     off [B,Nq,2] fp32, x first; lse_win [B,Nq] fp32.  Non-finite
 *     scores are not sanitised (they make lse_win and off NaN).  No atomics: bitwise reproducible.
 *     A null pointer, a non-positive size, hk wk != Nk, radius outside 1..COCOS_MATCH_REFINE_MAX_RADIUS, non-positive inv_temperature /
 *     operand_scale, misaligned planes: COCOS_ERR_INVALID; K != 256, B Nq or B Nk at or above the 32-bit tables: COCOS_ERR_UNSUPPORTED
 *     — all before any HIP call.
 *   cocos_gather_patches_subcell: cocos_gather_patches at a sub-cell position.  img [B or 1,C,hk down,wk down] (img_batch_stride as
 *     cocos_gather_patches), idx [B,fh fw] int32 (clamped into [0, hk wk)), off [B,fh fw,2] as above, out [B,C,fh down,fw down].  For
 *     pixel (Y, X) of cell (Y / down, X / down):  sx = (xk + off_x) down + X % down clamped into [0, wk down - 1], x0 = floor(sx),
 *     fx = sx - x0, x1 = min(x0 + 1, wk down - 1), y likewise;  out = top + fy (bottom - top), top = v00 + fx (v01 - v00),
 *     bottom = v10 + fx (v11 - v10), no contraction: with off == 0 the output is cocos_gather_patches' copy.  floor(sx) and fx are formed from the integer xk down + X % down and from off_x down
 *     separately (no fp32 rounding of the position for a power-of-two down).  A non-finite offset makes the cell's pixels NaN.  Null pointers, non-positive sizes, a batch stride that is neither 0 nor dense: COCOS_ERR_INVALID; an image
 *     side of 2^24 pixels or more, a launch grid above 2^31 blocks: COCOS_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------- */
#define COCOS_MATCH_REFINE_MAX_RADIUS 3
int cocos_match_refine_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const int* idx, float* off, float* lse_win,
                             int B, int K, int Nq, int Nk, int hk, int wk, int radius, float inv_temperature, float operand_scale,
                             cocos_stream_t stream);
int cocos_gather_patches_subcell(const float* img, const int* idx, const float* off, float* out, int B, int C, int fh, int fw, int hk,
                                 int wk, int down, long long img_batch_stride, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K46 Gradients of the sub-cell refinement (plane_pair.hip, gather_warp.hip): K44's offset becomes trainable — the
 *     backward of cocos_match_refine_f16x3 to the two operands and of cocos_gather_patches_subcell to the offset.
 *     Common to the two match kernels: planes, idx, grids, radius and scales as cocos_match_refine_f16x3; W = (2 radius + 1)^2 window
 *     slots per query, slot s = (dy + radius) (2 radius + 1) + (dx + radius); ds [B,Nq,W] fp32; dq_t [B,Nq,256], dk_t [B,Nk,256]
 *     POSITION-major fp32, 16-byte aligned (cocos_transpose_f32 turns them into the channel-major gradients).  fp32 in a fixed order,
 *     contraction off, no atomics: bitwise reproducible.  A null pointer, a non-positive size, hk wk != Nk, radius outside
 *     1..COCOS_MATCH_REFINE_MAX_RADIUS, non-positive inv_temperature / operand_scale, misaligned planes: COCOS_ERR_INVALID; K != 256,
 *     B Nq W or B Nk at or above 2^31: COCOS_ERR_UNSUPPORTED — all before any HIP call.
 *   cocos_match_refine_bwd_query_f16x3: one wave per query.  Recomputes the window's logits as cocos_match_refine_f16x3 forms them, bit
 *     for bit (membership, visiting order, arithmetic), p = exp(s - m) / sum exp(s - m) (= exp(s - lse_win), formed without the
 *     rounding of lse_win) and the expectation o = (sum p dx, sum p dy) WITHOUT the
 *     forward's limit to [-radius, radius]: that limit only absorbs an ulp of rounding and is treated as the identity.  With doff
 *     [B,Nq,2] the incoming gradient of off:  ds_s = p_s ((dx_s - o_x) doff_x + (dy_s - o_y) doff_y), 0 for a slot outside the key
 *     grid — every slot is written; unless dq_t is null, dq_t[i] = inv_temperature sum_s ds_s kn[j_s], slots ascending.
 *   cocos_match_refine_bwd_key_f16x3: one wave per key j at (yj, xj), a gather: for dy ascending, then dx ascending, the centre
 *     c = (yj - dy, xj - dx) (skipped outside the grid) and, for every query i of c's group in table order,
 *     dk_t[j] += inv_temperature ds[i, s(dy, dx)] qn[i].  entries [B Nq] / offsets [B Nk + 1] int32 are the inverse table of the
 *     CLAMPED centre table as cocos_sparse_softmax_warp_bwd_key_f16x3 takes it with k = 1 (rows b Nq + i grouped by the centre
 *     b Nk + j they name, ascending).  A key in nobody's window gets zeros, written by the kernel.  Table positions and offsets are
 *     clamped into the tables.  A centre all queries share is one serial list for each key around it.
 *   cocos_gather_patches_subcell_bwd_off: img, idx, off, sizes and img_batch_stride as cocos_gather_patches_subcell; dout
 *     [B,C,fh down,fw down]; doff [B,fh fw,2] = per cell the sum over its C down^2 pixels of dout * d out / d off, with the integer
 *     pixel and the fraction formed exactly as the forward forms them:  d out / d off_x = down ((1 - fy) (v01 - v00) + fy (v11 - v10)),
 *     d out / d off_y = down (bottom - top), each 0 where that axis' clamp acted (the sample left of 0 or at or beyond the last column
 *     / row).  At an exact integer off down the segment [x0, x0 + 1] is used (the right derivative, consistent with floor).  One wave
 *     per cell, a lane-strided loop and a xor butterfly: a fixed order, no atomics.  The image gradient is not built.  Errors as
 *     cocos_gather_patches_subcell.
 * ------------------------------------------------------------------------------------- */
int cocos_match_refine_bwd_query_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const int* idx, const float* doff,
                                       float* ds, float* dq_t /* nullable */, int B, int K, int Nq, int Nk, int hk, int wk, int radius,
                                       float inv_temperature, float operand_scale, cocos_stream_t stream);
int cocos_match_refine_bwd_key_f16x3(const void* qh, const void* ql, const float* ds, const int* entries, const int* offsets, float* dk_t,
                                     int B, int K, int Nq, int Nk, int hk, int wk, int radius, float inv_temperature, float operand_scale,
                                     cocos_stream_t stream);
int cocos_gather_patches_subcell_bwd_off(const float* img, const int* idx, const float* off, const float* dout, float* doff, int B, int C,
                                         int fh, int fw, int hk, int wk, int down, long long img_batch_stride, cocos_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K52 Trainable sub-cell refinement on the match_kernel-3 route (box3_pair.hip, the WindowSet candidate policy): K44 / K46's window soft-argmax on K51's logit.
 *     Grids, taps, R, the statistics, the 2-D in-grid rule and the fp32 position-major rows th_t [B,Nq,256], ph_t [B,Nk,256] as K51:
 *         c[p,q] = R[p,q] - kc mu_p nu_q,   z[p,q] = inv_temperature a_p b_q c[p,q],   kc = 9 * 256.
 *     idx [B,Nq] int32 is the centre key of every query, clamped into [0, Nk) first, at (yk, xk) of the gh x gw exemplar grid.  With
 *     W1 = 2 radius + 1 the window has W = W1^2 slots, slot s = (dy + radius) W1 + (dx + radius), and holds the keys (yk + dy, xk + dx)
 *     INSIDE the grid (a position outside is left out: neither clamped nor wrapped), visited dy ascending outside, dx ascending inside —
 *     cocos_match_refine_f16x3's rules.  fp32 in a fixed order, contraction off, no atomics: bitwise reproducible.  A null pointer, a
 *     non-positive size, radius outside 1..COCOS_MATCH_REFINE_MAX_RADIUS, a non-positive inv_temperature, misaligned rows:
 *     COCOS_ERR_INVALID; K != 256, B Nq W or B Nk at or above 2^31: COCOS_ERR_UNSUPPORTED — all before any HIP call.
 *   cocos_box3_match_refine_fwd: one wave per query.  m = max z over the window, lse_win = m + log sum exp(z - m), p = exp(z - lse_win),
 *       off = (sum p dx, sum p dy) in visiting order, limited to [-radius, radius].  Writes off [B,Nq,2] (x first), lse_win [B,Nq] and
 *       c [B,Nq,W], 0 in the slots outside the grid.  Non-finite scores are not sanitised.
 *   cocos_box3_match_refine_bwd_pair: one wave per query.  Recomputes z from c and the statistics in the forward's arithmetic,
 *       p = exp(z - m) / sum exp(z - m) (without the rounding of lse_win), o = (sum p dx, sum p dy) NOT limited (the limit is the
 *       identity);  with doff [B,Nq,2] the incoming gradient of off:  dz_s = p_s ((dx_s - o_x) doff_x + (dy_s - o_y) doff_y), 0 for a
 *       slot outside the grid.  Writes g [B,Nq,W] = dz inv_temperature a_p b_q (the coefficient on R) and, each unless null,
 *       hb [B,Nq,W] = dz inv_temperature a_p c (the pair's share of db_q), dmu [B,Nq] = -kc sum_s g_s nu_q,
 *       da [B,Nq] = sum_s dz_s inv_temperature b_q c_s — every slot of g and hb is written.
 *   cocos_box3_match_refine_bwd_theta: one wave per content position m, a gather:
 *       dth_t[m] = sum over d (raster order) with p = m - d in the content grid, over the slots s of p's window ascending, of
 *                  g[p,s] [q_s + d in the exemplar grid] phi[q_s + d];  a position nobody reaches gets zeros, written here.
 *   cocos_box3_match_refine_bwd_key: one wave per exemplar position n, a gather over the inverse table of the CLAMPED centre table
 *       (entries [B Nq] / offsets [B Nk + 1] int32 as cocos_match_refine_bwd_key_f16x3 takes them):
 *       dph_t[n] = sum over d (raster order) with q = n - d in the exemplar grid, over the window offsets e in visiting order with the
 *                  centre q - e in the grid, over that centre's list in table order, of g[p, s(e)] [p + d in the content grid] theta[p + d];
 *       and from d = 0 alone dnu [B,Nk] = -kc sum g[p, s(e)] mu_p, db [B,Nk] = sum hb[p, s(e)].  Each output may be null (not all
 *       three), with the inputs only it reads: dph_t reads th_t, g; dnu reads g, mu; db reads hb.  A key in nobody's window gets zeros.
 *       A centre all queries name is one serial list of Nq entries, walked for up to 9 W (tap, offset) pairs.  Positions and offsets
 *       are clamped into the tables.
 * ------------------------------------------------------------------------------------- */
int cocos_box3_match_refine_fwd(const float* th_t, const float* ph_t, const float* mu, const float* a, const float* nu, const float* b,
                                const int* idx, float* off, float* lse_win, float* c, int B, int K, int fh, int fw, int gh, int gw,
                                int radius, float inv_temperature, cocos_stream_t stream);
int cocos_box3_match_refine_bwd_pair(const int* idx, const float* c, const float* a, const float* nu, const float* b, const float* doff,
                                     float* g, float* hb /* nullable */, float* dmu /* nullable */, float* da /* nullable */, int B, int K,
                                     int fh, int fw, int gh, int gw, int radius, float inv_temperature, cocos_stream_t stream);
int cocos_box3_match_refine_bwd_theta(const float* ph_t, const int* idx, const float* g, float* dth_t, int B, int K, int fh, int fw, int gh,
                                      int gw, int radius, cocos_stream_t stream);
int cocos_box3_match_refine_bwd_key(const float* th_t, const float* g, const float* hb, const float* mu, const int* entries,
                                    const int* offsets, float* dph_t /* nullable */, float* dnu /* nullable */, float* db /* nullable */,
                                    int B, int K, int fh, int fw, int gh, int gw, int radius, cocos_stream_t stream);

/* Debug: runs one v_mfma_f32_32x32x2_f32 with known operands and dumps the 64x16 accumulator
 * registers to out[64*16] so the host can verify the lane/register -> (row, col) map. */
int cocos_debug_mfma_probe(float* out, cocos_stream_t stream);

/* K16b (round 3): the stride-1 convolutions of the feature producers in ONE bf16 MFMA term on operands that are bf16 in
 * memory (csrc/conv_nhwc_bf16.hip) — replaces, under COCOS_CONV=bf16, the same reference lines as cocos_conv2d_fwd_f16x3 /
 * cocos_conv2d_wgrad_bf16 (ResidualBlock correspondence.py:13-36, adaptors :150-173, SPADE mlp normalization.py:118-127).
 *   cocos_conv2d_nhwc_prep_bf16:  x fp32 [B][C][H][W] -> xp bf16 [B][H+2 pad][W+2 pad][Cp], Cp = 32 ceil(C/32), channels
 *       beyond C zero, the border zero (reflect = 0) or mirrored as nn.ReflectionPad2d (reflect = 1).
 *   cocos_conv2d_nhwc_bf16:  y fp32 [B][Cout][OH][OW] = bias + conv(xp) with NO further padding,
 *       OH = (Hp - dil (KH-1) - 1) / stride + 1, OW likewise; w_planes = cocos_conv2d_weight_planes(mode | 2) ([KH*KW*Cp/32][Cout][32] bf16).
 *       The input gradient of a stride-1 layer is this call on prep(dy, dil (K-1) - pad, 0) with the mode-1 planes.
 *       fold_ring (input gradient of a layer behind nn.ReflectionPad2d(1), stride 1): y is then dx [B][Cout][OH-2][OW-2] — the
 *       interior of the (OH x OW) padded gradient is stored straight into it, the border ring goes to fold_ring
 *       ([B][Cout][2 OW + 2 (OH-2)] floats) and a second small launch adds it back mirrored: nn.ReflectionPad2d's backward without
 *       the padded tensor or a pass over it.
 *       workspace: zero-initialised scratch of cocos_conv2d_nhwc_bf16_workspace_bytes() bytes, one per stream, cleared once by
 *       the caller (every launch leaves its flags zero): with it, a layer whose tile count is just above a multiple of the CU
 *       count runs as ONE workgroup per CU over contiguous ranges of (tile, k-step) units ("stream-K"; a cut tile's two parts
 *       meet through the workspace) instead of paying a whole extra round; without it every workgroup owns one tile.
 *   cocos_conv2d_nhwc_wgrad_bf16:  partial fp32 [S][Cout][KH*KW*Cp] (summed / re-ordered by cocos_conv2d_wgrad_reduce),
 *       S = cocos_conv2d_nhwc_wgrad_bf16_slices(...) (0: shape not taken — OW must be a multiple of 32); dyp = prep(dy, q, 0).
 *   cocos_conv2d_nhwc_bf16_supported: 1 when the layer shape takes this path (>= 128 output rows, >= 32 input channels; strided layers: forward and weight
 *       gradient — their input gradient stays on cocos_conv2d_fwd_scatter_f16x3's parity classes). */
int cocos_conv2d_nhwc_bf16_supported(int Cin, int Cout, int KH, int KW, int stride);
/* K16c: the same three kernels for the fp32-accurate flavour — every operand as TWO f16 planes (hi, lo; the lo plane directly
 * behind the hi plane: [2][B][Hp][Wp][Cp]) of x * 2^k, k from the tensor's max|x| cell, three MFMA terms per product, results
 * scaled back in the epilogues: the arithmetic of cocos_conv2d_fwd_f16x3 / cocos_conv2d_wgrad_f16x3 (same reference lines) on
 * K16b's data path.  w_hi / w_lo / *w_scale_dev = cocos_conv2d_weight_planes(mode 0 | 1). */
int cocos_conv2d_nhwc_prep_f16x3(const float* x, void* xp, const float* amax_dev /* nullable: scale 1 */, int B, int C, int H, int W,
                                 int pad, int reflect, cocos_stream_t stream);
int cocos_conv2d_nhwc_f16x3(const void* xp, const void* w_hi, const void* w_lo, const float* w_scale_dev, const float* x_amax_dev,
                            const float* bias /* nullable */, float* y, float* fold_ring /* nullable */,
                            void* workspace /* nullable: as cocos_conv2d_nhwc_bf16 */, long long workspace_bytes, int B, int Cp, int Hp,
                            int Wp, int Cout, int KH, int KW, int dil, int stride, cocos_stream_t stream);
int cocos_conv2d_nhwc_wgrad_f16x3(const void* xp, const void* dyp, const float* x_amax_dev, const float* g_amax_dev, float* partial,
                                  int B, int Cp, int Hp, int Wp, int Cout, int q, int KH, int KW, int dil, int stride,
                                  cocos_stream_t stream);
int cocos_conv2d_nhwc_prep_bf16(const float* x, void* xp, int B, int C, int H, int W, int pad, int reflect, cocos_stream_t stream);
long long cocos_conv2d_nhwc_bf16_workspace_bytes(void);
int cocos_conv2d_nhwc_bf16(const void* xp, const void* w_planes, const float* bias /* nullable */, float* y,
                           float* fold_ring /* nullable */, void* workspace /* nullable */, long long workspace_bytes, int B, int Cp,
                           int Hp, int Wp, int Cout, int KH, int KW, int dil, int stride, cocos_stream_t stream);
int cocos_conv2d_nhwc_wgrad_bf16_slices(int B, int OH, int OW, int Cp, int Cout, int KH, int KW);
int cocos_conv2d_nhwc_wgrad_bf16(const void* xp, const void* dyp, float* partial, int B, int Cp, int Hp, int Wp, int Cout, int q,
                                 int KH, int KW, int dil, int stride, cocos_stream_t stream);

/* K21 (round 3): the weight of torch.nn.utils.spectral_norm — every convolution of the reference's generator / discriminator and of
 * netCorr's feature producers is wrapped in it (normalization.py:21-61, architecture.py:41-52).  W viewed as [R = out channels][K],
 * u [R] / v [K] the module's buffers.  fwd: (power_iteration: v <- normalize(W^T u), u <- normalize(W v), in place, ONE iteration)
 * sigma = u . (W v), wsn = W / sigma, *sigma_out = sigma; workspace: cocos_spectral_weight_workspace_floats(R, K) floats.
 * bwd: dW = G / sigma - (sum(G o W) / sigma^2) u v^T with the u, v sigma was taken with; workspace: 1024 floats. */
long long cocos_spectral_weight_workspace_floats(int R, int K);
int cocos_spectral_weight_fwd(const float* W, float* u, float* v, float* wsn, float* sigma_out,
                              float* amax_inout_dev /* nullable: max(*cell, max|wsn|), cell zeroed by the caller */, float* workspace,
                              int R, int K, float eps, int power_iteration, cocos_stream_t stream);
int cocos_spectral_weight_bwd(const float* G, const float* W, const float* u, const float* v, const float* sigma_dev, float* dW,
                              float* workspace, int R, int K, cocos_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* COCOS_HIP_H */
