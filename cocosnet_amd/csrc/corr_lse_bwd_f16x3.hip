// K49: the backward of the two log-sum-exp vectors of the correlation (K48's row_lse / col_lse), and the pair terms that turn them
// into the correspondence negative log-likelihood.  Nothing here has an Nq x Nk extent.
//
// cocos_corr_lse_bwd_f16x3 — one dense sweep with a recomputed S:
//   out_t[b,i,:] = inv_t * sum_j w_ij kn[b,j,:],   w_ij = g_row[i] exp(s_ij - row_lse[i]) + g_col[j] exp(s_ij - col_lse[j])
// which is d qn when (row_lse, g_row) belong to the queries; the key side is the SAME entry with the operand planes and the two
// (lse, g) pairs exchanged.
//
// Operands and QK arithmetic are the readout kernels' (corr_topk_kernel.h): position-major f16 hi/lo planes [B,N,256] of unit-norm
// columns x operand_scale, S^T (32 keys x 32 queries) = K_tile . Q on v_mfma_f32_32x32x16_f16, the three terms hi.hi, hi.lo, lo.hi
// into one fp32 register set in the same order — the logits are the forward's bit for bit, so the weights sum to what the forward
// summed.
//
// Tile: a workgroup is 4 waves = 128 queries, one wave per SIMD; a wave keeps its 32 queries resident (hi + lo: 128 VGPRs) and
// O (32 queries x 256 channels) in 8 x 16 accumulator registers, and walks ALL keys in tiles of 32 (double-buffered LDS stages, one
// barrier per stage, the next stage's 16-byte pieces ride in the QK loop as in the readout kernel).
//
// W comes straight from the accumulator: lane (c = query, h) holds the keys 8g + 4h + u of the tile in registers 4g + u, and registers
// 8p .. 8p + 7 are directly the 8 k-slots of step p of the second product O = W . Kn (A = W: row = query, B = Kn: column = channel).
// The k order inside an MFMA is free as long as both operands use the same one, so the B fragment is read from the SAME key tile in
// LDS with ds_read_b64_tr_b16 (the scheme of hgemm_f16x3.hip): two transposed reads of 4 keys x 16 channels per 16 lanes, key rows
// 16p + 4h + 0..3 and 16p + 8 + 4h + 0..3.  The kernel has no divergent branch around them (EXEC is all ones) and every lane's address
// lies inside the tile.  Rows are 256 + 40 halfs = 592 B: the b128 row reads of the first product are conflict-free (16 consecutive
// rows fall into 16 distinct 4-bank groups), the transposed reads are 2-way on 12 of the 64 banks.
//
// W is split hi/lo (truncating hi, lo = w - hi) as the forward correlation kernel splits P: Wh.Kh + Wh.Kl + Wl.Kh.  Upstream gradients
// have any magnitude, so every workgroup first takes max|g_row| + max|g_col| of its sample — an upper bound of |w|, exp(.) <= 1 — and
// scales both g by the power of two that puts this bound in [2^14, 2^15): the top of f16's range, the truncation floor of the split
// (2^-24) is 2^-38 of it.  The scale is exact and is divided out with inv_t / operand_scale at the store.  A maximum is independent of
// the order it is taken in: no atomics anywhere, two calls give the same bits.
//
// Exponents: d = fma(s, scale_nat, -lse) — ONE rounding, of the difference, so for the entries that carry the weight (d near 0) the
// kernel adds nothing to the rounding the forward's fp32 lse already holds — then 2^(min(d log2(e), 0)): never positive, nothing can
// overflow at any temperature.  Keys past Nk (zero rows: logit 0, not -inf) and queries past Nq get w = 0 in both terms.  A padded
// key's kn row is zero and a padded query's row of O is never stored, so the mask cannot change a finite result: what it guards
// against is a non-finite w (an lse far below 0 against the padded logit 0 before the clamp, NaN bits behind a vector) reaching the MFMA.
//
// Pair terms: cocos_pair_logits_f16x3 forms s[b,i] = inv_t <qn_i, kn_t(i)> exactly as K42 forms its pair logits (sparse_row.h), and
// cocos_pair_logits_bwd_query_f16x3 is the query-side gather; the key side is K42's cocos_sparse_softmax_warp_bwd_key_f16x3 with k = 1.
#include "sparse_row.h"

namespace cocos {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int LB_BQ = 128;               // queries per workgroup
constexpr int LB_BK = 32;                // keys per tile = per LDS stage
constexpr int LB_KD = 256;               // channels
constexpr int LB_KROW = LB_KD + 40;      // halfs per key row in LDS (592 B)
constexpr int LB_THREADS = 256;
constexpr int LB_PLANE = LB_BK * LB_KROW;                               // halfs per plane per stage
constexpr size_t LB_TILE_BYTES = (size_t)2 * 2 * LB_PLANE * sizeof(_Float16);   // [2 stages][hi|lo]: 75776 B
constexpr int LB_COL_WORDS = 2 * 2 * LB_BK;                             // [2 stages][g x scale | lse][32 keys]
constexpr size_t LB_SMEM = LB_TILE_BYTES + (size_t)(LB_COL_WORDS + 8) * 4;

// HAS_ROW / HAS_COL: which of the two terms exist (a null g skips that term's exp); at least one does
template <bool HAS_ROW, bool HAS_COL>
__global__ __launch_bounds__(LB_THREADS) void corr_lse_bwd_f16x3_kernel(
    const _Float16* __restrict__ qh, const _Float16* __restrict__ ql, const _Float16* __restrict__ kh, const _Float16* __restrict__ kl,
    const float* __restrict__ row_lse, const float* __restrict__ col_lse, const float* __restrict__ g_row, const float* __restrict__ g_col,
    float* __restrict__ out_t, int Nq, int Nk, float scale_nat /* inv_temperature / operand_scale^2 */,
    float out_scale /* inv_temperature / operand_scale */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    _Float16* const kt = reinterpret_cast<_Float16*>(smem_raw);                          // [2 stages][hi|lo][32 keys][KROW]
    float* const cv = reinterpret_cast<float*>(smem_raw + LB_TILE_BYTES);                // [2 stages][2][32 keys]
    float* const red = cv + LB_COL_WORDS;                                                // [4 waves] of the max |g|

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, c = lane & 31;

    const int nqb = (Nq + LB_BQ - 1) / LB_BQ;
    const int vb = xcd_remap(blockIdx.x, gridDim.x);
    const int b = vb / nqb, qb = vb % nqb;
    const int q0 = qb * LB_BQ + wave * 32;            // first query of this wave
    const int i_lane = q0 + c;                        // this lane's query position

    const size_t qbytes = (size_t)Nq * LB_KD * 2, kbytes = (size_t)Nk * LB_KD * 2;
    const __amdgpu_buffer_rsrc_t qh_rs = make_rsrc(qh + (size_t)b * Nq * LB_KD, qbytes);
    const __amdgpu_buffer_rsrc_t ql_rs = make_rsrc(ql + (size_t)b * Nq * LB_KD, qbytes);
    const __amdgpu_buffer_rsrc_t kh_rs = make_rsrc(kh + (size_t)b * Nk * LB_KD, kbytes);
    const __amdgpu_buffer_rsrc_t kl_rs = make_rsrc(kl + (size_t)b * Nk * LB_KD, kbytes);
    // the per-key vectors through bounds-checked descriptors: keys past Nk read zeros (and are masked below)
    const __amdgpu_buffer_rsrc_t gc_rs = make_rsrc(HAS_COL ? g_col + (size_t)b * Nk : nullptr, HAS_COL ? (size_t)Nk * 4 : 0);
    const __amdgpu_buffer_rsrc_t cl_rs = make_rsrc(HAS_COL ? col_lse + (size_t)b * Nk : nullptr, HAS_COL ? (size_t)Nk * 4 : 0);

    // ---- the scale of W: the power of two that takes max|g_row| + max|g_col| of this sample into [2^14, 2^15) ------------------------
    float gscale, gunscale;
    {
        float mr = 0.f, mc = 0.f;
        if constexpr (HAS_ROW)
            for (int i = tid; i < Nq; i += LB_THREADS) mr = fmaxf(mr, fabsf(g_row[(size_t)b * Nq + i]));
        if constexpr (HAS_COL)
            for (int j = tid; j < Nk; j += LB_THREADS) mc = fmaxf(mc, fabsf(g_col[(size_t)b * Nk + j]));
        mr = wave_max_dpp(mr);
        mc = wave_max_dpp(mc);
        if (lane == 0) {
            red[wave] = mr;
            red[4 + wave] = mc;
        }
        __syncthreads();
        mr = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        mc = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        const float g = mr + mc;
        int e = 15;                                   // g == 0 (or not finite): scale 1, every w is 0 (or not finite) anyway
        if (g > 0.f && g < INFINITY) (void)frexpf(g, &e);      // g = m 2^e, m in [0.5, 1)
        e = min(max(e, -100), 100);
        gscale = ldexpf(1.f, 15 - e);
        gunscale = ldexpf(1.f, e - 15);
    }

    // ---- resident query slice: B operand of step s = channels 16s + 8h .. +7 of query c (queries past Nq: zeros) ------------
    f16x8 qhr[LB_KD / 16], qlr[LB_KD / 16];
    {
        const unsigned q_off = i_lane < Nq ? (unsigned)(i_lane * LB_KD + h * 8) * 2u : kBufOob;
#pragma unroll
        for (int s = 0; s < LB_KD / 16; ++s) {
            qhr[s] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(qh_rs, (int)(q_off + (unsigned)s * 32u), 0, 0));
            qlr[s] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(ql_rs, (int)(q_off + (unsigned)s * 32u), 0, 0));
        }
    }
    const bool q_ok = i_lane < Nq;
    float a_s = 0.f, rl = 0.f;                        // g_row x scale and row_lse of this lane's query
    if constexpr (HAS_ROW) {
        if (q_ok) {
            a_s = g_row[(size_t)b * Nq + i_lane] * gscale;
            rl = row_lse[(size_t)b * Nq + i_lane];
        }
    }

    // ---- staging: 32 keys x 512 B per plane = 1024 16-byte chunks, 4 per thread and plane; a key row is contiguous in HBM.
    //      Rows past Nk lie past the end of the descriptor: it returns zeros without touching memory (they are masked below).
    u32x4 kst[2][4];
    unsigned k_voff[4];
    int k_lds[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int g = u * LB_THREADS + tid, key = g >> 5, cc = g & 31;
        k_voff[u] = (unsigned)(key * LB_KD + cc * 8) * 2u;
        k_lds[u] = key * LB_KROW + cc * 8;
    }
    auto fetch = [&](int pl, int u, int j0) {
        kst[pl][u] = __builtin_amdgcn_raw_buffer_load_b128(pl ? kl_rs : kh_rs, (int)(k_voff[u] + (unsigned)j0 * (unsigned)(LB_KD * 2)), 0, 0);
    };
    auto commit = [&](int pl, int u, int buf) {
        *reinterpret_cast<u32x4*>(kt + (buf * 2 + pl) * LB_PLANE + k_lds[u]) = kst[pl][u];
    };
    // the per-key pair (g_col x scale, col_lse) of a stage: threads 0 .. 31, one key each
    float cst_g = 0.f, cst_l = 0.f;
    auto col_fetch = [&](int j0) {
        if constexpr (HAS_COL) {
            if (tid < LB_BK) {
                cst_g = buf_load1(gc_rs, (unsigned)(j0 + tid) * 4u);
                cst_l = buf_load1(cl_rs, (unsigned)(j0 + tid) * 4u);
            }
        }
    };
    auto col_commit = [&](int buf) {
        if constexpr (HAS_COL) {
            if (tid < LB_BK) {
                cv[(buf * 2 + 0) * LB_BK + tid] = cst_g * gscale;
                cv[(buf * 2 + 1) * LB_BK + tid] = cst_l;
            }
        }
    };

    const int nstages = (Nk + LB_BK - 1) / LB_BK;
#pragma unroll
    for (int i = 0; i < 8; ++i) fetch(i & 1, i >> 1, 0);
    col_fetch(0);
#pragma unroll
    for (int i = 0; i < 8; ++i) commit(i & 1, i >> 1, 0);
    col_commit(0);
#pragma unroll
    for (int i = 0; i < 8; ++i) fetch(i & 1, i >> 1, LB_BK);        // (past Nk when there is one stage: zeros, never read)
    col_fetch(LB_BK);
    __syncthreads();

    f32x16 o[LB_KD / 32];
#pragma unroll
    for (int cb = 0; cb < LB_KD / 32; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[cb][r] = 0.f;

    // transposed read: lane 4q + p of a group of 16 supplies row q, columns 4p .. 4p + 3 of its 4-key x 16-channel block; the two
    // groups of a half-wave take channels 0 .. 15 and 16 .. 31 of the 32-channel block, the half-waves the keys 4h .. 4h + 3
    const int tr_off = (4 * h + ((lane & 15) >> 2)) * LB_KROW + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    const bool last_qb = qb * LB_BQ + LB_BQ > Nq;                    // (workgroup-uniform)
    constexpr int RA = 4, NS = LB_KD / 16;

    // One barrier per stage.  Stage t + 1 is committed during the QK loop of stage t into the buffer that stage t - 1 used: every
    // wave finished reading it (both products) before it passed the barrier that ended stage t - 1.
    for (int t = 0; t < nstages; ++t) {
        const int buf = t & 1;
        const int j0 = t * LB_BK;
        const int jn = (t + 2) * LB_BK;
        const _Float16* const tile = kt + buf * 2 * LB_PLANE;
        const _Float16* kb = tile + c * LB_KROW + h * 8;
        f16x8 ah[RA], al[RA];
#pragma unroll
        for (int s = 0; s < RA - 1; ++s) {
            ah[s] = *reinterpret_cast<const f16x8*>(kb + s * 16);
            al[s] = *reinterpret_cast<const f16x8*>(kb + LB_PLANE + s * 16);
        }
        f32x16 sa;
#pragma unroll
        for (int r = 0; r < 16; ++r) sa[r] = 0.f;
        // ---- S^T = K_tile . Q : 16 k-steps x 3 terms into one accumulator, in the readout kernel's order
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int cur = s % RA;
            sa = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cur], qhr[s], sa, 0, 0, 0);
            if (s + RA - 1 < NS) ah[(s + RA - 1) % RA] = *reinterpret_cast<const f16x8*>(kb + (s + RA - 1) * 16);
            __builtin_amdgcn_sched_barrier(0);
            sa = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cur], qlr[s], sa, 0, 0, 0);
            if (s + RA - 1 < NS) al[(s + RA - 1) % RA] = *reinterpret_cast<const f16x8*>(kb + LB_PLANE + (s + RA - 1) * 16);
            __builtin_amdgcn_sched_barrier(0);
            sa = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[cur], qhr[s], sa, 0, 0, 0);
            if ((s & 1) == 0) {
                const int i = s >> 1;
                commit(i & 1, i >> 1, buf ^ 1);
                fetch(i & 1, i >> 1, jn);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        col_commit(buf ^ 1);
        col_fetch(jn);

        // ---- W: this lane's 16 keys j0 + acc_row_base(r) + 4h; register r pairs with the column vectors' entry acc_row_base(r) + 4h
        float w[16];
        f32x4 cg[4], cl[4];
        if constexpr (HAS_COL) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                cg[g] = *reinterpret_cast<const f32x4*>(cv + (buf * 2 + 0) * LB_BK + 8 * g + 4 * h);
                cl[g] = *reinterpret_cast<const f32x4*>(cv + (buf * 2 + 1) * LB_BK + 8 * g + 4 * h);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float wv = 0.f;
            if constexpr (HAS_ROW) wv = a_s * fast_exp2(fminf(__builtin_fmaf(sa[r], scale_nat, -rl) * kLog2e, 0.f));
            if constexpr (HAS_COL)
                wv = __builtin_fmaf(cg[r >> 2][r & 3], fast_exp2(fminf(__builtin_fmaf(sa[r], scale_nat, -cl[r >> 2][r & 3]) * kLog2e, 0.f)), wv);
            w[r] = wv;
        }
        // keys past Nk (only the last stage can hold any) and queries past Nq (only the last block): nothing, in either term
        if (j0 + LB_BK > Nk || last_qb) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (j0 + acc_row_base(r) + 4 * h >= Nk || !q_ok) w[r] = 0.f;
        }
        u32x4 whi[2], wlo[2];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            unsigned hi, lo;
            split_pair_rtz(w[2 * u], w[2 * u + 1], hi, lo);
            whi[u >> 2][u & 3] = hi;
            wlo[u >> 2][u & 3] = lo;
        }
        // ---- O += W . Kn : 2 k-steps x 8 channel blocks x 3 terms; the B fragments come transposed from the tile the first product read
        const _Float16* tb = tile + tr_off;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const f16x8 wh = __builtin_bit_cast(f16x8, whi[p]), wl = __builtin_bit_cast(f16x8, wlo[p]);
#pragma unroll
            for (int cb = 0; cb < LB_KD / 32; ++cb) {
                const _Float16* src = tb + p * 16 * LB_KROW + cb * 32;
                const s16x4 h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(src));
                const s16x4 h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(src + 8 * LB_KROW));
                const s16x4 l0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(src + LB_PLANE));
                const s16x4 l1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(src + LB_PLANE + 8 * LB_KROW));
                const f16x8 bh = __builtin_bit_cast(f16x8, __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7));
                const f16x8 bl = __builtin_bit_cast(f16x8, __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7));
                o[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, bh, o[cb], 0, 0, 0);
                o[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, bl, o[cb], 0, 0, 0);
                o[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, bh, o[cb], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // ---- store: register r of block cb is query q0 + acc_row_base(r) + 4h, channel 32 cb + c — 128 contiguous bytes per half-wave
    const float fin = out_scale * gunscale;
    float* const ob = out_t + (size_t)b * Nq * LB_KD;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = q0 + acc_row_base(r) + 4 * h;
        if (i < Nq) {
#pragma unroll
            for (int cb = 0; cb < LB_KD / 32; ++cb) ob[(size_t)i * LB_KD + cb * 32 + c] = o[cb][r] * fin;
        }
    }
}

template <bool HAS_ROW, bool HAS_COL>
static int launch_corr_lse_bwd(const void* qh, const void* ql, const void* kh, const void* kl, const float* row_lse, const float* col_lse,
                               const float* g_row, const float* g_col, float* out_t, int B, int Nq, int Nk, float inv_temperature,
                               float operand_scale, cocos_stream_t stream) {
    const int nqb = (Nq + LB_BQ - 1) / LB_BQ;
    const float s2 = operand_scale * operand_scale;
    auto kern = corr_lse_bwd_f16x3_kernel<HAS_ROW, HAS_COL>;
    COCOS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LB_SMEM));
    hipLaunchKernelGGL(kern, dim3(B * nqb), dim3(LB_THREADS), LB_SMEM, as_stream(stream), static_cast<const _Float16*>(qh),
                       static_cast<const _Float16*>(ql), static_cast<const _Float16*>(kh), static_cast<const _Float16*>(kl), row_lse, col_lse,
                       g_row, g_col, out_t, Nq, Nk, inv_temperature / s2, inv_temperature / operand_scale);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

// ---- pair terms: one wave per query ---------------------------------------------------------------------------------------------
constexpr int PL_WAVES = 4;
constexpr int PL_THREADS = PL_WAVES * kWave;

__global__ __launch_bounds__(PL_THREADS) void pair_logits_kernel(const _Float16* __restrict__ qh, const _Float16* __restrict__ ql,
                                                                 const _Float16* __restrict__ kh, const _Float16* __restrict__ kl,
                                                                 const int* __restrict__ target, float* __restrict__ s_out, long long rows,
                                                                 int Nq, int Nk, float logit_scale) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * PL_WAVES + (threadIdx.x >> 6);      // b * Nq + i
    if (row >= rows) return;                                                          // (whole waves; the kernel has no barrier)
    const int t = target[row];
    float s = 0.f;
    if (t >= 0) {                                                                     // (wave-uniform)
        const f32x4 q = load_row4(qh, ql, row, lane);
        const f32x4 kv = load_row4(kh, kl, (row / Nq) * Nk + clamp_key(t, Nk), lane);
        s = wave_sum(lane_dot4(q, kv)) * logit_scale;                                 // K42's logit of the pair, bit for bit
    }
    if (lane == 0) s_out[row] = s;
}

__global__ __launch_bounds__(PL_THREADS) void pair_logits_bwd_query_kernel(const _Float16* __restrict__ kh, const _Float16* __restrict__ kl,
                                                                           const int* __restrict__ target, const float* __restrict__ g,
                                                                           float* __restrict__ dq_t, long long rows, int Nq, int Nk,
                                                                           float grad_scale, int accumulate) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * PL_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int t = target[row];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (t >= 0) acc = (g[row] * grad_scale) * load_row4(kh, kl, (row / Nq) * Nk + clamp_key(t, Nk), lane);
    f32x4* const dst = reinterpret_cast<f32x4*>(dq_t + row * SW_KD + lane * 4);
    *dst = accumulate ? *dst + acc : acc;
}

static int pair_logits_check(const char* name, int B, int K, int Nq, int Nk, float inv_temperature, float operand_scale) {
    COCOS_REQUIRE(B >= 1 && Nq >= 1 && Nk >= 1 && operand_scale > 0.f && inv_temperature > 0.f, COCOS_ERR_INVALID,
                  "%s: bad dims B=%d Nq=%d Nk=%d", name, B, Nq, Nk);
    COCOS_REQUIRE(K == SW_KD, COCOS_ERR_UNSUPPORTED, "%s: needs K == 256 (got %d)", name, K);
    COCOS_REQUIRE((long long)B * Nq < 0x7fffffffll && (long long)B * Nk < 0x7fffffffll, COCOS_ERR_UNSUPPORTED,
                  "%s: B Nq = %lld queries / B Nk = %lld keys exceed the 32-bit tables", name, (long long)B * Nq, (long long)B * Nk);
    return COCOS_OK;
}

}  // namespace cocos

extern "C" int cocos_corr_lse_bwd_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const float* row_lse,
                                        const float* col_lse, const float* g_row, const float* g_col, float* out_t, int B, int K, int Nq,
                                        int Nk, float inv_temperature, float operand_scale, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "corr_lse_bwd_f16x3";
    COCOS_REQUIRE(qh && ql && kh && kl && out_t, COCOS_ERR_INVALID, "%s: null pointer", name);
    COCOS_REQUIRE(g_row || g_col, COCOS_ERR_INVALID, "%s: null pointer (g_row and g_col are both null)", name);
    COCOS_REQUIRE((!g_row || row_lse) && (!g_col || col_lse), COCOS_ERR_INVALID, "%s: null pointer (a gradient without its lse)", name);
    COCOS_REQUIRE(B >= 1 && Nq >= 1 && Nk >= 1 && operand_scale > 0.f && inv_temperature > 0.f, COCOS_ERR_INVALID,
                  "%s: bad dims B=%d Nq=%d Nk=%d", name, B, Nq, Nk);
    COCOS_REQUIRE(K == LB_KD, COCOS_ERR_UNSUPPORTED, "%s: needs K == 256 (got %d)", name, K);
    COCOS_REQUIRE(Nq % 4 == 0 && Nk % 4 == 0, COCOS_ERR_UNSUPPORTED, "%s: Nq=%d and Nk=%d must be multiples of 4", name, Nq, Nk);
    COCOS_REQUIRE((size_t)K * Nq * 4 < 0x7fffffffull && (size_t)K * ((size_t)Nk + 2 * LB_BK) * 2 < 0x7fffffffull, COCOS_ERR_UNSUPPORTED,
                  "%s: per-sample tensor exceeds 2 GiB", name);
    for (const void* p : {qh, ql, kh, kl, (const void*)out_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: q/k planes and out_t must be 16-byte aligned", name);
    for (const void* p : {(const void*)row_lse, (const void*)col_lse, (const void*)g_row, (const void*)g_col})
        COCOS_REQUIRE((reinterpret_cast<uintptr_t>(p) & 3) == 0, COCOS_ERR_INVALID, "%s: lse and g vectors must be 4-byte aligned", name);
    COCOS_REQUIRE((long long)B * ((Nq + LB_BQ - 1) / LB_BQ) < 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "%s: grid too large", name);
    if (g_row && g_col)
        return launch_corr_lse_bwd<true, true>(qh, ql, kh, kl, row_lse, col_lse, g_row, g_col, out_t, B, Nq, Nk, inv_temperature, operand_scale, stream);
    if (g_row)
        return launch_corr_lse_bwd<true, false>(qh, ql, kh, kl, row_lse, col_lse, g_row, g_col, out_t, B, Nq, Nk, inv_temperature, operand_scale, stream);
    return launch_corr_lse_bwd<false, true>(qh, ql, kh, kl, row_lse, col_lse, g_row, g_col, out_t, B, Nq, Nk, inv_temperature, operand_scale, stream);
}

extern "C" int cocos_pair_logits_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const int* target, float* s, int B,
                                       int K, int Nq, int Nk, float inv_temperature, float operand_scale, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "pair_logits_f16x3";
    COCOS_REQUIRE(qh && ql && kh && kl && target && s, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (int rc = pair_logits_check(name, B, K, Nq, Nk, inv_temperature, operand_scale)) return rc;
    for (const void* p : {qh, ql, kh, kl})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: q/k planes must be 16-byte aligned", name);
    const long long rows = (long long)B * Nq;
    hipLaunchKernelGGL(pair_logits_kernel, dim3((unsigned)((rows + PL_WAVES - 1) / PL_WAVES)), dim3(PL_THREADS), 0, as_stream(stream),
                       (const _Float16*)qh, (const _Float16*)ql, (const _Float16*)kh, (const _Float16*)kl, target, s, rows, Nq, Nk,
                       inv_temperature / (operand_scale * operand_scale));
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_pair_logits_bwd_query_f16x3(const void* kh, const void* kl, const int* target, const float* g, float* dq_t, int B,
                                                 int K, int Nq, int Nk, float inv_temperature, float operand_scale, int accumulate,
                                                 cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "pair_logits_bwd_query_f16x3";
    COCOS_REQUIRE(kh && kl && target && g && dq_t, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (int rc = pair_logits_check(name, B, K, Nq, Nk, inv_temperature, operand_scale)) return rc;
    for (const void* p : {kh, kl, (const void*)dq_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the key planes and dq_t must be 16-byte aligned", name);
    const long long rows = (long long)B * Nq;
    hipLaunchKernelGGL(pair_logits_bwd_query_kernel, dim3((unsigned)((rows + PL_WAVES - 1) / PL_WAVES)), dim3(PL_THREADS), 0,
                       as_stream(stream), (const _Float16*)kh, (const _Float16*)kl, target, g, dq_t, rows, Nq, Nk,
                       inv_temperature / operand_scale, accumulate);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
