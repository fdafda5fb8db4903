// K36a / K39a: match readout of the split-precision correlation — per query the k largest logits, their key indices and the row
// log-sum-exp, without a value tensor and without anything HWxHW in HBM (correspondence.py:291, :304-307 followed by the caller's
// max / argmax or topk / logsumexp over the returned matrix).  One kernel template, K = 1, 2, 4, 8 candidates per lane: K = 1 is the
// hard match (cocos_corr_match_f16x3), the same instantiation serves cocos_corr_topk_f16x3 at k = 1.
//
// Operands and QK arithmetic are those of corr_fused_fwd_f16x3.hip: position-major f16 hi/lo planes [B,N,256] of unit-norm
// columns x operand_scale, S^T (32 keys x 32 queries) = K_tile . Q on v_mfma_f32_32x32x16_f16 with the three terms hi.hi, hi.lo,
// lo.hi accumulated into one fp32 register set in the same order: the logits are the forward's logits bit for bit.
//
// What is different from the forward: no V tile, no P split, no O accumulators — 16 accumulator registers instead of up to 96, 33 KB
// of LDS per key tile instead of up to 72.  The room goes into a second wave per SIMD: a workgroup is 8 waves = 128 queries; waves w
// and w + 4 own the SAME 32 queries and take the even / the odd 32-key tile of each 64-key stage, so while one wave of a SIMD runs
// its max / exp arithmetic the other one has the matrix pipe.
//
// Per lane (lane & 31 = query, lane >> 5 = which 16 of the tile's 32 keys) the state is the (m, l) pair of the online log-sum-exp and
// a sorted list of K (logit, key) pairs (topk_list.h); m is the list's head.  A lane meets its keys in ascending index, so a strict
// compare keeps the lower index among equal logits.  A tile's values are offered to the list only when the tile maximum exceeds the
// list's tail, and then only the elements that exceed it are inserted.  The four partial states of a query (two half-waves x two wave
// groups) are merged ONCE after the last stage, comparing (logit, index): cross-lane for the half-waves, through LDS (free after the
// loop's last barrier) for the wave groups — 128 x (2K + 2) words.  Padded keys are -inf and never enter a list.
#pragma once
#include "common.h"
#include "topk_list.h"

namespace cocos {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int CT_BQ = 128;               // queries per workgroup
constexpr int CT_BK = 32;                // keys per MFMA tile
constexpr int CT_STAGE = 64;             // keys per LDS stage: one tile for each of the two wave groups
constexpr int CT_KD = 256;               // channels
constexpr int CT_KROW = CT_KD + 8;       // halfs per key row in LDS: 528 B -> conflict-free b128 reads
constexpr int CT_THREADS = 512;
constexpr int CT_PLANE = CT_STAGE * CT_KROW;                         // halfs per plane per stage
constexpr size_t CT_SMEM = (size_t)2 * 2 * CT_PLANE * sizeof(_Float16);   // [2 stages][hi|lo]: 135168 B

// ref(m) = m * scale_log2, 0 while m is -inf (nothing seen): the reference of the sum of exponentials
__device__ __forceinline__ float topk_ref(float m, float scale_log2) { return m == -INFINITY ? 0.f : m * scale_log2; }

// (m, l) <- merged with (bm, bl): the larger maximum becomes the common reference and both sums are brought to it (the lists carry
// the indices).  These two functions DEFINE the rounding of the lse, for every K: contraction is switched off and every fused
// multiply-add is written as one, so no compiler heuristic has a say.  After the half-wave exchange both products are rounded
// before the add; after the LDS exchange bl * fb is fused into the rounded l * fa and the own exponent is the rounded product
// m * scale_log2 minus the reference.
__device__ __forceinline__ void topk_merge_sum_halves(float& m, float& l, float bm, float bl, float scale_log2) {
#pragma clang fp contract(off)
    const float mm = fmaxf(m, bm);
    const float ref = topk_ref(mm, scale_log2);
    const float fa = m == -INFINITY ? 0.f : fast_exp2(__builtin_fmaf(scale_log2, m, -ref));
    const float fb = bm == -INFINITY ? 0.f : fast_exp2(__builtin_fmaf(scale_log2, bm, -ref));
    const float pa = l * fa, pb = bl * fb;
    l = pa + pb;
    m = mm;
}
__device__ __forceinline__ void topk_merge_sum_groups(float& m, float& l, float bm, float bl, float scale_log2) {
#pragma clang fp contract(off)
    const float mm = fmaxf(m, bm);
    const float ref = topk_ref(mm, scale_log2);
    const float own = m * scale_log2;
    const float fa = m == -INFINITY ? 0.f : fast_exp2(own - ref);
    const float fb = bm == -INFINITY ? 0.f : fast_exp2(__builtin_fmaf(scale_log2, bm, -ref));
    const float pa = l * fa;
    l = __builtin_fmaf(bl, fb, pa);
    m = mm;
}

// ---- MUTUAL (K48): the column side of the same tiles -----------------------------------------------------------------------------
// A key's column state is the triple (m, l, i): the largest logit over the queries seen, the sum of 2^((s - m) * scale_log2) and the
// query of m, the lowest one among bitwise-equal logits.  col_combine merges two of them; every level of the reduction (lanes, waves,
// query blocks) uses it, so the result does not depend on who ran first: comparing (logit, index) makes the index exact, one exp2 of
// the smaller maximum's distance rescales its sum.  Contraction is off and the one fused multiply-add is written as one.
constexpr int CT_COL_WORDS = 2 * 2 * 4 * CT_BK;                       // LDS words per quantity: [2 stages][2 groups][4 waves][32 keys]
constexpr size_t CT_SMEM_MUTUAL = CT_SMEM + (size_t)3 * CT_COL_WORDS * 4;   // + 6144 B behind the key tiles

__device__ __forceinline__ void col_combine(float& m, float& l, int& i, float bm, float bl, int bi, float scale_log2) {
#pragma clang fp contract(off)
    const bool take_b = bm > m || (bm == m && bi < i);
    const bool a_high = m >= bm;
    const float hi = fmaxf(m, bm), lo = fminf(m, bm);
    const float e = lo == -INFINITY ? 0.f : fast_exp2((lo - hi) * scale_log2);      // both -inf: nothing seen on either side
    const float l_hi = a_high ? l : bl, l_lo = a_high ? bl : l;
    l = __builtin_fmaf(l_lo, e, l_hi);
    m = hi;
    i = take_b ? bi : i;
}

template <int CTRL>
__device__ __forceinline__ float col_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ int col_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }

// v_permlane16_swap_b32 a, b (gfx950): the odd rows of 16 lanes of a trade places with the even rows of b.  Inline assembly because
// __builtin_amdgcn_permlane16_swap loses its second result in hipcc's code (both elements of the returned pair come out as the first
// register); s_nop 1 is the two wait states the instruction needs after a VALU write of either operand.
__device__ __forceinline__ void col_swap_rows(float& a, float& b) {
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

// One level of the transposing reduction: the lane and its partner (the DPP pattern CTRL, an involution that flips the lane bit
// `upper` was taken from) each hold the states a and b of two keys; the lane keeps a when `upper` is false and b when it is true,
// receives the partner's state of the same key and merges it in.  Result in a.
template <int CTRL>
__device__ __forceinline__ void col_step(bool upper, float& am, float& al, int& ai, float bm, float bl, int bi, float scale_log2) {
    const float sm = upper ? am : bm, sl = upper ? al : bl;
    const int si = upper ? ai : bi;
    am = upper ? bm : am, al = upper ? bl : al, ai = upper ? bi : ai;
    col_combine(am, al, ai, col_dpp<CTRL>(sm), col_dpp<CTRL>(sl), col_dpp<CTRL>(si), scale_log2);
}

// The 16 logits of a lane (16 keys x its one query) -> the state of ONE key over the 32 queries of the half-wave: 16 + 8 + 4 + 2 + 1
// merges instead of 16 x 5, because every level halves the keys a lane still carries.  Level 1 exchanges whole rows of 16 lanes with
// v_permlane16_swap (registers r and r + 8 of the two rows trade places: no select), levels 2 .. 5 are DPP inside the row (rotate by
// 8, half mirror, the two quad permutes).  Afterwards lane c holds accumulator register (c >> 1) & 15, in both lanes of a pair.
__device__ __forceinline__ void col_reduce_tile(const f32x16& sa, int i_lane, float scale_log2, float& m, float& l, int& idx) {
    const int c = i_lane & 31;
    const int i_lo = i_lane & ~16, i_hi = i_lane | 16;
    float m8[8], l8[8];
    int i8[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        // even rows of lanes: (own sa[r], the odd row's sa[r]); odd rows: (the even row's sa[r + 8], own sa[r + 8]) — in both the
        // first value belongs to the query with bit 4 clear
        float x = sa[r], y = sa[r + 8];
        col_swap_rows(x, y);
        m8[r] = x;
        l8[r] = 1.f;
        i8[r] = i_lo;
        col_combine(m8[r], l8[r], i8[r], y, 1.f, i_hi, scale_log2);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) col_step<0x128>((c & 8) != 0, m8[r], l8[r], i8[r], m8[r + 4], l8[r + 4], i8[r + 4], scale_log2);   // row_ror:8
#pragma unroll
    for (int r = 0; r < 2; ++r) col_step<0x141>((c & 4) != 0, m8[r], l8[r], i8[r], m8[r + 2], l8[r + 2], i8[r + 2], scale_log2);   // row_half_mirror
    col_step<0x4E>((c & 2) != 0, m8[0], l8[0], i8[0], m8[1], l8[1], i8[1], scale_log2);                                             // quad_perm [2,3,0,1]
    m = m8[0], l = l8[0], idx = i8[0];
    col_combine(m, l, idx, col_dpp<0xB1>(m8[0]), col_dpp<0xB1>(l8[0]), col_dpp<0xB1>(i8[0]), scale_log2);                           // quad_perm [1,0,3,2]
}

// LABELS (K47): q_label [B,Nq], k_label [B,Nk] (one [Nk] row when k_bstride is 0) int32; pair (i, j) is allowed when q_label[i] < 0 or
// q_label[i] == k_label[j], every other logit is -inf before it meets the tile maximum, the list or the sum.  Without LABELS the two
// pointers are not read (null).
// MUTUAL (K48): after the row side has consumed a tile, the same 16 registers go through col_reduce_tile (queries past Nq, loaded
// as zeros, are -inf first — the row side never writes them); the four waves of a group leave their keys' states in LDS behind the key
// tiles, double-buffered by stage, and after the stage's barrier wave 0 merges them in ascending wave (= query) order and writes one
// partial per (query block, key) to col_ws [3][B * nqb][Nk] (m, l, index).  The barrier of the NEXT stage orders wave 0's reads before
// the writes of the stage after it.  Without MUTUAL col_ws is not read (null) and none of this is compiled.
// BIAS (K50): k_bias fp32 [B,Nk] (one [Nk] row when k_bstride is 0) is added to every logit of its key, z_ij = s_ij + bias_j, after the
// past-Nk mask and before the tile maximum, the list and the sum — LABELS is the special case 0 / -inf.  The bias meets the RAW
// accumulator: sa <- fma(bias, bias_raw, sa) with bias_raw = operand_scale^2 / inv_temperature, one rounding, so everything after it
// (the list, the sums, the merges, val = raw * scale_nat) is the unbiased kernel's code; a bias of zeros leaves every register as it
// was.  -inf excludes the key (fma(-inf, positive, finite) = -inf; a masked -inf plus the zero a read past Nk returns stays -inf).
// Without BIAS k_bias is not read (null).
template <int K, bool LABELS, bool MUTUAL = false, bool BIAS = false>
__global__ __launch_bounds__(CT_THREADS) void corr_topk_f16x3_kernel(
    const _Float16* __restrict__ qh, const _Float16* __restrict__ ql, const _Float16* __restrict__ kh,
    const _Float16* __restrict__ kl, const int* __restrict__ q_label, const int* __restrict__ k_label, int* __restrict__ idx_out, float* __restrict__ val_out, float* __restrict__ lse_out,
    int B, int Nq, int Nk, int k_out /* columns written: 1 .. K */, float scale_log2 /* inv_temperature * log2(e) / operand_scale^2 */,
    float scale_nat /* inv_temperature / operand_scale^2 */, size_t k_bstride /* halfs: Nk * 256, or 0 = one key set for all */,
    float* __restrict__ col_ws = nullptr, const float* __restrict__ k_bias = nullptr, float bias_raw = 0.f /* operand_scale^2 / inv_temperature */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    _Float16* const kt = reinterpret_cast<_Float16*>(smem_raw);   // [2 stages][hi|lo][64 keys][KROW]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // wave-uniform by construction, but only a readfirstlane makes that a fact for the compiler (anything derived from threadIdx
    // is divergent to it: branches on `grp` would be lane-masked and its LDS offsets per-lane arithmetic)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;                        // 0: even tiles, 1: odd tiles
    const int h = lane >> 5, c = lane & 31;

    const int nqb = (Nq + CT_BQ - 1) / CT_BQ;
    const int vb = xcd_remap(blockIdx.x, gridDim.x);
    const int b = vb / nqb, qb = vb % nqb;
    const int i_lane = qb * CT_BQ + (wave & 3) * 32 + c;   // this lane's query position

    const size_t qbytes = (size_t)Nq * CT_KD * 2, kbytes = (size_t)Nk * CT_KD * 2;
    const __amdgpu_buffer_rsrc_t qh_rs = make_rsrc(qh + (size_t)b * Nq * CT_KD, qbytes);
    const __amdgpu_buffer_rsrc_t ql_rs = make_rsrc(ql + (size_t)b * Nq * CT_KD, qbytes);
    const __amdgpu_buffer_rsrc_t kh_rs = make_rsrc(kh + (size_t)b * k_bstride, kbytes);
    const __amdgpu_buffer_rsrc_t kl_rs = make_rsrc(kl + (size_t)b * k_bstride, kbytes);

    // ---- resident query slice: B operand of step s = channels 16s + 8h .. +7 of query c (queries past Nq: zeros) ------------
    f16x8 qhr[CT_KD / 16], qlr[CT_KD / 16];
    {
        const unsigned q_off = i_lane < Nq ? (unsigned)(i_lane * CT_KD + h * 8) * 2u : kBufOob;
#pragma unroll
        for (int s = 0; s < CT_KD / 16; ++s) {
            qhr[s] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(qh_rs, (int)(q_off + (unsigned)s * 32u), 0, 0));
            qlr[s] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(ql_rs, (int)(q_off + (unsigned)s * 32u), 0, 0));
        }
    }

    // ---- staging: 64 keys x 512 B per plane = 2048 16-byte chunks, 4 per thread and plane; a key row is contiguous in HBM.
    //      Rows past Nk lie past the end of the descriptor: it returns zeros without touching memory (they are masked below).
    u32x4 kst[2][4];
    unsigned k_voff[4];
    int k_lds[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int g = u * CT_THREADS + tid, key = g >> 5, cc = g & 31;
        k_voff[u] = (unsigned)(key * CT_KD + cc * 8) * 2u;
        k_lds[u] = key * CT_KROW + cc * 8;
    }
    auto fetch = [&](int pl, int u, int j0) {
        kst[pl][u] = __builtin_amdgcn_raw_buffer_load_b128(pl ? kl_rs : kh_rs, (int)(k_voff[u] + (unsigned)j0 * (unsigned)(CT_KD * 2)), 0, 0);
    };
    auto commit = [&](int pl, int u, int buf) {
        *reinterpret_cast<u32x4*>(kt + (buf * 2 + pl) * CT_PLANE + k_lds[u]) = kst[pl][u];
    };

    // ---- labels: the query's in a register (past Nq: unrestricted, never written); the keys' through a bounds-checked descriptor
    //      over this sample's Nk labels — a lane's 16 keys are four runs of four, and since Nk % 4 == 0 a run lies wholly inside the
    //      row or wholly past it (zeros, never dereferenced: those keys are -inf already)
    int q_lab = -1;
    __amdgpu_buffer_rsrc_t lab_rs;
    if constexpr (LABELS) {
        if (i_lane < Nq) q_lab = q_label[(size_t)b * Nq + i_lane];
        lab_rs = make_rsrc(k_label + (k_bstride ? (size_t)b * Nk : (size_t)0), (size_t)Nk * 4);
    }
    // ---- bias: the keys' through a descriptor over this sample's Nk values, in the same four runs of four as the labels (a run past
    //      Nk reads zeros, and those keys are -inf already)
    __amdgpu_buffer_rsrc_t bias_rs;
    if constexpr (BIAS) bias_rs = make_rsrc(k_bias + (k_bstride ? (size_t)b * Nk : (size_t)0), (size_t)Nk * 4);

    const int nstages = (Nk + CT_STAGE - 1) / CT_STAGE;
#pragma unroll
    for (int i = 0; i < 8; ++i) fetch(i & 1, i >> 1, 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) commit(i & 1, i >> 1, 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) fetch(i & 1, i >> 1, CT_STAGE);      // (past Nk when there is one stage: zeros, never read)
    __syncthreads();

    TopkList<K> best;        // raw accumulator values (operand_scale^2 * cos); head = the running maximum m of the log-sum-exp
    best.clear();
    float st_l = 0.f;        // sum of 2^(s * scale_log2 - ref(m))
    constexpr int RA = 4, NS = CT_KD / 16;
    // MUTUAL: wave 0 merges the four waves' column states of stage tp (lane >> 5 = wave group, lane & 31 = key of its tile)
    [[maybe_unused]] float* const cx = reinterpret_cast<float*>(smem_raw + CT_SMEM);       // [m | l | i][2 stages][2 groups][4 waves][32 keys]
    [[maybe_unused]] auto col_flush = [&](int tp) {
        const float* src = cx + (((tp & 1) * 2 + h) * 4) * CT_BK + c;
        float m = src[0], l = src[CT_COL_WORDS];
        int i = __builtin_bit_cast(int, src[2 * CT_COL_WORDS]);
#pragma unroll
        for (int w = 1; w < 4; ++w)
            col_combine(m, l, i, src[w * CT_BK], src[CT_COL_WORDS + w * CT_BK], __builtin_bit_cast(int, src[2 * CT_COL_WORDS + w * CT_BK]), scale_log2);
        const int j = tp * CT_STAGE + h * CT_BK + c;
        if (j < Nk) {
            const size_t plane = (size_t)B * nqb * Nk, at = ((size_t)b * nqb + qb) * Nk + j;
            col_ws[at] = m;
            col_ws[plane + at] = l;
            col_ws[2 * plane + at] = __builtin_bit_cast(float, i);
        }
    };
    // One barrier per stage.  Stage t + 1 is committed during the QK loop of stage t into the buffer that stage t - 1 used: every
    // wave finished reading it before it passed the barrier that ended stage t - 1; it is read after the barrier that ends stage t.
    for (int t = 0; t < nstages; ++t) {
        const int buf = t & 1;
        const int j0 = t * CT_STAGE + grp * CT_BK;          // first key of this wave's tile
        const int jn = (t + 2) * CT_STAGE;                  // the stage whose loads take the freed staging registers
        if constexpr (MUTUAL) {
            if (t > 0 && wave == 0) col_flush(t - 1);
        }
        const _Float16* kb = kt + buf * 2 * CT_PLANE + (grp * CT_BK + c) * CT_KROW + h * 8;
        f16x8 ah[RA], al[RA];
#pragma unroll
        for (int s = 0; s < RA - 1; ++s) {
            ah[s] = *reinterpret_cast<const f16x8*>(kb + s * 16);
            al[s] = *reinterpret_cast<const f16x8*>(kb + CT_PLANE + s * 16);
        }
        f32x16 sa;
#pragma unroll
        for (int r = 0; r < 16; ++r) sa[r] = 0.f;
        u32x4 klab[4];           // labels (BIAS: the biases' bits) of keys j0 + 8g + 4h .. + 3: rows 4g .. 4g + 3 of the accumulator
        // ---- S^T = K_tile . Q : 16 k-steps x 3 terms into one accumulator, in the forward kernel's order; the A fragments come
        //      from LDS RA - 1 steps ahead and the eight staged pieces of the next stage ride in the gaps, one every other step
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int cur = s % RA;
            sa = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cur], qhr[s], sa, 0, 0, 0);
            if (s + RA - 1 < NS) ah[(s + RA - 1) % RA] = *reinterpret_cast<const f16x8*>(kb + (s + RA - 1) * 16);
            __builtin_amdgcn_sched_barrier(0);
            sa = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cur], qlr[s], sa, 0, 0, 0);
            if (s + RA - 1 < NS) al[(s + RA - 1) % RA] = *reinterpret_cast<const f16x8*>(kb + CT_PLANE + (s + RA - 1) * 16);
            __builtin_amdgcn_sched_barrier(0);
            sa = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[cur], qhr[s], sa, 0, 0, 0);
            if ((s & 1) == 0) {
                const int i = s >> 1;
                commit(i & 1, i >> 1, buf ^ 1);
                fetch(i & 1, i >> 1, jn);
            }
            if constexpr (LABELS) {
                // the tile's labels ride in the last steps, where no A fragment is fetched ahead any more and its registers are free
                if (s >= NS - 4)
                    klab[s - (NS - 4)] = __builtin_amdgcn_raw_buffer_load_b128(lab_rs, (j0 + 8 * (s - (NS - 4)) + 4 * h) * 4, 0, 0);
            }
            if constexpr (BIAS) {      // the same slot of the schedule, the same registers
                if (s >= NS - 4)
                    klab[s - (NS - 4)] = __builtin_amdgcn_raw_buffer_load_b128(bias_rs, (j0 + 8 * (s - (NS - 4)) + 4 * h) * 4, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- this lane's 16 keys: j0 + acc_row_base(r) + 4h, ascending in r.  Keys past Nk (zero rows: logit 0, which would beat
        //      an all-negative row and would enter the sum) are masked; only the last stage can hold any (wave-uniform test)
        if (j0 + CT_BK > Nk) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (j0 + acc_row_base(r) + 4 * h >= Nk) sa[r] = -INFINITY;
        }
        if constexpr (LABELS) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (q_lab >= 0 && (int)klab[r >> 2][r & 3] != q_lab) sa[r] = -INFINITY;
        }
        if constexpr (BIAS) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // (the element is copied out first: a bit_cast applied to the vector-element expression itself reads element 0)
                const unsigned bits = klab[r >> 2][r & 3];
                sa[r] = __builtin_fmaf(__builtin_bit_cast(float, bits), bias_raw, sa[r]);
            }
        }
        float tmax = sa[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, sa[r]);
        const float m_old = best.head();
        if (tmax > best.tail()) {     // strictly: an equal value in a later tile has a higher index and stays behind
            if constexpr (K == 1) {   // one slot takes the tile maximum at its lowest row: 15 compare / selects where 16 insertions
                int at = acc_row_base(15);      // cost 48 (most tiles come here: one of a wave's 64 lanes suffices) — 0.5 % of the kernel
#pragma unroll
                for (int r = 14; r >= 0; --r) at = sa[r] == tmax ? acc_row_base(r) : at;
                best.v[0] = tmax;
                best.i[0] = j0 + at + 4 * h;
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (sa[r] > best.tail()) best.push_ascending(sa[r], j0 + acc_row_base(r) + 4 * h);
            }
        }
        const float m_new = fmaxf(m_old, tmax);              // = best.head()
        const float ref = topk_ref(m_new, scale_log2);
        const float alpha = fast_exp2(m_old * scale_log2 - ref);     // m_old = -inf: 2^-inf = 0 (and l is 0)
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += fast_exp2(__builtin_fmaf(sa[r], scale_log2, -ref));
        st_l = st_l * alpha + sum;
        if constexpr (MUTUAL) {
            if (qb * CT_BQ + CT_BQ > Nq) {        // the last query block (workgroup-uniform test)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (i_lane >= Nq) sa[r] = -INFINITY;
            }
            float cm, cl;
            int ci;
            col_reduce_tile(sa, i_lane, scale_log2, cm, cl, ci);
            if ((c & 1) == 0) {
                const int r = c >> 1;             // the accumulator register this lane ended up with
                float* dst = cx + (((t & 1) * 2 + grp) * 4 + (wave & 3)) * CT_BK + acc_row_base(r) + 4 * h;
                dst[0] = cm;
                dst[CT_COL_WORDS] = cl;
                dst[2 * CT_COL_WORDS] = __builtin_bit_cast(float, ci);
            }
        }
        __syncthreads();
    }
    if constexpr (MUTUAL) {
        if (wave == 0) col_flush(nstages - 1);
    }

    // ---- one merge per query: the other half-wave (executed by ALL lanes: a cross-lane read under a divergent branch would read
    //      inactive lanes), then the other wave group through LDS (free after the loop's last barrier) -----------------------------
    float st_m = best.head();
    {
        const float om = swap_half(st_m), ol = swap_half(st_l);
        topk_merge_sum_halves(st_m, st_l, om, ol, scale_log2);
        best.merge(best.from_lane_xor(32));
    }
    float* const xm = reinterpret_cast<float*>(smem_raw);            // [2 + 2K][128]: m, l, values, indices of wave group 1
    const int slot = (wave & 3) * 32 + c;
    if (grp == 1 && h == 0) {
        xm[slot] = st_m;
        xm[CT_BQ + slot] = st_l;
#pragma unroll
        for (int p = 0; p < K; ++p) {
            xm[(2 + p) * CT_BQ + slot] = best.v[p];
            xm[(2 + K + p) * CT_BQ + slot] = __builtin_bit_cast(float, best.i[p]);
        }
    }
    __syncthreads();
    if (grp == 0 && h == 0 && i_lane < Nq) {
        topk_merge_sum_groups(st_m, st_l, xm[slot], xm[CT_BQ + slot], scale_log2);
        TopkList<K> o;
#pragma unroll
        for (int p = 0; p < K; ++p) {
            o.v[p] = xm[(2 + p) * CT_BQ + slot];
            o.i[p] = __builtin_bit_cast(int, xm[(2 + K + p) * CT_BQ + slot]);
        }
        best.merge(o);
        const size_t at = (size_t)b * Nq + i_lane;
#pragma unroll
        for (int p = 0; p < K; ++p) {
            if (p < k_out) {
                // always a valid key position, also for non-finite input (a NaN never enters a list: index 0)
                idx_out[at * k_out + p] = min(max(best.i[p], 0), Nk - 1);
                val_out[at * k_out + p] = best.v[p] * scale_nat;
            }
        }
        lse_out[at] = (topk_ref(st_m, scale_log2) + log2f(st_l)) * kLn2;
    }
}

template <int K, bool LABELS = false, bool MUTUAL = false, bool BIAS = false>
static int launch_corr_topk(const void* qh, const void* ql, const void* kh, const void* kl, int* idx_out, float* val_out,
                            float* lse_out, int B, int Nq, int Nk, int k, float inv_temperature, float operand_scale,
                            long long k_batch_stride, cocos_stream_t stream, const int* q_label = nullptr,
                            const int* k_label = nullptr, float* col_ws = nullptr, const float* k_bias = nullptr) {
    const int nqb = (Nq + CT_BQ - 1) / CT_BQ;
    const float s2 = operand_scale * operand_scale;
    auto kern = corr_topk_f16x3_kernel<K, LABELS, MUTUAL, BIAS>;
    constexpr size_t smem = MUTUAL ? CT_SMEM_MUTUAL : CT_SMEM;
    COCOS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kern, dim3(B * nqb), dim3(CT_THREADS), smem, as_stream(stream), static_cast<const _Float16*>(qh),
                       static_cast<const _Float16*>(ql), static_cast<const _Float16*>(kh), static_cast<const _Float16*>(kl), q_label,
                       k_label, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature * kLog2e / s2, inv_temperature / s2, (size_t)k_batch_stride,
                       col_ws, k_bias, s2 / inv_temperature);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

// the largest k a shipped instantiation serves (an instantiation ships only with zero scratch at two waves per SIMD)
constexpr int CT_MAX_K = 8;

// what both entry points ask of their arguments; `name` is the entry's prefix in the messages, `fallback` the one-sweep reader of
// a materialised matrix that takes the shapes this kernel does not
static int check_corr_readout(const char* name, const char* fallback, const void* qh, const void* ql, const void* kh, const void* kl,
                              const void* idx_out, const void* val_out, const void* lse_out, int B, int K, int Nq, int Nk, int k,
                              float inv_temperature, float operand_scale, long long k_batch_stride) {
    COCOS_REQUIRE(qh && ql && kh && kl && idx_out && val_out && lse_out, COCOS_ERR_INVALID, "%s: null pointer", name);
    COCOS_REQUIRE(B >= 1 && Nq >= 1 && Nk >= 1 && operand_scale > 0.f && inv_temperature > 0.f, COCOS_ERR_INVALID,
                  "%s: bad dims B=%d Nq=%d Nk=%d", name, B, Nq, Nk);
    COCOS_REQUIRE(k >= 1 && k <= COCOS_MATCH_TOPK_MAX && k <= Nk, COCOS_ERR_INVALID, "%s: k=%d: expected 1 <= k <= min(%d, Nk=%d)", name,
                  k, COCOS_MATCH_TOPK_MAX, Nk);
    COCOS_REQUIRE(K == CT_KD, COCOS_ERR_UNSUPPORTED, "%s: needs K == 256 (got %d)", name, K);
    COCOS_REQUIRE(Nk % 4 == 0, COCOS_ERR_UNSUPPORTED, "%s: Nk=%d must be a multiple of 4 (use %s)", name, Nk, fallback);
    COCOS_REQUIRE(k <= CT_MAX_K, COCOS_ERR_UNSUPPORTED, "%s: k=%d: no fused instantiation above %d (use %s)", name, k, CT_MAX_K, fallback);
    COCOS_REQUIRE((size_t)K * Nq * 2 < 0x7fffffffull && (size_t)K * ((size_t)Nk + 2 * CT_STAGE) * 2 < 0x7fffffffull,
                  COCOS_ERR_UNSUPPORTED, "%s: per-sample tensor exceeds 2 GiB", name);
    COCOS_REQUIRE(k_batch_stride == 0 || k_batch_stride == (long long)Nk * K, COCOS_ERR_INVALID,
                  "%s: k_batch_stride %lld: expected 0 (one key set for all samples) or the dense %lld", name, k_batch_stride,
                  (long long)Nk * K);
    for (const void* p : {qh, ql, kh, kl})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: q/k planes must be 16-byte aligned", name);
    COCOS_REQUIRE((long long)B * ((Nq + CT_BQ - 1) / CT_BQ) < 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "%s: grid too large", name);
    return COCOS_OK;
}

}  // namespace cocos
