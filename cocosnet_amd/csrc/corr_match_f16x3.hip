// K36a: hard match readout of the split-precision correlation — per query the row maximum of the logits, its key index and
// the row log-sum-exp, without a value tensor and without anything HWxHW in HBM (correspondence.py:291, :304-307 followed by
// the caller's max / argmax over the returned matrix).
//
// Operands and QK arithmetic are those of corr_fused_fwd_f16x3.hip: position-major f16 hi/lo planes [B,N,256] of unit-norm
// columns x operand_scale, S^T (32 keys x 32 queries) = K_tile . Q on v_mfma_f32_32x32x16_f16 with the three terms hi.hi, hi.lo,
// lo.hi accumulated into one fp32 register set in the same order: the logits are the forward's logits bit for bit.
//
// What is different: no V tile, no P split, no O accumulators — 16 accumulator registers instead of up to 96, 33 KB of LDS per
// key tile instead of up to 72.  The room goes into a second wave per SIMD: a workgroup is 8 waves = 128 queries; waves w and
// w + 4 own the SAME 32 queries and take the even / the odd 32-key tile of each 64-key stage, so while one wave of a SIMD runs
// its max / exp arithmetic the other one has the matrix pipe.  Per lane (lane & 31 = query, lane >> 5 = which 16 of the tile's
// 32 keys) the state is (raw maximum, its key index, sum of exp relative to that maximum); the four partial states of a query
// (two half-waves x two waves) are merged ONCE, after the last stage.
#include "common.h"

namespace cocos {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int CM_BQ = 128;               // queries per workgroup
constexpr int CM_BK = 32;                // keys per MFMA tile
constexpr int CM_STAGE = 64;             // keys per LDS stage: one tile for each of the two wave groups
constexpr int CM_KD = 256;               // channels
constexpr int CM_KROW = CM_KD + 8;       // halfs per key row in LDS: 528 B -> conflict-free b128 reads
constexpr int CM_THREADS = 512;
constexpr int CM_PLANE = CM_STAGE * CM_KROW;                         // halfs per plane per stage
constexpr size_t CM_SMEM = (size_t)2 * 2 * CM_PLANE * sizeof(_Float16);   // [2 stages][hi|lo]: 135168 B

// Per-lane state of a query: m = maximum of the raw accumulator (operand_scale^2 * cos) seen so far (-inf: nothing seen), idx = its key
// index (the lowest one among equals), l = sum of 2^(s * scale_log2 - ref(m)) with ref(m) = m * scale_log2 (0 while m is -inf).
__device__ __forceinline__ float match_ref(float m, float scale_log2) { return m == -INFINITY ? 0.f : m * scale_log2; }

// (m, l, idx) <- merged with (bm, bl, bidx): the larger maximum wins, among equals the lower index; the sums are brought to the
// common reference
__device__ __forceinline__ void match_merge(float& m, float& l, int& idx, float bm, float bl, int bidx, float scale_log2) {
    const float mm = fmaxf(m, bm);
    const float ref = match_ref(mm, scale_log2);
    const float fa = m == -INFINITY ? 0.f : fast_exp2(m * scale_log2 - ref);
    const float fb = bm == -INFINITY ? 0.f : fast_exp2(bm * scale_log2 - ref);
    const bool take_b = bm > m || (bm == m && bidx < idx);
    l = l * fa + bl * fb;
    idx = take_b ? bidx : idx;
    m = mm;
}

__global__ __launch_bounds__(CM_THREADS) void corr_match_f16x3_kernel(
    const _Float16* __restrict__ qh, const _Float16* __restrict__ ql, const _Float16* __restrict__ kh,
    const _Float16* __restrict__ kl, int* __restrict__ idx_out, float* __restrict__ max_out, float* __restrict__ lse_out,
    int B, int Nq, int Nk, float scale_log2 /* inv_temperature * log2(e) / operand_scale^2 */,
    float scale_nat /* inv_temperature / operand_scale^2 */, size_t k_bstride /* halfs: Nk * 256, or 0 = one key set for all */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    _Float16* const kt = reinterpret_cast<_Float16*>(smem_raw);   // [2 stages][hi|lo][64 keys][KROW]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // wave-uniform by construction, but only a readfirstlane makes that a fact for the compiler (anything derived from threadIdx
    // is divergent to it: branches on `grp` would be lane-masked and its LDS offsets per-lane arithmetic)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;                        // 0: even tiles, 1: odd tiles
    const int h = lane >> 5, c = lane & 31;

    const int nqb = (Nq + CM_BQ - 1) / CM_BQ;
    const int vb = xcd_remap(blockIdx.x, gridDim.x);
    const int b = vb / nqb, qb = vb % nqb;
    const int i_lane = qb * CM_BQ + (wave & 3) * 32 + c;   // this lane's query position

    const size_t qbytes = (size_t)Nq * CM_KD * 2, kbytes = (size_t)Nk * CM_KD * 2;
    const __amdgpu_buffer_rsrc_t qh_rs = make_rsrc(qh + (size_t)b * Nq * CM_KD, qbytes);
    const __amdgpu_buffer_rsrc_t ql_rs = make_rsrc(ql + (size_t)b * Nq * CM_KD, qbytes);
    const __amdgpu_buffer_rsrc_t kh_rs = make_rsrc(kh + (size_t)b * k_bstride, kbytes);
    const __amdgpu_buffer_rsrc_t kl_rs = make_rsrc(kl + (size_t)b * k_bstride, kbytes);

    // ---- resident query slice: B operand of step s = channels 16s + 8h .. +7 of query c (queries past Nq: zeros) ------------
    f16x8 qhr[CM_KD / 16], qlr[CM_KD / 16];
    {
        const unsigned q_off = i_lane < Nq ? (unsigned)(i_lane * CM_KD + h * 8) * 2u : kBufOob;
#pragma unroll
        for (int s = 0; s < CM_KD / 16; ++s) {
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
        const int g = u * CM_THREADS + tid, key = g >> 5, cc = g & 31;
        k_voff[u] = (unsigned)(key * CM_KD + cc * 8) * 2u;
        k_lds[u] = key * CM_KROW + cc * 8;
    }
    auto fetch = [&](int pl, int u, int j0) {
        kst[pl][u] = __builtin_amdgcn_raw_buffer_load_b128(pl ? kl_rs : kh_rs, (int)(k_voff[u] + (unsigned)j0 * (unsigned)(CM_KD * 2)), 0, 0);
    };
    auto commit = [&](int pl, int u, int buf) {
        *reinterpret_cast<u32x4*>(kt + (buf * 2 + pl) * CM_PLANE + k_lds[u]) = kst[pl][u];
    };

    const int nstages = (Nk + CM_STAGE - 1) / CM_STAGE;
#pragma unroll
    for (int i = 0; i < 8; ++i) fetch(i & 1, i >> 1, 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) commit(i & 1, i >> 1, 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) fetch(i & 1, i >> 1, CM_STAGE);      // (past Nk when there is one stage: zeros, never read)
    __syncthreads();

    float st_m = -INFINITY, st_l = 0.f;
    int st_idx = 0;
    constexpr int RA = 4, NS = CM_KD / 16;
    // One barrier per stage.  Stage t + 1 is committed during the QK loop of stage t into the buffer that stage t - 1 used: every
    // wave finished reading it before it passed the barrier that ended stage t - 1; it is read after the barrier that ends stage t.
    for (int t = 0; t < nstages; ++t) {
        const int buf = t & 1;
        const int j0 = t * CM_STAGE + grp * CM_BK;          // first key of this wave's tile
        const int jn = (t + 2) * CM_STAGE;                  // the stage whose loads take the freed staging registers
        const _Float16* kb = kt + buf * 2 * CM_PLANE + (grp * CM_BK + c) * CM_KROW + h * 8;
        f16x8 ah[RA], al[RA];
#pragma unroll
        for (int s = 0; s < RA - 1; ++s) {
            ah[s] = *reinterpret_cast<const f16x8*>(kb + s * 16);
            al[s] = *reinterpret_cast<const f16x8*>(kb + CM_PLANE + s * 16);
        }
        f32x16 sa;
#pragma unroll
        for (int r = 0; r < 16; ++r) sa[r] = 0.f;
        // ---- S^T = K_tile . Q : 16 k-steps x 3 terms into one accumulator, in the forward kernel's order; the A fragments come
        //      from LDS RA - 1 steps ahead and the eight staged pieces of the next stage ride in the gaps, one every other step
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int cur = s % RA;
            sa = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cur], qhr[s], sa, 0, 0, 0);
            if (s + RA - 1 < NS) ah[(s + RA - 1) % RA] = *reinterpret_cast<const f16x8*>(kb + (s + RA - 1) * 16);
            __builtin_amdgcn_sched_barrier(0);
            sa = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cur], qlr[s], sa, 0, 0, 0);
            if (s + RA - 1 < NS) al[(s + RA - 1) % RA] = *reinterpret_cast<const f16x8*>(kb + CM_PLANE + (s + RA - 1) * 16);
            __builtin_amdgcn_sched_barrier(0);
            sa = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[cur], qhr[s], sa, 0, 0, 0);
            if ((s & 1) == 0) {
                const int i = s >> 1;
                commit(i & 1, i >> 1, buf ^ 1);
                fetch(i & 1, i >> 1, jn);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- this lane's 16 keys: j0 + acc_row_base(r) + 4h, ascending in r.  Keys past Nk (zero rows: logit 0, which would beat
        //      an all-negative row and would enter the sum) are masked; only the last stage can hold any (wave-uniform test)
        if (j0 + CM_BK > Nk) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (j0 + acc_row_base(r) + 4 * h >= Nk) sa[r] = -INFINITY;
        }
        float tmax = sa[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, sa[r]);
        if (tmax > st_m) {            // strictly: an equal value in a later tile has a higher index
            int at = acc_row_base(15);
#pragma unroll
            for (int r = 14; r >= 0; --r) at = sa[r] == tmax ? acc_row_base(r) : at;
            st_idx = j0 + at + 4 * h;
        }
        const float m_new = fmaxf(st_m, tmax);
        const float ref = match_ref(m_new, scale_log2);
        const float alpha = fast_exp2(st_m * scale_log2 - ref);      // st_m = -inf: 2^-inf = 0 (and l is 0)
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += fast_exp2(__builtin_fmaf(sa[r], scale_log2, -ref));
        st_l = st_l * alpha + sum;
        st_m = m_new;
        __syncthreads();
    }

    // ---- one merge per query: the other half-wave (executed by ALL lanes: a cross-lane read under a divergent branch would read
    //      inactive lanes), then the other wave group through LDS (free after the loop's last barrier) -----------------------------
    {
        const float om = swap_half(st_m), ol = swap_half(st_l);
        const int oi = __shfl_xor(st_idx, 32, 64);
        match_merge(st_m, st_l, st_idx, om, ol, oi, scale_log2);
    }
    float* const xm = reinterpret_cast<float*>(smem_raw);            // [3][128]: m, l, idx of wave group 1
    const int slot = (wave & 3) * 32 + c;
    if (grp == 1 && h == 0) {
        xm[slot] = st_m;
        xm[CM_BQ + slot] = st_l;
        xm[2 * CM_BQ + slot] = __builtin_bit_cast(float, st_idx);
    }
    __syncthreads();
    if (grp == 0 && h == 0 && i_lane < Nq) {
        match_merge(st_m, st_l, st_idx, xm[slot], xm[CM_BQ + slot], __builtin_bit_cast(int, xm[2 * CM_BQ + slot]), scale_log2);
        const size_t at = (size_t)b * Nq + i_lane;
        // always a valid key position, also for non-finite input (a NaN row never passes `tmax > m`: index 0)
        idx_out[at] = min(max(st_idx, 0), Nk - 1);
        max_out[at] = st_m * scale_nat;
        lse_out[at] = (match_ref(st_m, scale_log2) + log2f(st_l)) * kLn2;
    }
}

}  // namespace cocos

extern "C" int cocos_corr_match_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, int* idx_out,
                                      float* max_out, float* lse_out, int B, int K, int Nq, int Nk, float inv_temperature,
                                      float operand_scale, long long k_batch_stride, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(qh && ql && kh && kl && idx_out && max_out && lse_out, COCOS_ERR_INVALID, "corr_match_f16x3: null pointer");
    COCOS_REQUIRE(B >= 1 && Nq >= 1 && Nk >= 1 && operand_scale > 0.f && inv_temperature > 0.f, COCOS_ERR_INVALID,
                  "corr_match_f16x3: bad dims B=%d Nq=%d Nk=%d", B, Nq, Nk);
    COCOS_REQUIRE(K == CM_KD, COCOS_ERR_UNSUPPORTED, "corr_match_f16x3: needs K == 256 (got %d)", K);
    COCOS_REQUIRE(Nk % 4 == 0, COCOS_ERR_UNSUPPORTED, "corr_match_f16x3: Nk=%d must be a multiple of 4 (use cocos_row_argmax_lse)", Nk);
    COCOS_REQUIRE((size_t)K * Nq * 2 < 0x7fffffffull && (size_t)K * ((size_t)Nk + 2 * CM_STAGE) * 2 < 0x7fffffffull,
                  COCOS_ERR_UNSUPPORTED, "corr_match_f16x3: per-sample tensor exceeds 2 GiB");
    COCOS_REQUIRE(k_batch_stride == 0 || k_batch_stride == (long long)Nk * K, COCOS_ERR_INVALID,
                  "corr_match_f16x3: k_batch_stride %lld: expected 0 (one key set for all samples) or the dense %lld",
                  k_batch_stride, (long long)Nk * K);
    for (const void* p : {qh, ql, kh, kl})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "corr_match_f16x3: q/k planes must be 16-byte aligned");
    const int nqb = (Nq + CM_BQ - 1) / CM_BQ;
    COCOS_REQUIRE((long long)B * nqb < 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "corr_match_f16x3: grid too large");
    const float s2 = operand_scale * operand_scale;
    auto kern = corr_match_f16x3_kernel;
    COCOS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CM_SMEM));
    hipLaunchKernelGGL(kern, dim3(B * nqb), dim3(CM_THREADS), CM_SMEM, as_stream(stream), static_cast<const _Float16*>(qh),
                       static_cast<const _Float16*>(ql), static_cast<const _Float16*>(kh), static_cast<const _Float16*>(kl), idx_out,
                       max_out, lse_out, B, Nq, Nk, inv_temperature * kLog2e / s2, inv_temperature / s2, (size_t)k_batch_stride);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
