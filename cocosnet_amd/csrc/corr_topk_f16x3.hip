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

// LABELS (K47): q_label [B,Nq], k_label [B,Nk] (one [Nk] row when k_bstride is 0) int32; pair (i, j) is allowed when q_label[i] < 0 or
// q_label[i] == k_label[j], every other logit is -inf before it meets the tile maximum, the list or the sum.  Without LABELS the two
// pointers are not read (null).
template <int K, bool LABELS>
__global__ __launch_bounds__(CT_THREADS) void corr_topk_f16x3_kernel(
    const _Float16* __restrict__ qh, const _Float16* __restrict__ ql, const _Float16* __restrict__ kh,
    const _Float16* __restrict__ kl, const int* __restrict__ q_label, const int* __restrict__ k_label, int* __restrict__ idx_out, float* __restrict__ val_out, float* __restrict__ lse_out,
    int B, int Nq, int Nk, int k_out /* columns written: 1 .. K */, float scale_log2 /* inv_temperature * log2(e) / operand_scale^2 */,
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
    // One barrier per stage.  Stage t + 1 is committed during the QK loop of stage t into the buffer that stage t - 1 used: every
    // wave finished reading it before it passed the barrier that ended stage t - 1; it is read after the barrier that ends stage t.
    for (int t = 0; t < nstages; ++t) {
        const int buf = t & 1;
        const int j0 = t * CT_STAGE + grp * CT_BK;          // first key of this wave's tile
        const int jn = (t + 2) * CT_STAGE;                  // the stage whose loads take the freed staging registers
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
        u32x4 klab[4];           // labels of keys j0 + 8g + 4h .. + 3: rows 4g .. 4g + 3 of the accumulator
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
        __syncthreads();
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

template <int K, bool LABELS = false>
static int launch_corr_topk(const void* qh, const void* ql, const void* kh, const void* kl, int* idx_out, float* val_out,
                            float* lse_out, int B, int Nq, int Nk, int k, float inv_temperature, float operand_scale,
                            long long k_batch_stride, cocos_stream_t stream, const int* q_label = nullptr,
                            const int* k_label = nullptr) {
    const int nqb = (Nq + CT_BQ - 1) / CT_BQ;
    const float s2 = operand_scale * operand_scale;
    auto kern = corr_topk_f16x3_kernel<K, LABELS>;
    COCOS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CT_SMEM));
    hipLaunchKernelGGL(kern, dim3(B * nqb), dim3(CT_THREADS), CT_SMEM, as_stream(stream), static_cast<const _Float16*>(qh),
                       static_cast<const _Float16*>(ql), static_cast<const _Float16*>(kh), static_cast<const _Float16*>(kl), q_label,
                       k_label, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature * kLog2e / s2, inv_temperature / s2, (size_t)k_batch_stride);
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

extern "C" int cocos_corr_topk_max_k(void) { return cocos::CT_MAX_K; }

// idx_out / max_out [B,Nq] is the same memory as the [B,Nq,1] of the K = 1 instantiation
extern "C" int cocos_corr_match_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, int* idx_out,
                                      float* max_out, float* lse_out, int B, int K, int Nq, int Nk, float inv_temperature,
                                      float operand_scale, long long k_batch_stride, cocos_stream_t stream) {
    using namespace cocos;
    if (const int rc = check_corr_readout("corr_match_f16x3", "cocos_row_argmax_lse", qh, ql, kh, kl, idx_out, max_out, lse_out, B, K, Nq,
                                          Nk, 1, inv_temperature, operand_scale, k_batch_stride))
        return rc;
    return launch_corr_topk<1>(qh, ql, kh, kl, idx_out, max_out, lse_out, B, Nq, Nk, 1, inv_temperature, operand_scale, k_batch_stride, stream);
}

extern "C" int cocos_corr_topk_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, int* idx_out, float* val_out,
                                     float* lse_out, int B, int K, int Nq, int Nk, int k, float inv_temperature,
                                     float operand_scale, long long k_batch_stride, cocos_stream_t stream) {
    using namespace cocos;
    if (const int rc = check_corr_readout("corr_topk_f16x3", "cocos_row_topk_lse", qh, ql, kh, kl, idx_out, val_out, lse_out, B, K, Nq, Nk,
                                          k, inv_temperature, operand_scale, k_batch_stride))
        return rc;
    if (k == 1)
        return launch_corr_topk<1>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale, k_batch_stride, stream);
    if (k == 2)
        return launch_corr_topk<2>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale, k_batch_stride, stream);
    if (k <= 4)
        return launch_corr_topk<4>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale, k_batch_stride, stream);
    return launch_corr_topk<8>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale, k_batch_stride, stream);
}

// K47: the same readout over the keys each query's label allows
extern "C" int cocos_corr_topk_labels_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const int* q_label,
                                            const int* k_label, int* idx_out, float* val_out, float* lse_out, int B, int K, int Nq,
                                            int Nk, int k, float inv_temperature, float operand_scale, long long k_batch_stride,
                                            cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(q_label && k_label, COCOS_ERR_INVALID, "corr_topk_labels_f16x3: null label pointer");
    if (const int rc = check_corr_readout("corr_topk_labels_f16x3", "a host-side mask of materialised logits and cocos_row_topk_lse", qh, ql,
                                          kh, kl, idx_out, val_out, lse_out, B, K, Nq, Nk, k, inv_temperature, operand_scale, k_batch_stride))
        return rc;
    COCOS_REQUIRE((reinterpret_cast<uintptr_t>(q_label) & 3) == 0 && (reinterpret_cast<uintptr_t>(k_label) & 3) == 0, COCOS_ERR_INVALID,
                  "corr_topk_labels_f16x3: label arrays must be 4-byte aligned");
    if (k == 1)
        return launch_corr_topk<1, true>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale,
                                         k_batch_stride, stream, q_label, k_label);
    if (k == 2)
        return launch_corr_topk<2, true>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale,
                                         k_batch_stride, stream, q_label, k_label);
    if (k <= 4)
        return launch_corr_topk<4, true>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale,
                                         k_batch_stride, stream, q_label, k_label);
    return launch_corr_topk<8, true>(qh, ql, kh, kl, idx_out, val_out, lse_out, B, Nq, Nk, k, inv_temperature, operand_scale,
                                     k_batch_stride, stream, q_label, k_label);
}
