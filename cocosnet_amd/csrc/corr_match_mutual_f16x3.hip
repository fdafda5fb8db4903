// K48: mutual match — both softmax directions of the split-precision correlation from ONE sweep of Q.K^T, and the round trip on top.
//
// cocos_corr_match_mutual_f16x3 is the MUTUAL instantiation of the match readout's kernel (corr_topk_kernel.h, K = 1, no labels):
// operands, staging, QK arithmetic and the row state are corr_topk_f16x3_kernel<1, false>'s, so the row outputs are
// cocos_corr_match_f16x3's bit for bit.  The S^T tile a wave holds (32 keys x 32 queries) is then consumed along the queries as well:
// col_reduce_tile folds it to one (max, sum, query) state per key inside the wave, the four waves of a group meet in LDS, and one
// partial per (query block, key) goes to the workspace.  corr_match_mutual_finish_kernel merges a key's partials in ascending block
// order, comparing (logit, index).  No atomics anywhere: two calls on the same inputs give the same bits.
//
// cocos_match_round_trip is plain integer code over the two index maps: where does a position come back to, and how far from itself.
#include "corr_topk_kernel.h"

namespace cocos {

constexpr int CM_FIN_THREADS = 256;

__global__ __launch_bounds__(CM_FIN_THREADS) void corr_match_mutual_finish_kernel(
    const float* __restrict__ ws /* [3][B * nqb][Nk] */, int* __restrict__ col_idx, float* __restrict__ col_max, float* __restrict__ col_lse,
    int B, int Nq, int Nk, int nqb, float scale_log2, float scale_nat) {
    const long long t = (long long)blockIdx.x * CM_FIN_THREADS + threadIdx.x;
    if (t >= (long long)B * Nk) return;
    const int b = (int)(t / Nk), j = (int)(t % Nk);
    const size_t plane = (size_t)B * nqb * Nk;
    size_t at = (size_t)b * nqb * Nk + j;
    float m = ws[at], l = ws[plane + at];
    int i = __builtin_bit_cast(int, ws[2 * plane + at]);
    for (int qb = 1; qb < nqb; ++qb) {
        at += Nk;
        col_combine(m, l, i, ws[at], ws[plane + at], __builtin_bit_cast(int, ws[2 * plane + at]), scale_log2);
    }
    // always a valid query position, also for non-finite input
    col_idx[t] = min(max(i, 0), Nq - 1);
    col_max[t] = m * scale_nat;
    col_lse[t] = (topk_ref(m, scale_log2) + log2f(l)) * kLn2;
}

// threads [0, Nq): the query side; [Nq, Nq + Nk): the key side of sample blockIdx.y
__global__ __launch_bounds__(256) void match_round_trip_kernel(const int* __restrict__ row_idx, const int* __restrict__ col_idx,
                                                               int* __restrict__ q_back, int* __restrict__ q_dist, int* __restrict__ k_back,
                                                               int* __restrict__ k_dist, int wq, int Nq, int wk, int Nk) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const size_t b = blockIdx.y;
    if (t >= Nq + Nk) return;
    const bool qside = t < Nq;
    const int p = qside ? t : t - Nq;                                   // the position that asks, on its own grid of width w
    const int* there = (qside ? row_idx : col_idx) + b * (qside ? Nq : Nk);
    const int* back = (qside ? col_idx : row_idx) + b * (qside ? Nk : Nq);
    const int n_own = qside ? Nq : Nk, n_other = qside ? Nk : Nq, w = qside ? wq : wk;
    const int j = min(max(there[p], 0), n_other - 1);
    const int r = min(max(back[j], 0), n_own - 1);
    const int dx = abs(r % w - p % w), dy = abs(r / w - p / w);
    (qside ? q_back : k_back)[b * n_own + p] = r;
    (qside ? q_dist : k_dist)[b * n_own + p] = max(dx, dy);
}

// words of workspace: three planes of one partial per (sample, query block, key); 0 = bad dims (or beyond size_t / the grid)
static size_t mutual_workspace_words(int B, int Nq, int Nk) {
    if (B < 1 || Nq < 1 || Nk < 1) return 0;
    const unsigned long long nqb = ((unsigned long long)Nq + CT_BQ - 1) / CT_BQ;
    const unsigned long long per = (unsigned long long)B * nqb;
    if (per > 0x7fffffffull || per * (unsigned long long)Nk > (1ull << 58)) return 0;
    return (size_t)(3ull * per * (unsigned long long)Nk);
}

}  // namespace cocos

extern "C" size_t cocos_corr_match_mutual_workspace_bytes(int B, int Nq, int Nk) { return cocos::mutual_workspace_words(B, Nq, Nk) * 4; }

extern "C" int cocos_corr_match_mutual_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, int* row_idx, float* row_max,
                                             float* row_lse, int* col_idx, float* col_max, float* col_lse, void* workspace,
                                             size_t workspace_bytes, int B, int K, int Nq, int Nk, float inv_temperature,
                                             float operand_scale, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "corr_match_mutual_f16x3";
    COCOS_REQUIRE(col_idx && col_max && col_lse && workspace, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (const int rc = check_corr_readout(name, "two cocos_corr_match_f16x3 calls", qh, ql, kh, kl, row_idx, row_max, row_lse, B, K, Nq, Nk, 1,
                                          inv_temperature, operand_scale, (long long)Nk * K))
        return rc;
    COCOS_REQUIRE(Nq % 4 == 0, COCOS_ERR_UNSUPPORTED, "%s: Nq=%d must be a multiple of 4 (use two cocos_corr_match_f16x3 calls)", name, Nq);
    COCOS_REQUIRE((size_t)B * Nk < 0x7fffffffull * CM_FIN_THREADS, COCOS_ERR_UNSUPPORTED, "%s: grid too large", name);
    for (const void* p : {(const void*)row_idx, (const void*)row_max, (const void*)row_lse, (const void*)col_idx, (const void*)col_max,
                          (const void*)col_lse, (const void*)workspace})
        COCOS_REQUIRE((reinterpret_cast<uintptr_t>(p) & 3) == 0, COCOS_ERR_INVALID, "%s: outputs and workspace must be 4-byte aligned", name);
    const size_t need = cocos_corr_match_mutual_workspace_bytes(B, Nq, Nk);
    COCOS_REQUIRE(need != 0 && workspace_bytes >= need, COCOS_ERR_INVALID, "%s: workspace of %zu bytes, need %zu (cocos_corr_match_mutual_workspace_bytes)",
                  name, workspace_bytes, need);
    if (const int rc = launch_corr_topk<1, false, true>(qh, ql, kh, kl, row_idx, row_max, row_lse, B, Nq, Nk, 1, inv_temperature, operand_scale,
                                                        (long long)Nk * K, stream, nullptr, nullptr, static_cast<float*>(workspace)))
        return rc;
    const int nqb = (Nq + CT_BQ - 1) / CT_BQ;
    const float s2 = operand_scale * operand_scale;
    const unsigned blocks = (unsigned)(((size_t)B * Nk + CM_FIN_THREADS - 1) / CM_FIN_THREADS);
    hipLaunchKernelGGL(corr_match_mutual_finish_kernel, dim3(blocks), dim3(CM_FIN_THREADS), 0, as_stream(stream),
                       static_cast<const float*>(workspace), col_idx, col_max, col_lse, B, Nq, Nk, nqb, inv_temperature * kLog2e / s2,
                       inv_temperature / s2);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_match_round_trip(const int* row_idx, const int* col_idx, int* q_back, int* q_dist, int* k_back, int* k_dist, int B,
                                      int hq, int wq, int hk, int wk, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(row_idx && col_idx && q_back && q_dist && k_back && k_dist, COCOS_ERR_INVALID, "match_round_trip: null pointer");
    COCOS_REQUIRE(B >= 1 && hq >= 1 && wq >= 1 && hk >= 1 && wk >= 1, COCOS_ERR_INVALID, "match_round_trip: bad dims B=%d grids %dx%d, %dx%d", B,
                  hq, wq, hk, wk);
    COCOS_REQUIRE((long long)hq * wq + (long long)hk * wk < 0x7fffffffll && B <= 65535, COCOS_ERR_UNSUPPORTED,
                  "match_round_trip: grids or batch too large");
    for (const void* p : {(const void*)row_idx, (const void*)col_idx, (const void*)q_back, (const void*)q_dist, (const void*)k_back,
                          (const void*)k_dist})
        COCOS_REQUIRE((reinterpret_cast<uintptr_t>(p) & 3) == 0, COCOS_ERR_INVALID, "match_round_trip: arrays must be 4-byte aligned");
    const int Nq = hq * wq, Nk = hk * wk;
    hipLaunchKernelGGL(match_round_trip_kernel, dim3((Nq + Nk + 255) / 256, B), dim3(256), 0, as_stream(stream), row_idx, col_idx, q_back,
                       q_dist, k_back, k_dist, wq, Nq, wk, Nk);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
