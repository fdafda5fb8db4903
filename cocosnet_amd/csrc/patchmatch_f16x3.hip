// K43: one PatchMatch iteration of the top-k candidate search that feeds the k-sparse warp (K42) — the selector whose work does not
// grow with the number of keys.  Per query (b, y, x) of an hq x wq grid the kernel scores a small POOL of keys of the hk x wk key grid
// and returns the k best distinct ones:
//   own           idx_in[b,i,r], r < k (clamped into [0, Nk)); with idx_in == null the hashed positions pm_init_list makes
//   propagation   for the neighbours n = (y -+ d, x), (y, x -+ d) inside the query grid and r < k: the key position of idx_in[b,n,r]
//                 minus the offset (n - i); a candidate outside the key grid is skipped
//   random search for s < S and r < k: the own key position + (oy, ox), clamped into the key grid, oy / ox = hash mod (2 rho + 1) - rho,
//                 rho = max(1, R >> s)
// One launch is one JACOBI iteration: idx_in is read, idx_out (another buffer) is written, no atomics, no communication between
// workgroups — the result is a pure function of the arguments.  Everything that chooses a candidate is 32-bit integer arithmetic
// (patchmatch_pool.h, shared with the box-logit step of patchmatch_box3.hip), so a host restatement reproduces every pool exactly
// (tests/patchmatch_case.py).
//
// A score is K42's logit of the pair, bit for bit (sparse_row.h): one wave per query, 512-byte row loads, four FMAs per lane, the xor
// butterfly, one multiply by inv_temperature / operand_scale^2.  The candidates of one source (the own list, one neighbour's list, one
// radius of the search) are scored together: their K row loads are issued before the first butterfly.  Every lane holds the same
// score bits, so the candidate list is wave-uniform; it is kept in the order of topk_list.h (score descending, equal bits: lower key
// first) by a general insert that first tests membership — the same key may reach the pool from several sources.
#include "patchmatch_pool.h"

namespace cocos {

template <int K>
__global__ __launch_bounds__(PM_THREADS) void patchmatch_step_kernel(const _Float16* __restrict__ qh, const _Float16* __restrict__ ql,
                                                                     const _Float16* __restrict__ kh, const _Float16* __restrict__ kl,
                                                                     const int* __restrict__ idx_in, int* __restrict__ idx_out,
                                                                     float* __restrict__ val_out, int rows, int hq, int wq, int hk, int wk,
                                                                     int k, int stride, int S, int R, int seed, int iteration,
                                                                     float logit_scale) {
    const int lane = threadIdx.x & (kWave - 1);
    // (the wave index is the same in all 64 lanes: saying so keeps the candidate arithmetic and the list on the scalar side)
    const int row = (int)blockIdx.x * PM_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // b * Nq + i
    if (row >= rows) return;                                                          // (whole waves; the kernel has no barrier)
    const int Nq = hq * wq, Nk = hk * wk;
    const int b = row / Nq, i = row - b * Nq;
    const int y = i / wq, x = i - y * wq;
    const long long kbase = (long long)b * Nk;
    const f32x4 q = load_row4(qh, ql, row, lane);

    int own[K];
    pm_list<K>(own, idx_in, row, k, Nk, seed, iteration);
    PoolList<K> best;
    best.clear();

    const PmStep step{hq, wq, hk, wk, Nq, Nk, k, stride, S, R, seed, iteration};
    for (int src = 0; src < pm_sources(step); ++src) {
        int cand[K];      // key index, or -1: no candidate
        pm_source<K>(cand, src, own, idx_in, row, b, y, x, step);
        // the K rows of this source first, then their reductions: K loads in flight instead of one load -> butterfly chain per key
        f32x4 kv[K];
#pragma unroll
        for (int r = 0; r < K; ++r) kv[r] = load_row4(kh, kl, kbase + max(cand[r], 0), lane);
        float sc[K];
#pragma unroll
        for (int r = 0; r < K; ++r) sc[r] = wave_sum(lane_dot4(q, kv[r])) * logit_scale;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            // (every lane holds the same bits: reading lane 0's makes the list wave-uniform for the compiler too)
            const float sr = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sc[r])));
            if (cand[r] >= 0) best.insert(sr, cand[r]);
        }
    }
    // fewer than k distinct keys in the pool (or scores that are NaN): the remaining slots repeat the last filled pair; a list that
    // stayed empty returns the own candidates with -inf
#pragma unroll
    for (int p = 0; p < K; ++p) {
        if (best.i[p] < 0) {
            best.i[p] = p > 0 ? best.i[p - 1] : own[0];
            best.v[p] = p > 0 ? best.v[p - 1] : -INFINITY;
        }
    }
#pragma unroll
    for (int p = 0; p < K; ++p) {
        if (p < k && lane == p) {
            idx_out[(long long)row * k + p] = best.i[p];
            val_out[(long long)row * k + p] = best.v[p];
        }
    }
}

template <int K>
static void patchmatch_launch(const void* qh, const void* ql, const void* kh, const void* kl, const int* idx_in, int* idx_out,
                              float* val_out, int rows, int hq, int wq, int hk, int wk, int k, int stride, int S, int R, int seed,
                              int iteration, float logit_scale, hipStream_t st) {
    hipLaunchKernelGGL(patchmatch_step_kernel<K>, dim3((unsigned)((rows + PM_WAVES - 1) / PM_WAVES)), dim3(PM_THREADS), 0, st,
                       (const _Float16*)qh, (const _Float16*)ql, (const _Float16*)kh, (const _Float16*)kl, idx_in, idx_out, val_out, rows,
                       hq, wq, hk, wk, k, stride, S, R, seed, iteration, logit_scale);
}

}  // namespace cocos

extern "C" int cocos_patchmatch_step_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const int* idx_in,
                                           int* idx_out, float* val_out, int B, int K, int hq, int wq, int hk, int wk, int k, int stride,
                                           int radii, int radius0, int seed, int iteration, float inv_temperature, float operand_scale,
                                           cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "patchmatch_step_f16x3";
    COCOS_REQUIRE(qh && ql && kh && kl && idx_out && val_out, COCOS_ERR_INVALID, "%s: null pointer", name);
    COCOS_REQUIRE(idx_in != idx_out, COCOS_ERR_INVALID, "%s: idx_in and idx_out are one buffer (a step reads one table and writes another)",
                  name);
    COCOS_REQUIRE(operand_scale > 0.f && inv_temperature > 0.f, COCOS_ERR_INVALID, "%s: inv_temperature and operand_scale must be positive",
                  name);
    COCOS_REQUIRE(K == SW_KD, COCOS_ERR_UNSUPPORTED, "%s: needs K == 256 (got %d)", name, K);
    COCOS_REQUIRE(B >= 1 && hq >= 1 && wq >= 1 && hk >= 1 && wk >= 1, COCOS_ERR_UNSUPPORTED, "%s: empty grid: B=%d query %dx%d key %dx%d",
                  name, B, hq, wq, hk, wk);
    const long long Nq = (long long)hq * wq, Nk = (long long)hk * wk;
    if (const int rc = pm_check_schedule(name, k, Nk, stride, radii, radius0)) return rc;
    if (const int rc = pm_check_tables(name, B, Nq, Nk, k)) return rc;
    for (const void* p : {qh, ql, kh, kl})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: q/k planes must be 16-byte aligned", name);
    const int rows = (int)(B * Nq);
    const float logit_scale = inv_temperature / (operand_scale * operand_scale);
    const hipStream_t st = as_stream(stream);
    // k between two instantiations runs the next larger one, truncated
#define COCOS_PM_LAUNCH(KK) \
    patchmatch_launch<KK>(qh, ql, kh, kl, idx_in, idx_out, val_out, rows, hq, wq, hk, wk, k, stride, radii, radius0, seed, iteration, logit_scale, st)
    if (k == 1) COCOS_PM_LAUNCH(1);
    else if (k == 2) COCOS_PM_LAUNCH(2);
    else if (k <= 4) COCOS_PM_LAUNCH(4);
    else COCOS_PM_LAUNCH(8);
#undef COCOS_PM_LAUNCH
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
