// K57: one PatchMatch iteration of the top-k candidate search on the match_kernel-3 route — K43's step (patchmatch_f16x3.hip) with the
// box logit of K51 (box3_pair.hip) as the score.  The pool of a query is K43's exactly: the own list, the four neighbours' lists shifted
// back, the hashed search, the hashed initialisation without a table — all of it patchmatch_pool.h, shared with K43, 32-bit integer
// arithmetic on the scalar side that tests/patchmatch_case.py restates.  One launch is one JACOBI iteration: idx_in is read, idx_out
// (another buffer) is written, no atomics, no LDS, nothing between workgroups — the result is a pure function of the arguments.
//
// A score is K51's logit of the pair (p, q) on fp32 position-major rows [B,N,256] and the K12 statistics [B,N]:
//   R[p,q] = sum over the taps d in {-1,0,1}^2 of [p+d inside the content grid] [q+d inside the exemplar grid] <theta[:,p+d], phi[:,q+d]>
//   c = R[p,q] - kc mu_p nu_q,   z = inv_t a_p b_q c,   kc = 9 * 256
// R is box3_rows.h's: the query's nine tap rows are loaded once per wave (load_query_taps), a candidate is one pair_R — nine row loads
// in flight, the one place that decides "inside" for a pair, on the 2-D coordinates.  c and z are formed in the expressions of
// box3_sparse_fwd_kernel, under the same contraction regime (this unit's default, as that kernel's), so softmax(val) and K51's w on the
// returned table differ by rounding at most.  Candidates are scored one at a time: the nine taps already fill the load queue, and the
// 36 registers of the query's taps leave no room to hold K candidates' rows at eight waves per SIMD.  Every lane holds the same score
// bits (pair_R ends in the xor butterfly), so the candidate list is wave-uniform, as K43's.
#include "box3_rows.h"
#include "patchmatch_pool.h"

namespace cocos {

template <int K>
__global__ __launch_bounds__(PM_THREADS) void patchmatch_step_box3_kernel(const float* __restrict__ th_t, const float* __restrict__ ph_t,
                                                                          const float* __restrict__ mu, const float* __restrict__ a,
                                                                          const float* __restrict__ nu, const float* __restrict__ b,
                                                                          const int* __restrict__ idx_in, int* __restrict__ idx_out,
                                                                          float* __restrict__ val_out, int rows, int fh, int fw, int gh,
                                                                          int gw, int k, int stride, int S, int R, int seed, int iteration,
                                                                          float inv_t, float kc) {
    const int lane = threadIdx.x & (kWave - 1);
    // (the wave index is the same in all 64 lanes: saying so keeps the candidate arithmetic and the list on the scalar side)
    const int row = (int)blockIdx.x * PM_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // b * Nq + p
    if (row >= rows) return;                                                          // (whole waves; the kernel has no barrier)
    const int Nq = fh * fw, Nk = gh * gw;
    const int bq = row / Nq, p = row - bq * Nq;
    const int py = p / fw, px = p - py * fw;
    const long long kbase = (long long)bq * Nk;
    const QueryTaps taps = load_query_taps(th_t, row, py, px, fh, fw, lane);
    const float kmu = kc * mu[row], za = inv_t * a[row];

    int own[K];
    pm_list<K>(own, idx_in, row, k, Nk, seed, iteration);
    PoolList<K> best;
    best.clear();

    const PmStep step{fh, fw, gh, gw, Nq, Nk, k, stride, S, R, seed, iteration};
    for (int src = 0; src < pm_sources(step); ++src) {
        int cand[K];      // key index, or -1: no candidate
        pm_source<K>(cand, src, own, idx_in, row, bq, py, px, step);
#pragma unroll
        for (int r = 0; r < K; ++r) {
            if (cand[r] < 0) continue;      // (wave-uniform: a whole-wave branch)
            const int j = cand[r], qy = j / gw, qx = j - qy * gw;
            const long long key = kbase + j;
            const float c = pair_R(taps, ph_t, key, qy, qx, gh, gw, lane) - kmu * nu[key];
            const float z = za * b[key] * c;
            // (every lane holds the same bits: reading lane 0's makes the list wave-uniform for the compiler too)
            best.insert(uniform_f32(z), j);
        }
    }
    // fewer than k distinct keys in the pool (or scores that are NaN): the remaining slots repeat the last filled pair; a list that
    // stayed empty returns the own candidates with -inf
#pragma unroll
    for (int r = 0; r < K; ++r) {
        if (best.i[r] < 0) {
            best.i[r] = r > 0 ? best.i[r - 1] : own[0];
            best.v[r] = r > 0 ? best.v[r - 1] : -INFINITY;
        }
    }
#pragma unroll
    for (int r = 0; r < K; ++r) {
        if (r < k && lane == r) {
            idx_out[(long long)row * k + r] = best.i[r];
            val_out[(long long)row * k + r] = best.v[r];
        }
    }
}

template <int K>
static void patchmatch_box3_launch(const float* th_t, const float* ph_t, const float* mu, const float* a, const float* nu, const float* b,
                                   const int* idx_in, int* idx_out, float* val_out, int rows, int fh, int fw, int gh, int gw, int k,
                                   int stride, int S, int R, int seed, int iteration, float inv_t, hipStream_t st) {
    hipLaunchKernelGGL(patchmatch_step_box3_kernel<K>, dim3((unsigned)((rows + PM_WAVES - 1) / PM_WAVES)), dim3(PM_THREADS), 0, st, th_t,
                       ph_t, mu, a, nu, b, idx_in, idx_out, val_out, rows, fh, fw, gh, gw, k, stride, S, R, seed, iteration, inv_t,
                       (float)(9 * BOX3_ROW_C));
}

}  // namespace cocos

extern "C" int cocos_patchmatch_step_box3(const float* th_t, const float* ph_t, const float* mu, const float* a, const float* nu,
                                          const float* b, const int* idx_in, int* idx_out, float* val_out, int B, int K, int fh, int fw,
                                          int gh, int gw, int k, int stride, int radii, int radius0, int seed, int iteration,
                                          float inv_temperature, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "patchmatch_step_box3";
    COCOS_REQUIRE(th_t && ph_t && mu && a && nu && b && idx_out && val_out, COCOS_ERR_INVALID, "%s: null pointer", name);
    COCOS_REQUIRE(idx_in != idx_out, COCOS_ERR_INVALID, "%s: idx_in and idx_out are one buffer (a step reads one table and writes another)",
                  name);
    COCOS_REQUIRE(inv_temperature > 0.f, COCOS_ERR_INVALID, "%s: inv_temperature must be positive", name);
    COCOS_REQUIRE(K == BOX3_ROW_C, COCOS_ERR_UNSUPPORTED, "%s: needs K == 256 (got %d)", name, K);
    COCOS_REQUIRE(B >= 1 && fh >= 1 && fw >= 1 && gh >= 1 && gw >= 1, COCOS_ERR_UNSUPPORTED,
                  "%s: empty grid: B=%d content grid %dx%d exemplar grid %dx%d", name, B, fh, fw, gh, gw);
    const long long Nq = (long long)fh * fw, Nk = (long long)gh * gw;
    if (const int rc = pm_check_schedule(name, k, Nk, stride, radii, radius0)) return rc;
    if (const int rc = pm_check_tables(name, B, Nq, Nk, k)) return rc;
    for (const void* p : {th_t, ph_t}) COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the theta / phi rows must be 16-byte aligned", name);
    const int rows = (int)(B * Nq);
    const hipStream_t st = as_stream(stream);
    // k between two instantiations runs the next larger one, truncated
#define COCOS_PM_LAUNCH(KK)                                                                                                                   \
    patchmatch_box3_launch<KK>(th_t, ph_t, mu, a, nu, b, idx_in, idx_out, val_out, rows, fh, fw, gh, gw, k, stride, radii, radius0, seed, \
                               iteration, inv_temperature, st)
    if (k == 1) COCOS_PM_LAUNCH(1);
    else if (k == 2) COCOS_PM_LAUNCH(2);
    else if (k <= 4) COCOS_PM_LAUNCH(4);
    else COCOS_PM_LAUNCH(8);
#undef COCOS_PM_LAUNCH
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
