// K44: sub-cell refinement of a hard match — a soft-argmax over the (2 r + 1)^2 window of keys around the match.  Per query (b, i) with
// centre key idx[b,i] (clamped into [0, Nk)) at (yk, xk) of the hk x wk key grid:
//   window   the keys (yk + dy, xk + dx), |dy|, |dx| <= r, INSIDE the key grid (a position outside is left out: not clamped, not
//            wrapped), visited dy ascending outside, dx ascending inside
//   s        inv_temperature <q, k> of every window key: K42's logit of the pair, bit for bit (sparse_row.h)
//   m        max s;  lse_win = m + log sum exp(s - m);  p = exp(s - lse_win)
//   off      (sum p dx, sum p dy), summed in visiting order, then limited to [-r, r] (the rounded p may sum to an ulp above 1)
// One wave per query, four per workgroup, no LDS, no atomics, no communication: the result is a pure function of the arguments.  The
// 2 r + 1 row loads of one window row are issued before the first butterfly (as K43 batches a source).  Every lane holds the same score
// bits; they are read through readfirstlane, so the window state (scores, maximum, sums) is wave-uniform.  Contraction is off in the
// softmax and every fused multiply-add is written out: these lines DEFINE the rounding of lse_win and off.  Non-finite scores are
// not sanitised: a NaN or +inf score makes lse_win and off NaN.
#include "sparse_row.h"

namespace cocos {

constexpr int MR_WAVES = 4;              // queries per workgroup, one per wave
constexpr int MR_THREADS = MR_WAVES * kWave;

template <int R>
__global__ __launch_bounds__(MR_THREADS) void match_refine_kernel(const _Float16* __restrict__ qh, const _Float16* __restrict__ ql,
                                                                  const _Float16* __restrict__ kh, const _Float16* __restrict__ kl,
                                                                  const int* __restrict__ idx, float* __restrict__ off,
                                                                  float* __restrict__ lse_win, int rows, int Nq, int hk, int wk,
                                                                  float logit_scale) {
#pragma clang fp contract(off)
    constexpr int W = 2 * R + 1;
    const int lane = threadIdx.x & (kWave - 1);
    // (the wave index is the same in all 64 lanes: saying so keeps the window arithmetic on the scalar side)
    const int row = (int)blockIdx.x * MR_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // b * Nq + i
    if (row >= rows) return;                                                          // (whole waves; the kernel has no barrier)
    const int Nk = hk * wk;
    const int b = row / Nq;
    const long long kbase = (long long)b * Nk;
    const int j = clamp_key(__builtin_amdgcn_readfirstlane(idx[row]), Nk);
    const int yk = j / wk, xk = j - yk * wk;
    const f32x4 q = load_row4(qh, ql, row, lane);

    float s[W * W];
    bool in[W * W];
#pragma unroll
    for (int a = 0; a < W; ++a) {
        const int ky = yk + a - R;
        const bool row_in = ky >= 0 && ky < hk;      // wave-uniform
#pragma unroll
        for (int c = 0; c < W; ++c) {
            in[a * W + c] = row_in && xk + c - R >= 0 && xk + c - R < wk;
            s[a * W + c] = 0.f;
        }
        if (!row_in) continue;
        // the W rows of this window row first, then their reductions; a column outside the grid loads the nearest one inside (the
        // address stays in the buffer) and its score is not used
        f32x4 kv[W];
#pragma unroll
        for (int c = 0; c < W; ++c) kv[c] = load_row4(kh, kl, kbase + (long long)ky * wk + min(max(xk + c - R, 0), wk - 1), lane);
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const float sc = wave_sum(lane_dot4(q, kv[c])) * logit_scale;
            s[a * W + c] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sc)));
        }
    }
    // the centre is always inside: the window is never empty
    float m = -INFINITY;
#pragma unroll
    for (int e = 0; e < W * W; ++e) m = in[e] ? fmaxf(m, s[e]) : m;
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < W * W; ++e) sum = in[e] ? sum + expf(s[e] - m) : sum;
    const float lse = m + logf(sum);
    float ox = 0.f, oy = 0.f;
#pragma unroll
    for (int e = 0; e < W * W; ++e) {
        if (in[e]) {
            const float p = expf(s[e] - lse);
            ox = __builtin_fmaf(p, (float)(e % W - R), ox);
            oy = __builtin_fmaf(p, (float)(e / W - R), oy);
        }
    }
    // the rounded weights may sum to an ulp above 1: |off| <= R is kept exactly (comparisons, not fmin / fmax: a NaN stays a NaN)
    ox = ox > (float)R ? (float)R : (ox < -(float)R ? -(float)R : ox);
    oy = oy > (float)R ? (float)R : (oy < -(float)R ? -(float)R : oy);
    if (lane == 0) {
        off[(long long)row * 2] = ox;
        off[(long long)row * 2 + 1] = oy;
        lse_win[row] = lse;
    }
}

template <int R>
static void match_refine_launch(const void* qh, const void* ql, const void* kh, const void* kl, const int* idx, float* off, float* lse_win,
                                int rows, int Nq, int hk, int wk, float logit_scale, hipStream_t st) {
    hipLaunchKernelGGL(match_refine_kernel<R>, dim3((unsigned)((rows + MR_WAVES - 1) / MR_WAVES)), dim3(MR_THREADS), 0, st,
                       (const _Float16*)qh, (const _Float16*)ql, (const _Float16*)kh, (const _Float16*)kl, idx, off, lse_win, rows, Nq, hk,
                       wk, logit_scale);
}

}  // namespace cocos

extern "C" int cocos_match_refine_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const int* idx, float* off,
                                        float* lse_win, int B, int K, int Nq, int Nk, int hk, int wk, int radius, float inv_temperature,
                                        float operand_scale, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "match_refine_f16x3";
    COCOS_REQUIRE(qh && ql && kh && kl && idx && off && lse_win, COCOS_ERR_INVALID, "%s: null pointer (qh, ql, kh, kl, idx, off, lse_win)", name);
    COCOS_REQUIRE(B >= 1 && Nq >= 1 && Nk >= 1 && hk >= 1 && wk >= 1, COCOS_ERR_INVALID,
                  "%s: non-positive size: B=%d Nq=%d Nk=%d hk=%d wk=%d", name, B, Nq, Nk, hk, wk);
    COCOS_REQUIRE((long long)hk * wk == Nk, COCOS_ERR_INVALID, "%s: hk=%d x wk=%d is not the key grid of Nk=%d keys", name, hk, wk, Nk);
    COCOS_REQUIRE(radius >= 1 && radius <= COCOS_MATCH_REFINE_MAX_RADIUS, COCOS_ERR_INVALID, "%s: radius=%d: expected 1 .. %d", name, radius,
                  COCOS_MATCH_REFINE_MAX_RADIUS);
    COCOS_REQUIRE(operand_scale > 0.f && inv_temperature > 0.f, COCOS_ERR_INVALID, "%s: inv_temperature and operand_scale must be positive",
                  name);
    COCOS_REQUIRE(K == SW_KD, COCOS_ERR_UNSUPPORTED, "%s: needs K == 256 (got %d)", name, K);
    COCOS_REQUIRE((long long)B * Nq < 0x3ffffff0ll && (long long)B * Nk < 0x7fffffffll, COCOS_ERR_UNSUPPORTED,
                  "%s: B Nq = %lld queries / B Nk = %lld keys exceed the 32-bit tables", name, (long long)B * Nq, (long long)B * Nk);
    for (const void* p : {qh, ql, kh, kl})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: q/k planes must be 16-byte aligned", name);
    const int rows = B * Nq;
    const float logit_scale = inv_temperature / (operand_scale * operand_scale);
    const hipStream_t st = as_stream(stream);
    if (radius == 1) match_refine_launch<1>(qh, ql, kh, kl, idx, off, lse_win, rows, Nq, hk, wk, logit_scale, st);
    else if (radius == 2) match_refine_launch<2>(qh, ql, kh, kl, idx, off, lse_win, rows, Nq, hk, wk, logit_scale, st);
    else match_refine_launch<3>(qh, ql, kh, kl, idx, off, lse_win, rows, Nq, hk, wk, logit_scale, st);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
