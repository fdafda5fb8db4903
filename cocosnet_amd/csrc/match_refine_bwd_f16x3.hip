// K46: the backward of K44's window soft-argmax (match_refine_f16x3.hip) — gradients of the refined offset to the two operands.
// With W = 2 r + 1, slot e = (dy + r) W + (dx + r) of query (b, i) whose centre key (clamped) sits at (yk, xk):
//   s_e      the window's logits, recomputed as match_refine_kernel forms them, bit for bit: the same membership, the same visiting
//            order, the same sparse_row.h helpers;  m = max s,  p_e = exp(s_e - m) / sum exp(s - m)  (= exp(s_e - lse_win), formed
//            without rounding lse_win)
//   o        = (sum p dx, sum p dy), summed in visiting order and NOT limited to [-r, r]: the forward's limit only absorbs an ulp of
//            rounding and is the identity here
//   ds_e     = p_e ((dx_e - o_x) doff_x + (dy_e - o_y) doff_y)   (d off / d s_e contracted with the incoming doff);  0 for a slot
//            outside the key grid — every one of the W^2 slots is written
//   dq_t[i]  = inv_t sum_e ds_e kn[j_e]   (query kernel, slots ascending)
//   dk_t[j]  = inv_t sum ds[i, e] qn[i]   (key kernel) over the queries i whose window holds key j in slot e
// The key side is a GATHER, as K42's: key j at (yj, xj) lies in slot (dy, dx) of exactly the queries whose centre is
// (yj - dy, xj - dx), and the inverse table of the clamped centre table (k = 1) lists those per centre.  One wave per query / key, four
// per workgroup, no LDS, no atomics; fp32 in a fixed order with contraction off and every fused multiply-add written out, so the
// results are bitwise reproducible.  A centre all queries share is one serial list per neighbouring key (K42's documented worst case).
#include "sparse_row.h"

namespace cocos {

constexpr int MRB_WAVES = 4;             // queries or keys per workgroup, one per wave
constexpr int MRB_THREADS = MRB_WAVES * kWave;

__device__ __forceinline__ float uniform_f32(float v) {      // the same bits in all lanes, said so: the value moves to the scalar side
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

template <int R>
__global__ __launch_bounds__(MRB_THREADS) void match_refine_bwd_query_kernel(
    const _Float16* __restrict__ qh, const _Float16* __restrict__ ql, const _Float16* __restrict__ kh, const _Float16* __restrict__ kl,
    const int* __restrict__ idx, const float* __restrict__ doff, float* __restrict__ ds, float* __restrict__ dq_t, int rows, int Nq, int hk,
    int wk, float logit_scale, float grad_scale) {
#pragma clang fp contract(off)
    constexpr int W = 2 * R + 1;
    const int lane = threadIdx.x & (kWave - 1);
    const int row = (int)blockIdx.x * MRB_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // b * Nq + i
    if (row >= rows) return;                                                          // (whole waves; the kernel has no barrier)
    const int Nk = hk * wk;
    const int b = row / Nq;
    const long long kbase = (long long)b * Nk;
    const int j = clamp_key(__builtin_amdgcn_readfirstlane(idx[row]), Nk);
    const int yk = j / wk, xk = j - yk * wk;
    const f32x4 q = load_row4(qh, ql, row, lane);

    // ---- the forward's scores, maximum and sum, line for line (match_refine_kernel), and the expected offset
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
        f32x4 kv[W];
#pragma unroll
        for (int c = 0; c < W; ++c) kv[c] = load_row4(kh, kl, kbase + (long long)ky * wk + min(max(xk + c - R, 0), wk - 1), lane);
#pragma unroll
        for (int c = 0; c < W; ++c) s[a * W + c] = uniform_f32(wave_sum(lane_dot4(q, kv[c])) * logit_scale);
    }
    float m = -INFINITY;
#pragma unroll
    for (int e = 0; e < W * W; ++e) m = in[e] ? fmaxf(m, s[e]) : m;
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < W * W; ++e) sum = in[e] ? sum + expf(s[e] - m) : sum;
    // p = exp(s - m) / sum: exp(s - lse_win) without the rounding of lse_win = m + log(sum), which would move every weight by the same
    // relative half ulp of lse_win (4e-6 at |lse_win| = 100) — the gradient is judged by its own error, not by the forward's bits
    const float inv = 1.0f / sum;
    float ox = 0.f, oy = 0.f;
#pragma unroll
    for (int e = 0; e < W * W; ++e) {
        if (in[e]) {
            const float p = expf(s[e] - m) * inv;
            ox = __builtin_fmaf(p, (float)(e % W - R), ox);
            oy = __builtin_fmaf(p, (float)(e / W - R), oy);
        }
    }

    // ---- the backward: ds per slot (lane e keeps slot e: W^2 <= 49 < 64) and, row of the window by row, dq
    const float gx = uniform_f32(doff[(long long)row * 2]), gy = uniform_f32(doff[(long long)row * 2 + 1]);
    float mine = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < W; ++a) {
        const int ky = yk + a - R;
        if (ky < 0 || ky >= hk) continue;            // wave-uniform: the slots of this window row stay 0
        f32x4 kv[W];
        if (dq_t) {
#pragma unroll
            for (int c = 0; c < W; ++c) kv[c] = load_row4(kh, kl, kbase + (long long)ky * wk + min(max(xk + c - R, 0), wk - 1), lane);
        }
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const int e = a * W + c;
            if (!in[e]) continue;
            const float p = expf(s[e] - m) * inv;
            const float d = p * (((float)(c - R) - ox) * gx + ((float)(a - R) - oy) * gy);
            mine = lane == e ? d : mine;
            if (dq_t) {
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = __builtin_fmaf(d, kv[c][u], acc[u]);
            }
        }
    }
    if (lane < W * W) ds[(long long)row * (W * W) + lane] = mine;
    if (dq_t) {
        const f32x4 out = {acc[0] * grad_scale, acc[1] * grad_scale, acc[2] * grad_scale, acc[3] * grad_scale};
        *reinterpret_cast<f32x4*>(dq_t + (long long)row * SW_KD + lane * 4) = out;
    }
}

// entries[offsets[c] .. offsets[c + 1]) are the rows b Nq + i of the queries whose (clamped) centre is c = b Nk + j', ascending: K42's
// inverse table with k = 1.  Positions and ranges are clamped into the tables: a malformed table cannot send a read outside ds / the planes.
__global__ __launch_bounds__(MRB_THREADS) void match_refine_bwd_key_kernel(const _Float16* __restrict__ qh, const _Float16* __restrict__ ql,
                                                                           const float* __restrict__ ds, const int* __restrict__ entries,
                                                                           const int* __restrict__ offsets, float* __restrict__ dk_t,
                                                                           int keys, int total, int hk, int wk, int r, float grad_scale) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const int key = (int)blockIdx.x * MRB_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // b * Nk + j
    if (key >= keys) return;
    const int Nk = hk * wk, W = 2 * r + 1;
    const int b = key / Nk, j = key - b * Nk;
    const int yj = j / wk, xj = j - yj * wk;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int dy = -r; dy <= r; ++dy) {
        const int cy = yj - dy;
        if (cy < 0 || cy >= hk) continue;
        for (int dx = -r; dx <= r; ++dx) {
            const int cx = xj - dx;
            if (cx < 0 || cx >= wk) continue;
            const long long centre = (long long)b * Nk + (long long)cy * wk + cx;
            const int slot = (dy + r) * W + (dx + r);
            const int beg = min(max(offsets[centre], 0), total), end = min(max(offsets[centre + 1], beg), total);
            for (int e = beg; e < end; ++e) {
                const int p = min(max(entries[e], 0), total - 1);
                const float d = ds[(long long)p * (W * W) + slot];
                const f32x4 qv = load_row4(qh, ql, p, lane);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = __builtin_fmaf(d, qv[u], acc[u]);
            }
        }
    }
    const f32x4 out = {acc[0] * grad_scale, acc[1] * grad_scale, acc[2] * grad_scale, acc[3] * grad_scale};
    *reinterpret_cast<f32x4*>(dk_t + (long long)key * SW_KD + lane * 4) = out;      // a key in nobody's window: zeros
}

template <int R>
static void match_refine_bwd_query_launch(const void* qh, const void* ql, const void* kh, const void* kl, const int* idx, const float* doff,
                                          float* ds, float* dq_t, int rows, int Nq, int hk, int wk, float logit_scale, float grad_scale,
                                          hipStream_t st) {
    hipLaunchKernelGGL(match_refine_bwd_query_kernel<R>, dim3((unsigned)((rows + MRB_WAVES - 1) / MRB_WAVES)), dim3(MRB_THREADS), 0, st,
                       (const _Float16*)qh, (const _Float16*)ql, (const _Float16*)kh, (const _Float16*)kl, idx, doff, ds, dq_t, rows, Nq,
                       hk, wk, logit_scale, grad_scale);
}

// the checks the two entry points share (before any HIP call)
static int match_refine_bwd_check(const char* name, int B, int K, int Nq, int Nk, int hk, int wk, int radius, float inv_temperature,
                                  float operand_scale) {
    COCOS_REQUIRE(B >= 1 && Nq >= 1 && Nk >= 1 && hk >= 1 && wk >= 1, COCOS_ERR_INVALID,
                  "%s: non-positive size: B=%d Nq=%d Nk=%d hk=%d wk=%d", name, B, Nq, Nk, hk, wk);
    COCOS_REQUIRE((long long)hk * wk == Nk, COCOS_ERR_INVALID, "%s: hk=%d x wk=%d is not the key grid of Nk=%d keys", name, hk, wk, Nk);
    COCOS_REQUIRE(radius >= 1 && radius <= COCOS_MATCH_REFINE_MAX_RADIUS, COCOS_ERR_INVALID, "%s: radius=%d: expected 1 .. %d", name, radius,
                  COCOS_MATCH_REFINE_MAX_RADIUS);
    COCOS_REQUIRE(operand_scale > 0.f && inv_temperature > 0.f, COCOS_ERR_INVALID, "%s: inv_temperature and operand_scale must be positive",
                  name);
    COCOS_REQUIRE(K == SW_KD, COCOS_ERR_UNSUPPORTED, "%s: needs K == 256 (got %d)", name, K);
    const long long slots = (long long)(2 * radius + 1) * (2 * radius + 1);
    COCOS_REQUIRE((long long)B * Nq * slots < 0x7fffffffll && (long long)B * Nk < 0x7fffffffll, COCOS_ERR_UNSUPPORTED,
                  "%s: B Nq W = %lld window slots / B Nk = %lld keys exceed the 32-bit tables", name, (long long)B * Nq * slots,
                  (long long)B * Nk);
    return COCOS_OK;
}

}  // namespace cocos

extern "C" int cocos_match_refine_bwd_query_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const int* idx,
                                                  const float* doff, float* ds, float* dq_t, int B, int K, int Nq, int Nk, int hk, int wk,
                                                  int radius, float inv_temperature, float operand_scale, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "match_refine_bwd_query_f16x3";
    COCOS_REQUIRE(qh && ql && kh && kl && idx && doff && ds, COCOS_ERR_INVALID, "%s: null pointer (qh, ql, kh, kl, idx, doff, ds)", name);
    if (int rc = match_refine_bwd_check(name, B, K, Nq, Nk, hk, wk, radius, inv_temperature, operand_scale)) return rc;
    for (const void* p : {qh, ql, kh, kl, (const void*)dq_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the q/k planes and dq_t must be 16-byte aligned", name);
    const int rows = B * Nq;
    const float logit_scale = inv_temperature / (operand_scale * operand_scale), grad_scale = inv_temperature / operand_scale;
    const hipStream_t st = as_stream(stream);
    if (radius == 1) match_refine_bwd_query_launch<1>(qh, ql, kh, kl, idx, doff, ds, dq_t, rows, Nq, hk, wk, logit_scale, grad_scale, st);
    else if (radius == 2) match_refine_bwd_query_launch<2>(qh, ql, kh, kl, idx, doff, ds, dq_t, rows, Nq, hk, wk, logit_scale, grad_scale, st);
    else match_refine_bwd_query_launch<3>(qh, ql, kh, kl, idx, doff, ds, dq_t, rows, Nq, hk, wk, logit_scale, grad_scale, st);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_match_refine_bwd_key_f16x3(const void* qh, const void* ql, const float* ds, const int* entries, const int* offsets,
                                                float* dk_t, int B, int K, int Nq, int Nk, int hk, int wk, int radius, float inv_temperature,
                                                float operand_scale, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "match_refine_bwd_key_f16x3";
    COCOS_REQUIRE(qh && ql && ds && entries && offsets && dk_t, COCOS_ERR_INVALID, "%s: null pointer (qh, ql, ds, entries, offsets, dk_t)", name);
    if (int rc = match_refine_bwd_check(name, B, K, Nq, Nk, hk, wk, radius, inv_temperature, operand_scale)) return rc;
    for (const void* p : {qh, ql, (const void*)dk_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the query planes and dk_t must be 16-byte aligned", name);
    const int keys = B * Nk;
    hipLaunchKernelGGL(match_refine_bwd_key_kernel, dim3((unsigned)((keys + MRB_WAVES - 1) / MRB_WAVES)), dim3(MRB_THREADS), 0,
                       as_stream(stream), (const _Float16*)qh, (const _Float16*)ql, ds, entries, offsets, dk_t, keys, B * Nq, hk, wk, radius,
                       inv_temperature / operand_scale);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
