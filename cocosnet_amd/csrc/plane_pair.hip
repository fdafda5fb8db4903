// K42 / K44 / K46: the trainable sparse kernels of the match_kernel-1 route — a softmax over a few CANDIDATE keys per query, on the
// logit of ONE pair  s = inv_temperature <qn[b,:,i], kn[b,:,j]>.  Nothing here has an Nq x Nk extent.
//   K42  the candidates are the k keys j_r = idx[b,i,r] (clamped into [0, Nk)) that the match readout (K39a) selected; w = softmax_r s,
//        out[b,:,i] = sum_r w[b,i,r] v[b,:,j_r] — the k-sparse correspondence warp, and its three gradients.  State: idx, w, ds [B,Nq,k].
//        With a bias (K50) s_r += k_bias[b, j_r] before the softmax.
//   K44  the candidates are the keys INSIDE the hk x wk key grid of the (2 r + 1)^2 window around the hard match idx[b,i] (Window,
//        below); lse_win = m + log sum exp(s - m), p = exp(s - lse_win), off = (sum p dx, sum p dy) in visiting order, then limited to
//        [-r, r] (the rounded p may sum to an ulp above 1) — the sub-cell refinement.
//   K46  K44's backward, on the SAME window (the one definition below): p_e = exp(s_e - m) / sum exp(s - m) (= exp(s_e - lse_win),
//        formed without rounding lse_win), o = (sum p dx, sum p dy) NOT limited (the forward's limit only absorbs an ulp of rounding and
//        is the identity here), ds_e = p_e ((dx_e - o_x) doff_x + (dy_e - o_y) doff_y), 0 for a slot outside the key grid — every one
//        of the W^2 slots is written; dq_t[i] = inv_t sum_e ds_e kn[j_e] (slots ascending), dk_t[j] = inv_t sum ds[i, e] qn[i].
// Operands are the position-major f16 hi/lo planes [B,N,256] of unit-norm columns x operand_scale that K39a chose the candidates from
// (value = (hi + lo) / operand_scale: split_f16.hip), read as whole 512-byte rows (sparse_row.h).  Every tensor a wave gathers rows
// from is position-major ([B,N,C]: v^T, dout^T), and so is everything it writes (out^T, dqn^T, dkn^T, dv^T): one contiguous row per
// wave.  The channel-major tensors of the public ops are made from / turned into these by cocos_transpose_f32 below, once per tensor
// and call, never per query.  One wave per row, four per workgroup, no LDS, no atomics; every sum has a fixed order: the results are
// bitwise reproducible.
//   forward, query backward   one wave per query
//   key backward              one wave per key, a GATHER over the inverse table of idx (sparse_row.h: list_begin / list_end /
//                             list_entry), summed serially in table order; a key nobody names gets zeros from these kernels.  A key
//                             every query names is a serial list of Nq entries.
// K42's kernels are compiled with contraction on and keep their x * y + z expressions in their own bodies; the window, K44 and K46 are
// compiled with contraction off and every fused multiply-add written out: those lines DEFINE the rounding of lse_win and off.
#include <type_traits>

#include "sparse_row.h"

namespace cocos {

constexpr int SW_MAXK = COCOS_MATCH_TOPK_MAX;

// ---- K42 ----------------------------------------------------------------------------------------------------------------------------
// BIAS (K50): k_bias [B,Nk] fp32, or one [Nk] row when bias_bstride is 0; finite or -inf.  A row whose k candidates all carry -inf has
// no largest logit to refer to: its w is the uniform 1 / k.  The bias is a constant of the backward, which consumes the saved w.
// Without BIAS the pointer is not read.
template <bool BIAS>
__global__ __launch_bounds__(ROW_THREADS) void sparse_warp_fwd_kernel(const _Float16* __restrict__ qh, const _Float16* __restrict__ ql,
                                                                      const _Float16* __restrict__ kh, const _Float16* __restrict__ kl,
                                                                      const float* __restrict__ vt, const int* __restrict__ idx,
                                                                      float* __restrict__ out_t, float* __restrict__ w_out,
                                                                      long long rows, int Nq, int Nk, int Cv, int k, float logit_scale,
                                                                      const float* __restrict__ k_bias, long long bias_bstride) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);     // b * Nq + i
    if (row >= rows) return;                                                          // (whole waves; the kernel has no barrier)
    const long long kbase = (row / Nq) * Nk;
    const f32x4 q = load_row4(qh, ql, row, lane);
    long long key[SW_MAXK];
    float s[SW_MAXK];
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < SW_MAXK; ++r) {
        key[r] = kbase;
        s[r] = -INFINITY;
        if (r < k) {
            key[r] = kbase + clamp_key(idx[row * k + r], Nk);
            const f32x4 kv = load_row4(kh, kl, key[r], lane);
            s[r] = wave_sum(lane_dot4(q, kv)) * logit_scale;
            if constexpr (BIAS) s[r] += k_bias[(row / Nq) * bias_bstride + (key[r] - kbase)];
            m = fmaxf(m, s[r]);
        }
    }
    if constexpr (BIAS) {
        if (m == -INFINITY) {      // every candidate excluded: uniform weights
            m = 0.f;
#pragma unroll
            for (int r = 0; r < SW_MAXK; ++r) s[r] = 0.f;
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < SW_MAXK; ++r) {
        s[r] = r < k ? expf(s[r] - m) : 0.f;
        sum += s[r];
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int r = 0; r < SW_MAXK; ++r) {
        s[r] *= inv;
        if (r < k && lane == r) w_out[row * k + r] = s[r];
    }
    for (int c = lane; c < Cv; c += kWave) {
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < SW_MAXK; ++r)
            if (r < k) acc = __builtin_fmaf(s[r], vt[key[r] * Cv + c], acc);
        out_t[row * Cv + c] = acc;
    }
}

//   dw_r = <dout^T[i], v^T[j_r]>, ds_r = w_r (dw_r - sum w dw), dqn^T[i] = inv_t sum_r ds_r kn[j_r].  dq_t may be null.
__global__ __launch_bounds__(ROW_THREADS) void sparse_warp_bwd_query_kernel(const _Float16* __restrict__ kh, const _Float16* __restrict__ kl,
                                                                            const float* __restrict__ vt, const float* __restrict__ dout_t,
                                                                            const int* __restrict__ idx, const float* __restrict__ w,
                                                                            float* __restrict__ ds_out, float* __restrict__ dq_t,
                                                                            long long rows, int Nq, int Nk, int Cv, int k, float grad_scale) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long long kbase = (row / Nq) * Nk;
    long long key[SW_MAXK];
    float wr[SW_MAXK], dw[SW_MAXK];
#pragma unroll
    for (int r = 0; r < SW_MAXK; ++r) {
        key[r] = kbase + (r < k ? clamp_key(idx[row * k + r], Nk) : 0);
        wr[r] = r < k ? w[row * k + r] : 0.f;
        dw[r] = 0.f;
    }
    for (int c = lane; c < Cv; c += kWave) {
        const float g = dout_t[row * Cv + c];
#pragma unroll
        for (int r = 0; r < SW_MAXK; ++r)
            if (r < k) dw[r] = __builtin_fmaf(g, vt[key[r] * Cv + c], dw[r]);
    }
    float dot = 0.f;
#pragma unroll
    for (int r = 0; r < SW_MAXK; ++r) {
        if (r < k) dw[r] = wave_sum(dw[r]);
        dot = __builtin_fmaf(wr[r], dw[r], dot);
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < SW_MAXK; ++r) {
        if (r < k) {
            const float ds = wr[r] * (dw[r] - dot);
            if (lane == r) ds_out[row * k + r] = ds;
            if (dq_t) acc += ds * load_row4(kh, kl, key[r], lane);
        }
    }
    if (dq_t) *reinterpret_cast<f32x4*>(dq_t + row * SW_KD + lane * 4) = acc * grad_scale;
}

// An entry of the inverse table is the flat position p = (b Nq + i) k + r of an idx entry that names the key:
//   dkn^T[j] = inv_t sum ds[p] qn[i],  dv^T[j] = sum w[p] dout^T[i].  dk_t or dv_t may be null.
__global__ __launch_bounds__(ROW_THREADS) void sparse_warp_bwd_key_kernel(const _Float16* __restrict__ qh, const _Float16* __restrict__ ql,
                                                                          const float* __restrict__ dout_t, const float* __restrict__ ds,
                                                                          const float* __restrict__ w, const int* __restrict__ entries,
                                                                          const int* __restrict__ offsets, float* __restrict__ dk_t,
                                                                          float* __restrict__ dv_t, long long keys, int total, int Cv, int k,
                                                                          float grad_scale) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long key = (long long)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);     // b * Nk + j
    if (key >= keys) return;
    const int beg = list_begin(offsets, key, total), end = list_end(offsets, key, total);
    if (dk_t) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int e = beg; e < end; ++e) {
            const int p = list_entry(entries, e, total);
            acc += ds[p] * load_row4(qh, ql, p / k, lane);
        }
        *reinterpret_cast<f32x4*>(dk_t + key * SW_KD + lane * 4) = acc * grad_scale;
    }
    if (dv_t) {
        for (int c0 = 0; c0 < Cv; c0 += 4 * kWave) {          // four channels per lane and walk of the list
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int e = beg; e < end; ++e) {
                const int p = list_entry(entries, e, total);
                const float wp = w[p];
                const float* const g = dout_t + (long long)(p / k) * Cv;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = c0 + u * kWave + lane;
                    if (c < Cv) acc[u] = __builtin_fmaf(wp, g[c], acc[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * kWave + lane;
                if (c < Cv) dv_t[key * Cv + c] = acc[u];
            }
        }
    }
}

// ---- K44 / K46 ----------------------------------------------------------------------------------------------------------------------
// The window of query `row` = b Nq + i, W = 2 R + 1 wide around the centre key idx[row] (clamped into [0, Nk)) at (yk, xk) of the
// hk x wk key grid.  Slot e = (dy + R) W + (dx + R), visited dy ascending outside, dx ascending inside; in[e]: the key
// (yk + dy, xk + dx) lies INSIDE the grid (a position outside is left out: not clamped, not wrapped) — this is the one place that
// decides it; s[e]: K42's logit of the pair, bit for bit (0 where !in[e]); m = max and sum = sum exp(s - m) over the slots inside, in
// visiting order.  The centre is always inside: the window is never empty, and in[a W + R] says whether window row a is.  Every lane
// holds the same score bits; they are read through uniform_f32, so the whole state is wave-uniform.  Non-finite scores are not
// sanitised.  This is what the forward reads out and what the backward differentiates: one definition, the same bits.
template <int R>
struct Window {
    static constexpr int W = 2 * R + 1;
    long long kbase;      // b Nk
    int yk, xk, wk;
    float s[W * W], m, sum;
    bool in[W * W];

    // the row of the key planes that slot (a, c) reads; a column outside the grid names the nearest one inside (the address stays in
    // the buffer; what is read there is not used).  Only for a window row inside the grid
    __device__ __forceinline__ long long key_row(int a, int c) const {
        return kbase + (long long)(yk + a - R) * wk + min(max(xk + c - R, 0), wk - 1);
    }

    __device__ __forceinline__ Window(const _Float16* __restrict__ qh, const _Float16* __restrict__ ql, const _Float16* __restrict__ kh,
                                      const _Float16* __restrict__ kl, const int* __restrict__ idx, int row, int Nq, int hk, int wk_,
                                      float logit_scale, int lane) {
#pragma clang fp contract(off)
        wk = wk_;
        const int Nk = hk * wk;
        kbase = (long long)(row / Nq) * Nk;
        const int j = clamp_key(__builtin_amdgcn_readfirstlane(idx[row]), Nk);
        yk = j / wk, xk = j - yk * wk;
        const f32x4 q = load_row4(qh, ql, row, lane);
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
            // the W rows of this window row first, then their reductions (as K43 batches a source)
            f32x4 kv[W];
#pragma unroll
            for (int c = 0; c < W; ++c) kv[c] = load_row4(kh, kl, key_row(a, c), lane);
#pragma unroll
            for (int c = 0; c < W; ++c) s[a * W + c] = uniform_f32(wave_sum(lane_dot4(q, kv[c])) * logit_scale);
        }
        m = -INFINITY;
#pragma unroll
        for (int e = 0; e < W * W; ++e) m = in[e] ? fmaxf(m, s[e]) : m;
        sum = 0.f;
#pragma unroll
        for (int e = 0; e < W * W; ++e) sum = in[e] ? sum + expf(s[e] - m) : sum;
    }
};

template <int R>
__global__ __launch_bounds__(ROW_THREADS) void match_refine_kernel(const _Float16* __restrict__ qh, const _Float16* __restrict__ ql,
                                                                   const _Float16* __restrict__ kh, const _Float16* __restrict__ kl,
                                                                   const int* __restrict__ idx, float* __restrict__ off,
                                                                   float* __restrict__ lse_win, int rows, int Nq, int hk, int wk,
                                                                   float logit_scale) {
#pragma clang fp contract(off)
    constexpr int W = 2 * R + 1;
    const int lane = threadIdx.x & (kWave - 1);
    const int row = (int)wave_row();                                                  // b * Nq + i
    if (row >= rows) return;                                                          // (whole waves; the kernel has no barrier)
    const Window<R> win(qh, ql, kh, kl, idx, row, Nq, hk, wk, logit_scale, lane);
    const float lse = win.m + logf(win.sum);
    float ox = 0.f, oy = 0.f;
#pragma unroll
    for (int e = 0; e < W * W; ++e) {
        if (win.in[e]) {
            const float p = expf(win.s[e] - lse);
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
__global__ __launch_bounds__(ROW_THREADS) void match_refine_bwd_query_kernel(
    const _Float16* __restrict__ qh, const _Float16* __restrict__ ql, const _Float16* __restrict__ kh, const _Float16* __restrict__ kl,
    const int* __restrict__ idx, const float* __restrict__ doff, float* __restrict__ ds, float* __restrict__ dq_t, int rows, int Nq, int hk,
    int wk, float logit_scale, float grad_scale) {
#pragma clang fp contract(off)
    constexpr int W = 2 * R + 1;
    const int lane = threadIdx.x & (kWave - 1);
    const int row = (int)wave_row();                                                  // b * Nq + i
    if (row >= rows) return;                                                          // (whole waves; the kernel has no barrier)
    const Window<R> win(qh, ql, kh, kl, idx, row, Nq, hk, wk, logit_scale, lane);
    // p = exp(s - m) / sum: exp(s - lse_win) without the rounding of lse_win = m + log(sum), which would move every weight by the same
    // relative half ulp of lse_win (4e-6 at |lse_win| = 100) — the gradient is judged by its own error, not by the forward's bits
    const float inv = 1.0f / win.sum;
    float ox = 0.f, oy = 0.f;
#pragma unroll
    for (int e = 0; e < W * W; ++e) {
        if (win.in[e]) {
            const float p = expf(win.s[e] - win.m) * inv;
            ox = __builtin_fmaf(p, (float)(e % W - R), ox);
            oy = __builtin_fmaf(p, (float)(e / W - R), oy);
        }
    }

    // ds per slot (lane e keeps slot e: W^2 <= 49 < 64) and, row of the window by row, dq
    const float gx = uniform_f32(doff[(long long)row * 2]), gy = uniform_f32(doff[(long long)row * 2 + 1]);
    float mine = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < W; ++a) {
        if (!win.in[a * W + R]) continue;            // wave-uniform: the slots of a window row outside the grid stay 0
        f32x4 kv[W];
        if (dq_t) {
#pragma unroll
            for (int c = 0; c < W; ++c) kv[c] = load_row4(kh, kl, win.key_row(a, c), lane);
        }
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const int e = a * W + c;
            if (!win.in[e]) continue;
            const float p = expf(win.s[e] - win.m) * inv;
            const float d = p * (((float)(c - R) - ox) * gx + ((float)(a - R) - oy) * gy);
            mine = lane == e ? d : mine;
            if (dq_t) acc = fma4(d, kv[c], acc);
        }
    }
    if (lane < W * W) ds[(long long)row * (W * W) + lane] = mine;
    if (dq_t) *reinterpret_cast<f32x4*>(dq_t + (long long)row * SW_KD + lane * 4) = acc * grad_scale;
}

// Key j at (yj, xj) lies in slot (dy, dx) of exactly the queries whose centre is (yj - dy, xj - dx), and the inverse table of the
// clamped centre table (K42's, with k = 1) lists those per centre: an entry is the row b Nq + i of such a query.  A centre all queries
// share is one serial list per neighbouring key.
__global__ __launch_bounds__(ROW_THREADS) void match_refine_bwd_key_kernel(const _Float16* __restrict__ qh, const _Float16* __restrict__ ql,
                                                                           const float* __restrict__ ds, const int* __restrict__ entries,
                                                                           const int* __restrict__ offsets, float* __restrict__ dk_t,
                                                                           int keys, int total, int hk, int wk, int r, float grad_scale) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const int key = (int)wave_row();                                                  // b * Nk + j
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
            for (int e = list_begin(offsets, centre, total), end = list_end(offsets, centre, total); e < end; ++e) {
                const int p = list_entry(entries, e, total);
                acc = fma4(ds[(long long)p * (W * W) + slot], load_row4(qh, ql, p, lane), acc);
            }
        }
    }
    *reinterpret_cast<f32x4*>(dk_t + (long long)key * SW_KD + lane * 4) = acc * grad_scale;      // a key in nobody's window: zeros
}

// in [B,R,C] -> out [B,C,R] through a 32 x 32 LDS tile (row stride 33: both sweeps conflict-free)
__global__ __launch_bounds__(256) void transpose_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int C) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const float* const src = in + (long long)blockIdx.z * R * C;
    float* const dst = out + (long long)blockIdx.z * R * C;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int r = r0 + ty + 8 * u, c = c0 + tx;
        if (r < R && c < C) tile[ty + 8 * u][tx] = src[(long long)r * C + c];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = c0 + ty + 8 * u, r = r0 + tx;
        if (r < R && c < C) dst[(long long)c * R + r] = tile[tx][ty + 8 * u];
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// What the seven entry points require alike (before any HIP call), after their own requirements (topk_check / window_check, in the
// order and the words they always had): the channel count and the 32-bit tables — `state` the entries of the widest table the entry
// point indexes, named by `width` and `noun`, below `limit`.
static int plane_pair_check(const char* name, int B, int K, int Nk, long long state, long long limit, const char* width, const char* noun) {
    COCOS_REQUIRE(K == SW_KD, COCOS_ERR_UNSUPPORTED, "%s: needs K == 256 (got %d)", name, K);
    COCOS_REQUIRE(state < limit && (long long)B * Nk < 0x7fffffffll, COCOS_ERR_UNSUPPORTED,
                  "%s: B Nq%s = %lld %s / B Nk = %lld keys exceed the 32-bit tables", name, width, state, noun, (long long)B * Nk);
    return COCOS_OK;
}

// K42's four entry points: sizes, Cv, the temperature and the scale in one refusal, then k
static int topk_check(const char* name, int B, int K, int Nq, int Nk, int Cv, int k, float inv_temperature, float operand_scale) {
    COCOS_REQUIRE(B >= 1 && Nq >= 1 && Nk >= 1 && Cv >= 1 && operand_scale > 0.f && inv_temperature > 0.f, COCOS_ERR_INVALID,
                  "%s: bad dims B=%d Nq=%d Nk=%d Cv=%d", name, B, Nq, Nk, Cv);
    COCOS_REQUIRE(k >= 1 && k <= COCOS_MATCH_TOPK_MAX && k <= Nk, COCOS_ERR_INVALID, "%s: k=%d: expected 1 <= k <= min(%d, Nk=%d)", name, k,
                  COCOS_MATCH_TOPK_MAX, Nk);
    return plane_pair_check(name, B, K, Nk, (long long)B * Nq * k, 0x7fffffffll, " k", "entries");
}

// K44 / K46: sizes, the key grid, the radius, the temperature and the scale.  `slots`: the entry point indexes ds [B,Nq,W] (K46);
// K44 indexes off [B,Nq,2] through a 32-bit row
static int window_check(const char* name, int B, int K, int Nq, int Nk, int hk, int wk, int radius, float inv_temperature,
                        float operand_scale, bool slots) {
    COCOS_REQUIRE(B >= 1 && Nq >= 1 && Nk >= 1 && hk >= 1 && wk >= 1, COCOS_ERR_INVALID,
                  "%s: non-positive size: B=%d Nq=%d Nk=%d hk=%d wk=%d", name, B, Nq, Nk, hk, wk);
    COCOS_REQUIRE((long long)hk * wk == Nk, COCOS_ERR_INVALID, "%s: hk=%d x wk=%d is not the key grid of Nk=%d keys", name, hk, wk, Nk);
    COCOS_REQUIRE(radius >= 1 && radius <= COCOS_MATCH_REFINE_MAX_RADIUS, COCOS_ERR_INVALID, "%s: radius=%d: expected 1 .. %d", name, radius,
                  COCOS_MATCH_REFINE_MAX_RADIUS);
    COCOS_REQUIRE(operand_scale > 0.f && inv_temperature > 0.f, COCOS_ERR_INVALID, "%s: inv_temperature and operand_scale must be positive",
                  name);
    const long long W = (long long)(2 * radius + 1) * (2 * radius + 1);
    return slots ? plane_pair_check(name, B, K, Nk, (long long)B * Nq * W, 0x7fffffffll, " W", "window slots")
                 : plane_pair_check(name, B, K, Nk, (long long)B * Nq, 0x3ffffff0ll, "", "queries");
}

static unsigned plane_pair_blocks(long long rows) { return (unsigned)((rows + ROW_WAVES - 1) / ROW_WAVES); }

// f(std::integral_constant<int, radius>): the window kernels are compiled per radius
template <class F>
static void for_radius(int radius, F&& f) {
    if (radius == 1) f(std::integral_constant<int, 1>{});
    else if (radius == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 3>{});
}

// the K42 forward, with (K50) or without the bias; bias_batch_stride (floats): Nk, or 0 = one [Nk] row for every sample
template <bool BIAS>
static int sparse_warp_fwd(const char* name, const void* qh, const void* ql, const void* kh, const void* kl, const float* v_t, const int* idx,
                           const float* k_bias, float* out_t, float* w, int B, int K, int Nq, int Nk, int Cv, int k, float inv_temperature,
                           float operand_scale, long long bias_batch_stride, cocos_stream_t stream) {
    COCOS_REQUIRE(qh && ql && kh && kl && v_t && idx && (!BIAS || k_bias) && out_t && w, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (const int rc = topk_check(name, B, K, Nq, Nk, Cv, k, inv_temperature, operand_scale)) return rc;
    COCOS_REQUIRE(!BIAS || bias_batch_stride == 0 || bias_batch_stride == (long long)Nk, COCOS_ERR_INVALID,
                  "%s: bias_batch_stride %lld: expected 0 (one bias row for all samples) or the dense %d", name, bias_batch_stride, Nk);
    for (const void* p : {qh, ql, kh, kl})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: q/k planes must be 16-byte aligned", name);
    COCOS_REQUIRE(!BIAS || (reinterpret_cast<uintptr_t>(k_bias) & 3) == 0, COCOS_ERR_INVALID, "%s: the bias must be 4-byte aligned", name);
    const long long rows = (long long)B * Nq;
    hipLaunchKernelGGL(sparse_warp_fwd_kernel<BIAS>, dim3(plane_pair_blocks(rows)), dim3(ROW_THREADS), 0, as_stream(stream),
                       (const _Float16*)qh, (const _Float16*)ql, (const _Float16*)kh, (const _Float16*)kl, v_t, idx, out_t, w, rows, Nq, Nk,
                       Cv, k, inv_temperature / (operand_scale * operand_scale), k_bias, bias_batch_stride);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

}  // namespace cocos

extern "C" int cocos_sparse_softmax_warp_fwd_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const float* v_t,
                                                   const int* idx, float* out_t, float* w, int B, int K, int Nq, int Nk, int Cv, int k,
                                                   float inv_temperature, float operand_scale, cocos_stream_t stream) {
    return cocos::sparse_warp_fwd<false>("sparse_softmax_warp_fwd_f16x3", qh, ql, kh, kl, v_t, idx, nullptr, out_t, w, B, K, Nq, Nk, Cv, k,
                                         inv_temperature, operand_scale, 0, stream);
}

extern "C" int cocos_sparse_softmax_warp_bias_fwd_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const float* v_t,
                                                        const int* idx, const float* k_bias, float* out_t, float* w, int B, int K, int Nq,
                                                        int Nk, int Cv, int k, float inv_temperature, float operand_scale,
                                                        long long bias_batch_stride, cocos_stream_t stream) {
    return cocos::sparse_warp_fwd<true>("sparse_softmax_warp_bias_fwd_f16x3", qh, ql, kh, kl, v_t, idx, k_bias, out_t, w, B, K, Nq, Nk, Cv, k,
                                        inv_temperature, operand_scale, bias_batch_stride, stream);
}

extern "C" int cocos_sparse_softmax_warp_bwd_query_f16x3(const void* kh, const void* kl, const float* v_t, const float* dout_t,
                                                         const int* idx, const float* w, float* ds, float* dq_t, int B, int K, int Nq,
                                                         int Nk, int Cv, int k, float inv_temperature, float operand_scale,
                                                         cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "sparse_softmax_warp_bwd_query_f16x3";
    COCOS_REQUIRE(kh && kl && v_t && dout_t && idx && w && ds, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (const int rc = topk_check(name, B, K, Nq, Nk, Cv, k, inv_temperature, operand_scale)) return rc;
    for (const void* p : {kh, kl, (const void*)dq_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the key planes and dq_t must be 16-byte aligned", name);
    const long long rows = (long long)B * Nq;
    hipLaunchKernelGGL(sparse_warp_bwd_query_kernel, dim3(plane_pair_blocks(rows)), dim3(ROW_THREADS), 0, as_stream(stream),
                       (const _Float16*)kh, (const _Float16*)kl, v_t, dout_t, idx, w, ds, dq_t, rows, Nq, Nk, Cv, k,
                       inv_temperature / operand_scale);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_sparse_softmax_warp_bwd_key_f16x3(const void* qh, const void* ql, const float* dout_t, const float* ds, const float* w,
                                                       const int* entries, const int* offsets, float* dk_t, float* dv_t, int B, int K,
                                                       int Nq, int Nk, int Cv, int k, float inv_temperature, float operand_scale,
                                                       cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "sparse_softmax_warp_bwd_key_f16x3";
    COCOS_REQUIRE(dout_t && w && entries && offsets && (dk_t || dv_t), COCOS_ERR_INVALID, "%s: null pointer", name);
    COCOS_REQUIRE(!dk_t || (qh && ql && ds), COCOS_ERR_INVALID, "%s: null pointer (dk_t needs the query planes and ds)", name);
    if (const int rc = topk_check(name, B, K, Nq, Nk, Cv, k, inv_temperature, operand_scale)) return rc;
    for (const void* p : {qh, ql, (const void*)dk_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the query planes and dk_t must be 16-byte aligned", name);
    const long long keys = (long long)B * Nk;
    hipLaunchKernelGGL(sparse_warp_bwd_key_kernel, dim3(plane_pair_blocks(keys)), dim3(ROW_THREADS), 0, as_stream(stream),
                       (const _Float16*)qh, (const _Float16*)ql, dout_t, ds, w, entries, offsets, dk_t, dv_t, keys, B * Nq * k, Cv, k,
                       inv_temperature / operand_scale);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_match_refine_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const int* idx, float* off,
                                        float* lse_win, int B, int K, int Nq, int Nk, int hk, int wk, int radius, float inv_temperature,
                                        float operand_scale, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "match_refine_f16x3";
    COCOS_REQUIRE(qh && ql && kh && kl && idx && off && lse_win, COCOS_ERR_INVALID, "%s: null pointer (qh, ql, kh, kl, idx, off, lse_win)", name);
    if (const int rc = window_check(name, B, K, Nq, Nk, hk, wk, radius, inv_temperature, operand_scale, false)) return rc;
    for (const void* p : {qh, ql, kh, kl})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: q/k planes must be 16-byte aligned", name);
    const int rows = B * Nq;
    for_radius(radius, [&](auto R) {
        hipLaunchKernelGGL(match_refine_kernel<decltype(R)::value>, dim3(plane_pair_blocks(rows)), dim3(ROW_THREADS), 0, as_stream(stream),
                           (const _Float16*)qh, (const _Float16*)ql, (const _Float16*)kh, (const _Float16*)kl, idx, off, lse_win, rows, Nq,
                           hk, wk, inv_temperature / (operand_scale * operand_scale));
    });
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_match_refine_bwd_query_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const int* idx,
                                                  const float* doff, float* ds, float* dq_t, int B, int K, int Nq, int Nk, int hk, int wk,
                                                  int radius, float inv_temperature, float operand_scale, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "match_refine_bwd_query_f16x3";
    COCOS_REQUIRE(qh && ql && kh && kl && idx && doff && ds, COCOS_ERR_INVALID, "%s: null pointer (qh, ql, kh, kl, idx, doff, ds)", name);
    if (const int rc = window_check(name, B, K, Nq, Nk, hk, wk, radius, inv_temperature, operand_scale, true)) return rc;
    for (const void* p : {qh, ql, kh, kl, (const void*)dq_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the q/k planes and dq_t must be 16-byte aligned", name);
    const int rows = B * Nq;
    for_radius(radius, [&](auto R) {
        hipLaunchKernelGGL(match_refine_bwd_query_kernel<decltype(R)::value>, dim3(plane_pair_blocks(rows)), dim3(ROW_THREADS), 0,
                           as_stream(stream), (const _Float16*)qh, (const _Float16*)ql, (const _Float16*)kh, (const _Float16*)kl, idx, doff,
                           ds, dq_t, rows, Nq, hk, wk, inv_temperature / (operand_scale * operand_scale), inv_temperature / operand_scale);
    });
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_match_refine_bwd_key_f16x3(const void* qh, const void* ql, const float* ds, const int* entries, const int* offsets,
                                                float* dk_t, int B, int K, int Nq, int Nk, int hk, int wk, int radius, float inv_temperature,
                                                float operand_scale, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "match_refine_bwd_key_f16x3";
    COCOS_REQUIRE(qh && ql && ds && entries && offsets && dk_t, COCOS_ERR_INVALID, "%s: null pointer (qh, ql, ds, entries, offsets, dk_t)", name);
    if (const int rc = window_check(name, B, K, Nq, Nk, hk, wk, radius, inv_temperature, operand_scale, true)) return rc;
    for (const void* p : {qh, ql, (const void*)dk_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the query planes and dk_t must be 16-byte aligned", name);
    const int keys = B * Nk;
    hipLaunchKernelGGL(match_refine_bwd_key_kernel, dim3(plane_pair_blocks(keys)), dim3(ROW_THREADS), 0, as_stream(stream),
                       (const _Float16*)qh, (const _Float16*)ql, ds, entries, offsets, dk_t, keys, B * Nq, hk, wk, radius,
                       inv_temperature / operand_scale);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_transpose_f32(const float* in, float* out, int B, int R, int C, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(in && out, COCOS_ERR_INVALID, "transpose_f32: null pointer");
    COCOS_REQUIRE(B >= 1 && R >= 1 && C >= 1, COCOS_ERR_INVALID, "transpose_f32: bad dims B=%d R=%d C=%d", B, R, C);
    COCOS_REQUIRE(B <= 65535 && (R + 31) / 32 <= 65535, COCOS_ERR_UNSUPPORTED, "transpose_f32: B=%d R=%d exceed the launch grid", B, R);
    hipLaunchKernelGGL(transpose_f32_kernel, dim3((C + 31) / 32, (R + 31) / 32, B), dim3(256), 0, as_stream(stream), in, out, R, C);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
