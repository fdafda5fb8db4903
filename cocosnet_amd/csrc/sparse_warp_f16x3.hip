// K42: the k-sparse correspondence warp with gradients — attention over the k keys per query that the match readout (K39a) selected,
//   s[b,i,r] = inv_temperature <qn[b,:,i], kn[b,:,j_r]>,  j_r = idx[b,i,r] (clamped into [0, Nk)),  w = softmax_r s,
//   out[b,:,i] = sum_r w[b,i,r] v[b,:,j_r]
// and its three gradients.  Nothing here has an Nq x Nk extent: the state is idx, w and ds, each [B,Nq,k].
//
// Operands are the position-major f16 hi/lo planes [B,N,256] of unit-norm columns x operand_scale that K39a chose the candidates from
// (value = (hi + lo) / operand_scale: split_f16.hip), read as whole 512-byte rows: lane l of a wave holds channels 4 l .. 4 l + 3.  Dot
// products are fp32 FMAs per lane and a butterfly over the 64 lanes (every lane ends with the same sum: fixed order, no atomics).
// Every tensor a wave gathers rows from is position-major ([B,N,C]: v^T, dout^T), and so is everything it writes (out^T, dqn^T, dkn^T,
// dv^T): one contiguous row per wave.  The channel-major tensors of the public op are made from / turned into these by
// cocos_transpose_f32 below, once per tensor and call (C N elements each), never per query.
//
//   forward          one wave per query: k dot products, softmax over k in registers, out^T row, w
//   query backward   one wave per query: dw_r = <dout^T[i], v^T[j_r]>, ds_r = w_r (dw_r - sum w dw), dqn^T[i] = inv_t sum_r ds_r kn[j_r]
//   key backward     one wave per key, a GATHER over the inverse table of idx (per key the entries (i, r) that name it, ascending):
//                    dkn^T[j] = inv_t sum ds qn[i],  dv^T[j] = sum w dout^T[i], summed serially in table order — bitwise reproducible;
//                    a key nobody names gets zeros from this kernel.  A key every query names is a serial list of Nq entries.
#include "sparse_row.h"      // wave_sum, load_row4, lane_dot4, clamp_key: shared with K43 (patchmatch_f16x3.hip)

namespace cocos {

constexpr int SW_WAVES = 4;              // rows (queries or keys) per workgroup, one per wave
constexpr int SW_THREADS = SW_WAVES * kWave;
constexpr int SW_MAXK = COCOS_MATCH_TOPK_MAX;

// BIAS (K50, cocos_sparse_softmax_warp_bias_fwd_f16x3): s_r += k_bias[b, j_r] before the softmax over r — the row-conditional
// transport plan softmax_j(s_ij + g_j) restricted to the k candidates.  k_bias [B,Nk] fp32, or one [Nk] row when bias_bstride is 0;
// finite or -inf.  A row whose k candidates all carry -inf has no largest logit to refer to: its w is the uniform 1 / k.  The bias is a
// constant of the backward, which consumes the saved w.  Without BIAS the pointer is not read and the code is the K42 forward's.
template <bool BIAS>
__global__ __launch_bounds__(SW_THREADS) void sparse_warp_fwd_kernel(const _Float16* __restrict__ qh, const _Float16* __restrict__ ql,
                                                                     const _Float16* __restrict__ kh, const _Float16* __restrict__ kl,
                                                                     const float* __restrict__ vt, const int* __restrict__ idx,
                                                                     float* __restrict__ out_t, float* __restrict__ w_out,
                                                                     long long rows, int Nq, int Nk, int Cv, int k, float logit_scale,
                                                                     const float* __restrict__ k_bias = nullptr, long long bias_bstride = 0) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * SW_WAVES + (threadIdx.x >> 6);      // b * Nq + i
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

__global__ __launch_bounds__(SW_THREADS) void sparse_warp_bwd_query_kernel(const _Float16* __restrict__ kh, const _Float16* __restrict__ kl,
                                                                           const float* __restrict__ vt, const float* __restrict__ dout_t,
                                                                           const int* __restrict__ idx, const float* __restrict__ w,
                                                                           float* __restrict__ ds_out, float* __restrict__ dq_t,
                                                                           long long rows, int Nq, int Nk, int Cv, int k, float grad_scale) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * SW_WAVES + (threadIdx.x >> 6);
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

// entries[offsets[key] .. offsets[key + 1]) are the flat positions p = (b Nq + i) k + r of the idx entries that name `key` = b Nk + j,
// ascending.  Positions and ranges are clamped into the tables: a malformed table cannot send a read outside ds / w / the planes.
__global__ __launch_bounds__(SW_THREADS) void sparse_warp_bwd_key_kernel(const _Float16* __restrict__ qh, const _Float16* __restrict__ ql,
                                                                         const float* __restrict__ dout_t, const float* __restrict__ ds,
                                                                         const float* __restrict__ w, const int* __restrict__ entries,
                                                                         const int* __restrict__ offsets, float* __restrict__ dk_t,
                                                                         float* __restrict__ dv_t, long long keys, int total, int Cv, int k,
                                                                         float grad_scale) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long key = (long long)blockIdx.x * SW_WAVES + (threadIdx.x >> 6);
    if (key >= keys) return;
    const int beg = min(max(offsets[key], 0), total), end = min(max(offsets[key + 1], beg), total);
    if (dk_t) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int e = beg; e < end; ++e) {
            const int p = min(max(entries[e], 0), total - 1);
            acc += ds[p] * load_row4(qh, ql, p / k, lane);
        }
        *reinterpret_cast<f32x4*>(dk_t + key * SW_KD + lane * 4) = acc * grad_scale;
    }
    if (dv_t) {
        for (int c0 = 0; c0 < Cv; c0 += 4 * kWave) {          // four channels per lane and walk of the list
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int e = beg; e < end; ++e) {
                const int p = min(max(entries[e], 0), total - 1);
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

static int sparse_warp_check(const char* name, int B, int K, int Nq, int Nk, int Cv, int k, float inv_temperature, float operand_scale) {
    COCOS_REQUIRE(B >= 1 && Nq >= 1 && Nk >= 1 && Cv >= 1 && operand_scale > 0.f && inv_temperature > 0.f, COCOS_ERR_INVALID,
                  "%s: bad dims B=%d Nq=%d Nk=%d Cv=%d", name, B, Nq, Nk, Cv);
    COCOS_REQUIRE(k >= 1 && k <= COCOS_MATCH_TOPK_MAX && k <= Nk, COCOS_ERR_INVALID, "%s: k=%d: expected 1 <= k <= min(%d, Nk=%d)", name, k,
                  COCOS_MATCH_TOPK_MAX, Nk);
    COCOS_REQUIRE(K == SW_KD, COCOS_ERR_UNSUPPORTED, "%s: needs K == 256 (got %d)", name, K);
    COCOS_REQUIRE((long long)B * Nq * k < 0x7fffffffll && (long long)B * Nk < 0x7fffffffll, COCOS_ERR_UNSUPPORTED,
                  "%s: B Nq k = %lld entries / B Nk = %lld keys exceed the 32-bit tables", name, (long long)B * Nq * k, (long long)B * Nk);
    return COCOS_OK;
}

static unsigned sparse_warp_blocks(long long rows) { return (unsigned)((rows + SW_WAVES - 1) / SW_WAVES); }

}  // namespace cocos

extern "C" int cocos_sparse_softmax_warp_fwd_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const float* v_t,
                                                   const int* idx, float* out_t, float* w, int B, int K, int Nq, int Nk, int Cv, int k,
                                                   float inv_temperature, float operand_scale, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "sparse_softmax_warp_fwd_f16x3";
    COCOS_REQUIRE(qh && ql && kh && kl && v_t && idx && out_t && w, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (int rc = sparse_warp_check(name, B, K, Nq, Nk, Cv, k, inv_temperature, operand_scale)) return rc;
    for (const void* p : {qh, ql, kh, kl})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: q/k planes must be 16-byte aligned", name);
    const long long rows = (long long)B * Nq;
    hipLaunchKernelGGL(sparse_warp_fwd_kernel<false>, dim3(sparse_warp_blocks(rows)), dim3(SW_THREADS), 0, as_stream(stream),
                       (const _Float16*)qh, (const _Float16*)ql, (const _Float16*)kh, (const _Float16*)kl, v_t, idx, out_t, w, rows, Nq, Nk,
                       Cv, k, inv_temperature / (operand_scale * operand_scale), (const float*)nullptr, 0ll);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

// K50: the same forward with s_r += k_bias[b, j_r]; bias_batch_stride (floats): Nk, or 0 = one [Nk] row for every sample
extern "C" int cocos_sparse_softmax_warp_bias_fwd_f16x3(const void* qh, const void* ql, const void* kh, const void* kl, const float* v_t,
                                                        const int* idx, const float* k_bias, float* out_t, float* w, int B, int K, int Nq,
                                                        int Nk, int Cv, int k, float inv_temperature, float operand_scale,
                                                        long long bias_batch_stride, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "sparse_softmax_warp_bias_fwd_f16x3";
    COCOS_REQUIRE(qh && ql && kh && kl && v_t && idx && k_bias && out_t && w, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (int rc = sparse_warp_check(name, B, K, Nq, Nk, Cv, k, inv_temperature, operand_scale)) return rc;
    COCOS_REQUIRE(bias_batch_stride == 0 || bias_batch_stride == (long long)Nk, COCOS_ERR_INVALID,
                  "%s: bias_batch_stride %lld: expected 0 (one bias row for all samples) or the dense %d", name, bias_batch_stride, Nk);
    for (const void* p : {qh, ql, kh, kl})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: q/k planes must be 16-byte aligned", name);
    COCOS_REQUIRE((reinterpret_cast<uintptr_t>(k_bias) & 3) == 0, COCOS_ERR_INVALID, "%s: the bias must be 4-byte aligned", name);
    const long long rows = (long long)B * Nq;
    hipLaunchKernelGGL(sparse_warp_fwd_kernel<true>, dim3(sparse_warp_blocks(rows)), dim3(SW_THREADS), 0, as_stream(stream),
                       (const _Float16*)qh, (const _Float16*)ql, (const _Float16*)kh, (const _Float16*)kl, v_t, idx, out_t, w, rows, Nq, Nk,
                       Cv, k, inv_temperature / (operand_scale * operand_scale), k_bias, bias_batch_stride);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_sparse_softmax_warp_bwd_query_f16x3(const void* kh, const void* kl, const float* v_t, const float* dout_t,
                                                         const int* idx, const float* w, float* ds, float* dq_t, int B, int K, int Nq,
                                                         int Nk, int Cv, int k, float inv_temperature, float operand_scale,
                                                         cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "sparse_softmax_warp_bwd_query_f16x3";
    COCOS_REQUIRE(kh && kl && v_t && dout_t && idx && w && ds, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (int rc = sparse_warp_check(name, B, K, Nq, Nk, Cv, k, inv_temperature, operand_scale)) return rc;
    for (const void* p : {kh, kl, (const void*)dq_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the key planes and dq_t must be 16-byte aligned", name);
    const long long rows = (long long)B * Nq;
    hipLaunchKernelGGL(sparse_warp_bwd_query_kernel, dim3(sparse_warp_blocks(rows)), dim3(SW_THREADS), 0, as_stream(stream),
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
    if (int rc = sparse_warp_check(name, B, K, Nq, Nk, Cv, k, inv_temperature, operand_scale)) return rc;
    for (const void* p : {qh, ql, (const void*)dk_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the query planes and dk_t must be 16-byte aligned", name);
    const long long keys = (long long)B * Nk;
    hipLaunchKernelGGL(sparse_warp_bwd_key_kernel, dim3(sparse_warp_blocks(keys)), dim3(SW_THREADS), 0, as_stream(stream),
                       (const _Float16*)qh, (const _Float16*)ql, dout_t, ds, w, entries, offsets, dk_t, dv_t, keys, B * Nq * k, Cv, k,
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
