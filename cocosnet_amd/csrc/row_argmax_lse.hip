// K36b: per row of a materialised logit matrix [rows][Nk] its maximum, the (lowest) index of the maximum and the row
// log-sum-exp, in ONE sweep — what the caller of forward(return_corr=True) gets from torch.max plus torch.logsumexp
// (correspondence.py:304-307) in three more sweeps of the matrix.
//
// One wave per row, four rows per workgroup.  A lane walks the row in 16-byte steps (Nk % 4 == 0 and an aligned base; else
// dword by dword) with an online (maximum, index, sum of exp) state; the 64 states are merged once at the end: the maximum
// and its index exactly (compare / select only), the sums after ONE rescale per lane to the row maximum.
#include "common.h"

namespace cocos {

constexpr int RA_ROWS = 4;      // waves (= rows) per workgroup

__device__ __forceinline__ void ral_take(float v, int j, float& m, int& idx) {
    if (v > m) { m = v; idx = j; }            // strictly: ascending j keeps the lowest index among equals; a NaN never wins
}

template <bool VEC>
__global__ __launch_bounds__(RA_ROWS * 64) void row_argmax_lse_kernel(const float* __restrict__ logits, int* __restrict__ idx_out,
                                                                      float* __restrict__ max_out, float* __restrict__ lse_out,
                                                                      long long rows, int Nk) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * RA_ROWS + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // (whole waves: no barrier below)
    const float* __restrict__ x = logits + (size_t)row * Nk;
    float m = -INFINITY, mref = 0.f, l = 0.f;                  // mref: the finite reference of l (m once an element was seen)
    int idx = 0;
    auto rescale = [&](float cand) {                           // the reference moves up to max(m, cand) before new terms are added
        if (cand > m) {
            l *= m == -INFINITY ? 0.f : __expf(m - cand);
            mref = cand;
        }
    };
    if (VEC) {
        for (int j = lane * 4; j < Nk; j += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + j);
            const float m4 = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
            rescale(m4);
            ral_take(v.x, j, m, idx);
            ral_take(v.y, j + 1, m, idx);
            ral_take(v.z, j + 2, m, idx);
            ral_take(v.w, j + 3, m, idx);
            l += (__expf(v.x - mref) + __expf(v.y - mref)) + (__expf(v.z - mref) + __expf(v.w - mref));
        }
    } else {
        for (int j = lane; j < Nk; j += 64) {
            const float v = x[j];
            rescale(v);
            ral_take(v, j, m, idx);
            l += __expf(v - mref);
        }
    }
    // ---- merge: the row maximum and its lowest index (exact), then every lane's sum brought to it once ----------------------
    float M = m;
    int I = idx;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float om = __shfl_xor(M, d, 64);
        const int oi = __shfl_xor(I, d, 64);
        const bool take = om > M || (om == M && oi < I);
        M = take ? om : M;
        I = take ? oi : I;
    }
    float s = m == -INFINITY ? 0.f : l * __expf(mref - M);     // (a lane that saw nothing, or only -inf, contributes nothing)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) {
        idx_out[row] = min(max(I, 0), Nk - 1);                 // a valid position also for non-finite rows
        max_out[row] = M;
        lse_out[row] = (float)((double)M + log((double)s));    // one rounding
    }
}

}  // namespace cocos

extern "C" int cocos_row_argmax_lse(const float* logits, int* idx, float* max, float* lse, int B, int Nq, int Nk,
                                    cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(logits && idx && max && lse, COCOS_ERR_INVALID, "row_argmax_lse: null pointer");
    COCOS_REQUIRE(B >= 1 && Nq >= 1 && Nk >= 1, COCOS_ERR_INVALID, "row_argmax_lse: bad dims B=%d Nq=%d Nk=%d", B, Nq, Nk);
    const long long rows = (long long)B * Nq;
    const long long blocks = (rows + RA_ROWS - 1) / RA_ROWS;
    COCOS_REQUIRE(blocks < 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "row_argmax_lse: %lld rows", rows);
    const bool vec = Nk % 4 == 0 && aligned16(logits);
    if (vec)
        hipLaunchKernelGGL(row_argmax_lse_kernel<true>, dim3((unsigned)blocks), dim3(RA_ROWS * 64), 0, as_stream(stream), logits, idx,
                           max, lse, rows, Nk);
    else
        hipLaunchKernelGGL(row_argmax_lse_kernel<false>, dim3((unsigned)blocks), dim3(RA_ROWS * 64), 0, as_stream(stream), logits, idx,
                           max, lse, rows, Nk);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
