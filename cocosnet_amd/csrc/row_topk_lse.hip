// K36b / K39b: per row of a materialised logit matrix [rows][Nk] its k largest elements, their indices (logit descending, the lower
// index first among equals) and the row log-sum-exp, in ONE sweep — what the caller of forward(return_corr=True) gets from torch.max
// or torch.topk plus torch.logsumexp (correspondence.py:304-307) in further sweeps of the matrix.  One kernel template, K = 1, 2, 4, 8
// candidates per lane: K = 1 is cocos_row_argmax_lse, the same instantiation serves cocos_row_topk_lse at k = 1.
//
// One wave per row, four rows per workgroup, 16-byte steps when Nk % 4 == 0 and the base is aligned, dword by dword otherwise.  A lane
// keeps a sorted list of K candidates (topk_list.h; its head is the running maximum m of the online log-sum-exp) and meets its
// elements in ascending index.  The 64 lists are merged by a butterfly of six (value, index) merges (exact: compare / select only);
// the sums are brought to the row maximum with ONE rescale per lane and added in the same butterfly order for every K.
#include "common.h"
#include "topk_list.h"

namespace cocos {

constexpr int RT_ROWS = 4;      // waves (= rows) per workgroup

template <int K, bool VEC>
__global__ __launch_bounds__(RT_ROWS * 64) void row_topk_lse_kernel(const float* __restrict__ logits, int* __restrict__ idx_out,
                                                                    float* __restrict__ val_out, float* __restrict__ lse_out,
                                                                    long long rows, int Nk, int k_out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * RT_ROWS + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // (whole waves: no barrier below)
    const float* __restrict__ x = logits + (size_t)row * Nk;
    TopkList<K> best;
    best.clear();
    float mref = 0.f, l = 0.f;                                 // mref: the finite reference of l (the head once an element was seen)
    auto rescale = [&](float cand) {                           // the reference moves up to max(m, cand) before new terms are added
        const float m = best.head();
        if (cand > m) {
            l *= m == -INFINITY ? 0.f : __expf(m - cand);
            mref = cand;
        }
    };
    auto offer = [&](float v, int j) {
        if (v > best.tail()) best.push_ascending(v, j);        // strictly: ascending j keeps the lower index among equals in front
    };
    if (VEC) {
        for (int j = lane * 4; j < Nk; j += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + j);
            const float m4 = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
            rescale(m4);
            if (K == 1 || m4 > best.tail()) {                  // (one slot: four compare / selects cost less than the branch, 1 % of the sweep)
                offer(v.x, j);
                offer(v.y, j + 1);
                offer(v.z, j + 2);
                offer(v.w, j + 3);
            }
            l += (__expf(v.x - mref) + __expf(v.y - mref)) + (__expf(v.z - mref) + __expf(v.w - mref));
        }
    } else {
        for (int j = lane; j < Nk; j += 64) {
            const float v = x[j];
            rescale(v);
            offer(v, j);
            l += __expf(v - mref);
        }
    }
    // ---- merge: the row's K candidates (exact: compare / select only), then every lane's sum brought to the row maximum once --
    const float m = best.head();
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) best.merge(best.from_lane_xor(d));
    const float M = best.head();
    float s = m == -INFINITY ? 0.f : l * __expf(mref - M);     // (a lane that saw nothing, or only -inf, contributes nothing)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) {
#pragma unroll
        for (int p = 0; p < K; ++p) {
            if (p < k_out) {
                idx_out[row * k_out + p] = min(max(best.i[p], 0), Nk - 1);     // a valid position also for non-finite rows
                val_out[row * k_out + p] = best.v[p];
            }
        }
        lse_out[row] = (float)((double)M + log((double)s));    // one rounding
    }
}

template <int K>
static int launch_row_topk(const float* logits, int* idx, float* val, float* lse, long long rows, int Nk, int k, cocos_stream_t stream) {
    const unsigned blocks = (unsigned)((rows + RT_ROWS - 1) / RT_ROWS);
    if (Nk % 4 == 0 && aligned16(logits))
        hipLaunchKernelGGL((row_topk_lse_kernel<K, true>), dim3(blocks), dim3(RT_ROWS * 64), 0, as_stream(stream), logits, idx, val, lse,
                           rows, Nk, k);
    else
        hipLaunchKernelGGL((row_topk_lse_kernel<K, false>), dim3(blocks), dim3(RT_ROWS * 64), 0, as_stream(stream), logits, idx, val, lse,
                           rows, Nk, k);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

// what both entry points ask of their arguments; `name` is the entry's prefix in the messages
static int check_row_readout(const char* name, const void* logits, const void* idx, const void* val, const void* lse, int B, int Nq, int Nk,
                             int k) {
    COCOS_REQUIRE(logits && idx && val && lse, COCOS_ERR_INVALID, "%s: null pointer", name);
    COCOS_REQUIRE(B >= 1 && Nq >= 1 && Nk >= 1, COCOS_ERR_INVALID, "%s: bad dims B=%d Nq=%d Nk=%d", name, B, Nq, Nk);
    COCOS_REQUIRE(k >= 1 && k <= COCOS_MATCH_TOPK_MAX && k <= Nk, COCOS_ERR_INVALID, "%s: k=%d: expected 1 <= k <= min(%d, Nk=%d)", name, k,
                  COCOS_MATCH_TOPK_MAX, Nk);
    COCOS_REQUIRE(((long long)B * Nq + RT_ROWS - 1) / RT_ROWS < 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "%s: %lld rows", name, (long long)B * Nq);
    return COCOS_OK;
}

}  // namespace cocos

// idx / max [B,Nq] is the same memory as the [B,Nq,1] of the K = 1 instantiation
extern "C" int cocos_row_argmax_lse(const float* logits, int* idx, float* max, float* lse, int B, int Nq, int Nk,
                                    cocos_stream_t stream) {
    using namespace cocos;
    if (const int rc = check_row_readout("row_argmax_lse", logits, idx, max, lse, B, Nq, Nk, 1)) return rc;
    return launch_row_topk<1>(logits, idx, max, lse, (long long)B * Nq, Nk, 1, stream);
}

extern "C" int cocos_row_topk_lse(const float* logits, int* idx, float* val, float* lse, int B, int Nq, int Nk, int k,
                                  cocos_stream_t stream) {
    using namespace cocos;
    if (const int rc = check_row_readout("row_topk_lse", logits, idx, val, lse, B, Nq, Nk, k)) return rc;
    const long long rows = (long long)B * Nq;
    if (k == 1) return launch_row_topk<1>(logits, idx, val, lse, rows, Nk, k, stream);
    if (k == 2) return launch_row_topk<2>(logits, idx, val, lse, rows, Nk, k, stream);
    if (k <= 4) return launch_row_topk<4>(logits, idx, val, lse, rows, Nk, k, stream);
    return launch_row_topk<8>(logits, idx, val, lse, rows, Nk, k, stream);
}
