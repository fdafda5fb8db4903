// K39: the sorted candidate list of the top-k match readout (corr_topk_f16x3.hip, row_topk_lse.hip).
//
// A list is K (value, index) pairs in registers, ordered by value descending and, among bitwise-equal values, by index ascending —
// the order the readout returns.  Empty slots are (-inf, 0).  Every loop below is fully unrolled: the arrays never leave registers.
#pragma once
#include "common.h"

namespace cocos {

// (v, i) goes before (w, j) in the returned order
__device__ __forceinline__ bool topk_before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

template <int K>
struct TopkList {
    float v[K];
    int i[K];

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int p = 0; p < K; ++p) { v[p] = -INFINITY; i[p] = 0; }
    }
    __device__ __forceinline__ float head() const { return v[0]; }
    __device__ __forceinline__ float tail() const { return v[K - 1]; }

    // Insert a key that comes AFTER every key already seen by this list in index order: a strict compare on the value alone then
    // keeps the lower index among equals in front.  A NaN and a -inf (a padded key) never enter.
    __device__ __forceinline__ void push_ascending(float x, int j) {
#pragma unroll
        for (int p = K - 1; p >= 1; --p) {
            const bool up = x > v[p - 1], here = x > v[p];
            v[p] = up ? v[p - 1] : (here ? x : v[p]);
            i[p] = up ? i[p - 1] : (here ? j : i[p]);
        }
        const bool first = x > v[0];
        v[0] = first ? x : v[0];
        i[0] = first ? j : i[0];
    }

    // this <- the K first of (this U o) in the returned order.  max(a[p], b[K-1-p]) over two sorted lists is a bitonic sequence
    // that holds exactly those K; log2 K half-cleaner stages sort it.  Compare / select only: values and indices pass through unchanged.
    __device__ __forceinline__ void merge(const TopkList& o) {
#pragma unroll
        for (int p = 0; p < K; ++p) {
            const bool take = topk_before(o.v[K - 1 - p], o.i[K - 1 - p], v[p], i[p]);
            v[p] = take ? o.v[K - 1 - p] : v[p];
            i[p] = take ? o.i[K - 1 - p] : i[p];
        }
#pragma unroll
        for (int s = K / 2; s >= 1; s >>= 1) {
#pragma unroll
            for (int p = 0; p < K; ++p) {
                if ((p & s) == 0) {
                    const bool swap = topk_before(v[p + s], i[p + s], v[p], i[p]);
                    const float tv = v[p];
                    const int ti = i[p];
                    v[p] = swap ? v[p + s] : tv;
                    i[p] = swap ? i[p + s] : ti;
                    v[p + s] = swap ? tv : v[p + s];
                    i[p + s] = swap ? ti : i[p + s];
                }
            }
        }
    }

    // the list of lane ^ d (executed by every lane of the wave)
    __device__ __forceinline__ TopkList from_lane_xor(int d) const {
        TopkList o;
#pragma unroll
        for (int p = 0; p < K; ++p) {
            o.v[p] = __shfl_xor(v[p], d, 64);
            o.i[p] = __shfl_xor(i[p], d, 64);
        }
        return o;
    }
};

}  // namespace cocos
