// The pair core of the match_kernel-3 sparse kernels (box3_pair.hip: K51, K52): what forms, or differentiates, the logit of ONE
// (query, key) pair on fp32 position-major rows [B,N,256].  A wave reads one 1 KiB row, lane l holds channels 4 l .. 4 l + 3.
// K52's kernels are compiled with contraction off, K51's with it on, and a helper has the regime of its own definition: the helpers
// hold explicit fused multiply-adds, plain multiplies, plain adds and shuffles only; x * y + z stays in the kernel that owns it.
// What knows nothing of taps or statistics (the wave's row, the lane exchanges, in_grid, fma4, the inverse-table walk) is sparse_row.h's.
#pragma once
#include "sparse_row.h"

namespace cocos {

constexpr int BOX3_ROW_C = 256;          // channels of theta / phi
constexpr int BOX3_WAVES = ROW_WAVES;    // rows (queries, content positions or keys) per workgroup, one per wave: wave_row()'s
constexpr int BOX3_THREADS = ROW_THREADS;

__device__ __forceinline__ f32x4 row4(const float* __restrict__ t, long long row, int lane) {
    return *reinterpret_cast<const f32x4*>(t + row * BOX3_ROW_C + lane * 4);
}

// acc + this lane's share of <q, kv>, in the order every R is formed in
__device__ __forceinline__ float lane_fma4(const f32x4& q, const f32x4& kv, float acc) {
    return __builtin_fmaf(q[3], kv[3], __builtin_fmaf(q[2], kv[2], __builtin_fmaf(q[1], kv[1], __builtin_fmaf(q[0], kv[0], acc))));
}

// the (up to) nine neighbour rows of query (py, px), row `row` of th_t; bit t of mask: tap t lies inside the content grid
struct QueryTaps {
    f32x4 q[9];
    unsigned mask;
};

__device__ __forceinline__ QueryTaps load_query_taps(const float* __restrict__ th_t, long long row, int py, int px, int fh, int fw, int lane) {
    QueryTaps taps;
    taps.mask = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        taps.q[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (in_grid(py + dy, px + dx, fh, fw)) {
            taps.mask |= 1u << t;
            taps.q[t] = row4(th_t, row + dy * fw + dx, lane);
        }
    }
    return taps;
}

// R of the pair (taps' query, key `key` at (ky, kx)): the taps inside BOTH grids, in raster order, the same sum in every lane.  This
// is the one place that decides "inside" for a pair — on the 2-D coordinates, never on the flat index
__device__ __forceinline__ float pair_R(const QueryTaps& taps, const float* __restrict__ ph_t, long long key, int ky, int kx, int gh,
                                        int gw, int lane) {
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        if (((taps.mask >> t) & 1u) && in_grid(ky + dy, kx + dx, gh, gw)) acc = lane_fma4(taps.q[t], row4(ph_t, key + dy * gw + dx, lane), acc);
    }
    return wave_sum(acc);
}

// what one pair gives the backward, from dzt = dz inv_t: g = dzt a_p b (the coefficient on R), hb = dzt a_p c (the pair's share of
// db), ab = dzt b (times c: the pair's share of da_p)
struct PairGrad { float g, hb, ab; };

__device__ __forceinline__ PairGrad pair_grad(float dzt, float a_p, float b, float c) { return PairGrad{dzt * a_p * b, dzt * a_p * c, dzt * b}; }

}  // namespace cocos
