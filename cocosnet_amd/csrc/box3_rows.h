// The pair core of the match_kernel-3 sparse kernels (box3_pair.hip: K51, K52): what forms, or differentiates, the logit of ONE
// (query, key) pair on fp32 position-major rows [B,N,256].  A wave reads one 1 KiB row, lane l holds channels 4 l .. 4 l + 3.
// K52's kernels are compiled with contraction off, K51's with it on, and a helper has the regime of its own definition: the helpers
// hold explicit fused multiply-adds, plain multiplies, plain adds and shuffles only; x * y + z stays in the kernel that owns it.
#pragma once
#include "sparse_row.h"      // wave_sum, clamp_key

namespace cocos {

constexpr int BOX3_ROW_C = 256;          // channels of theta / phi
constexpr int BOX3_WAVES = 4;            // rows (queries, content positions or keys) per workgroup, one per wave
constexpr int BOX3_THREADS = BOX3_WAVES * kWave;

// (the wave index is the same in all 64 lanes: saying so keeps the row, its coordinates and the candidate walk on the scalar side)
__device__ __forceinline__ long long wave_row() {
    return (long long)blockIdx.x * BOX3_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// lane s's value in every lane; s is wave-uniform
__device__ __forceinline__ float lane_value(float v, int s) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), s));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, kWave));
    return v;
}

__device__ __forceinline__ f32x4 row4(const float* __restrict__ t, long long row, int lane) {
    return *reinterpret_cast<const f32x4*>(t + row * BOX3_ROW_C + lane * 4);
}

__device__ __forceinline__ bool in_grid(int y, int x, int h, int w) { return (unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w; }

// acc + this lane's share of <q, kv>, in the order every R is formed in
__device__ __forceinline__ float lane_fma4(const f32x4& q, const f32x4& kv, float acc) {
    return __builtin_fmaf(q[3], kv[3], __builtin_fmaf(q[2], kv[2], __builtin_fmaf(q[1], kv[1], __builtin_fmaf(q[0], kv[0], acc))));
}

__device__ __forceinline__ f32x4 fma4(float s, const f32x4& v, const f32x4& acc) {
    return f32x4{__builtin_fmaf(s, v[0], acc[0]), __builtin_fmaf(s, v[1], acc[1]), __builtin_fmaf(s, v[2], acc[2]),
                 __builtin_fmaf(s, v[3], acc[3])};
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

// The inverse table of an index table (ops._inverse_index_table): entries[offsets[key] .. offsets[key + 1]) name `key`, ascending.
// Ranges and positions are clamped into the tables: a malformed table cannot send a read outside them.
__device__ __forceinline__ int list_begin(const int* __restrict__ offsets, long long key, int total) { return min(max(offsets[key], 0), total); }

__device__ __forceinline__ int list_end(const int* __restrict__ offsets, long long key, int total) {
    return min(max(offsets[key + 1], list_begin(offsets, key, total)), total);
}

__device__ __forceinline__ int list_entry(const int* __restrict__ entries, int e, int total) { return min(max(entries[e], 0), total - 1); }

}  // namespace cocos
