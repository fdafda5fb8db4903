// Row arithmetic shared by the kernels that score single (query, key) pairs, one wave per row of a position-major tensor [B,N,256]:
// K42 / K44 / K46 (plane_pair.hip) and K43 (patchmatch_f16x3.hip) on the f16 hi/lo operand planes, K51 / K52 (box3_pair.hip, through
// box3_rows.h) on fp32 rows.  A wave reads one 512-byte row per plane, lane l holds channels 4 l .. 4 l + 3; a dot product is four fp32
// FMAs per lane in a fixed order and a xor butterfly over the 64 lanes.  The plane kernels form a logit as
// wave_sum(lane_dot4(q, k)) * logit_scale, so a pair has ONE score, bit for bit, whichever kernel computes it.
// Kernels compiled with contraction on and kernels compiled under `#pragma clang fp contract(off)` share these helpers, and a helper has
// the regime of its own definition: they hold explicit fused multiply-adds, plain multiplies, plain adds, shuffles and integer min / max
// only; x * y + z stays in the kernel that owns it.
#pragma once
#include "common.h"

namespace cocos {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int SW_KD = 256;               // channels of the operand planes
constexpr int ROW_WAVES = 4;             // rows (queries, content positions or keys) per workgroup, one per wave
constexpr int ROW_THREADS = ROW_WAVES * kWave;

// (the wave index is the same in all 64 lanes: saying so keeps the row, its coordinates and the candidate walk on the scalar side)
__device__ __forceinline__ long long wave_row() {
    return (long long)blockIdx.x * ROW_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// the same bits in all lanes, said so: the value moves to the scalar side
__device__ __forceinline__ float uniform_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// lane s's value in every lane; s is wave-uniform
__device__ __forceinline__ float lane_value(float v, int s) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), s));
}

// sum over the 64 lanes, the same bits in every lane (xor butterfly: both partners add the same two numbers)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, kWave));
    return v;
}

// channels 4 lane .. 4 lane + 3 of row `row` of a [rows,256] hi/lo plane pair, hi + lo in fp32 (still x operand_scale)
__device__ __forceinline__ f32x4 load_row4(const _Float16* __restrict__ hi, const _Float16* __restrict__ lo, long long row, int lane) {
    const f16x4 h = *reinterpret_cast<const f16x4*>(hi + row * SW_KD + lane * 4);
    const f16x4 l = *reinterpret_cast<const f16x4*>(lo + row * SW_KD + lane * 4);
    return f32x4{(float)h[0] + (float)l[0], (float)h[1] + (float)l[1], (float)h[2] + (float)l[2], (float)h[3] + (float)l[3]};
}

// this lane's share of <q, kv>: the FMA order every logit of K42 / K43 / K44 is formed in
__device__ __forceinline__ float lane_dot4(const f32x4& q, const f32x4& kv) {
    return __builtin_fmaf(q[3], kv[3], __builtin_fmaf(q[2], kv[2], __builtin_fmaf(q[1], kv[1], q[0] * kv[0])));
}

__device__ __forceinline__ f32x4 fma4(float s, const f32x4& v, const f32x4& acc) {
    return f32x4{__builtin_fmaf(s, v[0], acc[0]), __builtin_fmaf(s, v[1], acc[1]), __builtin_fmaf(s, v[2], acc[2]),
                 __builtin_fmaf(s, v[3], acc[3])};
}

__device__ __forceinline__ int clamp_key(int j, int Nk) { return min(max(j, 0), Nk - 1); }

__device__ __forceinline__ bool in_grid(int y, int x, int h, int w) { return (unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w; }

// The inverse table of an index table (ops._inverse_index_table): entries[offsets[key] .. offsets[key + 1]) name `key`, ascending.
// Ranges and positions are clamped into the tables: a malformed table cannot send a read outside them.
__device__ __forceinline__ int list_begin(const int* __restrict__ offsets, long long key, int total) {
    const int first = offsets[key];
    return min(max(first, 0), total);
}

__device__ __forceinline__ int list_end(const int* __restrict__ offsets, long long key, int total) {
    const int past = offsets[key + 1];
    return min(max(past, list_begin(offsets, key, total)), total);
}

__device__ __forceinline__ int list_entry(const int* __restrict__ entries, int e, int total) { return min(max(entries[e], 0), total - 1); }

}  // namespace cocos
