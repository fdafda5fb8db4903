// Row arithmetic shared by the kernels that score single (query, key) pairs on the position-major f16 hi/lo operand planes [B,N,256]:
// K42 (sparse_warp_f16x3.hip) and K43 (patchmatch_f16x3.hip).  A wave reads one 512-byte row per plane, lane l holds channels
// 4 l .. 4 l + 3; a dot product is four fp32 FMAs per lane in a fixed order and a xor butterfly over the 64 lanes.  Both files form a
// logit as wave_sum(lane_dot4(q, k)) * logit_scale, so a pair has ONE score, bit for bit, whichever kernel computes it.
#pragma once
#include "common.h"

namespace cocos {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int SW_KD = 256;               // channels of the operand planes

// sum over the 64 lanes, the same bits in every lane (xor butterfly: both partners add the same two numbers)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// channels 4 lane .. 4 lane + 3 of row `row` of a [rows,256] hi/lo plane pair, hi + lo in fp32 (still x operand_scale)
__device__ __forceinline__ f32x4 load_row4(const _Float16* __restrict__ hi, const _Float16* __restrict__ lo, long long row, int lane) {
    const f16x4 h = *reinterpret_cast<const f16x4*>(hi + row * SW_KD + lane * 4);
    const f16x4 l = *reinterpret_cast<const f16x4*>(lo + row * SW_KD + lane * 4);
    return f32x4{(float)h[0] + (float)l[0], (float)h[1] + (float)l[1], (float)h[2] + (float)l[2], (float)h[3] + (float)l[3]};
}

// this lane's share of <q, kv>: the FMA order every logit of K42 / K43 is formed in
__device__ __forceinline__ float lane_dot4(const f32x4& q, const f32x4& kv) {
    return __builtin_fmaf(q[3], kv[3], __builtin_fmaf(q[2], kv[2], __builtin_fmaf(q[1], kv[1], q[0] * kv[0])));
}

__device__ __forceinline__ int clamp_key(int j, int Nk) { return min(max(j, 0), Nk - 1); }

}  // namespace cocos
