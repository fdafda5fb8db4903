// Row helpers shared by the kernels that form the match_kernel-3 logit of single (query, key) pairs on fp32 position-major rows
// [B,N,256]: K51 (box3_sparse_warp.hip) and K52 (box3_match_refine.hip).  A wave reads one 1 KiB row, lane l holds channels
// 4 l .. 4 l + 3; R of a pair is lane_fma4 over the in-grid taps in raster order and one wave_sum (sparse_row.h).
#pragma once
#include "sparse_row.h"      // wave_sum, clamp_key

namespace cocos {

constexpr int BOX3_ROW_C = 256;          // channels of theta / phi

__device__ __forceinline__ f32x4 row4(const float* __restrict__ t, long long row, int lane) {
    return *reinterpret_cast<const f32x4*>(t + row * BOX3_ROW_C + lane * 4);
}

__device__ __forceinline__ bool in_grid(int y, int x, int h, int w) { return (unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w; }

// acc + this lane's share of <q, kv>, in the order every R of the two files is formed in
__device__ __forceinline__ float lane_fma4(const f32x4& q, const f32x4& kv, float acc) {
    return __builtin_fmaf(q[3], kv[3], __builtin_fmaf(q[2], kv[2], __builtin_fmaf(q[1], kv[1], __builtin_fmaf(q[0], kv[0], acc))));
}

}  // namespace cocos
