// K32: weight preparation for frozen-weight inference (cocosnet_amd/inference.py), table driven like K29 (optim_step.hip): the host
// hands over an array of entries, the entry points copy COCOS_WPREP_TABLE_ENTRIES of them at a time into the kernel arguments of one
// launch.  gfx950.
//
//   cocos_weight_absmax_multi   max|w| of every entry: one workgroup per COCOS_WPREP_ABSMAX_CHUNK elements leaves its maximum in the
//                               workspace, a finishing workgroup per entry reduces those and WRITES the cell (two stream-ordered
//                               launches per table: no atomics at all, no cell to pre-zero).  max is exact, so the cell holds the bits
//                               cocos_absmax leaves for the same tensor.
//   cocos_weight_planes_multi   the f16 hi/lo (or bf16) planes of one layout per entry, scaled by the power of two of the entry's cell:
//                               byte for byte what the single-tensor routine of that layout writes (the item bodies below restate
//                               conv_weight_planes_kernel, split_f16_rows_kernel and pf_weight_frag_item: same products, same
//                               round-to-nearest split, same scale rule).  Every lane writes 16 bytes per plane and item.
//
// Memory-bound streaming passes over a few MB: the point is the launch count (a frozen Pix2PixModel: two absmax tables and two or
// three plane tables instead of ~6 launches per layer), not the bytes.
#include <algorithm>

#include "common.h"
#include "proj_frag.h"

namespace cocos {
namespace {

constexpr int kWpThreads = 256;
constexpr int kWpCap = COCOS_WPREP_TABLE_ENTRIES;
constexpr int kWpAbsChunk = COCOS_WPREP_ABSMAX_CHUNK;
constexpr int kWpAbsVec = kWpAbsChunk / (kWpThreads * 4);      // 16-byte loads per lane
constexpr int kWpItems = 1024;                                  // plane items (16 bytes per plane each) per workgroup
static_assert(kWpAbsChunk == kWpThreads * 4 * kWpAbsVec, "chunk = whole 16-byte pieces per lane");

typedef _Float16 wp_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 wp_bf16x2 __attribute__((ext_vector_type(2)));
typedef float wp_f32x2 __attribute__((ext_vector_type(2)));

struct WpAbsTable {
    const float* w[kWpCap];
    float* cell[kWpCap];
    long long n[kWpCap];
    int blk0[kWpCap + 1];          // first workgroup of each entry; blk0[nent] = grid size
    int nent;
};
struct WpPlaneTable {
    const float* w[kWpCap];
    const float* amax[kWpCap];
    void* hi[kWpCap];
    void* lo[kWpCap];
    float* scale_out[kWpCap];
    int Cout[kWpCap], Cin[kWpCap], aux[kWpCap];
    unsigned char KH[kWpCap], KW[kWpCap], layout[kWpCap];
    int blk0[kWpCap + 1];
    int nent;
};
static_assert(sizeof(WpAbsTable) <= 4096 && sizeof(WpPlaneTable) <= 4096, "kernel-argument segment");

template <class T>
__device__ __forceinline__ int wp_find_entry(const T& t) {      // the last e with blk0[e] <= blockIdx.x (uniform)
    int lo = 0, hi = t.nent - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.blk0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ float wp_scale_from_amax(const float* amax) {      // as conv_f16x3.hip / split_f16.hip / proj_frag.h
    if (!amax) return 1.0f;
    const float a = *amax;
    if (!(a > 0.f) || !(a < INFINITY)) return 1.0f;
    int e;
    frexpf(a, &e);
    return ldexpf(1.0f, 10 - e);
}

__device__ __forceinline__ float wp_block_max(float m) {      // result valid in thread 0
    __shared__ float red[kWpThreads / 64];
    m = wave_max_dpp(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(kWpThreads) void weight_absmax_partial_kernel(const WpAbsTable t, float* __restrict__ part) {
    const int e = wp_find_entry(t);
    const long long first = (long long)((int)blockIdx.x - t.blk0[e]) * kWpAbsChunk;
    const float* __restrict__ x = t.w[e] + first;
    const long long left = t.n[e] - first;
    const int cnt = left < kWpAbsChunk ? (int)left : kWpAbsChunk;
    float m = 0.f;
    if ((reinterpret_cast<uintptr_t>(x) & 15u) == 0) {
        const int cnt4 = cnt >> 2;
        f32x4 v[kWpAbsVec];
#pragma unroll
        for (int u = 0; u < kWpAbsVec; ++u) {      // every load in flight before the first max
            const int i = u * kWpThreads + (int)threadIdx.x;
            v[u] = i < cnt4 ? reinterpret_cast<const f32x4*>(x)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < kWpAbsVec; ++u)
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v[u].x), fabsf(v[u].y))), fmaxf(fabsf(v[u].z), fabsf(v[u].w)));
        const int i = 4 * cnt4 + (int)threadIdx.x;      // up to 3 elements behind the last whole piece
        if (i < cnt) m = fmaxf(m, fabsf(x[i]));
    } else {
        for (int i = threadIdx.x; i < cnt; i += kWpThreads) m = fmaxf(m, fabsf(x[i]));
    }
    m = wp_block_max(m);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// one workgroup per entry: the maxima its chunks left (written by the launch in front of this one on the same stream)
__global__ __launch_bounds__(kWpThreads) void weight_absmax_finish_kernel(const WpAbsTable t, const float* __restrict__ part) {
    const int e = blockIdx.x;
    float m = 0.f;
    for (int p = t.blk0[e] + (int)threadIdx.x; p < t.blk0[e + 1]; p += kWpThreads) m = fmaxf(m, part[p]);
    m = wp_block_max(m);
    if (threadIdx.x == 0) *t.cell[e] = m;
}

// ---- plane items: 8 consecutive halfs of each plane --------------------------------------------------------------------------------
// K16's planes [K/32][M][32] (conv_weight_planes_kernel): item = pairs 4 it .. 4 it + 3 of that kernel's pair index
__device__ __forceinline__ void wp_conv_item(const float* __restrict__ w, void* __restrict__ hi, void* __restrict__ lo, int Cout, int Cin,
                                             int KH, int KW, int mode_full, float scale, unsigned it) {
    const bool bf = (mode_full & 2) != 0;
    const int mode = mode_full & 1;
    const int M = mode == 0 ? Cout : Cin, C = mode == 0 ? Cin : Cout;
    const int T = KH * KW;
    const int j0 = (int)(it & 3u) * 8;
    const unsigned r = it >> 2;
    const int m = (int)(r % (unsigned)M), kb = (int)(r / (unsigned)M);
    const int cb = kb / T, tap = kb - cb * T;
    const int kyp = tap / KW, kxp = tap - kyp * KW;
    const int ky = mode == 0 ? kyp : KH - 1 - kyp, kx = mode == 0 ? kxp : KW - 1 - kxp;
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int c = cb * 32 + j0 + q;
        const int co = mode == 0 ? m : c, ci = mode == 0 ? c : m;
        v[q] = c < C ? w[(((size_t)co * Cin + ci) * KH + ky) * KW + kx] * scale : 0.f;
    }
    u32x4 h4, l4;
    if (bf) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            h4[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(wp_f32x2{v[2 * q], v[2 * q + 1]}, wp_bf16x2));      // round to nearest even
        reinterpret_cast<u32x4*>(hi)[it] = h4;
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned a, b;
        split_pair_rn(v[2 * q], v[2 * q + 1], a, b);
        h4[q] = a; l4[q] = b;
    }
    reinterpret_cast<u32x4*>(hi)[it] = h4;
    reinterpret_cast<u32x4*>(lo)[it] = l4;
}

// split_f16_rows_kernel: x [rows][cols] -> planes [rows][cols_pad], zero beyond cols; item = 8 consecutive columns (cols_pad % 8 == 0)
__device__ __forceinline__ void wp_rows_item(const float* __restrict__ x, void* __restrict__ hi, void* __restrict__ lo, int cols,
                                             int cols_pad, float scale, unsigned it) {
    const unsigned per_row = (unsigned)cols_pad >> 3;
    const int r = (int)(it / per_row), c0 = (int)(it - (unsigned)r * per_row) * 8;
    wp_f16x8 h, l;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        _Float16 a = (_Float16)0.f, b = (_Float16)0.f;
        if (c0 + q < cols) {
            const float v = x[(size_t)r * cols + c0 + q] * scale;
            a = (_Float16)v;
            b = (_Float16)(v - (float)a);
        }
        h[q] = a; l[q] = b;
    }
    reinterpret_cast<wp_f16x8*>(hi)[it] = h;
    reinterpret_cast<wp_f16x8*>(lo)[it] = l;
}

__global__ __launch_bounds__(kWpThreads) void weight_planes_multi_kernel(const WpPlaneTable t) {
    const int e = wp_find_entry(t);
    const int layout = t.layout[e];
    const int Cout = t.Cout[e], Cin = t.Cin[e], KH = t.KH[e], KW = t.KW[e], aux = t.aux[e];
    const float* __restrict__ w = t.w[e];
    const float scale = (layout == COCOS_WPREP_CONV_FWD_BF16 || layout == COCOS_WPREP_CONV_DGRAD_BF16) ? 1.0f : wp_scale_from_amax(t.amax[e]);
    unsigned total;
    if (layout <= COCOS_WPREP_CONV_DGRAD_BF16) {
        const int M = (layout & 1) == 0 ? Cout : Cin, C = (layout & 1) == 0 ? Cin : Cout;
        total = (unsigned)(KH * KW * ((C + 31) / 32)) * (unsigned)M * 4u;
    } else if (layout == COCOS_WPREP_ROWS) {
        total = (unsigned)Cout * ((unsigned)aux >> 3);
    } else {
        total = (unsigned)((Cin + 15) / 16) * 8u * 64u;
    }
    const unsigned base = (unsigned)((int)blockIdx.x - t.blk0[e]) * (unsigned)kWpItems;
    if (base == 0 && threadIdx.x == 0 && t.scale_out[e]) *t.scale_out[e] = scale;
#pragma unroll
    for (int u = 0; u < kWpItems / kWpThreads; ++u) {
        const unsigned it = base + (unsigned)u * kWpThreads + threadIdx.x;
        if (it >= total) break;
        if (layout <= COCOS_WPREP_CONV_DGRAD_BF16) {
            wp_conv_item(w, t.hi[e], t.lo[e], Cout, Cin, KH, KW, layout, scale, it);
        } else if (layout == COCOS_WPREP_ROWS) {
            wp_rows_item(w, t.hi[e], t.lo[e], Cin * KH * KW, aux, scale, it);
        } else {      // K23 / K25 fragment order: item (stage, row block) of 64 lanes, as proj_weight_frag_kernel
            pf_weight_frag_item(w, scale, static_cast<unsigned char*>(t.hi[e]), Cin, nullptr, nullptr, (int)(it >> 9), (int)((it >> 6) & 7u),
                                (int)(it & 63u));
        }
    }
}

long long wp_plane_items(const cocos_wprep_planes_entry& p) {
    if (p.layout <= COCOS_WPREP_CONV_DGRAD_BF16) {
        const long long M = (p.layout & 1) == 0 ? p.Cout : p.Cin, C = (p.layout & 1) == 0 ? p.Cin : p.Cout;
        return (long long)p.KH * p.KW * ((C + 31) / 32) * M * 4;
    }
    if (p.layout == COCOS_WPREP_ROWS) return (long long)p.Cout * (p.aux / 8);
    return (long long)((p.Cin + 15) / 16) * 8 * 64;
}

}  // namespace
}  // namespace cocos

extern "C" int cocos_weight_prepare_constant(int which) {
    switch (which) {
        case COCOS_WPREP_CONST_TABLE_ENTRIES: return COCOS_WPREP_TABLE_ENTRIES;
        case COCOS_WPREP_CONST_ABSMAX_CHUNK: return COCOS_WPREP_ABSMAX_CHUNK;
        default: return 0;
    }
}

extern "C" long long cocos_weight_absmax_multi_workspace_floats(const cocos_wprep_absmax_entry* entries, int n_entries) {
    if (!entries || n_entries < 1) return 0;
    long long most = 0, cur = 0;
    for (int i = 0; i < n_entries; ++i) {
        if (i % COCOS_WPREP_TABLE_ENTRIES == 0) cur = 0;
        cur += entries[i].n < 1 ? 0 : (entries[i].n + COCOS_WPREP_ABSMAX_CHUNK - 1) / COCOS_WPREP_ABSMAX_CHUNK;
        most = std::max(most, cur);
    }
    return most;
}

extern "C" int cocos_weight_absmax_multi(const cocos_wprep_absmax_entry* entries, int n_entries, float* workspace, long long workspace_floats,
                                         int* launches_out, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(entries && workspace, COCOS_ERR_INVALID, "weight_absmax_multi: null table or workspace");
    COCOS_REQUIRE(n_entries >= 1, COCOS_ERR_INVALID, "weight_absmax_multi: %d entries", n_entries);
    for (int i = 0; i < n_entries; ++i) {
        COCOS_REQUIRE(entries[i].w && entries[i].cell, COCOS_ERR_INVALID, "weight_absmax_multi: entry %d: null pointer", i);
        COCOS_REQUIRE(entries[i].n >= 1, COCOS_ERR_INVALID, "weight_absmax_multi: entry %d: n=%lld", i, entries[i].n);
        COCOS_REQUIRE(entries[i].n <= (1ll << 40), COCOS_ERR_UNSUPPORTED, "weight_absmax_multi: entry %d: n=%lld", i, entries[i].n);
    }
    COCOS_REQUIRE(workspace_floats >= cocos_weight_absmax_multi_workspace_floats(entries, n_entries), COCOS_ERR_INVALID,
                  "weight_absmax_multi: workspace of %lld floats, needs %lld", workspace_floats,
                  cocos_weight_absmax_multi_workspace_floats(entries, n_entries));
    if (launches_out) *launches_out = 0;
    int launched = 0;
    for (int i0 = 0; i0 < n_entries; i0 += kWpCap) {
        WpAbsTable t;
        t.nent = std::min(kWpCap, n_entries - i0);
        t.blk0[0] = 0;
        for (int k = 0; k < t.nent; ++k) {
            const cocos_wprep_absmax_entry& e = entries[i0 + k];
            t.w[k] = e.w; t.cell[k] = e.cell; t.n[k] = e.n;
            const long long chunks = (e.n + kWpAbsChunk - 1) / kWpAbsChunk;
            COCOS_REQUIRE(t.blk0[k] + chunks < 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "weight_absmax_multi: table too large");
            t.blk0[k + 1] = t.blk0[k] + (int)chunks;
        }
        for (int k = t.nent; k < kWpCap; ++k) { t.w[k] = nullptr; t.cell[k] = nullptr; t.n[k] = 0; t.blk0[k + 1] = t.blk0[t.nent]; }
        hipLaunchKernelGGL(weight_absmax_partial_kernel, dim3((unsigned)t.blk0[t.nent]), dim3(kWpThreads), 0, as_stream(stream), t, workspace);
        COCOS_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(weight_absmax_finish_kernel, dim3((unsigned)t.nent), dim3(kWpThreads), 0, as_stream(stream), t, workspace);
        COCOS_HIP_CHECK(hipGetLastError());
        launched += 2;
        if (launches_out) *launches_out = launched;
    }
    return COCOS_OK;
}

extern "C" int cocos_weight_planes_multi(const cocos_wprep_planes_entry* entries, int n_entries, int* launches_out, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(entries, COCOS_ERR_INVALID, "weight_planes_multi: null table");
    COCOS_REQUIRE(n_entries >= 1, COCOS_ERR_INVALID, "weight_planes_multi: %d entries", n_entries);
    for (int i = 0; i < n_entries; ++i) {
        const cocos_wprep_planes_entry& p = entries[i];
        COCOS_REQUIRE(p.layout >= COCOS_WPREP_CONV_FWD && p.layout <= COCOS_WPREP_FRAG, COCOS_ERR_INVALID, "weight_planes_multi: entry %d: layout %d", i,
                      p.layout);
        const bool bf = p.layout == COCOS_WPREP_CONV_FWD_BF16 || p.layout == COCOS_WPREP_CONV_DGRAD_BF16;
        const bool one_plane = bf || p.layout == COCOS_WPREP_FRAG;
        COCOS_REQUIRE(p.w && p.hi && (p.lo || one_plane) && (p.amax || bf), COCOS_ERR_INVALID, "weight_planes_multi: entry %d: null pointer", i);
        COCOS_REQUIRE(p.scale_out || bf, COCOS_ERR_INVALID, "weight_planes_multi: entry %d: no scale cell", i);
        COCOS_REQUIRE(aligned16(p.hi) && aligned16(p.lo), COCOS_ERR_INVALID, "weight_planes_multi: entry %d: planes must be 16-byte aligned", i);
        COCOS_REQUIRE(p.Cout >= 1 && p.Cin >= 1 && p.KH >= 1 && p.KW >= 1 && p.KH <= 255 && p.KW <= 255, COCOS_ERR_INVALID,
                      "weight_planes_multi: entry %d: bad dims %dx%dx%dx%d", i, p.Cout, p.Cin, p.KH, p.KW);
        if (p.layout == COCOS_WPREP_ROWS)
            COCOS_REQUIRE(p.aux >= p.Cin * p.KH * p.KW && p.aux % 8 == 0, COCOS_ERR_UNSUPPORTED,
                          "weight_planes_multi: entry %d: padded row length %d for %d columns (a multiple of 8, >= columns)", i, p.aux,
                          p.Cin * p.KH * p.KW);
        if (p.layout == COCOS_WPREP_FRAG)
            COCOS_REQUIRE(p.Cout == PN_M && p.KH == 1 && p.KW == 1 && p.Cin <= 4096, COCOS_ERR_UNSUPPORTED,
                          "weight_planes_multi: entry %d: the fragment layout needs a [256][K <= 4096] weight (%dx%d)", i, p.Cout, p.Cin);
        COCOS_REQUIRE(wp_plane_items(p) < 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "weight_planes_multi: entry %d: weight too large", i);
    }
    if (launches_out) *launches_out = 0;
    int launched = 0;
    for (int i0 = 0; i0 < n_entries; i0 += kWpCap) {
        WpPlaneTable t;
        t.nent = std::min(kWpCap, n_entries - i0);
        t.blk0[0] = 0;
        for (int k = 0; k < kWpCap; ++k) {
            if (k >= t.nent) {
                t.w[k] = nullptr; t.amax[k] = nullptr; t.hi[k] = nullptr; t.lo[k] = nullptr; t.scale_out[k] = nullptr;
                t.Cout[k] = t.Cin[k] = t.aux[k] = 0; t.KH[k] = t.KW[k] = t.layout[k] = 0;
                t.blk0[k + 1] = t.blk0[t.nent];
                continue;
            }
            const cocos_wprep_planes_entry& p = entries[i0 + k];
            t.w[k] = p.w; t.amax[k] = p.amax; t.hi[k] = p.hi; t.lo[k] = p.lo; t.scale_out[k] = p.scale_out;
            t.Cout[k] = p.Cout; t.Cin[k] = p.Cin; t.aux[k] = p.aux;
            t.KH[k] = (unsigned char)p.KH; t.KW[k] = (unsigned char)p.KW; t.layout[k] = (unsigned char)p.layout;
            const long long blocks = (wp_plane_items(p) + kWpItems - 1) / kWpItems;
            COCOS_REQUIRE(t.blk0[k] + blocks < 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "weight_planes_multi: table too large");
            t.blk0[k + 1] = t.blk0[k] + (int)blocks;
        }
        hipLaunchKernelGGL(weight_planes_multi_kernel, dim3((unsigned)t.blk0[t.nent]), dim3(kWpThreads), 0, as_stream(stream), t);
        COCOS_HIP_CHECK(hipGetLastError());
        if (launches_out) *launches_out = ++launched;
    }
    return COCOS_OK;
}
