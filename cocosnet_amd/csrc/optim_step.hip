// K29: the tail of the training step — torch.optim.Adam over a whole parameter list and the reference's EMA update
// (trainers/pix2pix_trainer.py:57,61-62,73; models/networks/generator.py:268-274) as multi-tensor streaming kernels (gfx950).
//
// One launch serves up to COCOS_OPTIM_TABLE_ENTRIES tensors (apex multi_tensor_apply's shape).  The tensor list is a BY-VALUE kernel
// argument: per entry the operand pointers, the element count and the first workgroup of the entry (blk0, a prefix sum: workgroup ->
// entry by binary search, chunk = workgroup - blk0[entry]); Adam's per-group scalars are rows of the same argument, indexed from
// the entry.  Nothing is copied to the device, allocated or synchronised.  A workgroup of 256 threads owns one contiguous chunk of
// COCOS_OPTIM_CHUNK_ELEMS elements: 16-byte loads and stores when the entry's pointers are 16-byte aligned (every chunk then
// starts 16-byte aligned too), all 4 loads per operand issued before the first use; a gradient that is only 4-byte aligned (a view
// into a flat bucket) is read with dword loads while p, m, v stay on the 16-byte route; anything else takes the dword route.
//
// Arithmetic: fp32, in the order of the framework's single-tensor route, every operation rounded on its own (no contraction into
// fma: the pragma below), square root and division correctly rounded (hipcc's default for HIP sources; this file is built without
// -ffast-math).  EMA: two rounded products and one rounded sum, which is bitwise what `(1 - mu) * p + mu * shadow` gives in torch.
#include <algorithm>

#include "common.h"

#pragma clang fp contract(off)

namespace cocos {

constexpr int kThreads = 256;
constexpr int kCap = COCOS_OPTIM_TABLE_ENTRIES;
constexpr int kRows = COCOS_OPTIM_TABLE_GROUPS;
constexpr int kChunk = COCOS_OPTIM_CHUNK_ELEMS;
constexpr long long kEntryMax = COCOS_OPTIM_ENTRY_ELEMS;
constexpr int kVecPerLane = kChunk / (kThreads * 4);      // 16-byte pieces per lane and operand
static_assert(kChunk == kThreads * 4 * kVecPerLane && kEntryMax % kChunk == 0, "chunk = whole 16-byte pieces per lane");
static_assert(kEntryMax / kChunk * kCap < (1ll << 31), "grid size is an int");

struct AdamRow {
    float step_size, bc2_sqrt, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
};

// by-value kernel arguments (2888 and 1544 bytes; the limit is 4096)
struct AdamTable {
    float* p[kCap];
    const float* g[kCap];
    float* m[kCap];
    float* v[kCap];
    int n[kCap];
    int blk0[kCap + 1];        // first workgroup of each entry; blk0[nent] = grid size
    unsigned char row[kCap];
    AdamRow rows[kRows];
    int nent;
};
struct EmaTable {
    float* s[kCap];
    const float* p[kCap];
    int n[kCap];
    int blk0[kCap + 1];
    int nent;
};
static_assert(sizeof(AdamTable) <= 4096 && sizeof(EmaTable) <= 4096, "kernel-argument segment");

namespace {


__device__ __forceinline__ bool dev_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// entry of this workgroup: the last e with blk0[e] <= blockIdx.x (uniform: scalar loads from the argument segment)
template <class T>
__device__ __forceinline__ int find_entry(const T& t) {
    int lo = 0, hi = t.nent - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.blk0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamRow& r) {
    if (r.weight_decay != 0.f) g = g + r.weight_decay * p;
    m = r.beta1 != 0.f ? m + r.one_minus_beta1 * (g - m) : g;
    v = r.beta2 * v + (r.one_minus_beta2 * g) * g;
    const float denom = sqrtf(v) / r.bc2_sqrt + r.eps;
    p = p - (r.step_size * m) / denom;
}

// GVEC: the gradient pointer is 16-byte aligned too
template <bool GVEC>
__device__ __forceinline__ void adam_chunk_vec(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, int cnt, const AdamRow& r) {
    const bool read_m = r.beta1 != 0.f;
    const int cnt4 = cnt >> 2;
    f32x4 vp[kVecPerLane], vg[kVecPerLane], vm[kVecPerLane], vv[kVecPerLane];
#pragma unroll
    for (int u = 0; u < kVecPerLane; ++u) {
        const int i = u * kThreads + threadIdx.x;
        if (i < cnt4) {
            vp[u] = reinterpret_cast<const f32x4*>(p)[i];
            vv[u] = reinterpret_cast<const f32x4*>(v)[i];
            if (read_m) vm[u] = reinterpret_cast<const f32x4*>(m)[i];
            if (GVEC) {
                vg[u] = reinterpret_cast<const f32x4*>(g)[i];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) vg[u][e] = g[4 * i + e];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kVecPerLane; ++u) {
        const int i = u * kThreads + threadIdx.x;
        if (i < cnt4) {
            if (!read_m) vm[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = vp[u][e], me = vm[u][e], ve = vv[u][e];
                adam_elem(pe, vg[u][e], me, ve, r);
                vp[u][e] = pe; vm[u][e] = me; vv[u][e] = ve;
            }
            reinterpret_cast<f32x4*>(p)[i] = vp[u];
            reinterpret_cast<f32x4*>(m)[i] = vm[u];
            reinterpret_cast<f32x4*>(v)[i] = vv[u];
        }
    }
    // the last chunk of an entry: up to 3 elements behind the last whole piece
    const int i = 4 * cnt4 + (int)threadIdx.x;
    if (i < cnt) {
        float pe = p[i], me = read_m ? m[i] : 0.f, ve = v[i];
        adam_elem(pe, g[i], me, ve, r);
        p[i] = pe; m[i] = me; v[i] = ve;
    }
}

__device__ __forceinline__ void adam_chunk_scalar(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, int cnt, const AdamRow& r) {
    const bool read_m = r.beta1 != 0.f;
    for (int i0 = 0; i0 < cnt; i0 += 4 * kThreads) {
        float sp[4], sg[4], sm[4], sv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * kThreads + threadIdx.x;
            if (i < cnt) {
                sp[u] = p[i]; sg[u] = g[i]; sv[u] = v[i];
                sm[u] = read_m ? m[i] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * kThreads + threadIdx.x;
            if (i < cnt) {
                adam_elem(sp[u], sg[u], sm[u], sv[u], r);
                p[i] = sp[u]; m[i] = sm[u]; v[i] = sv[u];
            }
        }
    }
}

}  // namespace

// (outside the anonymous namespace: the profiler's kernel names are cocos::adam_multi_kernel / cocos::ema_multi_kernel)
__global__ __launch_bounds__(kThreads) void adam_multi_kernel(const AdamTable t) {
    const int e = find_entry(t);
    const int base = ((int)blockIdx.x - t.blk0[e]) * kChunk;
    const int cnt = min(kChunk, t.n[e] - base);
    float* p = t.p[e] + base;
    const float* g = t.g[e] + base;
    float* m = t.m[e] + base;
    float* v = t.v[e] + base;
    const AdamRow r = t.rows[t.row[e]];
    if (dev_aligned16(p) && dev_aligned16(m) && dev_aligned16(v)) {
        if (dev_aligned16(g)) adam_chunk_vec<true>(p, g, m, v, cnt, r);
        else adam_chunk_vec<false>(p, g, m, v, cnt, r);
    } else {
        adam_chunk_scalar(p, g, m, v, cnt, r);
    }
}

// plain expressions under this file's contract(off) pragma: each operation is rounded on its own.  (__fmul_rn / __fadd_rn are
// header inlines compiled outside the pragma; the backend contracts their product and sum into one fma.)
__device__ __forceinline__ float ema_elem(float s, float p, float mu, float one_minus_mu) {
    const float a = one_minus_mu * p;
    const float b = mu * s;
    return a + b;
}

__global__ __launch_bounds__(kThreads) void ema_multi_kernel(const EmaTable t, float mu, float one_minus_mu) {
    const int e = find_entry(t);
    const int base = ((int)blockIdx.x - t.blk0[e]) * kChunk;
    const int cnt = min(kChunk, t.n[e] - base);
    float* __restrict__ s = t.s[e] + base;
    const float* __restrict__ p = t.p[e] + base;
    int done = 0;
    if (dev_aligned16(s) && dev_aligned16(p)) {
        const int cnt4 = cnt >> 2;
        f32x4 vs[kVecPerLane], vp[kVecPerLane];
#pragma unroll
        for (int u = 0; u < kVecPerLane; ++u) {
            const int i = u * kThreads + threadIdx.x;
            if (i < cnt4) {
                vs[u] = reinterpret_cast<const f32x4*>(s)[i];
                vp[u] = reinterpret_cast<const f32x4*>(p)[i];
            }
        }
#pragma unroll
        for (int u = 0; u < kVecPerLane; ++u) {
            const int i = u * kThreads + threadIdx.x;
            if (i < cnt4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) vs[u][k] = ema_elem(vs[u][k], vp[u][k], mu, one_minus_mu);
                reinterpret_cast<f32x4*>(s)[i] = vs[u];
            }
        }
        done = 4 * cnt4;
    }
    for (int i = done + threadIdx.x; i < cnt; i += kThreads) s[i] = ema_elem(s[i], p[i], mu, one_minus_mu);
}

namespace {

int chunks_of(long long n) { return (int)((n + kChunk - 1) / kChunk); }

}  // namespace
}  // namespace cocos

extern "C" int cocos_optim_constant(int which) {
    switch (which) {
        case COCOS_OPTIM_CONST_TABLE_ENTRIES: return COCOS_OPTIM_TABLE_ENTRIES;
        case COCOS_OPTIM_CONST_TABLE_GROUPS: return COCOS_OPTIM_TABLE_GROUPS;
        case COCOS_OPTIM_CONST_CHUNK_ELEMS: return COCOS_OPTIM_CHUNK_ELEMS;
        case COCOS_OPTIM_CONST_ENTRY_ELEMS: return COCOS_OPTIM_ENTRY_ELEMS;
        default: return 0;
    }
}

extern "C" int cocos_adam_multi_step(const cocos_adam_entry* entries, int n_entries, const cocos_adam_group* groups, int n_groups,
                                     int* launches_out, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(entries && groups, COCOS_ERR_INVALID, "adam_multi_step: null table");
    COCOS_REQUIRE(n_entries >= 1 && n_groups >= 1, COCOS_ERR_INVALID, "adam_multi_step: %d entries, %d groups", n_entries, n_groups);
    for (int i = 0; i < n_entries; ++i) {
        const cocos_adam_entry& e = entries[i];
        COCOS_REQUIRE(e.p && e.g && e.m && e.v, COCOS_ERR_INVALID, "adam_multi_step: entry %d: null pointer", i);
        COCOS_REQUIRE(e.n >= 1, COCOS_ERR_INVALID, "adam_multi_step: entry %d: n=%lld", i, e.n);
        COCOS_REQUIRE(e.group >= 0 && e.group < n_groups, COCOS_ERR_INVALID, "adam_multi_step: entry %d: group %d of %d", i, e.group, n_groups);
        COCOS_REQUIRE(e.p != e.g && e.p != e.m && e.p != e.v && e.m != e.v && e.g != e.m && e.g != e.v, COCOS_ERR_INVALID,
                      "adam_multi_step: entry %d: aliased operands", i);
    }
    for (int k = 0; k < n_groups; ++k) {
        const cocos_adam_group& q = groups[k];
        // amsgrad / maximize have no field; a bias correction of 0 (step 0) would divide by zero
        COCOS_REQUIRE(q.bc2_sqrt > 0.f && q.beta1 >= 0.f && q.beta1 < 1.f && q.beta2 >= 0.f && q.beta2 < 1.f && q.eps >= 0.f,
                      COCOS_ERR_UNSUPPORTED, "adam_multi_step: group %d: sqrt(bc2)=%g beta1=%g beta2=%g eps=%g", k, q.bc2_sqrt, q.beta1,
                      q.beta2, q.eps);
    }
    AdamTable t;
    int local[kRows];          // rows of this launch -> index into groups
    int launched = 0;
    if (launches_out) *launches_out = 0;
    auto reset = [&]() { t.nent = 0; t.blk0[0] = 0; };
    int nrow = 0;
    auto flush = [&]() -> int {
        if (t.nent == 0) return COCOS_OK;
        hipLaunchKernelGGL(adam_multi_kernel, dim3(t.blk0[t.nent]), dim3(kThreads), 0, as_stream(stream), t);
        COCOS_HIP_CHECK(hipGetLastError());
        if (launches_out) *launches_out = ++launched;
        reset();
        nrow = 0;
        return COCOS_OK;
    };
    reset();
    for (int i = 0; i < n_entries; ++i) {
        const cocos_adam_entry& e = entries[i];
        for (long long off = 0; off < e.n; off += kEntryMax) {
            int row = 0;
            while (row < nrow && local[row] != e.group) ++row;
            if (t.nent == kCap || (row == nrow && nrow == kRows)) {      // the table or its rows are full
                if (int rc = flush()) return rc;
                row = 0;
            }
            if (row == nrow) {
                const cocos_adam_group& q = groups[e.group];
                local[nrow] = e.group;
                t.rows[nrow++] = AdamRow{q.step_size, q.bc2_sqrt, q.beta1, q.one_minus_beta1, q.beta2, q.one_minus_beta2, q.eps, q.weight_decay};
            }
            const int k = t.nent++;
            const long long cnt = std::min(kEntryMax, e.n - off);
            t.p[k] = e.p + off; t.g[k] = e.g + off; t.m[k] = e.m + off; t.v[k] = e.v + off;
            t.n[k] = (int)cnt;
            t.row[k] = (unsigned char)row;
            t.blk0[k + 1] = t.blk0[k] + chunks_of(cnt);
        }
    }
    return flush();
}

extern "C" int cocos_ema_multi_update(const cocos_ema_entry* entries, int n_entries, double mu, int* launches_out,
                                      cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(entries, COCOS_ERR_INVALID, "ema_multi_update: null table");
    COCOS_REQUIRE(n_entries >= 1, COCOS_ERR_INVALID, "ema_multi_update: %d entries", n_entries);
    COCOS_REQUIRE(mu == mu, COCOS_ERR_INVALID, "ema_multi_update: mu is NaN");
    for (int i = 0; i < n_entries; ++i) {
        const cocos_ema_entry& e = entries[i];
        COCOS_REQUIRE(e.shadow && e.p && e.shadow != e.p, COCOS_ERR_INVALID, "ema_multi_update: entry %d: null or aliased pointer", i);
        COCOS_REQUIRE(e.n >= 1, COCOS_ERR_INVALID, "ema_multi_update: entry %d: n=%lld", i, e.n);
    }
    // the two coefficients as the framework forms them: (1.0 - mu) in double, each rounded once to fp32
    const float muf = (float)mu, omu = (float)(1.0 - mu);
    EmaTable t;
    t.nent = 0; t.blk0[0] = 0;
    int launched = 0;
    if (launches_out) *launches_out = 0;
    auto flush = [&]() -> int {
        if (t.nent == 0) return COCOS_OK;
        hipLaunchKernelGGL(ema_multi_kernel, dim3(t.blk0[t.nent]), dim3(kThreads), 0, as_stream(stream), t, muf, omu);
        COCOS_HIP_CHECK(hipGetLastError());
        if (launches_out) *launches_out = ++launched;
        t.nent = 0;
        return COCOS_OK;
    };
    for (int i = 0; i < n_entries; ++i) {
        const cocos_ema_entry& e = entries[i];
        for (long long off = 0; off < e.n; off += kEntryMax) {
            if (t.nent == kCap)
                if (int rc = flush()) return rc;
            const int k = t.nent++;
            const long long cnt = std::min(kEntryMax, e.n - off);
            t.s[k] = e.shadow + off; t.p[k] = e.p + off;
            t.n[k] = (int)cnt;
            t.blk0[k + 1] = t.blk0[k] + chunks_of(cnt);
        }
    }
    return flush();
}
