// K34: InstanceNorm (+ residual) + PReLU for planes of ANY size, a plane spread over several workgroups (gfx950).
//
// K13 (instnorm_prelu.hip) keeps a (sample, channel) plane in ONE workgroup's registers: up to 16384 positions.  The adaptors' layer1
// (correspondence.py:150-173) and the PatchGAN's first norm (discriminator.py:92-115) run at the full image size — 256 x 256 and up.
// Here a plane of N positions is cut into S = ceil(N / SLICE) slices of SLICE = 16384 positions (256 threads x 64 floats, K13's register
// tile); the grid is planes x S workgroups and each direction is TWO launches.  The dependency between the slices of a plane is the
// launch boundary: no workgroup waits for another, nothing is accumulated with atomics, every sum has a fixed order.
//   fwd stats : reads the slice once into registers; writes (mean, M2 about that mean) of the slice — mean first, then centred squares
//   fwd apply : Chan's combination of the S partials in fp64 (every workgroup of the plane, same order => same bits); re-reads the slice;
//               z = (x - mean) rstd (+ res);  y = z > 0 ? z : a z;  writes y, the slice's max|y|; slice 0 writes (mean, rstd) to `stats`
//   bwd sums  : reads x, dy (res);  writes the slice's sum dz, sum dz xn (fp32) and, when asked, the fp64 partial of da = sum_{z<=0} dy z
//   bwd apply : combines the S partials (fp64, fixed order);  dx = rstd (dz - mean(dz) - xn mean(dz xn)), dres = dz, the slice's max|dx|
// followed by the one-workgroup finishes K13 has (max over the per-slice maxima into the caller's cell; the fp64 da partials to one float).
// Bytes per element that cross the L2, by accounting: forward x twice + y = 12 (16 with the residual, which only the apply pass reads);
// backward (x, dy) twice + dx = 20 (32 with the residual and its gradient).  K13's register path: 8 (12) and 12 (20).  DESIGN §3.19.
#include "common.h"

namespace cocos {

constexpr int INS_SLICE = 16384;                  // positions per workgroup: 256 threads x 16 x float4
constexpr int INS_VPT = INS_SLICE / (256 * 4);    // float4 per thread

__device__ __forceinline__ float ins_block_sum(float v, float* red, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ double ins_block_sum_f64(double v, double* red, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ void ins_put_max(float vmax, float* redm, int tid, float* __restrict__ out) {
    vmax = wave_max_dpp(vmax);
    if ((tid & 63) == 0) redm[tid >> 6] = vmax;
    __syncthreads();
    if (tid == 0) *out = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
}

// Where a workgroup works: block b = plane * S + slice; `off` = the slice's first element in the tensor, `len` = its length (1..SLICE).
struct InsSlice {
    size_t off;
    int plane, len;
};
__device__ __forceinline__ InsSlice ins_slice(int N, int S) {
    InsSlice w;
    w.plane = blockIdx.x / S;
    const int s = blockIdx.x - w.plane * S;
    w.off = (size_t)w.plane * N + (size_t)s * INS_SLICE;
    w.len = min(INS_SLICE, N - s * INS_SLICE);
    return w;
}

// The element a thread holds in piece u, lane e.  VEC (N % 4 == 0, 16-byte aligned tensors): float4 number u * 256 + tid of the slice;
// otherwise element (4 u + e) * 256 + tid — 4-byte accesses, consecutive lanes on consecutive addresses.
template <bool VEC>
__device__ __forceinline__ int ins_index(int u, int e, int tid) {
    return VEC ? (u * 256 + tid) * 4 + e : (u * 4 + e) * 256 + tid;
}

template <bool VEC>
__device__ __forceinline__ f32x4 ins_load(const float* __restrict__ p, int u, int tid, int len) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
        const int i = (u * 256 + tid) * 4;
        if (i < len) v = *reinterpret_cast<const f32x4*>(p + i);      // (len % 4 == 0: a float4 is inside or outside as a whole)
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = (u * 4 + e) * 256 + tid;
            if (i < len) v[e] = p[i];
        }
    }
    return v;
}

template <bool VEC>
__device__ __forceinline__ void ins_store(float* __restrict__ p, f32x4 v, int u, int tid, int len) {
    if (VEC) {
        const int i = (u * 256 + tid) * 4;
        if (i < len) *reinterpret_cast<f32x4*>(p + i) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = (u * 4 + e) * 256 + tid;
            if (i < len) p[i] = v[e];
        }
    }
}

// ---- forward, launch 1: (mean, M2) of every slice ----------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void instnorm_split_stats_kernel(const float* __restrict__ x, float* __restrict__ part /* [planes*S][2] */,
                                                                   int N, int S) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const InsSlice w = ins_slice(N, S);
    const float* xs = x + w.off;
    f32x4 v[INS_VPT];
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < INS_VPT; ++u) {
        v[u] = ins_load<VEC>(xs, u, tid, w.len);
        s += (v[u].x + v[u].y) + (v[u].z + v[u].w);
    }
    const float mean = ins_block_sum(s, red, tid) / (float)w.len;
    float ss = 0.f;
#pragma unroll
    for (int u = 0; u < INS_VPT; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = ins_index<VEC>(u, e, tid) < w.len ? v[u][e] - mean : 0.f;
            ss += d * d;
        }
    const float m2 = ins_block_sum(ss, red, tid);
    if (tid == 0) {
        part[2 * (size_t)blockIdx.x] = mean;
        part[2 * (size_t)blockIdx.x + 1] = m2;
    }
}

// (mean, rstd) of a plane from its S slice partials: Chan's pairwise update, slice 0 first, in fp64.  Every lane of every workgroup of
// the plane runs the same instructions on the same numbers.
__device__ __forceinline__ void ins_combine_stats(const float* __restrict__ part, int plane, int N, int S, float eps, float& mean, float& rstd) {
    const float* p = part + 2 * (size_t)plane * S;
    double n = 0.0, mu = 0.0, m2 = 0.0;
    for (int s = 0; s < S; ++s) {
        const double nb = (double)min(INS_SLICE, N - s * INS_SLICE);
        const double d = (double)p[2 * s] - mu, nn = n + nb;
        mu += d * (nb / nn);
        m2 += (double)p[2 * s + 1] + d * d * (n * nb / nn);
        n = nn;
    }
    mean = (float)mu;
    rstd = (float)(1.0 / sqrt(m2 / (double)N + (double)eps));
}

// ---- forward, launch 2: y and the slice's max|y| ------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void instnorm_split_fwd_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                                 const float* __restrict__ aw, const float* __restrict__ part,
                                                                 float* __restrict__ y, float* __restrict__ stats /* [planes][2] */,
                                                                 float* __restrict__ amax_part /* nullable: [planes*S] */, int N, int S,
                                                                 float eps) {
    __shared__ float redm[4];
    const int tid = threadIdx.x;
    const InsSlice w = ins_slice(N, S);
    float mean, r;
    ins_combine_stats(part, w.plane, N, S, eps, mean, r);
    if (tid == 0 && blockIdx.x == w.plane * S) {
        stats[2 * (size_t)w.plane] = mean;
        stats[2 * (size_t)w.plane + 1] = r;
    }
    const float a = *aw;
    const float* xs = x + w.off;
    const float* rs = res ? res + w.off : nullptr;
    float* ys = y + w.off;
    float vmax = 0.f;
#pragma unroll 4
    for (int u = 0; u < INS_VPT; ++u) {
        const f32x4 xv = ins_load<VEC>(xs, u, tid, w.len);
        f32x4 z = (xv - mean) * r;
        if (rs) z += ins_load<VEC>(rs, u, tid, w.len);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            z[e] = z[e] > 0.f ? z[e] : a * z[e];
            if (ins_index<VEC>(u, e, tid) < w.len) vmax = fmaxf(vmax, fabsf(z[e]));
        }
        ins_store<VEC>(ys, z, u, tid, w.len);
    }
    if (amax_part) ins_put_max(vmax, redm, tid, amax_part + blockIdx.x);
}

// dz of four elements (and, SUMS, their contributions to sum dz, sum dz xn and da)
template <bool VEC, bool SUMS, bool DA64>
__device__ __forceinline__ f32x4 ins_dz(f32x4 xv, f32x4 rv, f32x4 g, float mean, float r, float a, int u, int tid, int len, f32x4& xn,
                                        float& s1, float& s2, double& sa) {
    f32x4 dz;
    xn = (xv - mean) * r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float z = xn[e] + rv[e];
        dz[e] = z > 0.f ? g[e] : g[e] * a;
        if (SUMS && ins_index<VEC>(u, e, tid) < len) {      // (outside the slice x, res and dy were loaded as 0, but xn = -mean r there)
            if (DA64 && z <= 0.f) sa += (double)g[e] * (double)z;
            s1 += dz[e];
            s2 += dz[e] * xn[e];
        }
    }
    return dz;
}

// ---- backward, launch 1: the slice's sum dz, sum dz xn (and the fp64 partial of da) --------------------------------------------------
template <bool VEC, bool DA64>
__global__ __launch_bounds__(256) void instnorm_split_bwd_sums_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                                      const float* __restrict__ dy, const float* __restrict__ aw,
                                                                      const float* __restrict__ stats, float* __restrict__ part /* [planes*S][2] */,
                                                                      double* __restrict__ da_part /* DA64: [planes*S] */, int N, int S) {
    __shared__ float red[4];
    __shared__ double red64[4];
    const int tid = threadIdx.x;
    const InsSlice w = ins_slice(N, S);
    const float mean = stats[2 * (size_t)w.plane], r = stats[2 * (size_t)w.plane + 1], a = *aw;
    const float* xs = x + w.off;
    const float* rs = res ? res + w.off : nullptr;
    const float* gs = dy + w.off;
    float s1 = 0.f, s2 = 0.f;
    double sa = 0.0;
#pragma unroll 4
    for (int u = 0; u < INS_VPT; ++u) {
        const f32x4 xv = ins_load<VEC>(xs, u, tid, w.len), g = ins_load<VEC>(gs, u, tid, w.len);
        f32x4 rv = {0.f, 0.f, 0.f, 0.f}, xn;
        if (rs) rv = ins_load<VEC>(rs, u, tid, w.len);
        ins_dz<VEC, true, DA64>(xv, rv, g, mean, r, a, u, tid, w.len, xn, s1, s2, sa);
    }
    const float t1 = ins_block_sum(s1, red, tid);
    const float t2 = ins_block_sum(s2, red, tid);
    if (tid == 0) {
        part[2 * (size_t)blockIdx.x] = t1;
        part[2 * (size_t)blockIdx.x + 1] = t2;
    }
    if (DA64) {
        const double ta = ins_block_sum_f64(sa, red64, tid);
        if (tid == 0) da_part[blockIdx.x] = ta;
    }
}

// ---- backward, launch 2: dx, dres and the slice's max|dx| -----------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void instnorm_split_bwd_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                                 const float* __restrict__ dy, const float* __restrict__ aw,
                                                                 const float* __restrict__ stats, const float* __restrict__ part,
                                                                 float* __restrict__ dx /* nullable */, float* __restrict__ dres /* nullable */,
                                                                 float* __restrict__ amax_part /* nullable: [planes*S] */, int N, int S) {
    __shared__ float redm[4];
    const int tid = threadIdx.x;
    const InsSlice w = ins_slice(N, S);
    const float mean = stats[2 * (size_t)w.plane], r = stats[2 * (size_t)w.plane + 1], a = *aw;
    float m1 = 0.f, m2 = 0.f;
    if (dx) {
        const float* p = part + 2 * (size_t)w.plane * S;
        double t1 = 0.0, t2 = 0.0;
        for (int s = 0; s < S; ++s) { t1 += (double)p[2 * s]; t2 += (double)p[2 * s + 1]; }
        m1 = (float)(t1 / (double)N);
        m2 = (float)(t2 / (double)N);
    }
    const float* xs = x + w.off;
    const float* rs = res ? res + w.off : nullptr;
    const float* gs = dy + w.off;
    float vmax = 0.f, n1 = 0.f, n2 = 0.f;
    double na = 0.0;
#pragma unroll 4
    for (int u = 0; u < INS_VPT; ++u) {
        const f32x4 xv = ins_load<VEC>(xs, u, tid, w.len), g = ins_load<VEC>(gs, u, tid, w.len);
        f32x4 rv = {0.f, 0.f, 0.f, 0.f}, xn;
        if (rs) rv = ins_load<VEC>(rs, u, tid, w.len);
        const f32x4 dz = ins_dz<VEC, false, false>(xv, rv, g, mean, r, a, u, tid, w.len, xn, n1, n2, na);
        if (dres) ins_store<VEC>(dres + w.off, dz, u, tid, w.len);
        if (dx) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] = r * (dz[e] - m1 - xn[e] * m2);
                if (ins_index<VEC>(u, e, tid) < w.len) vmax = fmaxf(vmax, fabsf(o[e]));
            }
            ins_store<VEC>(dx + w.off, o, u, tid, w.len);
        }
    }
    if (amax_part) ins_put_max(vmax, redm, tid, amax_part + blockIdx.x);
}

// *out = (float) sum of n doubles, one workgroup, fixed order (n = planes * S of a layer)
__global__ __launch_bounds__(256) void instnorm_split_da_finish_kernel(const double* __restrict__ p, long long n, float* __restrict__ out) {
    __shared__ double red64[4];
    double v = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) v += p[i];
    const double t = ins_block_sum_f64(v, red64, threadIdx.x);
    if (threadIdx.x == 0) *out = (float)t;
}

// *cell = max(*cell, max part[0..n)): the per-slice maxima -> the caller's cell
__global__ __launch_bounds__(256) void instnorm_split_amax_finish_kernel(const float* __restrict__ part, long long n, float* __restrict__ cell) {
    __shared__ float redm[4];
    float m = 0.f;
    for (long long i = threadIdx.x; i < n; i += 256) m = fmaxf(m, part[i]);
    m = wave_max_dpp(m);
    if ((threadIdx.x & 63) == 0) redm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
        if (m > *cell && m < INFINITY) *cell = m;
    }
}

}  // namespace cocos

// Workspace layout, in floats, with PS = planes * S:  [fp64 da partials: 2 PS][fwd (mean, M2): 2 PS][bwd (sum dz, sum dz xn): 2 PS][maxima: PS]
// (the doubles first: the workspace's own 8-byte alignment is then theirs)
static inline long long ins_slices(int N) { return ((long long)N + cocos::INS_SLICE - 1) / cocos::INS_SLICE; }

extern "C" size_t cocos_instnorm_prelu_split_workspace_floats(int planes, int N) {
    if (planes < 1 || N < 1) return 0;
    return (size_t)7 * (size_t)planes * (size_t)ins_slices(N);
}

static int ins_check_dims(int planes, int N, const char* who) {
    COCOS_REQUIRE(planes >= 1 && N >= 1, COCOS_ERR_INVALID, "%s: bad dims planes=%d N=%d", who, planes, N);
    COCOS_REQUIRE((long long)planes * ins_slices(N) <= 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "%s: planes=%d x %lld slices exceed the grid", who,
                  planes, ins_slices(N));
    return COCOS_OK;
}

extern "C" int cocos_instnorm_prelu_split_fwd(const float* x, const float* residual, const float* prelu_weight, float* y, float* stats,
                                              float* workspace, float* y_amax_inout_dev, int planes, int N, float eps,
                                              cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(x && prelu_weight && y && stats && workspace, COCOS_ERR_INVALID, "instnorm_prelu_split_fwd: null pointer");
    if (int rc = ins_check_dims(planes, N, "instnorm_prelu_split_fwd")) return rc;
    hipStream_t s = as_stream(stream);
    const int S = (int)ins_slices(N);
    const long long PS = (long long)planes * S;
    float* part = workspace + 2 * PS;
    float* maxima = y_amax_inout_dev ? workspace + 6 * PS : nullptr;
    const bool vec = N % 4 == 0 && aligned16(x) && aligned16(y) && (!residual || aligned16(residual));
    const dim3 grid((unsigned)PS), block(256);
    if (vec) {
        hipLaunchKernelGGL(instnorm_split_stats_kernel<true>, grid, block, 0, s, x, part, N, S);
        hipLaunchKernelGGL(instnorm_split_fwd_kernel<true>, grid, block, 0, s, x, residual, prelu_weight, part, y, stats, maxima, N, S, eps);
    } else {
        hipLaunchKernelGGL(instnorm_split_stats_kernel<false>, grid, block, 0, s, x, part, N, S);
        hipLaunchKernelGGL(instnorm_split_fwd_kernel<false>, grid, block, 0, s, x, residual, prelu_weight, part, y, stats, maxima, N, S, eps);
    }
    COCOS_HIP_CHECK(hipGetLastError());
    if (maxima) {
        hipLaunchKernelGGL(instnorm_split_amax_finish_kernel, dim3(1), block, 0, s, maxima, PS, y_amax_inout_dev);
        COCOS_HIP_CHECK(hipGetLastError());
    }
    return COCOS_OK;
}

extern "C" int cocos_instnorm_prelu_split_bwd(const float* x, const float* residual, const float* prelu_weight, const float* dy,
                                              const float* stats, float* dx, float* dresidual, float* da_out, float* workspace,
                                              float* dx_amax_inout_dev, int planes, int N, float eps, cocos_stream_t stream) {
    using namespace cocos;
    (void)eps;                                            // (the statistics come from the forward: nothing is recomputed)
    COCOS_REQUIRE(x && prelu_weight && dy && stats && workspace, COCOS_ERR_INVALID, "instnorm_prelu_split_bwd: null pointer");
    if (int rc = ins_check_dims(planes, N, "instnorm_prelu_split_bwd")) return rc;
    COCOS_REQUIRE(!dx_amax_inout_dev || dx, COCOS_ERR_INVALID, "instnorm_prelu_split_bwd: max|dx| without dx");
    COCOS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, COCOS_ERR_INVALID, "instnorm_prelu_split_bwd: workspace must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    const int S = (int)ins_slices(N);
    const long long PS = (long long)planes * S;
    double* da_part = reinterpret_cast<double*>(workspace);
    float* part = workspace + 4 * PS;
    float* maxima = dx_amax_inout_dev ? workspace + 6 * PS : nullptr;
    const bool vec = N % 4 == 0 && aligned16(x) && aligned16(dy) && (!residual || aligned16(residual)) && (!dx || aligned16(dx)) &&
                     (!dresidual || aligned16(dresidual));
    const dim3 grid((unsigned)PS), block(256);
    if (dx || da_out) {
        if (vec && da_out)  hipLaunchKernelGGL((instnorm_split_bwd_sums_kernel<true, true>), grid, block, 0, s, x, residual, dy, prelu_weight, stats, part, da_part, N, S);
        else if (vec)       hipLaunchKernelGGL((instnorm_split_bwd_sums_kernel<true, false>), grid, block, 0, s, x, residual, dy, prelu_weight, stats, part, da_part, N, S);
        else if (da_out)    hipLaunchKernelGGL((instnorm_split_bwd_sums_kernel<false, true>), grid, block, 0, s, x, residual, dy, prelu_weight, stats, part, da_part, N, S);
        else                hipLaunchKernelGGL((instnorm_split_bwd_sums_kernel<false, false>), grid, block, 0, s, x, residual, dy, prelu_weight, stats, part, da_part, N, S);
        COCOS_HIP_CHECK(hipGetLastError());
    }
    if (dx || dresidual) {
        if (vec) hipLaunchKernelGGL(instnorm_split_bwd_kernel<true>, grid, block, 0, s, x, residual, dy, prelu_weight, stats, part, dx, dresidual, maxima, N, S);
        else     hipLaunchKernelGGL(instnorm_split_bwd_kernel<false>, grid, block, 0, s, x, residual, dy, prelu_weight, stats, part, dx, dresidual, maxima, N, S);
        COCOS_HIP_CHECK(hipGetLastError());
    }
    if (da_out) {
        hipLaunchKernelGGL(instnorm_split_da_finish_kernel, dim3(1), block, 0, s, da_part, PS, da_out);
        COCOS_HIP_CHECK(hipGetLastError());
    }
    if (maxima) {
        hipLaunchKernelGGL(instnorm_split_amax_finish_kernel, dim3(1), block, 0, s, maxima, PS, dx_amax_inout_dev);
        COCOS_HIP_CHECK(hipGetLastError());
    }
    return COCOS_OK;
}
