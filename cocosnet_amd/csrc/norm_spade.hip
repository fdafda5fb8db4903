// K26: parameter-free batch / sync-batch / instance norm + SPADE modulation + LeakyReLU, forward and backward (gfx950).
//
// Replaces, for networks built WITHOUT `--PONO`, the chain
//     param_free_norm       normalization.py:93-101   xhat = (x - mean_g) * rsqrt(var_g + eps)   (biased variance)
//     SPADE.forward         normalization.py:148-151  z    = xhat * (1 + gamma) + beta
//     actvn (LeakyReLU 0.2) architecture.py:88-95     y    = z > 0 ? z : slope * z                 (slope 1: no activation)
// where the statistics group g is a channel over (B, H, W) (batch / sync-batch norm, per_sample = 0) or a plane (b, c) over (H, W)
// (instance norm, per_sample = 1).  The framework runs the norm as its own kernels (SyncBatchNorm2d as ~10 torch ops, keeping a
// full-size xhat for its backward) and K17 then reads the normalised tensor back.  Here four passes, nothing full-size saved:
//     forward   stats  (read x)                          + apply      (read x, gamma, beta; write y)          = 20 B / element
//     backward  stats  (read x, gamma, beta, dy)         + apply      (read the same four; write dx, dgamma, dbeta) = 44 B / element
// Per-group statistics leave the stats passes as (count, mean, M2) / (sum dxhat, sum dxhat * xhat): a caller with a process group
// combines the ranks' values between the passes (cocosnet_amd/ops.py).
//
// Work split: a row is the N = H*W contiguous floats of one (b, c); a SEGMENT is 1024 consecutive elements of a row (the last one
// of a row may be shorter) and belongs to ONE wave: 64 lanes x 4 float4.  The group of a segment is wave-uniform, so its mean /
// invstd are scalar loads.  The statistics passes leave one partial per segment (fp64), a finishing kernel of the same call merges
// a group's partials in a fixed order: no atomics, results are bitwise reproducible.  Means and M2 combine with Chan's merge, never
// as sum x^2 - n mean^2 (which loses the variance when |mean| >> std): inside a lane the deviations from the segment's first
// element are summed in fp32 (exact enough: they are O(std)), everything after that in fp64.
// N % 4 == 0 with 16-byte aligned tensors takes float4 accesses; anything else the same kernels with per-element accesses.
#include <initializer_list>

#include "common.h"

namespace cocos {

constexpr int NS_SEG = 1024;     // elements per segment (one wave: 64 lanes x 4 float4)
constexpr int NS_WAVES = 4;      // segments (waves) per workgroup

__device__ __forceinline__ int ns_wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// four consecutive elements i0..i0+3 of a row; elements at or beyond N read 0
template <bool VEC>
__device__ __forceinline__ f32x4 ns_load(__amdgpu_buffer_rsrc_t rs, int i0, int N) {
    if (VEC) return buf_load4(rs, i0 < N ? (unsigned)i0 * 4u : kBufOob);   // N % 4 == 0: a float4 is entirely in or out
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = buf_load1(rs, i0 + e < N ? (unsigned)(i0 + e) * 4u : kBufOob);
    return v;
}

template <bool VEC>
__device__ __forceinline__ void ns_put(float* row, int i0, int N, const f32x4& v) {
    if (VEC) {
        if (i0 < N) *reinterpret_cast<f32x4*>(row + i0) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < N) row[i0 + e] = v[e];
    }
}

// (n, m, M) <- merge of (n, m, M) and (nb, mb, Mb): count, mean, sum of squared deviations (Chan et al.)
__device__ __forceinline__ void chan_merge(double& n, double& m, double& M, double nb, double mb, double Mb) {
    if (nb == 0.0) return;
    if (n == 0.0) {
        n = nb; m = mb; M = Mb;
        return;
    }
    const double t = n + nb, d = mb - m;
    m += d * (nb / t);
    M += Mb + d * d * (n * (nb / t));
    n = t;
}

// merge over the 64 lanes; the lower lane of every pair is the left operand, so all lanes end with the same bits
__device__ __forceinline__ void wave_chan(double& n, double& m, double& M, int lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const double n2 = __shfl_xor(n, s, 64), m2 = __shfl_xor(m, s, 64), M2 = __shfl_xor(M, s, 64);
        if (lane & s) {
            double an = n2, am = m2, aM = M2;
            chan_merge(an, am, aM, n, m, M);
            n = an; m = am; M = aM;
        } else {
            chan_merge(n, m, M, n2, m2, M2);
        }
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);   // a + b == b + a: every lane ends with the same bits
    return v;
}

struct NsSeg {
    int row;
    int k;      // segment index inside its row
    int g;      // statistics group
};

__device__ __forceinline__ bool ns_locate(NsSeg& s, int seg, int nseg, int nch, int C, int per_sample) {
    if (seg >= nseg) return false;
    s.row = seg / nch;
    s.k = (int)(seg - s.row * nch);
    s.g = per_sample ? s.row : s.row % C;
    return true;
}

// ---- forward statistics: one (mean, M2) partial per segment ------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void ns_stats_kernel(const float* __restrict__ x, double* __restrict__ part, int C, int N, int nch,
                                                       int nseg, int per_sample) {
    const int lane = threadIdx.x & 63;
    const int seg = (int)blockIdx.x * NS_WAVES + ns_wave_id();
    NsSeg s;
    if (!ns_locate(s, seg, nseg, nch, C, per_sample)) return;     // wave-uniform
    const float* xr = x + (size_t)s.row * N;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(xr, (size_t)N * 4);
    const int s0 = s.k * NS_SEG;
    const float pivot = xr[s0];                                  // the segment's first element: deviations stay O(std)
    float d[16];
    float sum = 0.f;
    int nt = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i0 = s0 + (u * 64 + lane) * 4;
        const f32x4 a = ns_load<VEC>(rs, i0, N);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool ok = i0 + e < N;
            d[u * 4 + e] = ok ? a[e] - pivot : 0.f;
            sum += d[u * 4 + e];
            nt += ok;
        }
    }
    const float mt = nt ? sum / (float)nt : 0.f;
    float m2 = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float c = d[u * 4 + e] - mt;
            if (s0 + (u * 64 + lane) * 4 + e < N) m2 += c * c;
        }
    double n = (double)nt, m = (double)pivot + (double)mt, M = (double)m2;
    wave_chan(n, m, M, lane);
    if (lane == 0) {
        part[2 * seg] = m;
        part[2 * seg + 1] = M;
    }
}

// count of segment k of a row
__device__ __forceinline__ int ns_seg_count(int k, int N) { return min(NS_SEG, N - k * NS_SEG); }

// index of the j-th partial of group g (fixed order: sample-major, then segment)
__device__ __forceinline__ long long ns_part_index(int g, int j, int C, int nch, int per_sample) {
    const int kk = j % nch;
    return per_sample ? (long long)g * nch + kk : ((long long)(j / nch) * C + g) * nch + kk;
}

// one wave per group: stats [4][G] = count, mean, M2, 1/sqrt(M2/count + eps)
__global__ __launch_bounds__(256) void ns_stats_finish_kernel(const double* __restrict__ part, float* __restrict__ stats, int B, int C,
                                                              int N, int nch, int per_sample, int G, float eps) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * NS_WAVES + ns_wave_id();
    if (g >= G) return;
    const int np = per_sample ? nch : B * nch;
    double n = 0.0, m = 0.0, M = 0.0;
    for (int j = lane; j < np; j += 64) {
        const long long p = ns_part_index(g, j, C, nch, per_sample);
        chan_merge(n, m, M, (double)ns_seg_count(j % nch, N), part[2 * p], part[2 * p + 1]);
    }
    wave_chan(n, m, M, lane);
    if (lane == 0) {
        stats[g] = (float)n;
        stats[G + g] = (float)m;
        stats[2 * G + g] = (float)M;
        stats[3 * G + g] = (float)(1.0 / sqrt(M / n + (double)eps));
    }
}

// ---- forward apply --------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void ns_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd, float* __restrict__ y, int C, int N, int nch,
                                                       int nseg, int per_sample, float slope,
                                                       float* __restrict__ amax_part /* nullable: [nseg] max|y| */) {
    const int lane = threadIdx.x & 63;
    const int seg = (int)blockIdx.x * NS_WAVES + ns_wave_id();
    NsSeg s;
    if (!ns_locate(s, seg, nseg, nch, C, per_sample)) return;
    const size_t ro = (size_t)s.row * N, bytes = (size_t)N * 4;
    const __amdgpu_buffer_rsrc_t x_rs = make_rsrc(x + ro, bytes), g_rs = make_rsrc(gamma + ro, bytes), b_rs = make_rsrc(beta + ro, bytes);
    const float mu = mean[s.g], r = invstd[s.g];
    float* yr = y + ro;
    const int s0 = s.k * NS_SEG;
    float vm = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i0 = s0 + (u * 64 + lane) * 4;
        const f32x4 a = ns_load<VEC>(x_rs, i0, N), gm = ns_load<VEC>(g_rs, i0, N), bt = ns_load<VEC>(b_rs, i0, N);
        f32x4 z = (a - mu) * r * (1.0f + gm) + bt;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            z[e] = z[e] > 0.f ? z[e] : z[e] * slope;
            if (i0 + e < N) vm = fmaxf(vm, fabsf(z[e]));
        }
        ns_put<VEC>(yr, i0, N, z);
    }
    if (amax_part) {                          // uniform: kernel argument
        vm = wave_max_dpp(vm);
        if (lane == 0) amax_part[seg] = vm;
    }
}

// ---- backward statistics: one (sum dxhat, sum dxhat * xhat) partial per segment -----------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void ns_bwd_stats_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ dy,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           double* __restrict__ part, int C, int N, int nch, int nseg, int per_sample,
                                                           float slope) {
    const int lane = threadIdx.x & 63;
    const int seg = (int)blockIdx.x * NS_WAVES + ns_wave_id();
    NsSeg s;
    if (!ns_locate(s, seg, nseg, nch, C, per_sample)) return;
    const size_t ro = (size_t)s.row * N, bytes = (size_t)N * 4;
    const __amdgpu_buffer_rsrc_t x_rs = make_rsrc(x + ro, bytes), g_rs = make_rsrc(gamma + ro, bytes), b_rs = make_rsrc(beta + ro, bytes),
                                 d_rs = make_rsrc(dy + ro, bytes);
    const float mu = mean[s.g], r = invstd[s.g];
    const int s0 = s.k * NS_SEG;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i0 = s0 + (u * 64 + lane) * 4;
        const f32x4 a = ns_load<VEC>(x_rs, i0, N), gm = ns_load<VEC>(g_rs, i0, N), bt = ns_load<VEC>(b_rs, i0, N),
                    dv = ns_load<VEC>(d_rs, i0, N);
        const f32x4 xh = (a - mu) * r, g1 = 1.0f + gm, z = xh * g1 + bt;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float dxh = (z[e] > 0.f ? dv[e] : dv[e] * slope) * g1[e];
            if (i0 + e < N) {
                s1 += dxh;
                s2 += dxh * xh[e];
            }
        }
    }
    const double t1 = wave_sum((double)s1), t2 = wave_sum((double)s2);
    if (lane == 0) {
        part[2 * seg] = t1;
        part[2 * seg + 1] = t2;
    }
}

// one wave per group: sums [2][G] = sum dxhat, sum dxhat * xhat
__global__ __launch_bounds__(256) void ns_bwd_finish_kernel(const double* __restrict__ part, float* __restrict__ sums, int B, int C,
                                                            int nch, int per_sample, int G) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * NS_WAVES + ns_wave_id();
    if (g >= G) return;
    const int np = per_sample ? nch : B * nch;
    double t1 = 0.0, t2 = 0.0;
    for (int j = lane; j < np; j += 64) {
        const long long p = ns_part_index(g, j, C, nch, per_sample);
        t1 += part[2 * p];
        t2 += part[2 * p + 1];
    }
    t1 = wave_sum(t1);
    t2 = wave_sum(t2);
    if (lane == 0) {
        sums[g] = (float)t1;
        sums[G + g] = (float)t2;
    }
}

// ---- backward apply ---------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void ns_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ dy,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           const float* __restrict__ sums, float inv_count, float* __restrict__ dx,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, int C, int N, int nch,
                                                           int nseg, int per_sample, float slope,
                                                           float* __restrict__ amax_part /* nullable: [2][nseg] max|dgamma|, max|dbeta| */) {
    const int lane = threadIdx.x & 63;
    const int seg = (int)blockIdx.x * NS_WAVES + ns_wave_id();
    NsSeg s;
    if (!ns_locate(s, seg, nseg, nch, C, per_sample)) return;
    const size_t ro = (size_t)s.row * N, bytes = (size_t)N * 4;
    const __amdgpu_buffer_rsrc_t x_rs = make_rsrc(x + ro, bytes), g_rs = make_rsrc(gamma + ro, bytes), b_rs = make_rsrc(beta + ro, bytes),
                                 d_rs = make_rsrc(dy + ro, bytes);
    const int G = per_sample ? nseg / nch : C;
    const float mu = mean[s.g], r = invstd[s.g];
    const float m1 = sums ? sums[s.g] * inv_count : 0.f, m2 = sums ? sums[G + s.g] * inv_count : 0.f;
    const int s0 = s.k * NS_SEG;
    float vmg = 0.f, vmb = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i0 = s0 + (u * 64 + lane) * 4;
        const f32x4 a = ns_load<VEC>(x_rs, i0, N), gm = ns_load<VEC>(g_rs, i0, N), bt = ns_load<VEC>(b_rs, i0, N),
                    dv = ns_load<VEC>(d_rs, i0, N);
        const f32x4 xh = (a - mu) * r, g1 = 1.0f + gm, z = xh * g1 + bt;
        f32x4 dz;
#pragma unroll
        for (int e = 0; e < 4; ++e) dz[e] = z[e] > 0.f ? dv[e] : dv[e] * slope;
        const f32x4 dgv = dz * xh;
        if (dx) ns_put<VEC>(dx + ro, i0, N, r * (dz * g1 - m1 - xh * m2));
        if (dgamma) ns_put<VEC>(dgamma + ro, i0, N, dgv);
        if (dbeta) ns_put<VEC>(dbeta + ro, i0, N, dz);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < N) {
                vmg = fmaxf(vmg, fabsf(dgv[e]));
                vmb = fmaxf(vmb, fabsf(dz[e]));
            }
    }
    if (amax_part) {
        vmg = wave_max_dpp(dgamma ? vmg : 0.f);
        vmb = wave_max_dpp(dbeta ? vmb : 0.f);
        if (lane == 0) {
            amax_part[seg] = vmg;
            amax_part[nseg + seg] = vmb;
        }
    }
}

// cells[j] = max(cells[j], max part[j][0..n)), j = blockIdx.x
__global__ __launch_bounds__(256) void ns_amax_finish_kernel(const float* __restrict__ part, long long n, float* __restrict__ cells) {
    __shared__ float redm[4];
    const float* p = part + (size_t)blockIdx.x * n;
    float m = 0.f;
    for (long long i = threadIdx.x; i < n; i += 256) m = fmaxf(m, p[i]);
    m = wave_max_dpp(m);
    if ((threadIdx.x & 63) == 0) redm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
        if (m > cells[blockIdx.x] && m < INFINITY) cells[blockIdx.x] = m;
    }
}

static long long ns_segments(int B, int C, int N) {
    const int nch = (N + NS_SEG - 1) / NS_SEG;
    return (long long)B * C * nch;
}

static bool ns_vec(int N, std::initializer_list<const void*> ptrs) {
    if (N % 4 != 0) return false;
    for (const void* p : ptrs)
        if (p && !aligned16(p)) return false;
    return true;
}

static int ns_check_dims(const char* who, int B, int C, int N, int per_sample) {
    COCOS_REQUIRE(B >= 1 && C >= 1 && N >= 1 && N <= (1 << 28) && (per_sample == 0 || per_sample == 1), COCOS_ERR_INVALID,
                  "%s: bad dims B=%d C=%d N=%d per_sample=%d (N <= 2^28, per_sample 0 | 1)", who, B, C, N, per_sample);
    COCOS_REQUIRE((long long)B * C <= 0x7fffffffll && (ns_segments(B, C, N) + NS_WAVES - 1) / NS_WAVES <= 0x7fffffll, COCOS_ERR_INVALID,
                  "%s: B=%d C=%d N=%d is too large", who, B, C, N);
    return COCOS_OK;
}

}  // namespace cocos

// The four passes of K26: see include/cocos_hip.h.
extern "C" int cocos_norm_spade_workspace_floats(int B, int C, int N) {
    if (B < 1 || C < 1 || N < 1) return 0;
    const long long f = 4 * cocos::ns_segments(B, C, N);
    return f > 0x7fffffffll ? 0 : (int)f;
}

#define COCOS_NS_LAUNCH(KERNEL, vec, grid, ...)                                                                  \
    do {                                                                                                         \
        if (vec) hipLaunchKernelGGL((KERNEL<true>), dim3(grid), dim3(256), 0, st, __VA_ARGS__);                  \
        else hipLaunchKernelGGL((KERNEL<false>), dim3(grid), dim3(256), 0, st, __VA_ARGS__);                     \
    } while (0)

extern "C" int cocos_norm_spade_stats(const float* x, float* stats, float* workspace, int B, int C, int N, int per_sample, float eps,
                                      cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(x && stats && workspace, COCOS_ERR_INVALID, "norm_spade_stats: null pointer");
    COCOS_REQUIRE(aligned16(workspace), COCOS_ERR_INVALID, "norm_spade_stats: workspace must be 16-byte aligned");
    const int rc = ns_check_dims("norm_spade_stats", B, C, N, per_sample);
    if (rc != COCOS_OK) return rc;
    hipStream_t st = as_stream(stream);
    const int nch = (N + NS_SEG - 1) / NS_SEG, G = per_sample ? B * C : C;
    const int nseg = (int)ns_segments(B, C, N);
    double* part = reinterpret_cast<double*>(workspace);
    COCOS_NS_LAUNCH(ns_stats_kernel, ns_vec(N, {x}), (unsigned)((nseg + NS_WAVES - 1) / NS_WAVES), x, part, C, N, nch, nseg, per_sample);
    COCOS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ns_stats_finish_kernel, dim3((G + NS_WAVES - 1) / NS_WAVES), dim3(256), 0, st, part, stats, B, C, N, nch,
                       per_sample, G, eps);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_norm_spade_apply(const float* x, const float* gamma, const float* beta, const float* mean, const float* invstd,
                                      float* y, float* y_amax_inout_dev, float* workspace, int B, int C, int N, int per_sample, float slope,
                                      cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(x && gamma && beta && mean && invstd && y, COCOS_ERR_INVALID, "norm_spade_apply: null pointer");
    COCOS_REQUIRE(!y_amax_inout_dev || workspace, COCOS_ERR_INVALID, "norm_spade_apply: the max|y| epilogue needs the workspace");
    const int rc = ns_check_dims("norm_spade_apply", B, C, N, per_sample);
    if (rc != COCOS_OK) return rc;
    hipStream_t st = as_stream(stream);
    const int nch = (N + NS_SEG - 1) / NS_SEG;
    const int nseg = (int)ns_segments(B, C, N);
    float* part = y_amax_inout_dev ? workspace : nullptr;
    COCOS_NS_LAUNCH(ns_apply_kernel, ns_vec(N, {x, gamma, beta, y}), (unsigned)((nseg + NS_WAVES - 1) / NS_WAVES), x, gamma, beta, mean,
                    invstd, y, C, N, nch, nseg, per_sample, slope, part);
    COCOS_HIP_CHECK(hipGetLastError());
    if (part) {
        hipLaunchKernelGGL(ns_amax_finish_kernel, dim3(1), dim3(256), 0, st, part, nseg, y_amax_inout_dev);
        COCOS_HIP_CHECK(hipGetLastError());
    }
    return COCOS_OK;
}

extern "C" int cocos_norm_spade_bwd_stats(const float* x, const float* gamma, const float* beta, const float* dy, const float* mean,
                                          const float* invstd, float* sums, float* workspace, int B, int C, int N, int per_sample,
                                          float slope, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(x && gamma && beta && dy && mean && invstd && sums && workspace, COCOS_ERR_INVALID, "norm_spade_bwd_stats: null pointer");
    COCOS_REQUIRE(aligned16(workspace), COCOS_ERR_INVALID, "norm_spade_bwd_stats: workspace must be 16-byte aligned");
    const int rc = ns_check_dims("norm_spade_bwd_stats", B, C, N, per_sample);
    if (rc != COCOS_OK) return rc;
    hipStream_t st = as_stream(stream);
    const int nch = (N + NS_SEG - 1) / NS_SEG, G = per_sample ? B * C : C;
    const int nseg = (int)ns_segments(B, C, N);
    double* part = reinterpret_cast<double*>(workspace);
    COCOS_NS_LAUNCH(ns_bwd_stats_kernel, ns_vec(N, {x, gamma, beta, dy}), (unsigned)((nseg + NS_WAVES - 1) / NS_WAVES), x, gamma, beta,
                    dy, mean, invstd, part, C, N, nch, nseg, per_sample, slope);
    COCOS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ns_bwd_finish_kernel, dim3((G + NS_WAVES - 1) / NS_WAVES), dim3(256), 0, st, part, sums, B, C, nch, per_sample, G);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_norm_spade_bwd_apply(const float* x, const float* gamma, const float* beta, const float* dy, const float* mean,
                                          const float* invstd, const float* sums, float inv_count, float* dx, float* dgamma, float* dbeta,
                                          float* amax2_inout_dev, float* workspace, int B, int C, int N, int per_sample, float slope,
                                          cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(x && gamma && beta && dy && mean && invstd, COCOS_ERR_INVALID, "norm_spade_bwd_apply: null pointer");
    COCOS_REQUIRE(!amax2_inout_dev || workspace, COCOS_ERR_INVALID, "norm_spade_bwd_apply: the max|.| epilogue needs the workspace");
    const int rc = ns_check_dims("norm_spade_bwd_apply", B, C, N, per_sample);
    if (rc != COCOS_OK) return rc;
    if (!dx && !dgamma && !dbeta) return COCOS_OK;
    hipStream_t st = as_stream(stream);
    const int nch = (N + NS_SEG - 1) / NS_SEG;
    const int nseg = (int)ns_segments(B, C, N);
    float* part = amax2_inout_dev ? workspace : nullptr;
    COCOS_NS_LAUNCH(ns_bwd_apply_kernel, ns_vec(N, {x, gamma, beta, dy, dx, dgamma, dbeta}), (unsigned)((nseg + NS_WAVES - 1) / NS_WAVES),
                    x, gamma, beta, dy, mean, invstd, sums, inv_count, dx, dgamma, dbeta, C, N, nch, nseg, per_sample, slope, part);
    COCOS_HIP_CHECK(hipGetLastError());
    if (part) {
        hipLaunchKernelGGL(ns_amax_finish_kernel, dim3(2), dim3(256), 0, st, part, nseg, amax2_inout_dev);
        COCOS_HIP_CHECK(hipGetLastError());
    }
    return COCOS_OK;
}
