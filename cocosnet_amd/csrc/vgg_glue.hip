// K27: the glue between the convolutions of the fixed VGG19 feature extractor (gfx950).
//
// VGG19_feature_color_torchversion (reference models/networks/correspondence.py:79-146) runs three times per generator step
// (pix2pix_model.py:248, :306, :311).  Its convolutions are K16 (ops.conv2d); this file takes what sits between them:
//   vgg_preprocess (util/util.py:45-54): RGB -> BGR, minus the mean, x255 (and (x+1)/2 in front)     one pass, 24 B/element
//   F.relu                                                                                            one pass,  8 B/element
//   F.relu + MaxPool2d / AvgPool2d(2, 2): one read of the convolution output writes the pooled tensor (and relu(y) only when
//     the caller asked for that key); the backward recomputes the window's arg-max from the saved source, so there is no index
//     tensor at all.
// Every result is bitwise equal to the framework's fp32 ops on the same input: the same operations in the same order, no
// contraction into fma (the pragma below), NaN kept by relu, the first maximum of a window in scan order with NaN winning.
// The forward passes and the backward passes that feed a K16 layer leave max|out| in a cell (the scale of K16's f16 split),
// so the convolution takes no max|.| pass of its own: one same-address atomicMax on the uint bits per workgroup, after a
// wave64 + LDS reduction.  Max is order-free, so the cell is deterministic; a NaN's bits exceed inf's and win, as in the
// framework's abs().max().
// Pure streaming, HBM-bound: 16-byte accesses along W when the pointers allow it, a grid of at most 256 CUs x 8 workgroups
// striding over the rest, 64-bit element indices (32-bit arithmetic for the index decode when the work count fits).
#include <algorithm>

#include "common.h"

#pragma clang fp contract(off)

namespace cocos {
namespace {

constexpr int kThreads = 256;
constexpr size_t kMaxBlocks = 256 * 8;

unsigned vgg_grid(size_t work) {
    const size_t want = (work + kThreads - 1) / kThreads;
    return (unsigned)std::max<size_t>(1, std::min(want, kMaxBlocks));
}

// |v| as ordered bits: for non-negative floats (and NaN, whose bits lie above inf's) uint order is float order
__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// torch.relu = clamp_min(x, 0): a NaN comes back as it is (fmaxf would drop it)
__device__ __forceinline__ float relu_nan(float v) { return v > 0.f ? v : (v != v ? v : 0.f); }

// threshold_backward(grad, relu(src), 0): grad where !(relu(src) <= 0), i.e. where !(src <= 0) (a NaN passes).  A select, so an
// inf gradient next to a zero mask gives 0, never NaN.
__device__ __forceinline__ float relu_grad(float src, float g) { return src <= 0.f ? 0.f : g; }

// one atomicMax per workgroup; every thread of the block calls it
__device__ __forceinline__ void block_amax(unsigned m, unsigned* cell) {
    __shared__ unsigned red[kThreads / kWave];
#pragma unroll
    for (int o = kWave / 2; o >= 1; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned v = red[0];
#pragma unroll
        for (int w = 1; w < kThreads / kWave; ++w) v = max(v, red[w]);
        atomicMax(cell, v);
    }
}

// the framework's 2x2 pools of four relu'd values in scan order (0,0), (0,1), (1,0), (1,1)
//   max: max_pool2d's `val > maxval || isnan(val)` from -inf, so the FIRST maximum wins and a NaN wins; returns its slot
//   avg: avg_pool2d's `aveval += v` from 0 in scan order, then / 4
__device__ __forceinline__ int argmax4(float a, float b, float c, float d, float& m) {
    int j = 0;
    m = -INFINITY;
    if (a > m || a != a) { m = a; j = 0; }
    if (b > m || b != b) { m = b; j = 1; }
    if (c > m || c != c) { m = c; j = 2; }
    if (d > m || d != d) { m = d; j = 3; }
    return j;
}
__device__ __forceinline__ float pool4(float a, float b, float c, float d, int mode) {
    if (mode == 0) {
        float m;
        argmax4(a, b, c, d, m);
        return m;
    }
    float s = 0.f;
    s += a;
    s += b;
    s += c;
    s += d;
    return s / 4.f;
}

// ---- preprocess -------------------------------------------------------------------------------------------------------------
// the reference's three constants (BGR order), rounded to fp32 as torch.Tensor([...]) rounds them
__device__ __forceinline__ float bgr_mean(int c) { return c == 0 ? 0.40760392f : (c == 1 ? 0.45795686f : 0.48501961f); }

__device__ __forceinline__ float prep_one(float x, int c_out, bool nc) {
    if (nc) x = (x + 1.f) / 2.f;
    return (x - bgr_mean(c_out)) * 255.f;
}

template <typename I>
__global__ __launch_bounds__(kThreads) void preprocess_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                  unsigned* __restrict__ cell, I B, I N, bool nc, bool vec) {
    const I stride = (I)gridDim.x * kThreads;
    unsigned m = 0;
    if (vec) {
        const I N4 = N / 4, work = B * N4;
        for (I i = (I)blockIdx.x * kThreads + threadIdx.x; i < work; i += stride) {
            const I b = i / N4, q = i - b * N4;
            const size_t base = (size_t)b * 3 * N + (size_t)q * 4;
            f32x4 v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = *reinterpret_cast<const f32x4*>(x + base + (size_t)c * N);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = prep_one(v[2 - c][e], c, nc);
                    m = max(m, abs_bits(o[e]));
                }
                *reinterpret_cast<f32x4*>(y + base + (size_t)c * N) = o;
            }
        }
    } else {
        const I work = B * N;
        for (I i = (I)blockIdx.x * kThreads + threadIdx.x; i < work; i += stride) {
            const I b = i / N, q = i - b * N;
            const size_t base = (size_t)b * 3 * N + (size_t)q;
            const float v0 = x[base], v1 = x[base + N], v2 = x[base + 2 * (size_t)N];
            const float o0 = prep_one(v2, 0, nc), o1 = prep_one(v1, 1, nc), o2 = prep_one(v0, 2, nc);
            y[base] = o0;
            y[base + N] = o1;
            y[base + 2 * (size_t)N] = o2;
            m = max(m, max(abs_bits(o0), max(abs_bits(o1), abs_bits(o2))));
        }
    }
    if (cell) block_amax(m, cell);
}

// autograd of the above: mul's backward (dy * 255), the cat's slices (channel 2 - c), div's backward (/ 2)
__device__ __forceinline__ float prep_grad(float g, bool nc) {
    g = g * 255.f;
    return nc ? g / 2.f : g;
}

template <typename I>
__global__ __launch_bounds__(kThreads) void preprocess_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, I B, I N, bool nc,
                                                                  bool vec) {
    const I stride = (I)gridDim.x * kThreads;
    if (vec) {
        const I N4 = N / 4, work = B * N4;
        for (I i = (I)blockIdx.x * kThreads + threadIdx.x; i < work; i += stride) {
            const I b = i / N4, q = i - b * N4;
            const size_t base = (size_t)b * 3 * N + (size_t)q * 4;
            f32x4 g[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] = *reinterpret_cast<const f32x4*>(dy + base + (size_t)c * N);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = prep_grad(g[2 - c][e], nc);
                *reinterpret_cast<f32x4*>(dx + base + (size_t)c * N) = o;
            }
        }
    } else {
        const I work = B * N;
        for (I i = (I)blockIdx.x * kThreads + threadIdx.x; i < work; i += stride) {
            const I b = i / N, q = i - b * N;
            const size_t base = (size_t)b * 3 * N + (size_t)q;
            const float g0 = dy[base], g1 = dy[base + N], g2 = dy[base + 2 * (size_t)N];
            dx[base] = prep_grad(g2, nc);
            dx[base + N] = prep_grad(g1, nc);
            dx[base + 2 * (size_t)N] = prep_grad(g0, nc);
        }
    }
}

// ---- relu -------------------------------------------------------------------------------------------------------------------
// BWD = false: out = relu(a);  BWD = true: out = relu_grad(b = src, a = dr).  n4 float4 chunks (vec) then the scalar rest.
template <bool BWD>
__global__ __launch_bounds__(kThreads) void relu_kernel(const float* __restrict__ a, const float* __restrict__ src, float* __restrict__ out,
                                                        unsigned* __restrict__ cell, size_t n, bool vec) {
    const size_t stride = (size_t)gridDim.x * kThreads, t0 = (size_t)blockIdx.x * kThreads + threadIdx.x;
    unsigned m = 0;
    size_t done = 0;
    if (vec) {
        const size_t n4 = n / 4;
        for (size_t i = t0; i < n4; i += stride) {
            f32x4 v = reinterpret_cast<const f32x4*>(a)[i];
            if (BWD) {
                const f32x4 s = reinterpret_cast<const f32x4*>(src)[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = relu_grad(s[e], v[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = relu_nan(v[e]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) m = max(m, abs_bits(v[e]));
            reinterpret_cast<f32x4*>(out)[i] = v;
        }
        done = n4 * 4;
    }
    for (size_t i = done + t0; i < n; i += stride) {
        const float v = BWD ? relu_grad(src[i], a[i]) : relu_nan(a[i]);
        m = max(m, abs_bits(v));
        out[i] = v;
    }
    if (cell) block_amax(m, cell);
}

// ---- relu + 2x2 pool --------------------------------------------------------------------------------------------------------
// Work item of the vector path (W % 4 == 0, 16-byte aligned): two rows x four columns -> two pooled outputs.  Row pair hp < Ho
// pools; hp == Ho (odd H) is the row the floor cuts: relu only, forward with r, backward always (it gets dr or 0).
// Work item of the scalar path: one 2x2 window (clipped at the cut row / column).
template <typename I>
__global__ __launch_bounds__(kThreads) void relu_pool2_fwd_kernel(const float* __restrict__ y, float* __restrict__ r, float* __restrict__ p,
                                                                  unsigned* __restrict__ cell, I BC, I H, I W, int mode, bool vec) {
    const I stride = (I)gridDim.x * kThreads;
    const I Ho = H / 2, Wo = W / 2;
    const I Hr = r ? (H + 1) / 2 : Ho;
    unsigned m = 0;
    if (vec) {
        const I W4 = W / 4, work = BC * Hr * W4;
        for (I i = (I)blockIdx.x * kThreads + threadIdx.x; i < work; i += stride) {
            const I t = i / W4, w4 = i - t * W4;
            const I bc = t / Hr, hp = t - bc * Hr;
            const size_t o0 = ((size_t)bc * H + 2 * (size_t)hp) * W + 4 * (size_t)w4;
            f32x4 a = *reinterpret_cast<const f32x4*>(y + o0);
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = relu_nan(a[e]);
            if (r) *reinterpret_cast<f32x4*>(r + o0) = a;
            if (hp < Ho) {
                f32x4 b = *reinterpret_cast<const f32x4*>(y + o0 + W);
#pragma unroll
                for (int e = 0; e < 4; ++e) b[e] = relu_nan(b[e]);
                if (r) *reinterpret_cast<f32x4*>(r + o0 + W) = b;
                typedef float f32x2 __attribute__((ext_vector_type(2)));
                f32x2 q;
                q[0] = pool4(a[0], a[1], b[0], b[1], mode);
                q[1] = pool4(a[2], a[3], b[2], b[3], mode);
                *reinterpret_cast<f32x2*>(p + ((size_t)bc * Ho + hp) * Wo + 2 * (size_t)w4) = q;
                m = max(m, max(abs_bits(q[0]), abs_bits(q[1])));
            }
        }
    } else {
        const I Wr = r ? (W + 1) / 2 : Wo, work = BC * Hr * Wr;
        for (I i = (I)blockIdx.x * kThreads + threadIdx.x; i < work; i += stride) {
            const I t = i / Wr, wp = i - t * Wr;
            const I bc = t / Hr, hp = t - bc * Hr;
            const bool h1 = 2 * hp + 1 < H, w1 = 2 * wp + 1 < W;
            const size_t o0 = ((size_t)bc * H + 2 * (size_t)hp) * W + 2 * (size_t)wp;
            const float v00 = relu_nan(y[o0]);
            const float v01 = w1 ? relu_nan(y[o0 + 1]) : 0.f;
            const float v10 = h1 ? relu_nan(y[o0 + W]) : 0.f;
            const float v11 = h1 && w1 ? relu_nan(y[o0 + W + 1]) : 0.f;
            if (r) {
                r[o0] = v00;
                if (w1) r[o0 + 1] = v01;
                if (h1) r[o0 + W] = v10;
                if (h1 && w1) r[o0 + W + 1] = v11;
            }
            if (hp < Ho && wp < Wo) {
                const float q = pool4(v00, v01, v10, v11, mode);
                p[((size_t)bc * Ho + hp) * Wo + wp] = q;
                m = max(m, abs_bits(q));
            }
        }
    }
    if (cell) block_amax(m, cell);
}

// gradient of one element: dr (if any) + what the pool routes to it (if anything), masked by relu's backward.  The framework
// sums the two branches' buffers (dr + 0 off the arg-max: the same value); a window slot that receives nothing and no dr is 0.
__device__ __forceinline__ float pool_elem_grad(float s, bool has_dr, float dr, bool routed, float rv) {
    const float g = routed ? (has_dr ? dr + rv : rv) : (has_dr ? dr : 0.f);
    return relu_grad(s, g);
}

// one window: src (relu on read), dr (if any) and the pooled gradient g (if any) -> four gradients
__device__ __forceinline__ void window_grad(const float s[4], bool has_dr, const float dr[4], bool has_dp, float g, int mode, float o[4]) {
    int j = -1;
    float rv = 0.f;
    if (has_dp) {
        if (mode == 0) {
            float mx;
            j = argmax4(relu_nan(s[0]), relu_nan(s[1]), relu_nan(s[2]), relu_nan(s[3]), mx);
            rv = g;
        } else {
            rv = g / 4.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pool_elem_grad(s[e], has_dr, dr[e], has_dp && (mode != 0 || j == e), rv);
}

template <typename I>
__global__ __launch_bounds__(kThreads) void relu_pool2_bwd_kernel(const float* __restrict__ src, const float* __restrict__ dr,
                                                                  const float* __restrict__ dp, float* __restrict__ dy,
                                                                  unsigned* __restrict__ cell, I BC, I H, I W, int mode, bool vec) {
    const I stride = (I)gridDim.x * kThreads;
    const I Ho = H / 2, Wo = W / 2, Hr = (H + 1) / 2;
    const bool has_dr = dr != nullptr, has_dp = dp != nullptr;
    unsigned m = 0;
    if (vec) {
        const I W4 = W / 4, work = BC * Hr * W4;
        for (I i = (I)blockIdx.x * kThreads + threadIdx.x; i < work; i += stride) {
            const I t = i / W4, w4 = i - t * W4;
            const I bc = t / Hr, hp = t - bc * Hr;
            const size_t o0 = ((size_t)bc * H + 2 * (size_t)hp) * W + 4 * (size_t)w4;
            const f32x4 sa = *reinterpret_cast<const f32x4*>(src + o0);
            const f32x4 ra = has_dr ? *reinterpret_cast<const f32x4*>(dr + o0) : f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 ga;
            if (hp < Ho) {
                const f32x4 sb = *reinterpret_cast<const f32x4*>(src + o0 + W);
                const f32x4 rb = has_dr ? *reinterpret_cast<const f32x4*>(dr + o0 + W) : f32x4{0.f, 0.f, 0.f, 0.f};
                float g0 = 0.f, g1 = 0.f;
                if (has_dp) {
                    typedef float f32x2 __attribute__((ext_vector_type(2)));
                    const f32x2 gp = *reinterpret_cast<const f32x2*>(dp + ((size_t)bc * Ho + hp) * Wo + 2 * (size_t)w4);
                    g0 = gp[0];
                    g1 = gp[1];
                }
                f32x4 gb;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const float s[4] = {sa[2 * k], sa[2 * k + 1], sb[2 * k], sb[2 * k + 1]};
                    const float d[4] = {ra[2 * k], ra[2 * k + 1], rb[2 * k], rb[2 * k + 1]};
                    float o[4];
                    window_grad(s, has_dr, d, has_dp, k == 0 ? g0 : g1, mode, o);
                    ga[2 * k] = o[0];
                    ga[2 * k + 1] = o[1];
                    gb[2 * k] = o[2];
                    gb[2 * k + 1] = o[3];
                }
                *reinterpret_cast<f32x4*>(dy + o0 + W) = gb;
#pragma unroll
                for (int e = 0; e < 4; ++e) m = max(m, abs_bits(gb[e]));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) ga[e] = pool_elem_grad(sa[e], has_dr, ra[e], false, 0.f);
            }
            *reinterpret_cast<f32x4*>(dy + o0) = ga;
#pragma unroll
            for (int e = 0; e < 4; ++e) m = max(m, abs_bits(ga[e]));
        }
    } else {
        const I Wr = (W + 1) / 2, work = BC * Hr * Wr;
        for (I i = (I)blockIdx.x * kThreads + threadIdx.x; i < work; i += stride) {
            const I t = i / Wr, wp = i - t * Wr;
            const I bc = t / Hr, hp = t - bc * Hr;
            const bool h1 = 2 * hp + 1 < H, w1 = 2 * wp + 1 < W;
            const size_t o0 = ((size_t)bc * H + 2 * (size_t)hp) * W + 2 * (size_t)wp;
            const size_t off[4] = {o0, o0 + 1, o0 + W, o0 + W + 1};
            const bool live[4] = {true, w1, h1, h1 && w1};
            float s[4], d[4], o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s[e] = live[e] ? src[off[e]] : 0.f;
                d[e] = live[e] && has_dr ? dr[off[e]] : 0.f;
            }
            if (hp < Ho && wp < Wo) {
                window_grad(s, has_dr, d, has_dp, has_dp ? dp[((size_t)bc * Ho + hp) * Wo + wp] : 0.f, mode, o);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = pool_elem_grad(s[e], has_dr, d[e], false, 0.f);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (live[e]) {
                    dy[off[e]] = o[e];
                    m = max(m, abs_bits(o[e]));
                }
        }
    }
    if (cell) block_amax(m, cell);
}

bool fits32(size_t work) { return work + (size_t)kMaxBlocks * kThreads < 0xffffffffull; }

}  // namespace
}  // namespace cocos

extern "C" int cocos_vgg_preprocess_fwd(const float* x, float* y, float* amax_inout_dev, int B, int H, int W, int normal_correct,
                                        cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(x && y && x != y, COCOS_ERR_INVALID, "vgg_preprocess_fwd: null or aliased pointer");
    COCOS_REQUIRE(B >= 1 && H >= 1 && W >= 1, COCOS_ERR_INVALID, "vgg_preprocess_fwd: B=%d H=%d W=%d", B, H, W);
    const size_t N = (size_t)H * W, work = (size_t)B * N;
    const bool vec = N % 4 == 0 && aligned16(x) && aligned16(y);
    unsigned* cell = reinterpret_cast<unsigned*>(amax_inout_dev);
    const unsigned grid = vgg_grid(vec ? work / 4 : work);
    if (fits32(work))
        hipLaunchKernelGGL(preprocess_fwd_kernel<uint32_t>, dim3(grid), dim3(kThreads), 0, as_stream(stream), x, y, cell, (uint32_t)B,
                           (uint32_t)N, normal_correct != 0, vec);
    else
        hipLaunchKernelGGL(preprocess_fwd_kernel<uint64_t>, dim3(grid), dim3(kThreads), 0, as_stream(stream), x, y, cell, (uint64_t)B,
                           (uint64_t)N, normal_correct != 0, vec);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_vgg_preprocess_bwd(const float* dy, float* dx, int B, int H, int W, int normal_correct, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(dy && dx && dy != dx, COCOS_ERR_INVALID, "vgg_preprocess_bwd: null or aliased pointer");
    COCOS_REQUIRE(B >= 1 && H >= 1 && W >= 1, COCOS_ERR_INVALID, "vgg_preprocess_bwd: B=%d H=%d W=%d", B, H, W);
    const size_t N = (size_t)H * W, work = (size_t)B * N;
    const bool vec = N % 4 == 0 && aligned16(dy) && aligned16(dx);
    const unsigned grid = vgg_grid(vec ? work / 4 : work);
    if (fits32(work))
        hipLaunchKernelGGL(preprocess_bwd_kernel<uint32_t>, dim3(grid), dim3(kThreads), 0, as_stream(stream), dy, dx, (uint32_t)B,
                           (uint32_t)N, normal_correct != 0, vec);
    else
        hipLaunchKernelGGL(preprocess_bwd_kernel<uint64_t>, dim3(grid), dim3(kThreads), 0, as_stream(stream), dy, dx, (uint64_t)B,
                           (uint64_t)N, normal_correct != 0, vec);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_relu_fwd(const float* y, float* r, float* amax_inout_dev, long long n, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(y && r && y != r, COCOS_ERR_INVALID, "relu_fwd: null or aliased pointer");
    COCOS_REQUIRE(n >= 0, COCOS_ERR_INVALID, "relu_fwd: n=%lld", n);
    if (n == 0) return COCOS_OK;
    const bool vec = aligned16(y) && aligned16(r);
    hipLaunchKernelGGL(relu_kernel<false>, dim3(vgg_grid((size_t)n / 4)), dim3(kThreads), 0, as_stream(stream), y, nullptr, r,
                       reinterpret_cast<unsigned*>(amax_inout_dev), (size_t)n, vec);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_relu_bwd(const float* dr, const float* src, float* dy, float* amax_inout_dev, long long n, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(dr && src && dy && dy != dr && dy != src, COCOS_ERR_INVALID, "relu_bwd: null or aliased pointer");
    COCOS_REQUIRE(n >= 0, COCOS_ERR_INVALID, "relu_bwd: n=%lld", n);
    if (n == 0) return COCOS_OK;
    const bool vec = aligned16(dr) && aligned16(src) && aligned16(dy);
    hipLaunchKernelGGL(relu_kernel<true>, dim3(vgg_grid((size_t)n / 4)), dim3(kThreads), 0, as_stream(stream), dr, src, dy,
                       reinterpret_cast<unsigned*>(amax_inout_dev), (size_t)n, vec);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_relu_pool2_fwd(const float* y, float* r, float* p, float* amax_inout_dev, int BC, int H, int W, int mode,
                                    cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(BC >= 1 && H >= 1 && W >= 1 && (mode == 0 || mode == 1), COCOS_ERR_INVALID, "relu_pool2_fwd: BC=%d H=%d W=%d mode=%d",
                  BC, H, W, mode);
    COCOS_REQUIRE(H >= 2 && W >= 2, COCOS_ERR_UNSUPPORTED, "relu_pool2_fwd: %dx%d has no 2x2 window", H, W);
    COCOS_REQUIRE(y && p && y != p && y != r && r != p, COCOS_ERR_INVALID, "relu_pool2_fwd: null or aliased pointer");
    const bool vec = W % 4 == 0 && aligned16(y) && aligned16(p) && (!r || aligned16(r));
    const size_t Hr = r ? (H + 1) / 2 : H / 2, Wr = vec ? W / 4 : (r ? (W + 1) / 2 : W / 2);
    const size_t work = (size_t)BC * Hr * Wr;
    unsigned* cell = reinterpret_cast<unsigned*>(amax_inout_dev);
    if (fits32(work))
        hipLaunchKernelGGL(relu_pool2_fwd_kernel<uint32_t>, dim3(vgg_grid(work)), dim3(kThreads), 0, as_stream(stream), y, r, p, cell,
                           (uint32_t)BC, (uint32_t)H, (uint32_t)W, mode, vec);
    else
        hipLaunchKernelGGL(relu_pool2_fwd_kernel<uint64_t>, dim3(vgg_grid(work)), dim3(kThreads), 0, as_stream(stream), y, r, p, cell,
                           (uint64_t)BC, (uint64_t)H, (uint64_t)W, mode, vec);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_relu_pool2_bwd(const float* src, const float* dr, const float* dp, float* dy, float* amax_inout_dev, int BC, int H,
                                    int W, int mode, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(BC >= 1 && H >= 1 && W >= 1 && (mode == 0 || mode == 1), COCOS_ERR_INVALID, "relu_pool2_bwd: BC=%d H=%d W=%d mode=%d",
                  BC, H, W, mode);
    COCOS_REQUIRE(H >= 2 && W >= 2, COCOS_ERR_UNSUPPORTED, "relu_pool2_bwd: %dx%d has no 2x2 window", H, W);
    COCOS_REQUIRE(src && dy && dy != src && dy != dr && dy != dp, COCOS_ERR_INVALID, "relu_pool2_bwd: null or aliased pointer");
    const bool vec = W % 4 == 0 && aligned16(src) && aligned16(dy) && (!dr || aligned16(dr)) && (!dp || aligned16(dp));
    const size_t work = (size_t)BC * ((H + 1) / 2) * (vec ? W / 4 : (W + 1) / 2);
    unsigned* cell = reinterpret_cast<unsigned*>(amax_inout_dev);
    if (fits32(work))
        hipLaunchKernelGGL(relu_pool2_bwd_kernel<uint32_t>, dim3(vgg_grid(work)), dim3(kThreads), 0, as_stream(stream), src, dr, dp, dy,
                           cell, (uint32_t)BC, (uint32_t)H, (uint32_t)W, mode, vec);
    else
        hipLaunchKernelGGL(relu_pool2_bwd_kernel<uint64_t>, dim3(vgg_grid(work)), dim3(kThreads), 0, as_stream(stream), src, dr, dp, dy,
                           cell, (uint64_t)BC, (uint64_t)H, (uint64_t)W, mode, vec);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
