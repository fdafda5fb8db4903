// The head of the first row pass: what sits between its output o = softmax(f) @ [exemplar | ref_seg]  [B, Ci+Cs, h*w] and the two
// tensors the losses see (gfx950, round 6):
//     warp_out  = nearest x`d` up-sampling of o[:, :Ci]      (correspondence.py:188 at :327)
//     warp_mask = o[:, Ci:]                                   (:334, a view)
// Forward: the up-sampling straight from the channel slice (the strided slice used to be copied first).
// Backward: ONE kernel for everything autograd ran between the two loss gradients and the K2 / K19 backward —
//     d o[:, :Ci] = d x d window sums of d warp_out           (was cocos_upsample_nearest_bwd)
//     d o[:, Ci:] = d warp_mask                               (was cocos_concat2_amax: copy + max|.|)
//     max|d o|                                                (the scale source of the backward's f16 split)
//     D[b, n] = sum_c d o[b,c,n] * o[b,c,n]  in fp64          (was cocos_rowdot_f64: the D of the softmax backward)
// four launches and three passes over the 20 MB gradient at the benchmark shape, now one pass.
#include "common.h"

namespace cocos {

__global__ __launch_bounds__(256) void warp_head_fwd_kernel(const float* __restrict__ o, float* __restrict__ y, int Ci, int C,
                                                            int h, int w, int d, size_t n4) {
    const int W = w * d, H = h * d;
    const size_t i4 = (size_t)blockIdx.x * 256 + threadIdx.x;            // float4 index in y (W % 4 == 0)
    if (i4 >= n4) return;
    const int X4 = (int)(i4 % (W / 4));
    size_t r = i4 / (W / 4);
    const int Y = (int)(r % H);
    r /= H;
    const int c = (int)(r % Ci);
    const size_t b = r / Ci;
    const float* xr = o + ((b * C + c) * h + Y / d) * (size_t)w;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = xr[(X4 * 4 + e) / d];
    *reinterpret_cast<f32x4*>(y + i4 * 4) = v;
}

// The same head for the other two flag families (K30), one launch each:
//     bilinear  warp_out = F.interpolate(o[:, :Ci], scale_factor=d, mode="bilinear", align_corners=False)   (:184-186 at :327)
//     patch     warp_out = F.fold(o[:, :Ci], (H, W), d, stride=d): non-overlapping patches, a copy            (:321, :357)
// y_near (nearest) and y_bil (bilinear) may both be given: the inference --show_corr pair (:326-327) from one pass over o.
__device__ __forceinline__ void bilinear_src(int X, int n, float rd, int& i0, int& i1, float& l) {
    const float s = fmaxf(rd * ((float)X + 0.5f) - 0.5f, 0.f);
    i0 = min((int)s, n - 1);
    i1 = min(i0 + 1, n - 1);
    l = s - (float)i0;
}

__global__ __launch_bounds__(256) void warp_head_fwd_bilinear_kernel(const float* __restrict__ o, float* __restrict__ y_near,
                                                                     float* __restrict__ y_bil, int Ci, int C, int h, int w, int d,
                                                                     size_t n4) {
    const int W = w * d, H = h * d;
    const size_t i4 = (size_t)blockIdx.x * 256 + threadIdx.x;            // float4 index in y (W % 4 == 0)
    if (i4 >= n4) return;
    const int X4 = (int)(i4 % (W / 4));
    size_t r = i4 / (W / 4);
    const int Y = (int)(r % H);
    r /= H;
    const int c = (int)(r % Ci);
    const size_t b = r / Ci;
    const float* plane = o + (b * C + c) * (size_t)h * w;
    const float rd = 1.0f / (float)d;
    int y0, y1;
    float ly;
    bilinear_src(Y, h, rd, y0, y1, ly);
    const float* r0 = plane + (size_t)y0 * w;
    const float* r1 = plane + (size_t)y1 * w;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int x0, x1;
        float lx;
        bilinear_src(X4 * 4 + e, w, rd, x0, x1, lx);
        v[e] = (1.f - ly) * ((1.f - lx) * r0[x0] + lx * r0[x1]) + ly * ((1.f - lx) * r1[x0] + lx * r1[x1]);
    }
    *reinterpret_cast<f32x4*>(y_bil + i4 * 4) = v;
    if (y_near) {
        const float* xr = plane + (size_t)(Y / d) * w;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = xr[(X4 * 4 + e) / d];
        *reinterpret_cast<f32x4*>(y_near + i4 * 4) = v;
    }
}

// y[b, c, yy*d + i, xx*d + j] = o[b, c*d*d + i*d + j, yy*w + xx]   (Ci = (image channels) * d * d rows of o)
__global__ __launch_bounds__(256) void warp_head_fwd_patch_kernel(const float* __restrict__ o, float* __restrict__ y, int Ci, int C,
                                                                  int h, int w, int d, size_t n4) {
    const int W = w * d, H = h * d;
    const size_t i4 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i4 >= n4) return;
    const int X4 = (int)(i4 % (W / 4));
    size_t r = i4 / (W / 4);
    const int Y = (int)(r % H);
    r /= H;
    const int c = (int)(r % (Ci / (d * d)));
    const size_t b = r / (Ci / (d * d));
    const int yy = Y / d, i = Y - yy * d;
    const float* base = o + ((b * C + (size_t)c * d * d + (size_t)i * d) * h + yy) * (size_t)w;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int X = X4 * 4 + e, xx = X / d, j = X - xx * d;
        v[e] = base[(size_t)j * h * w + xx];
    }
    *reinterpret_cast<f32x4*>(y + i4 * 4) = v;
}

// ---- the adjoint of the bilinear up-sampling as a GATHER (fixed order, no atomics) ---------------------------------------------
// Source index x collects from every output index X whose lower tap is x (weight 1 - lambda_X) or whose upper tap is x (weight
// lambda_X); the clamped taps at both borders count under both rules.  For an even scale D the outputs that reach x are
// X = D*x - D/2 + idx, idx in [0, 2D), with weights (idx + .5) / D rising and 1 - (idx - D + .5) / D falling; at x = 0 the outputs
// below the first sample centre (idx in [D/2, D)) and at x = n - 1 those above the last one (idx in [D, D + D/2)) carry weight 1.
template <int D>
__host__ __device__ __forceinline__ float bilinear_tapw(int idx, bool first, bool last) {
    const float base = idx < D ? ((float)idx + 0.5f) / (float)D : 1.f - ((float)(idx - D) + 0.5f) / (float)D;
    const bool one = (first && idx >= D / 2 && idx < D) || (last && idx >= D && idx < D + D / 2);
    return one ? 1.f : base;
}

// g[e] = d loss / d source pixel (yy, xx + e), e = 0..3, of one [h*D, w*D] gradient plane (xx % 4 == 0, w % 4 == 0): a 2D x 2D window
// per pixel, read as D + 2 aligned float4 per output row, rows then columns in a fixed order.
template <int D>
__device__ __forceinline__ f32x4 bilinear_gather_quad(const float* __restrict__ plane, int yy, int xx, int h, int w) {
    const int W = w * D, H = h * D;
    const bool first = xx == 0, last = xx + 4 == w;
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 2 * D; ++a) {
        const int Y = D * yy - D / 2 + a;
        if (Y < 0 || Y >= H) continue;
        const float wy = bilinear_tapw<D>(a, yy == 0, yy == h - 1);
        const float* r = plane + (size_t)Y * W + (size_t)xx * D;
        float t[(D + 2) * 4];
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const f32x4 qa = first ? zero : *reinterpret_cast<const f32x4*>(r - 4);
        const f32x4 qb = last ? zero : *reinterpret_cast<const f32x4*>(r + 4 * D);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            t[e] = qa[e];
            t[(D + 1) * 4 + e] = qb[e];
        }
#pragma unroll
        for (int m = 0; m < D; ++m) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(r + 4 * m);
#pragma unroll
            for (int e = 0; e < 4; ++e) t[4 + 4 * m + e] = q[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float hs = 0.f;
#pragma unroll
            for (int k = 0; k < 2 * D; ++k)
                hs = fmaf(bilinear_tapw<D>(k, e == 0 && first, e == 3 && last), t[4 + D * e - D / 2 + k], hs);
            g[e] = fmaf(wy, hs, g[e]);
        }
    }
    return g;
}

// any other scale: the same sum with the taps recomputed per output index
__device__ __forceinline__ float bilinear_tap_generic(int X, int x, int n, float rd) {
    int i0, i1;
    float l;
    bilinear_src(X, n, rd, i0, i1, l);
    return (i0 == x ? 1.f - l : 0.f) + (i1 == x ? l : 0.f);
}

__device__ __forceinline__ f32x4 bilinear_gather_quad_generic(const float* __restrict__ plane, int yy, int xx, int h, int w, int d) {
    const int W = w * d, H = h * d;
    const float rd = 1.0f / (float)d;
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    for (int Y = max(0, d * yy - d); Y < min(H, d * yy + 2 * d); ++Y) {
        const float wy = bilinear_tap_generic(Y, yy, h, rd);
        if (wy == 0.f) continue;
        const float* r = plane + (size_t)Y * W;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float hs = 0.f;
            for (int X = max(0, d * (xx + e) - d); X < min(W, d * (xx + e) + 2 * d); ++X)
                hs = fmaf(bilinear_tap_generic(X, xx + e, w, rd), r[X], hs);
            g[e] = fmaf(wy, hs, g[e]);
        }
    }
    return g;
}

enum { kHeadNearest = COCOS_WARP_HEAD_NEAREST, kHeadBilinear = COCOS_WARP_HEAD_BILINEAR, kHeadPatch = COCOS_WARP_HEAD_PATCH };

// Workgroup = 64 positions (16 lanes x 4) x 16 channel groups, grid (N / 64, B): 512 workgroups at the benchmark shape (two per CU;
// with rowdot_f64's 128 x 8 decomposition the kernel was latency-bound at one workgroup per CU: 23 us for 66 MB).
// g_img / g_mask / g_y may each be NULL: a gradient that autograd did not deliver counts as zero.
template <int MODE, int D>
__global__ __launch_bounds__(256) void warp_head_bwd_kernel(const float* __restrict__ g_img, const float* __restrict__ g_mask,
                                                            const float* __restrict__ g_y, const float* __restrict__ o,
                                                            float* __restrict__ dout, float* __restrict__ drow,
                                                            unsigned* __restrict__ amax, int Ci, int Cs, int h, int w, int dd) {
    __shared__ double red[16][64];
    __shared__ float redm[4];
    const int d = D ? D : dd;
    const int N = h * w, C = Ci + Cs;
    const int q4 = threadIdx.x & 15, cg = threadIdx.x >> 4;
    const int i0 = blockIdx.x * 64 + q4 * 4, b = blockIdx.y;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    float vmax = 0.f;
    if (i0 < N) {                                          // N % 4 == 0, w % 4 == 0: a quad lies in one image row
        const int yy = i0 / w, xx = i0 - yy * w;
        const int W = w * d, H = h * d;
        for (int c = cg; c < C; c += 16) {
            f32x4 g = {0.f, 0.f, 0.f, 0.f};
            if (c < Ci) {
                if (g_img == nullptr) {
                } else if (MODE == kHeadNearest) {
                    const float* p = g_img + (((size_t)b * Ci + c) * h + yy) * d * (size_t)W + (size_t)xx * d;
                    if (D == 4) {
#pragma unroll
                        for (int a = 0; a < 4; ++a)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const f32x4 t = *reinterpret_cast<const f32x4*>(p + (size_t)a * W + 4 * e);
                                g[e] += (t[0] + t[1]) + (t[2] + t[3]);
                            }
                    } else {
                        for (int a = 0; a < d; ++a)
                            for (int e = 0; e < 4; ++e)
                                for (int j = 0; j < d; ++j) g[e] += p[(size_t)a * W + e * d + j];
                    }
                } else if (MODE == kHeadBilinear) {
                    const float* plane = g_img + ((size_t)b * Ci + c) * (size_t)H * W;
                    if (D == 4 || D == 2)
                        g = bilinear_gather_quad<(D ? D : 2)>(plane, yy, xx, h, w);
                    else
                        g = bilinear_gather_quad_generic(plane, yy, xx, h, w, d);
                } else {                                   // patch: row c of o is pixel (i, j) of every patch of image channel cc
                    const int cc = c / (d * d), ij = c - cc * d * d, i = ij / d, j = ij - i * d;
                    const float* p = g_img + (((size_t)b * (Ci / (d * d)) + cc) * H + (size_t)yy * d + i) * W + (size_t)xx * d + j;
#pragma unroll
                    for (int e = 0; e < 4; ++e) g[e] = p[e * d];
                }
                if (g_y) {                                 // the second use of the image channels: V of the column pass (:353-362)
                    const f32x4 t = *reinterpret_cast<const f32x4*>(g_y + ((size_t)b * Ci + c) * N + i0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) g[e] += t[e];
                }
            } else if (g_mask) {
                g = *reinterpret_cast<const f32x4*>(g_mask + ((size_t)b * Cs + (c - Ci)) * N + i0);
            }
            const size_t off = ((size_t)b * C + c) * N + i0;
            *reinterpret_cast<f32x4*>(dout + off) = g;
            const f32x4 y = *reinterpret_cast<const f32x4*>(o + off);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[e] += (double)g[e] * (double)y[e];
                vmax = fmaxf(vmax, fabsf(g[e]));
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[cg][q4 * 4 + e] = acc[e];
    vmax = wave_max_dpp(vmax);
    if ((threadIdx.x & 63) == 0) redm[threadIdx.x >> 6] = vmax;
    __syncthreads();
    if (threadIdx.x < 64) {
        const int i = blockIdx.x * 64 + threadIdx.x;
        double t = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += red[g][threadIdx.x];
        if (i < N) drow[(size_t)b * N + i] = (float)t;
    }
    if (threadIdx.x == 0) atomicMax(amax, __float_as_uint(fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]))));
}

}  // namespace cocos

// The head forward in one of three modes (COCOS_WARP_HEAD_*).  y: nearest / bilinear up-sampling of channels [0, Ci) of o [B, C, h, w]
// -> [B, Ci, h*down, w*down], or (patch) F.fold of those Ci = c * down^2 rows -> [B, c, h*down, w*down].  y_bi (nearest mode only,
// optional): the bilinear up-sampling as well, from the same launch.
extern "C" int cocos_warp_head_fwd_ex(const float* o, float* y, float* y_bi, int B, int Ci, int C, int h, int w, int down, int mode,
                                      cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(o && y, COCOS_ERR_INVALID, "warp_head_fwd: null pointer");
    COCOS_REQUIRE(mode == kHeadNearest || mode == kHeadBilinear || mode == kHeadPatch, COCOS_ERR_INVALID, "warp_head_fwd: bad mode %d",
                  mode);
    COCOS_REQUIRE(B >= 1 && Ci >= 1 && Ci <= C && h >= 1 && w >= 1 && down >= 1, COCOS_ERR_INVALID,
                  "warp_head_fwd: bad dims B=%d Ci=%d C=%d h=%d w=%d down=%d", B, Ci, C, h, w, down);
    COCOS_REQUIRE(y_bi == nullptr || mode == kHeadNearest, COCOS_ERR_INVALID, "warp_head_fwd: y_bi goes with the nearest mode only");
    COCOS_REQUIRE(mode != kHeadPatch || Ci % (down * down) == 0, COCOS_ERR_INVALID,
                  "warp_head_fwd: patch mode takes Ci = channels * down^2 rows, got Ci=%d down=%d", Ci, down);
    COCOS_REQUIRE((w * down) % 4 == 0 && aligned16(y) && aligned16(y_bi), COCOS_ERR_UNSUPPORTED,
                  "warp_head_fwd: output width %d must be a multiple of 4 and y 16-byte aligned", w * down);
    const int planes = mode == kHeadPatch ? Ci / (down * down) : Ci;
    const size_t n4 = (size_t)B * planes * h * down * (w * down / 4);
    COCOS_REQUIRE((n4 + 255) / 256 <= 0x7fffffffull, COCOS_ERR_UNSUPPORTED, "warp_head_fwd: tensor too large");
    const dim3 grid((unsigned)((n4 + 255) / 256));
    if (mode == kHeadPatch)
        hipLaunchKernelGGL(warp_head_fwd_patch_kernel, grid, dim3(256), 0, as_stream(stream), o, y, Ci, C, h, w, down, n4);
    else if (mode == kHeadBilinear)
        hipLaunchKernelGGL(warp_head_fwd_bilinear_kernel, grid, dim3(256), 0, as_stream(stream), o, (float*)nullptr, y, Ci, C, h, w,
                           down, n4);
    else if (y_bi)
        hipLaunchKernelGGL(warp_head_fwd_bilinear_kernel, grid, dim3(256), 0, as_stream(stream), o, y, y_bi, Ci, C, h, w, down, n4);
    else
        hipLaunchKernelGGL(warp_head_fwd_kernel, grid, dim3(256), 0, as_stream(stream), o, y, Ci, C, h, w, down, n4);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

// The head backward in one of three modes: g_img [B, Ci, h*down, w*down] (d loss / d warp_out), g_mask [B, Cs, h, w] (d loss /
// d warp_mask), o [B, Ci+Cs, h, w] -> dout [B, Ci+Cs, h, w], drow [B, h*w] = sum_c dout * o (fp64 accumulation), *amax_inout =
// max(*amax_inout, max|dout|) (a cell holding a finite value >= 0).  Rows [0, Ci) of dout are the adjoint of cocos_warp_head_fwd_ex's
// y (window sums | bilinear gather | un-fold), plus g_y [B, Ci, h*w] when given (the image channels' second consumer); rows
// [Ci, Ci+Cs) are g_mask.  In patch mode g_img is [B, Ci / down^2, h*down, w*down].  g_img, g_mask and g_y may each be NULL (a zero
// gradient); Cs may be 0.  w % 4 == 0; all tensors 16-byte aligned.
extern "C" int cocos_warp_head_bwd_ex(const float* g_img, const float* g_mask, const float* g_y, const float* o, float* dout,
                                      float* drow, float* amax_inout_dev, int B, int Ci, int Cs, int h, int w, int down, int mode,
                                      cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(o && dout && drow && amax_inout_dev, COCOS_ERR_INVALID, "warp_head_bwd: null pointer");
    COCOS_REQUIRE(mode == kHeadNearest || mode == kHeadBilinear || mode == kHeadPatch, COCOS_ERR_INVALID, "warp_head_bwd: bad mode %d",
                  mode);
    COCOS_REQUIRE(B >= 1 && B <= 65535 && Ci >= 0 && Cs >= 0 && Ci + Cs >= 1 && h >= 1 && w >= 1 && down >= 1, COCOS_ERR_INVALID,
                  "warp_head_bwd: bad dims B=%d Ci=%d Cs=%d h=%d w=%d down=%d", B, Ci, Cs, h, w, down);
    COCOS_REQUIRE(mode != kHeadPatch || Ci % (down * down) == 0, COCOS_ERR_INVALID,
                  "warp_head_bwd: patch mode takes Ci = channels * down^2 rows, got Ci=%d down=%d", Ci, down);
    COCOS_REQUIRE(w % 4 == 0, COCOS_ERR_UNSUPPORTED, "warp_head_bwd: grid width %d must be a multiple of 4", w);
    for (const void* p : {(const void*)g_img, (const void*)g_mask, (const void*)g_y, (const void*)o, (const void*)dout})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "warp_head_bwd: tensors must be 16-byte aligned");
    const int N = h * w;
    const dim3 grid((unsigned)((N + 63) / 64), (unsigned)B);
    unsigned* cell = reinterpret_cast<unsigned*>(amax_inout_dev);
#define COCOS_HEAD_BWD(MODE, D)                                                                                                     \
    hipLaunchKernelGGL((warp_head_bwd_kernel<MODE, D>), grid, dim3(256), 0, as_stream(stream), g_img, g_mask, g_y, o, dout, drow, cell, \
                       Ci, Cs, h, w, down)
    if (mode == kHeadNearest) {
        if (down == 4) COCOS_HEAD_BWD(kHeadNearest, 4);
        else COCOS_HEAD_BWD(kHeadNearest, 0);
    } else if (mode == kHeadBilinear) {
        if (down == 4) COCOS_HEAD_BWD(kHeadBilinear, 4);
        else if (down == 2) COCOS_HEAD_BWD(kHeadBilinear, 2);
        else COCOS_HEAD_BWD(kHeadBilinear, 0);
    } else {
        COCOS_HEAD_BWD(kHeadPatch, 0);
    }
#undef COCOS_HEAD_BWD
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

// The tap table of the bilinear backward for down = 2 / 4, readable without a device (tests): the weight of output index
// down * x - down / 2 + idx (idx in [0, 2 * down)) on source index x; first / last: x is the first / last source index.
// -1 for scales without a table (they take the generic loop).
extern "C" float cocos_warp_head_bilinear_tap(int down, int idx, int first, int last) {
    if ((down != 2 && down != 4) || idx < 0 || idx >= 2 * down) return -1.f;
    return down == 4 ? cocos::bilinear_tapw<4>(idx, first != 0, last != 0) : cocos::bilinear_tapw<2>(idx, first != 0, last != 0);
}
