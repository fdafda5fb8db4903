// K35: 3x3 convolution of a ONE-HOT label map as nine table look-ups per output pixel (gfx950).
//
// The segmentation map the networks read is a one-hot fp32 tensor [B, nc, H, W] built from an integer map [B, 1, H, W]
// (pix2pix_model.py:177-187).  A 3x3 convolution of it is  y[b, :, p] = bias + sum_tap W[:, label(p + tap), tap]:  no matrix product, no
// operand preparation, no max|x| pass — 4 bytes read per pixel instead of 4 nc, and exact fp32 sums of at most ten numbers.
//   one_hot : int64 labels -> the one-hot tensor (every element written) + the compact int32 index map; a label outside [0, nc) gives an
//             all-zero column and index -1
//   table   : W [Cout, nc, 3, 3] -> Wt [9][nc][Cout]  (tap-major: the Cout numbers of one (tap, class) are consecutive)
//   fwd     : a lane owns 4 consecutive pixels of a row x 16 output channels; per tap and pixel four 16-byte loads of Wt (L2 / L1
//             resident: 348 KB at nc = 151, Cout = 64; lanes of equal label read the same line), 16-byte stores along x, max|y| per
//             workgroup into the caller's cell (integer atomicMax on the bits of a non-negative float, as the other producers)
//   bwd     : dW[o, l, tap] = sum of dy[b, o, p] over the pixels whose tap lands on class l — a bucketed sum.  A workgroup takes a slice of
//             pixels x 16 channels; thread (tap, channel) is the ONLY writer of its accumulators acc[tap][class][channel] in LDS and walks
//             the slice in pixel order (runs of equal labels are summed in a register first), so nothing is atomic and the order is fixed.
//             Per-slice partials, then a second pass that adds them in slice order.  db rides along (the centre tap's threads).
// The sampling step s reads the index map at (y s, x s): F.interpolate(mode="nearest") for whole ratios.  DESIGN §3.21.
#include <algorithm>

#include "common.h"

namespace cocos {

constexpr int LC_CH = 16;               // output channels per workgroup (fwd: per lane)
constexpr int LC_BWD_THREADS = 192;     // 9 taps x 16 channels = 144 accumulating threads, three waves
constexpr int LC_BWD_TILE = 64;         // pixels staged per step of the backward
constexpr int LC_BWD_CLASSES = 192;     // classes per LDS window: 9 * 192 * 16 * 4 = 110592 bytes
constexpr int LC_BWD_MAX_SLICES = 192;
constexpr long long LC_BWD_PART_BYTES = 64ll << 20;      // bound of the partial sums

// ---- one-hot ----------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void labels_one_hot_kernel(const long long* __restrict__ lab, float* __restrict__ onehot,
                                                             int* __restrict__ idx, int nc, int N, int Nq, long long total) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int q = (int)(t % Nq);
    const long long plane = t / Nq;                  // b * nc + c
    const int c = (int)(plane % nc);
    const long long b = plane / nc;
    const int p0 = q * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    int li[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        li[e] = -1;
        if (p0 + e < N) {
            const long long l = lab[b * N + p0 + e];
            li[e] = (l >= 0 && l < nc) ? (int)l : -1;
            v[e] = li[e] == c ? 1.f : 0.f;
        }
    }
    float* o = onehot + plane * N + p0;
    int* ib = idx + b * N + p0;
    if (VEC) {
        *reinterpret_cast<f32x4*>(o) = v;            // (N % 4 == 0: the quad is inside as a whole)
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (p0 + e < N) o[e] = v[e];
    }
    if (c == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (p0 + e < N) ib[e] = li[e];
    }
}

// ---- tap table --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void label_conv_table_kernel(const float* __restrict__ w, float* __restrict__ wt, int Cout, int nc,
                                                               long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;       // index into Wt [9][nc][Cout]
    if (i >= total) return;
    const int o = (int)(i % Cout);
    const long long r = i / Cout;
    const int l = (int)(r % nc), tap = (int)(r / nc);
    wt[i] = w[((long long)o * nc + l) * 9 + tap];
}

// The class under tap (dy, dx) of output pixel (y, x), or -1: outside the zero padding, or a pixel without a class.
__device__ __forceinline__ int lc_tap_label(const int* __restrict__ idx_b, int Ws, int H, int W, int s, int reflect, int nc, int y, int x,
                                            int dy, int dx) {
    int yy = y + dy, xx = x + dx;
    if (reflect) {                                    // ReflectionPad2d(1): -1 -> 1, H -> H - 2   (H, W >= 2)
        yy = yy < 0 ? -yy : (yy >= H ? 2 * H - 2 - yy : yy);
        xx = xx < 0 ? -xx : (xx >= W ? 2 * W - 2 - xx : xx);
    } else if (yy < 0 || yy >= H || xx < 0 || xx >= W) {
        return -1;
    }
    const int l = idx_b[(long long)yy * s * Ws + (long long)xx * s];
    return (unsigned)l < (unsigned)nc ? l : -1;       // (an index map is -1 or a class; anything else reads nothing)
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void label_conv3x3_fwd_kernel(const int* __restrict__ idx, const float* __restrict__ wt,
                                                                const float* __restrict__ bias, float* __restrict__ y,
                                                                unsigned* __restrict__ amax, int B, int Hs, int Ws, int H, int W, int s,
                                                                int reflect, int relu, int nc, int Cout, long long total) {
    __shared__ float redm[4];
    const int tid = threadIdx.x;
    const long long t = (long long)blockIdx.x * 256 + tid;
    const int c0 = blockIdx.y * LC_CH;
    const int Wq = (W + 3) >> 2;
    float vmax = 0.f;
    if (t < total) {
        const int xq = (int)(t % Wq);
        const long long r = t / Wq;
        const int yy = (int)(r % H);
        const int b = (int)(r / H);
        const int x0 = xq * 4;
        const int* idx_b = idx + (long long)b * Hs * Ws;
        int lab[4][9];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
                lab[e][tap] = x0 + e < W ? lc_tap_label(idx_b, Ws, H, W, s, reflect, nc, yy, x0 + e, tap / 3 - 1, tap % 3 - 1) : -1;
        float* yb = y + (((long long)b * Cout + c0) * H + yy) * W + x0;
        const long long plane = (long long)H * W;
#pragma unroll 1
        for (int cc = 0; cc < LC_CH; cc += 4) {
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (bias) bv = *reinterpret_cast<const f32x4*>(bias + c0 + cc);
            f32x4 acc[4] = {bv, bv, bv, bv};
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (lab[e][tap] >= 0)
                        acc[e] += *reinterpret_cast<const f32x4*>(wt + ((long long)tap * nc + lab[e][tap]) * Cout + c0 + cc);
#pragma unroll
            for (int k = 0; k < 4; ++k) {             // channel c0 + cc + k: the four pixels of the lane
                f32x4 o = {acc[0][k], acc[1][k], acc[2][k], acc[3][k]};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (relu) o[e] = fmaxf(o[e], 0.f);
                    if (x0 + e < W) vmax = fmaxf(vmax, fabsf(o[e]));
                }
                float* yo = yb + (long long)(cc + k) * plane;
                if (VEC) {
                    *reinterpret_cast<f32x4*>(yo) = o;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (x0 + e < W) yo[e] = o[e];
                }
            }
        }
    }
    if (amax) {
        vmax = wave_max_dpp(vmax);
        if ((tid & 63) == 0) redm[tid >> 6] = vmax;
        __syncthreads();
        if (tid == 0) {
            const float m = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
            if (m > 0.f && m < INFINITY) atomicMax(amax, __float_as_uint(m));      // >= 0: ordered as integers
        }
    }
}

// ---- backward, launch 1: per-slice partial sums -------------------------------------------------------------------------------------
// grid (slices, Cout / 16, class windows).  part [slices][9][nc][Cout], db_part [slices][Cout] (window 0 writes it).
__global__ __launch_bounds__(LC_BWD_THREADS) void label_conv3x3_bwd_part_kernel(
    const int* __restrict__ idx, const float* __restrict__ dy, const float* __restrict__ ysaved, float* __restrict__ part,
    float* __restrict__ db_part, int B, int Hs, int Ws, int H, int W, int s, int reflect, int nc, int Cout, long long NP, long long SL,
    int LCW) {
    extern __shared__ __attribute__((aligned(16))) float lc_smem[];
    float* acc = lc_smem;                                         // [9][LCW][16]
    float* dyt = acc + 9 * LCW * LC_CH;                           // [64 pixels][16 channels]
    int* labt = reinterpret_cast<int*>(dyt + LC_BWD_TILE * LC_CH);  // [9][64 pixels]: class relative to the window, or -1
    const int tid = threadIdx.x;
    const int c0 = blockIdx.y * LC_CH;
    const int l0 = blockIdx.z * LCW;
    const int lw = min(LCW, nc - l0);                             // classes of this window
    const long long g0 = (long long)blockIdx.x * SL, g1 = min(NP, g0 + SL);
    const long long plane = (long long)H * W;
    for (int i = tid; i < 9 * LCW * LC_CH; i += LC_BWD_THREADS) acc[i] = 0.f;
    const bool worker = tid < 9 * LC_CH;
    const int tap = tid >> 4, o = tid & 15;                       // (worker threads)
    int cur = -1;                                                 // class of the run in progress (relative), -1: none
    float run = 0.f, dbsum = 0.f;
    for (long long t0 = g0; t0 < g1; t0 += LC_BWD_TILE) {
        const int np = (int)min((long long)LC_BWD_TILE, g1 - t0);
        __syncthreads();                                          // (the zeroing above; the previous tile has been read)
        for (int e = tid; e < LC_BWD_TILE * LC_CH; e += LC_BWD_THREADS) {
            const int c = e >> 6, p = e & 63;                     // consecutive lanes on consecutive pixels
            float v = 0.f;
            if (p < np) {
                const long long g = t0 + p;
                const long long b = g / plane, r = g - b * plane;
                const long long a = (b * Cout + c0 + c) * plane + r;
                v = dy[a];
                if (ysaved && !(ysaved[a] > 0.f)) v = 0.f;        // the fused ReLU: masked where the saved output is <= 0
            }
            dyt[p * LC_CH + c] = v;
        }
        for (int e = tid; e < 9 * LC_BWD_TILE; e += LC_BWD_THREADS) {
            const int tp = e >> 6, p = e & 63;
            int l = -1;
            if (p < np) {
                const long long g = t0 + p;
                const long long b = g / plane, r = g - b * plane;
                const int yy = (int)(r / W), xx = (int)(r - (long long)yy * W);
                l = lc_tap_label(idx + b * Hs * Ws, Ws, H, W, s, reflect, nc, yy, xx, tp / 3 - 1, tp % 3 - 1) - l0;
                if (l < 0 || l >= lw) l = -1;
            }
            labt[e] = l;
        }
        __syncthreads();
        if (worker) {
#pragma unroll 8
            for (int p = 0; p < np; ++p) {
                const int l = labt[tap * LC_BWD_TILE + p];
                const float v = dyt[p * LC_CH + o];
                if (l != cur) {
                    if (cur >= 0) acc[(tap * LCW + cur) * LC_CH + o] += run;
                    cur = l;
                    run = 0.f;
                }
                run += v;
                dbsum += v;
            }
        }
    }
    if (worker && cur >= 0) acc[(tap * LCW + cur) * LC_CH + o] += run;
    __syncthreads();
    float* pb = part + (long long)blockIdx.x * 9 * nc * Cout;
    for (int i = tid; i < 9 * lw * LC_CH; i += LC_BWD_THREADS) {
        const int oo = i & 15, r = i >> 4;
        const int l = r % lw, tp = r / lw;
        pb[((long long)tp * nc + l0 + l) * Cout + c0 + oo] = acc[(tp * LCW + l) * LC_CH + oo];
    }
    if (db_part && blockIdx.z == 0 && worker && tap == 4) db_part[(long long)blockIdx.x * Cout + c0 + o] = dbsum;
}

// ---- backward, launch 2: the slices added in slice order; dW back in [Cout][nc][3][3] -------------------------------------------------
__global__ __launch_bounds__(256) void label_conv3x3_bwd_reduce_kernel(const float* __restrict__ part, const float* __restrict__ db_part,
                                                                       float* __restrict__ dw, float* __restrict__ db, int S, int nc,
                                                                       int Cout, long long nW) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;       // index into one slice's [9][nc][Cout], then the Cout of db
    if (i < nW) {
        float v = 0.f;
        for (int sl = 0; sl < S; ++sl) v += part[(long long)sl * nW + i];
        const int o = (int)(i % Cout);
        const long long r = i / Cout;
        const int l = (int)(r % nc), tap = (int)(r / nc);
        dw[((long long)o * nc + l) * 9 + tap] = v;
    } else if (db && i < nW + Cout) {
        const int o = (int)(i - nW);
        float v = 0.f;
        for (int sl = 0; sl < S; ++sl) v += db_part[(long long)sl * Cout + o];
        db[o] = v;
    }
}

}  // namespace cocos

// ---- host side --------------------------------------------------------------------------------------------------------------------
namespace {

struct LcBwdPlan {
    long long NP, SL;
    int S, LCW, windows;
    size_t smem;
};

LcBwdPlan lc_bwd_plan(int B, int H, int W, int nc, int Cout) {
    using namespace cocos;
    LcBwdPlan p;
    p.NP = (long long)B * H * W;
    const long long per_slice = 9ll * nc * Cout * 4;
    long long S = (p.NP + 255) / 256;                            // at least 256 pixels per slice
    S = std::min<long long>(S, LC_BWD_MAX_SLICES);
    S = std::min<long long>(S, std::max<long long>(1, LC_BWD_PART_BYTES / per_slice));
    S = std::max<long long>(S, 1);
    p.SL = ((p.NP + S - 1) / S + LC_BWD_TILE - 1) / LC_BWD_TILE * LC_BWD_TILE;
    p.S = (int)((p.NP + p.SL - 1) / p.SL);
    p.LCW = std::min(nc, LC_BWD_CLASSES);
    p.windows = (nc + p.LCW - 1) / p.LCW;
    p.smem = ((size_t)9 * p.LCW * LC_CH + (size_t)LC_BWD_TILE * LC_CH + (size_t)9 * LC_BWD_TILE) * 4;
    return p;
}

int lc_check_shape(const char* who, int B, int Hs, int Ws, int sample, int reflect, int nc, int Cout) {
    COCOS_REQUIRE(B >= 1 && Hs >= 1 && Ws >= 1 && sample >= 1, COCOS_ERR_INVALID, "%s: bad dims B=%d Hs=%d Ws=%d sample=%d", who, B, Hs, Ws,
                  sample);
    COCOS_REQUIRE(reflect == 0 || reflect == 1, COCOS_ERR_INVALID, "%s: padding mode %d (0 zero, 1 reflect)", who, reflect);
    COCOS_REQUIRE(nc >= 1 && nc <= 32767, COCOS_ERR_UNSUPPORTED, "%s: 1 <= nc <= 32767 expected, got %d", who, nc);
    COCOS_REQUIRE(Cout >= 16 && Cout % 16 == 0 && Cout / 16 <= 65535, COCOS_ERR_UNSUPPORTED, "%s: Cout %% 16 == 0 expected, got %d", who, Cout);
    COCOS_REQUIRE(Hs % sample == 0 && Ws % sample == 0, COCOS_ERR_UNSUPPORTED, "%s: %dx%d is not a multiple of the sampling step %d", who, Hs,
                  Ws, sample);
    COCOS_REQUIRE(!reflect || (Hs / sample >= 2 && Ws / sample >= 2), COCOS_ERR_UNSUPPORTED, "%s: reflect padding needs a grid of 2x2 or more", who);
    COCOS_REQUIRE((long long)B * Cout * (Hs / sample) * (Ws / sample) < (1ll << 40) && (long long)B * Hs * Ws < (1ll << 31),
                  COCOS_ERR_UNSUPPORTED, "%s: tensor too large", who);
    return COCOS_OK;
}

}  // namespace

extern "C" int cocos_labels_one_hot(const long long* label_map, float* onehot, int* index, int B, int nc, int H, int W,
                                    cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(label_map && onehot && index, COCOS_ERR_INVALID, "labels_one_hot: null pointer");
    COCOS_REQUIRE(B >= 1 && H >= 1 && W >= 1, COCOS_ERR_INVALID, "labels_one_hot: bad dims B=%d H=%d W=%d", B, H, W);
    COCOS_REQUIRE(nc >= 1 && nc <= 32767, COCOS_ERR_UNSUPPORTED, "labels_one_hot: 1 <= nc <= 32767 expected, got %d", nc);
    const long long N = (long long)H * W;
    COCOS_REQUIRE(N <= 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "labels_one_hot: plane too large");
    const long long Nq = (N + 3) / 4, total = (long long)B * nc * Nq, blocks = (total + 255) / 256;
    COCOS_REQUIRE(blocks <= 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "labels_one_hot: tensor too large for one launch");
    const bool vec = N % 4 == 0 && aligned16(onehot);
    const dim3 grid((unsigned)blocks), block(256);
    if (vec) hipLaunchKernelGGL(labels_one_hot_kernel<true>, grid, block, 0, as_stream(stream), label_map, onehot, index, nc, (int)N, (int)Nq, total);
    else     hipLaunchKernelGGL(labels_one_hot_kernel<false>, grid, block, 0, as_stream(stream), label_map, onehot, index, nc, (int)N, (int)Nq, total);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_label_conv_table(const float* weight, float* table, int Cout, int nc, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(weight && table, COCOS_ERR_INVALID, "label_conv_table: null pointer");
    COCOS_REQUIRE(Cout >= 1 && nc >= 1 && nc <= 32767, COCOS_ERR_INVALID, "label_conv_table: bad dims Cout=%d nc=%d", Cout, nc);
    const long long total = 9ll * nc * Cout, blocks = (total + 255) / 256;
    COCOS_REQUIRE(blocks <= 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "label_conv_table: weight too large");
    hipLaunchKernelGGL(label_conv_table_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), weight, table, Cout, nc, total);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_label_conv3x3_fwd(const int* index, const float* table, const float* bias, float* y, float* y_amax_inout_dev, int B,
                                       int Hs, int Ws, int sample, int reflect, int relu, int nc, int Cout, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(index && table && y, COCOS_ERR_INVALID, "label_conv3x3_fwd: null pointer");
    if (int rc = lc_check_shape("label_conv3x3_fwd", B, Hs, Ws, sample, reflect, nc, Cout)) return rc;
    COCOS_REQUIRE(aligned16(table) && (!bias || aligned16(bias)), COCOS_ERR_INVALID, "label_conv3x3_fwd: table and bias must be 16-byte aligned");
    const int H = Hs / sample, W = Ws / sample;
    const long long total = (long long)B * H * ((W + 3) / 4), blocks = (total + 255) / 256;
    const bool vec = W % 4 == 0 && aligned16(y);
    const dim3 grid((unsigned)blocks, (unsigned)(Cout / LC_CH)), block(256);
    unsigned* cell = reinterpret_cast<unsigned*>(y_amax_inout_dev);
    if (vec) hipLaunchKernelGGL(label_conv3x3_fwd_kernel<true>, grid, block, 0, as_stream(stream), index, table, bias, y, cell, B, Hs, Ws, H, W,
                                sample, reflect, relu ? 1 : 0, nc, Cout, total);
    else     hipLaunchKernelGGL(label_conv3x3_fwd_kernel<false>, grid, block, 0, as_stream(stream), index, table, bias, y, cell, B, Hs, Ws, H, W,
                                sample, reflect, relu ? 1 : 0, nc, Cout, total);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" size_t cocos_label_conv3x3_bwd_workspace_floats(int B, int H, int W, int nc, int Cout) {
    if (B < 1 || H < 1 || W < 1 || nc < 1 || nc > 32767 || Cout < 1) return 0;
    const LcBwdPlan p = lc_bwd_plan(B, H, W, nc, Cout);
    return (size_t)p.S * ((size_t)9 * nc * Cout + (size_t)Cout);
}

extern "C" int cocos_label_conv3x3_bwd(const int* index, const float* dy, const float* y_saved, float* dweight, float* dbias,
                                       float* workspace, int B, int Hs, int Ws, int sample, int reflect, int nc, int Cout,
                                       cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(index && dy && dweight && workspace, COCOS_ERR_INVALID, "label_conv3x3_bwd: null pointer");
    if (int rc = lc_check_shape("label_conv3x3_bwd", B, Hs, Ws, sample, reflect, nc, Cout)) return rc;
    const int H = Hs / sample, W = Ws / sample;
    const LcBwdPlan p = lc_bwd_plan(B, H, W, nc, Cout);
    const long long nW = 9ll * nc * Cout;
    float* part = workspace;
    float* db_part = workspace + (size_t)p.S * (size_t)nW;
    hipStream_t s = as_stream(stream);
    auto kern = label_conv3x3_bwd_part_kernel;
    COCOS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.smem));
    hipLaunchKernelGGL(kern, dim3((unsigned)p.S, (unsigned)(Cout / LC_CH), (unsigned)p.windows), dim3(LC_BWD_THREADS), p.smem, s, index, dy,
                       y_saved, part, db_part, B, Hs, Ws, H, W, sample, reflect, nc, Cout, p.NP, p.SL, p.LCW);
    COCOS_HIP_CHECK(hipGetLastError());
    const long long blocks = (nW + Cout + 255) / 256;
    hipLaunchKernelGGL(label_conv3x3_bwd_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, part, db_part, dweight, dbias, p.S, nc, Cout, nW);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
