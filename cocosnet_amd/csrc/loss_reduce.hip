// K28: the loss block of the generator and discriminator steps as reduction kernels (gfx950).
//
// What Pix2PixModel runs between the networks' outputs and backward() (reference models/pix2pix_model.py:205-296,
// util/util.py:36-43, models/networks/loss.py:15-97) is a few dozen scalar-valued reductions.  Three families, each ONE launch
// for a whole group of tensors plus a one-workgroup finishing kernel inside the same C call:
//   pair_loss   up to 16 segments (a, b, n, inner, w, c_l1, c_mse):  c_l1 * mean(w[i / inner] * |a - b|) + c_mse * mean((a - b)^2)
//               (util.weighted_l1_loss, util.mse_loss, F.l1_loss / nn.L1Loss; `fm` + `perc` share one read of a VGG level)
//   gan_loss    up to 8 prediction tensors, the cases of GANLoss.loss, combined as GANLoss.__call__ combines a list
//   mask_nll    the warp-mask loss of pix2pix_model.py:261-276 without a host read: the classes present in the downsampled
//               reference label map are a 256-bit set in LDS, not a torch.unique + `in` loop
// Per-element arithmetic is fp32 in the framework's order (no contraction into fma: the pragma below); every sum is fp64 per
// lane -> wave -> workgroup -> one partial per workgroup, and the finishing kernel adds the partials in a fixed order.  No atomics
// on a value: the result is bitwise reproducible.  Nothing tensor-sized is saved; the backward kernels recompute a - b (or the
// weights) and write each gradient once.  The scalar upstream gradient is read from a device cell: no host synchronisation.
// Pure streaming: 16-byte loads where the pointers and `inner` allow it, a scalar route otherwise.
#include <algorithm>

#include "common.h"

#pragma clang fp contract(off)

namespace cocos {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr long long kElemsPerBlock = 256 * 16;      // what a workgroup is sized for: four 16-byte loads per lane and operand
constexpr int kMaxSegBlocks = 1024;                 // per segment: 256 CUs x 4 (the other segments of the launch fill the rest)
constexpr int kPairMax = COCOS_PAIR_LOSS_MAX_SEGMENTS;
constexpr int kGanMax = COCOS_GAN_LOSS_MAX_TENSORS;

// by-value kernel argument: the segments of one launch (964 bytes)
struct SegTable {
    const float* a[kPairMax];
    const float* b[kPairMax];
    const float* w[kPairMax];
    float* da[kPairMax];
    long long n[kPairMax];
    long long inner[kPairMax];
    float c1[kPairMax];        // pair: c_l1          gan: the constant label
    float c2[kPairMax];        // pair: c_mse
    int blk0[kPairMax + 1];    // first workgroup of each segment; blk0[nseg] = grid size
    int nseg;
};

int seg_blocks(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + kElemsPerBlock - 1) / kElemsPerBlock, kMaxSegBlocks)); }

// the alignment is tested in the kernel: the table's pointers are per segment
__device__ __forceinline__ bool dev_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// sum over the workgroup, result valid in thread 0; every thread of the block calls it
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = kWave / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
    __syncthreads();          // red may still be read from the previous call
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) s += red[k];
    return s;
}

__device__ __forceinline__ int find_segment(const SegTable& t) {
    int s = 0;
    while (s + 1 < t.nseg && (int)blockIdx.x >= t.blk0[s + 1]) ++s;
    return s;
}

// sample index of element i (only asked for when the segment has weights)
__device__ __forceinline__ long long sample_of(long long i, long long inner) {
    return (i | inner) >> 32 ? i / inner : (long long)((unsigned)i / (unsigned)inner);
}

// ---- pair loss --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pair_term(float a, float b, float w, bool has_w, double& s1, double& s2) {
    const float d = a - b;
    float t = fabsf(d);
    if (has_w) t = t * w;
    s1 += (double)t;
    s2 += (double)(d * d);
}

__global__ __launch_bounds__(kThreads) void pair_fwd_kernel(const SegTable t, double* __restrict__ partials) {
    __shared__ double red[kWaves];
    const int s = find_segment(t);
    const float* __restrict__ a = t.a[s];
    const float* __restrict__ b = t.b[s];
    const float* __restrict__ w = t.w[s];
    const long long n = t.n[s], inner = t.inner[s];
    const long long nblk = t.blk0[s + 1] - t.blk0[s], blk = (long long)blockIdx.x - t.blk0[s];
    const long long stride = nblk * kThreads, t0 = blk * kThreads + threadIdx.x;
    // with weights a 16-byte chunk must not straddle two samples (then inner | n leaves no scalar rest)
    const bool vec = dev_aligned16(a) && (!b || dev_aligned16(b)) && (!w || inner % 4 == 0);
    double s1 = 0.0, s2 = 0.0;
    long long done = 0;
    if (vec) {
        const long long n4 = n / 4, inner4 = w ? inner / 4 : 1;
        done = n4 * 4;
        for (long long i = t0; i < n4; i += stride) {
            const f32x4 va = reinterpret_cast<const f32x4*>(a)[i];
            const f32x4 vb = b ? reinterpret_cast<const f32x4*>(b)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
            const float wv = w ? w[sample_of(i, inner4)] : 1.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) pair_term(va[e], vb[e], wv, w != nullptr, s1, s2);
        }
    }
    for (long long i = done + t0; i < n; i += stride) {
        const float wv = w ? w[sample_of(i, inner)] : 1.f;
        pair_term(a[i], b ? b[i] : 0.f, wv, w != nullptr, s1, s2);
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (threadIdx.x == 0) {
        partials[2 * (size_t)blockIdx.x] = s1;
        partials[2 * (size_t)blockIdx.x + 1] = s2;
    }
}

// out[s][0] = c_l1 * S1 / n, out[s][1] = c_mse * S2 / n, out[nseg][.] = their sums over the segments (one rounding each)
__global__ __launch_bounds__(kThreads) void pair_finish_kernel(const SegTable t, const double* __restrict__ partials, float* __restrict__ out) {
    __shared__ double red[kWaves];
    double tot1 = 0.0, tot2 = 0.0;
    for (int s = 0; s < t.nseg; ++s) {
        double s1 = 0.0, s2 = 0.0;
        for (int k = t.blk0[s] + threadIdx.x; k < t.blk0[s + 1]; k += kThreads) {
            s1 += partials[2 * (size_t)k];
            s2 += partials[2 * (size_t)k + 1];
        }
        s1 = block_sum(s1, red);
        s2 = block_sum(s2, red);
        if (threadIdx.x == 0) {
            // a coefficient of exactly 0 switches its term off (an overflowing (a - b)^2 nobody asked for must not make 0 * inf)
            const double l1 = t.c1[s] != 0.f ? (double)t.c1[s] * (s1 / (double)t.n[s]) : 0.0;
            const double l2 = t.c2[s] != 0.f ? (double)t.c2[s] * (s2 / (double)t.n[s]) : 0.0;
            out[2 * s] = (float)l1;
            out[2 * s + 1] = (float)l2;
            tot1 += l1;
            tot2 += l2;
        }
    }
    if (threadIdx.x == 0) {
        out[2 * t.nseg] = (float)tot1;
        out[2 * t.nseg + 1] = (float)tot2;
    }
}

// da = g1 * c_l1 * w * sign(a - b) / n + g2 * c_mse * 2 (a - b) / n, formed in fp64 and rounded once; g1 / g2: the gradient of the
// segment's own cell plus that of the sum cell
__device__ __forceinline__ float pair_grad(float a, float b, double k1, double k2) {
    const float d = a - b;
    const double sg = d > 0.f ? 1.0 : (d < 0.f ? -1.0 : 0.0);
    return (float)(k2 != 0.0 ? k1 * sg + k2 * (double)d : k1 * sg);
}

__global__ __launch_bounds__(kThreads) void pair_bwd_kernel(const SegTable t, const float* __restrict__ gout) {
    const int s = find_segment(t);
    const float* __restrict__ a = t.a[s];
    const float* __restrict__ b = t.b[s];
    const float* __restrict__ w = t.w[s];
    float* __restrict__ da = t.da[s];
    const long long n = t.n[s], inner = t.inner[s];
    const long long nblk = t.blk0[s + 1] - t.blk0[s], blk = (long long)blockIdx.x - t.blk0[s];
    const long long stride = nblk * kThreads, t0 = blk * kThreads + threadIdx.x;
    const bool vec = dev_aligned16(a) && (!b || dev_aligned16(b)) && dev_aligned16(da) && (!w || inner % 4 == 0);
    long long done = 0;
    const double g1 = (double)gout[2 * s] + (double)gout[2 * t.nseg], g2 = (double)gout[2 * s + 1] + (double)gout[2 * t.nseg + 1];
    const double k1 = g1 * (double)t.c1[s] / (double)n, k2 = g2 * (double)t.c2[s] * 2.0 / (double)n;
    if (vec) {
        const long long n4 = n / 4, inner4 = w ? inner / 4 : 1;
        done = n4 * 4;
        for (long long i = t0; i < n4; i += stride) {
            const f32x4 va = reinterpret_cast<const f32x4*>(a)[i];
            const f32x4 vb = b ? reinterpret_cast<const f32x4*>(b)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
            const double kw = w ? k1 * (double)w[sample_of(i, inner4)] : k1;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = pair_grad(va[e], vb[e], kw, k2);
            reinterpret_cast<f32x4*>(da)[i] = o;
        }
    }
    for (long long i = done + t0; i < n; i += stride) {
        const double kw = w ? k1 * (double)w[sample_of(i, inner)] : k1;
        da[i] = pair_grad(a[i], b ? b[i] : 0.f, kw, k2);
    }
}

// ---- GAN loss ---------------------------------------------------------------------------------------------------------------
// one term of GANLoss.loss in fp32, the framework's operations in its order
__device__ __forceinline__ float gan_term(float x, int mode, float label) {
    switch (mode) {
        case COCOS_GAN_HINGE_D_REAL: return fminf(x - 1.f, 0.f);        // -mean(min(x - 1, 0)): the sign is applied to the mean
        case COCOS_GAN_HINGE_D_FAKE: return fminf(-x - 1.f, 0.f);
        case COCOS_GAN_NEG_MEAN:                                        // hinge for the generator, w with a real target
        case COCOS_GAN_MEAN: return x;                                  // w with a fake target
        case COCOS_GAN_LS: {
            const float d = x - label;
            return d * d;
        }
        default: {                                                      // BCE with logits against the constant label
            const float sp = fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x)));  // -log_sigmoid(x)
            return (1.f - label) * x + sp;
        }
    }
}
__device__ __forceinline__ double gan_sign(int mode) {
    return mode == COCOS_GAN_HINGE_D_REAL || mode == COCOS_GAN_HINGE_D_FAKE || mode == COCOS_GAN_NEG_MEAN ? -1.0 : 1.0;
}

// d loss / d x up to the factor g / (n T); a tie of torch.min gives each side half (the framework's rule)
__device__ __forceinline__ double gan_dterm(float x, int mode, float label) {
    switch (mode) {
        case COCOS_GAN_HINGE_D_REAL: {
            const float u = x - 1.f;
            return u < 0.f ? -1.0 : (u == 0.f ? -0.5 : 0.0);
        }
        case COCOS_GAN_HINGE_D_FAKE: {
            const float u = -x - 1.f;
            return u < 0.f ? 1.0 : (u == 0.f ? 0.5 : 0.0);
        }
        case COCOS_GAN_NEG_MEAN: return -1.0;
        case COCOS_GAN_MEAN: return 1.0;
        case COCOS_GAN_LS: return 2.0 * (double)(x - label);
        default: {                                                      // sigmoid(x) - label, the sigmoid without cancellation
            const float e = expf(-fabsf(x));
            const double sig = x >= 0.f ? 1.0 / (1.0 + (double)e) : (double)e / (1.0 + (double)e);
            return sig - (double)label;
        }
    }
}

__global__ __launch_bounds__(kThreads) void gan_fwd_kernel(const SegTable t, double* __restrict__ partials, int mode) {
    __shared__ double red[kWaves];
    const int s = find_segment(t);
    const float* __restrict__ x = t.a[s];
    const long long n = t.n[s];
    const long long nblk = t.blk0[s + 1] - t.blk0[s], blk = (long long)blockIdx.x - t.blk0[s];
    const long long stride = nblk * kThreads, t0 = blk * kThreads + threadIdx.x;
    const float label = t.c1[s];
    double acc = 0.0;
    long long done = 0;
    if (dev_aligned16(x)) {
        const long long n4 = n / 4;
        for (long long i = t0; i < n4; i += stride) {
            const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += (double)gan_term(v[e], mode, label);
        }
        done = n4 * 4;
    }
    for (long long i = done + t0; i < n; i += stride) acc += (double)gan_term(x[i], mode, label);
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// out[0] = (sum over the tensors of +-mean) / T
__global__ __launch_bounds__(kThreads) void gan_finish_kernel(const SegTable t, const double* __restrict__ partials, float* __restrict__ out, int mode) {
    __shared__ double red[kWaves];
    double tot = 0.0;
    for (int s = 0; s < t.nseg; ++s) {
        double acc = 0.0;
        for (int k = t.blk0[s] + threadIdx.x; k < t.blk0[s + 1]; k += kThreads) acc += partials[k];
        acc = block_sum(acc, red);
        tot += acc / (double)t.n[s];
    }
    if (threadIdx.x == 0) out[0] = (float)(gan_sign(mode) * tot / (double)t.nseg);
}

__global__ __launch_bounds__(kThreads) void gan_bwd_kernel(const SegTable t, const float* __restrict__ g, int mode) {
    const int s = find_segment(t);
    const float* __restrict__ x = t.a[s];
    float* __restrict__ dx = t.da[s];
    const long long n = t.n[s];
    const long long nblk = t.blk0[s + 1] - t.blk0[s], blk = (long long)blockIdx.x - t.blk0[s];
    const long long stride = nblk * kThreads, t0 = blk * kThreads + threadIdx.x;
    const float label = t.c1[s];
    const double k = (double)g[0] / ((double)n * (double)t.nseg);
    long long done = 0;
    if (dev_aligned16(x) && dev_aligned16(dx)) {
        const long long n4 = n / 4;
        for (long long i = t0; i < n4; i += stride) {
            const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (float)(k * gan_dterm(v[e], mode, label));
            reinterpret_cast<f32x4*>(dx)[i] = o;
        }
        done = n4 * 4;
    }
    for (long long i = done + t0; i < n; i += stride) dx[i] = (float)(k * gan_dterm(x[i], mode, label));
}

// ---- warp-mask loss ---------------------------------------------------------------------------------------------------------
constexpr int kMaskWords = COCOS_MASK_NLL_MAX_CLASSES / 32;
constexpr int kMaskPixPerBlock = kThreads * 4;
constexpr int kMaskChanPerBlock = 16;

// F.interpolate(scale_factor = 0.25, mode = 'nearest'): output size floor(H / 4), source index min(floor(4 * dst), H - 1)
__device__ __forceinline__ int nearest_src(int dst, int size) { return min(4 * dst, size - 1); }

// grid (chunks, B).  Every workgroup of sample b builds the set of classes present in b's downsampled reference map (LDS or),
// then weighs its own pixels; chunk 0 also leaves the set for the backward.
__global__ __launch_bounds__(kThreads) void mask_fwd_kernel(const float* __restrict__ p, const long long* __restrict__ gt,
                                                            const long long* __restrict__ ref, int nc, int H, int W, int Hr, int Wr,
                                                            double* __restrict__ partials, unsigned* __restrict__ present_out) {
    __shared__ unsigned present[kMaskWords];
    __shared__ double red[kWaves];
    const int b = blockIdx.y, h = H / 4, w = W / 4, hr = Hr / 4, wr = Wr / 4;
    if (threadIdx.x < kMaskWords) present[threadIdx.x] = 0u;
    __syncthreads();
    const long long* refb = ref + (size_t)b * Hr * Wr;
    for (int i = threadIdx.x; i < hr * wr; i += kThreads) {
        const int y = i / wr, x = i - y * wr;
        const long long c = refb[(size_t)nearest_src(y, Hr) * Wr + nearest_src(x, Wr)];
        if (c >= 0 && c < nc) atomicOr(&present[c >> 5], 1u << (c & 31));
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x < kMaskWords) present_out[b * kMaskWords + threadIdx.x] = present[threadIdx.x];
    const long long* gtb = gt + (size_t)b * H * W;
    const float* pb = p + (size_t)b * nc * h * w;
    double sl = 0.0, sw = 0.0;
    const int hw = h * w, end = min(hw, ((int)blockIdx.x + 1) * kMaskPixPerBlock);
    for (int i = blockIdx.x * kMaskPixPerBlock + threadIdx.x; i < end; i += kThreads) {
        const int y = i / w, x = i - y * w;
        const long long c = gtb[(size_t)nearest_src(y, H) * W + nearest_src(x, W)];
        if (c > 0 && c < nc && (present[c >> 5] >> (c & 31) & 1u)) {
            const float v = pb[(size_t)c * hw + i] + 1e-10f;
            sl += (double)(-logf(v));
            sw += 1.0;
        }
    }
    sl = block_sum(sl, red);
    sw = block_sum(sw, red);
    if (threadIdx.x == 0) {
        const size_t k = (size_t)b * gridDim.x + blockIdx.x;
        partials[2 * k] = sl;
        partials[2 * k + 1] = sw;
    }
}

// out[0] = sum / (sum_w + 1e-5), out[1] = sum_w
__global__ __launch_bounds__(kThreads) void mask_finish_kernel(const double* __restrict__ partials, int count, float* __restrict__ out) {
    __shared__ double red[kWaves];
    double sl = 0.0, sw = 0.0;
    for (int k = threadIdx.x; k < count; k += kThreads) {
        sl += partials[2 * (size_t)k];
        sw += partials[2 * (size_t)k + 1];
    }
    sl = block_sum(sl, red);
    sw = block_sum(sw, red);
    if (threadIdx.x == 0) {
        out[0] = (float)(sl / (sw + 1e-5));
        out[1] = (float)sw;
    }
}

// grid (pixel chunks, channel groups, B): dp[b, c, y, x] = -g / (sum_w + 1e-5) / (p + 1e-10) on the ground-truth channel of a
// weighted pixel, 0 everywhere else — the dense gradient in one pass
__global__ __launch_bounds__(kThreads) void mask_bwd_kernel(const float* __restrict__ p, const long long* __restrict__ gt,
                                                            const unsigned* __restrict__ present, const float* __restrict__ sum_w,
                                                            const float* __restrict__ g, float* __restrict__ dp, int nc, int H, int W) {
    const int b = blockIdx.z, h = H / 4, w = W / 4, hw = h * w;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= hw) return;
    const int y = i / w, x = i - y * w;
    const long long c = gt[(size_t)b * H * W + (size_t)nearest_src(y, H) * W + nearest_src(x, W)];
    const bool on = c > 0 && c < nc && (present[b * kMaskWords + (int)(c >> 5)] >> (c & 31) & 1u);
    const int c0 = blockIdx.y * kMaskChanPerBlock, c1 = min(nc, c0 + kMaskChanPerBlock);
    const size_t base = (size_t)b * nc * hw + i;
    float val = 0.f;
    if (on && c >= c0 && c < c1) {
        const double k = -(double)g[0] / ((double)sum_w[0] + 1e-5);
        val = (float)(k / (double)(p[base + (size_t)c * hw] + 1e-10f));
    }
    for (int ch = c0; ch < c1; ++ch) dp[base + (size_t)ch * hw] = on && ch == (int)c ? val : 0.f;
}

int mask_chunks(int h, int w) { return (h * w + kMaskPixPerBlock - 1) / kMaskPixPerBlock; }

// shared argument checks + table of the pair and GAN families; `what`: entry point name for the messages
int fill_table(SegTable& t, const char* what, int nseg, int max_seg, const float* const* a, const float* const* b, const float* const* w,
               float* const* da, const long long* n, const long long* inner, const float* c1, const float* c2, bool need_da) {
    COCOS_REQUIRE(nseg >= 1 && nseg <= max_seg, COCOS_ERR_INVALID, "%s: %d segments (1 ... %d)", what, nseg, max_seg);
    COCOS_REQUIRE(a && n, COCOS_ERR_INVALID, "%s: null table", what);
    int blocks = 0;
    for (int s = 0; s < nseg; ++s) {
        COCOS_REQUIRE(a[s], COCOS_ERR_INVALID, "%s: segment %d: null pointer", what, s);
        COCOS_REQUIRE(n[s] >= 1, COCOS_ERR_INVALID, "%s: segment %d: n=%lld", what, s, n[s]);
        const long long in = inner ? inner[s] : n[s];
        COCOS_REQUIRE(in >= 1 && n[s] % in == 0, COCOS_ERR_INVALID, "%s: segment %d: inner=%lld does not divide n=%lld", what, s, in, n[s]);
        COCOS_REQUIRE(!da || !da[s] || (da[s] != a[s] && (!b || da[s] != b[s])), COCOS_ERR_INVALID, "%s: segment %d: aliased gradient", what, s);
        t.a[s] = a[s];
        t.b[s] = b ? b[s] : nullptr;
        t.w[s] = w ? w[s] : nullptr;
        t.da[s] = da ? da[s] : nullptr;
        t.n[s] = n[s];
        t.inner[s] = in;
        t.c1[s] = c1 ? c1[s] : 0.f;
        t.c2[s] = c2 ? c2[s] : 0.f;
        t.blk0[s] = blocks;
        // a backward segment without a gradient pointer (an input that needs none) gets no workgroup
        if (!need_da || t.da[s]) blocks += seg_blocks(n[s]);
    }
    t.blk0[nseg] = blocks;
    t.nseg = nseg;
    return COCOS_OK;
}

}  // namespace
}  // namespace cocos

extern "C" int cocos_loss_partials(int nseg, const long long* n) {
    if (nseg < 1 || nseg > cocos::kPairMax || !n) return 0;
    int blocks = 0;
    for (int s = 0; s < nseg; ++s) blocks += n[s] >= 1 ? cocos::seg_blocks(n[s]) : 0;
    return blocks;
}

extern "C" int cocos_pair_loss_fwd(int nseg, const float* const* a, const float* const* b, const float* const* w, const long long* n,
                                   const long long* inner, const float* c_l1, const float* c_mse, double* partials, float* out,
                                   cocos_stream_t stream) {
    using namespace cocos;
    SegTable t = {};
    if (int rc = fill_table(t, "pair_loss_fwd", nseg, kPairMax, a, b, w, nullptr, n, inner, c_l1, c_mse, false)) return rc;
    COCOS_REQUIRE(c_l1 && c_mse && partials && out, COCOS_ERR_INVALID, "pair_loss_fwd: null pointer");
    hipLaunchKernelGGL(pair_fwd_kernel, dim3(t.blk0[nseg]), dim3(kThreads), 0, as_stream(stream), t, partials);
    COCOS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pair_finish_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), t, partials, out);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_pair_loss_bwd(int nseg, const float* const* a, const float* const* b, const float* const* w, float* const* da,
                                   const long long* n, const long long* inner, const float* c_l1, const float* c_mse, const float* gout,
                                   cocos_stream_t stream) {
    using namespace cocos;
    SegTable t = {};
    COCOS_REQUIRE(da && c_l1 && c_mse && gout, COCOS_ERR_INVALID, "pair_loss_bwd: null pointer");
    if (int rc = fill_table(t, "pair_loss_bwd", nseg, kPairMax, a, b, w, da, n, inner, c_l1, c_mse, true)) return rc;
    if (t.blk0[nseg] == 0) return COCOS_OK;
    // the workgroups of a segment without a gradient were dropped: find_segment() walks blk0, equal neighbours are skipped
    hipLaunchKernelGGL(pair_bwd_kernel, dim3(t.blk0[nseg]), dim3(kThreads), 0, as_stream(stream), t, gout);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_gan_loss_fwd(int nt, const float* const* x, const long long* n, int mode, float label, double* partials, float* out,
                                  cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(mode >= COCOS_GAN_HINGE_D_REAL && mode <= COCOS_GAN_BCE, COCOS_ERR_INVALID, "gan_loss_fwd: mode=%d", mode);
    SegTable t = {};
    if (int rc = fill_table(t, "gan_loss_fwd", nt, kGanMax, x, nullptr, nullptr, nullptr, n, nullptr, nullptr, nullptr, false)) return rc;
    COCOS_REQUIRE(partials && out, COCOS_ERR_INVALID, "gan_loss_fwd: null pointer");
    for (int s = 0; s < nt; ++s) t.c1[s] = label;
    hipLaunchKernelGGL(gan_fwd_kernel, dim3(t.blk0[nt]), dim3(kThreads), 0, as_stream(stream), t, partials, mode);
    COCOS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(gan_finish_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), t, partials, out, mode);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_gan_loss_bwd(int nt, const float* const* x, float* const* dx, const long long* n, int mode, float label,
                                  const float* g, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(mode >= COCOS_GAN_HINGE_D_REAL && mode <= COCOS_GAN_BCE, COCOS_ERR_INVALID, "gan_loss_bwd: mode=%d", mode);
    COCOS_REQUIRE(dx && g, COCOS_ERR_INVALID, "gan_loss_bwd: null pointer");
    SegTable t = {};
    if (int rc = fill_table(t, "gan_loss_bwd", nt, kGanMax, x, nullptr, nullptr, dx, n, nullptr, nullptr, nullptr, true)) return rc;
    if (t.blk0[nt] == 0) return COCOS_OK;
    for (int s = 0; s < nt; ++s) t.c1[s] = label;
    hipLaunchKernelGGL(gan_bwd_kernel, dim3(t.blk0[nt]), dim3(kThreads), 0, as_stream(stream), t, g, mode);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

namespace {
int mask_check(const char* what, int B, int nc, int H, int W) {
    COCOS_REQUIRE(B >= 1 && nc >= 1 && H >= 1 && W >= 1, COCOS_ERR_INVALID, "%s: B=%d nc=%d H=%d W=%d", what, B, nc, H, W);
    COCOS_REQUIRE(nc <= COCOS_MASK_NLL_MAX_CLASSES, COCOS_ERR_UNSUPPORTED, "%s: nc=%d (the class set holds %d)", what, nc,
                  COCOS_MASK_NLL_MAX_CLASSES);
    COCOS_REQUIRE(H >= 4 && W >= 4 && B <= 65535, COCOS_ERR_UNSUPPORTED, "%s: B=%d, %dx%d label map: nothing left at scale 0.25", what, B, H, W);
    COCOS_REQUIRE((long long)nc * (H / 4) * (W / 4) < (1ll << 31) && (long long)H * W < (1ll << 31), COCOS_ERR_UNSUPPORTED,
                  "%s: nc=%d H=%d W=%d exceeds the 32-bit index decode", what, nc, H, W);
    return COCOS_OK;
}
}  // namespace

extern "C" int cocos_mask_nll_partials(int B, int H, int W) {
    if (B < 1 || H < 4 || W < 4) return 0;
    return B * cocos::mask_chunks(H / 4, W / 4);
}

extern "C" int cocos_mask_nll_fwd(const float* p, const long long* gt, const long long* ref, int B, int nc, int H, int W, int Hr, int Wr,
                                  double* partials, unsigned* present, float* out, cocos_stream_t stream) {
    using namespace cocos;
    if (int rc = mask_check("mask_nll_fwd", B, nc, H, W)) return rc;
    COCOS_REQUIRE(Hr >= 1 && Wr >= 1, COCOS_ERR_INVALID, "mask_nll_fwd: Hr=%d Wr=%d", Hr, Wr);
    COCOS_REQUIRE(Hr >= 4 && Wr >= 4 && (long long)Hr * Wr < (1ll << 31), COCOS_ERR_UNSUPPORTED,
                  "mask_nll_fwd: reference label map %dx%d: nothing left at scale 0.25, or beyond the 32-bit index decode", Hr, Wr);
    COCOS_REQUIRE(p && gt && ref && partials && present && out, COCOS_ERR_INVALID, "mask_nll_fwd: null pointer");
    const int chunks = mask_chunks(H / 4, W / 4);
    hipLaunchKernelGGL(mask_fwd_kernel, dim3(chunks, B), dim3(kThreads), 0, as_stream(stream), p, gt, ref, nc, H, W, Hr, Wr, partials, present);
    COCOS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mask_finish_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), partials, B * chunks, out);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_mask_nll_bwd(const float* p, const long long* gt, const unsigned* present, const float* sum_w, const float* g, float* dp,
                                  int B, int nc, int H, int W, cocos_stream_t stream) {
    using namespace cocos;
    if (int rc = mask_check("mask_nll_bwd", B, nc, H, W)) return rc;
    COCOS_REQUIRE(p && gt && present && sum_w && g && dp && dp != p, COCOS_ERR_INVALID, "mask_nll_bwd: null or aliased pointer");
    const int hw = (H / 4) * (W / 4);
    const dim3 grid((hw + kThreads - 1) / kThreads, (nc + kMaskChanPerBlock - 1) / kMaskChanPerBlock, B);
    hipLaunchKernelGGL(mask_bwd_kernel, grid, dim3(kThreads), 0, as_stream(stream), p, gt, present, sum_w, g, dp, nc, H, W);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
