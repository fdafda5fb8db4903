// The full-resolution warps at the end of every match route: each content cell (y, x) of an h x w grid receives the down x down
// exemplar patch of its match j = idx[b, y*w + x] (b_e = b, or 0 with one exemplar for all samples):
//   K36c  copy      out[b,c,y*down+dy,x*down+dx] = img[b_e,c,(j/w)*down+dy,(j%w)*down+dx]                 a bitwise copy
//   K39c  blend     out = sum_r w[b,r,y,x] * (that pixel of match j_r = idx[b,r,y,x])                       k <= 8 taps, fixed order
//   K44   sub-cell  out = the exemplar sampled bilinearly around the match moved by off[b, y*w + x] cells   (its own key grid)
//   K46   the gradient of K44's output to the offset
#include "sparse_row.h"      // wave_sum (the K46 reduction); common.h

namespace cocos {

// One output element of a [B, C, h*down, w*down] image: its sample, channel, row and column, its cell (y, x) of the h x w grid, the
// cell's flat index y*w + x and the pixel (ry, rx) inside the cell.
struct WarpPixel {
    long long b, pos;
    int c, Y, X, y, x, ry, rx;
};

__device__ __forceinline__ WarpPixel warp_pixel(long long e, int C, int H, int W, int w, int down) {
    WarpPixel p;
    p.X = (int)(e % W), p.Y = (int)((e / W) % H);
    const long long bc = e / ((long long)W * H);
    p.c = (int)(bc % C), p.b = bc / C;
    p.x = p.X / down, p.y = p.Y / down;
    p.pos = (long long)p.y * w + p.x;
    p.ry = p.Y - p.y * down, p.rx = p.X - p.x * down;
    return p;
}

// The match of one cell: an index outside the grid of `cells` reads the nearest valid cell.
__device__ __forceinline__ int clamped_match(const int* __restrict__ idx, long long at, int cells) {
    return min(max(idx[at], 0), cells - 1);
}

// Channel c of sample b's exemplar (img_bstride 0: one exemplar for all samples).
__device__ __forceinline__ const float* exemplar_plane(const float* __restrict__ img, long long b, long long img_bstride, int c, int H,
                                                       int W) {
    return img + b * img_bstride + (long long)c * H * W;
}

// One thread per output element (a 3-channel image and k <= 8 taps: nothing to tune).  WEIGHTED: fp32, fixed order: acc = w_0 p_0,
// then acc = fma(w_r, p_r, acc).  Not WEIGHTED: K36c's copy, the first tap assigned and never multiplied (1 * p is p for every
// finite p, but not for a NaN's payload: the copy is bitwise); wgt and k are not read.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void gather_blend_patches_kernel(const float* __restrict__ img, const int* __restrict__ idx,
                                                                   const float* __restrict__ wgt, float* __restrict__ out,
                                                                   long long total, int C, int h, int w, int down, int k,
                                                                   long long img_bstride) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int W = w * down, H = h * down, taps = WEIGHTED ? k : 1;
    const WarpPixel p = warp_pixel(e, C, H, W, w, down);
    const long long cells = (long long)h * w;
    const long long cell = p.b * taps * cells + p.pos;                      // rank r of this cell: + r * cells
    const float* const plane = exemplar_plane(img, p.b, img_bstride, p.c, H, W);
    float acc = 0.f;
    for (int r = 0; r < taps; ++r) {
        const int j = clamped_match(idx, cell + r * cells, h * w);
        const int sy = (j / w) * down + p.ry, sx = (j % w) * down + p.rx;
        const float px = plane[(long long)sy * W + sx];
        if (!WEIGHTED) {
            acc = px;
        } else {
            const float wr = wgt[cell + r * cells];
            acc = r == 0 ? wr * px : __builtin_fmaf(wr, px, acc);
        }
    }
    out[e] = acc;
}

// K44: cell (y, x) of the fh x fw content grid samples the exemplar (an hk x wk grid of down x down cells) bilinearly around its match
// moved by off[b, y*fw + x] = (off_x, off_y) cells.  For pixel (Y, X), r = (Y % down, X % down):
//   sx = (xk + off_x) * down + rx, clamped into [0, Wr - 1];  x0 = floor(sx), fx = sx - x0, x1 = min(x0 + 1, Wr - 1);  y likewise
//   out = top + fy * (bottom - top),  top = v00 + fx * (v01 - v00),  bottom = v10 + fx * (v11 - v10)
// Contraction is off: with off == 0 both weights are 0 and the result is v00, the copy (bit for bit for finite pixels other than -0).
// A non-finite offset makes the pixel NaN (the address then falls back to column / row 0: it stays in the image).
//
// floor(sx) and sx - floor(sx) of one axis without forming sx in fp32 (a sum near Wr would round the fraction away): the integer
// part `base` = xk * down + rx stays an integer, t = off * down is exact for a power-of-two `down` (one rounding of a value of a few
// cells otherwise), and t - floor(t) is exact.  Returns the fraction, the sample's lower pixel in `p0`; a position below 0 or at or
// above `side` - 1 is the border pixel with fraction 0 — the clamp of sx.  A NaN or infinite offset returns NaN (p0 = 0).
// `clamped`: the clamp of sx acted (K46: the sample does not move with the offset there).
__device__ __forceinline__ float subcell_split(float off, int base, int down, int side, int& p0, bool& clamped) {
#pragma clang fp contract(off)
    const float t = off * (float)down;
    const float ti = floorf(t);
    float f = t - ti;                                          // exact; NaN for a non-finite t
    const float lim = (float)(1 << 25);                        // |base| < 2^24 (the entry point checks the image sides): no overflow
    const int p = base + (int)fminf(fmaxf(ti, -lim), lim);    // (fmaxf(NaN, -lim) = -lim: p < 0, the first clamp)
    const bool low = p < 0, high = p >= side - 1;
    p0 = low ? 0 : (high ? side - 1 : p);
    clamped = low || high;
    if (clamped && f == f) f = 0.f;
    return f;
}

// The bilinear sample of one pixel: both axes split, the four taps read from the exemplar plane, the two row interpolations.
struct SubcellSample {
    float fx, fy, v00, v01, v10, v11, top, bottom;
    bool xc, yc;
};

__device__ __forceinline__ SubcellSample subcell_sample(const float* __restrict__ plane, float ox, float oy, int j, int ry, int rx, int hk,
                                                        int wk, int down) {
#pragma clang fp contract(off)
    const int Hr = hk * down, Wr = wk * down;
    SubcellSample s;
    int x0, y0;
    s.fx = subcell_split(ox, (j % wk) * down + rx, down, Wr, x0, s.xc);
    s.fy = subcell_split(oy, (j / wk) * down + ry, down, Hr, y0, s.yc);
    const int x1 = min(x0 + 1, Wr - 1), y1 = min(y0 + 1, Hr - 1);
    s.v00 = plane[(long long)y0 * Wr + x0], s.v01 = plane[(long long)y0 * Wr + x1];
    s.v10 = plane[(long long)y1 * Wr + x0], s.v11 = plane[(long long)y1 * Wr + x1];
    s.top = s.v00 + s.fx * (s.v01 - s.v00), s.bottom = s.v10 + s.fx * (s.v11 - s.v10);
    return s;
}

__global__ __launch_bounds__(256) void gather_patches_subcell_kernel(const float* __restrict__ img, const int* __restrict__ idx,
                                                                     const float* __restrict__ off, float* __restrict__ out,
                                                                     long long total, int C, int fh, int fw, int hk, int wk, int down,
                                                                     long long img_bstride) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const WarpPixel p = warp_pixel(e, C, fh * down, fw * down, fw, down);
    const long long cell = p.b * ((long long)fh * fw) + p.pos;
    const int j = clamped_match(idx, cell, hk * wk);
    const SubcellSample s = subcell_sample(exemplar_plane(img, p.b, img_bstride, p.c, hk * down, wk * down), off[cell * 2],
                                           off[cell * 2 + 1], j, p.ry, p.rx, hk, wk, down);
    out[e] = s.top + s.fy * (s.bottom - s.top);
}

// K46: the gradient of gather_patches_subcell_kernel's output to the offset, doff[b, cell] = sum over the cell's C down^2 pixels of
// dout * d out / d off.  The integer pixel and the fraction are formed exactly as the forward forms them (subcell_sample), and
//   d out / d off_x = down ((1 - fy) (v01 - v00) + fy (v11 - v10)),   d out / d off_y = down (bottom - top),
// each 0 where that axis' clamp acted (the sample left of 0, or at or beyond the last column / row: it does not move with the offset).
// At an exact integer off * down the segment [x0, x0 + 1] is used: the right derivative, consistent with floor.  A non-finite offset
// gives NaN.  One wave per cell, four per workgroup: lane l takes pixels l, l + 64, ... of the cell (channel outside, then row, then
// column), accumulates with written-out FMAs, the xor butterfly adds the 64 partial sums and `down` multiplies the total — a fixed
// order, no atomics.  The image gradient is not built.
constexpr int GSB_WAVES = 4;
constexpr int GSB_THREADS = GSB_WAVES * kWave;

__global__ __launch_bounds__(GSB_THREADS) void gather_patches_subcell_bwd_off_kernel(const float* __restrict__ img, const int* __restrict__ idx,
                                                                                    const float* __restrict__ off, const float* __restrict__ dout,
                                                                                    float* __restrict__ doff, long long cells, int C, int fh,
                                                                                    int fw, int hk, int wk, int down, long long img_bstride) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const long long cell = (long long)blockIdx.x * GSB_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (cell >= cells) return;                                 // (whole waves; the kernel has no barrier)
    const int H = fh * down, W = fw * down;
    const long long b = cell / ((long long)fh * fw);
    const int pos = (int)(cell - b * ((long long)fh * fw));
    const int y = pos / fw, x = pos - y * fw;
    const int j = clamped_match(idx, cell, hk * wk);
    const float ox = off[cell * 2], oy = off[cell * 2 + 1];
    const int per = down * down, n = C * per;
    float ax = 0.f, ay = 0.f;
    for (int t = lane; t < n; t += kWave) {
        const int c = t / per, ry = (t - c * per) / down, rx = t - c * per - ry * down;
        const SubcellSample s = subcell_sample(exemplar_plane(img, b, img_bstride, c, hk * down, wk * down), ox, oy, j, ry, rx, hk, wk, down);
        // (a clamped axis contributes its fraction: 0, or the NaN of a non-finite offset)
        const float sx = s.xc ? s.fx : (1.f - s.fy) * (s.v01 - s.v00) + s.fy * (s.v11 - s.v10);
        const float sy = s.yc ? s.fy : s.bottom - s.top;
        const float g = dout[((b * C + c) * H + (long long)(y * down + ry)) * W + x * down + rx];
        ax = __builtin_fmaf(g, sx, ax);
        ay = __builtin_fmaf(g, sy, ay);
    }
    ax = wave_sum(ax) * (float)down;
    ay = wave_sum(ay) * (float)down;
    if (lane == 0) {
        doff[cell * 2] = ax;
        doff[cell * 2 + 1] = ay;
    }
}

// What the four entry points require alike, refused in the order and the words they always were: the pointers (`have`), positive
// sizes, the entry point's `own` requirements, the exemplar's batch stride and, with `total` (the output's elements, returned), a
// launch of one thread per element below 2^31 workgroups.  The copy and the blend have one grid for both sides and give the image
// sides H and W; the sub-cell pair names its pointers, gives the content grid and a key grid (hk, wk) of its own.
template <class Own>
static int check_gather_warp(const char* name, bool have, const char* pointers, int B, int C, int gh, int gw, int hk, int wk, int down,
                             Own own, long long img_batch_stride, long long* total) {
    if (pointers) {
        COCOS_REQUIRE(have, COCOS_ERR_INVALID, "%s: null pointer (%s)", name, pointers);
        COCOS_REQUIRE(B >= 1 && C >= 1 && gh >= 1 && gw >= 1 && hk >= 1 && wk >= 1 && down >= 1, COCOS_ERR_INVALID,
                      "%s: non-positive size: B=%d C=%d fh=%d fw=%d hk=%d wk=%d down=%d", name, B, C, gh, gw, hk, wk, down);
    } else {
        COCOS_REQUIRE(have, COCOS_ERR_INVALID, "%s: null pointer", name);
        COCOS_REQUIRE(B >= 1 && C >= 1 && gh >= 1 && gw >= 1 && down >= 1, COCOS_ERR_INVALID, "%s: bad dims B=%d C=%d H=%d W=%d down=%d",
                      name, B, C, gh, gw, down);
    }
    if (const int rc = own()) return rc;
    const long long per = pointers ? (long long)C * hk * down * wk * down : (long long)C * gh * gw;
    COCOS_REQUIRE(img_batch_stride == 0 || img_batch_stride == per, COCOS_ERR_INVALID,
                  "%s: img_batch_stride %lld: expected 0 (one exemplar for all samples) or the dense %lld", name, img_batch_stride, per);
    if (total) {
        *total = pointers ? (long long)B * C * gh * down * gw * down : per * B;
        COCOS_REQUIRE((*total + 255) / 256 < 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "%s: %lld elements", name, *total);
    }
    return COCOS_OK;
}

// the sub-cell pair's sides: fp32 sample positions are exact below 2^24 pixels
static int check_subcell_sides(const char* name, int fh, int fw, int hk, int wk, int down) {
    const long long Hr = (long long)hk * down, Wr = (long long)wk * down, H = (long long)fh * down, W = (long long)fw * down;
    COCOS_REQUIRE(Hr < (1 << 24) && Wr < (1 << 24) && H < (1 << 24) && W < (1 << 24) && (long long)hk * wk < 0x7fffffffll &&
                      (long long)fh * fw < 0x7fffffffll,
                  COCOS_ERR_UNSUPPORTED, "%s: an image side of 2^24 pixels or more (fp32 sample positions are exact below it)", name);
    return COCOS_OK;
}

// The copy (w null: the first tap, assigned) and the blend (k taps weighted by w): one launch of gather_blend_patches_kernel.
static int launch_gather_blend(const char* name, bool weighted, const float* img, const int* idx, const float* w, float* out, int B, int C,
                               int H, int W, int down, int k, long long img_batch_stride, cocos_stream_t stream) {
    long long total;
    const auto own = [&] {
        COCOS_REQUIRE(!weighted || (k >= 1 && k <= COCOS_MATCH_TOPK_MAX), COCOS_ERR_INVALID, "%s: k=%d: expected 1 <= k <= %d", name, k,
                      COCOS_MATCH_TOPK_MAX);
        COCOS_REQUIRE(H % down == 0 && W % down == 0, COCOS_ERR_UNSUPPORTED,
                      "%s: H=%d and W=%d must be multiples of down=%d (the match grid is (H / down) x (W / down))", name, H, W, down);
        return (int)COCOS_OK;
    };
    if (const int rc = check_gather_warp(name, img && idx && out && (w || !weighted), nullptr, B, C, H, W, 0, 0, down, own,
                                         img_batch_stride, &total))
        return rc;
    const auto kernel = weighted ? gather_blend_patches_kernel<true> : gather_blend_patches_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), img, idx, w, out, total, C, H / down,
                       W / down, down, k, img_batch_stride);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

}  // namespace cocos

extern "C" int cocos_gather_patches(const float* img, const int* idx, float* out, int B, int C, int H, int W, int down,
                                    long long img_batch_stride, cocos_stream_t stream) {
    return cocos::launch_gather_blend("gather_patches", false, img, idx, nullptr, out, B, C, H, W, down, 1, img_batch_stride, stream);
}

extern "C" int cocos_gather_blend_patches(const float* img, const int* idx, const float* w, float* out, int B, int C, int H, int W,
                                          int down, int k, long long img_batch_stride, cocos_stream_t stream) {
    return cocos::launch_gather_blend("gather_blend_patches", true, img, idx, w, out, B, C, H, W, down, k, img_batch_stride, stream);
}

extern "C" int cocos_gather_patches_subcell(const float* img, const int* idx, const float* off, float* out, int B, int C, int fh, int fw,
                                            int hk, int wk, int down, long long img_batch_stride, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "gather_patches_subcell";
    long long total;
    if (const int rc = check_gather_warp(name, img && idx && off && out, "img, idx, off, out", B, C, fh, fw, hk, wk, down,
                                         [&] { return check_subcell_sides(name, fh, fw, hk, wk, down); }, img_batch_stride, &total))
        return rc;
    hipLaunchKernelGGL(gather_patches_subcell_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), img, idx, off,
                       out, total, C, fh, fw, hk, wk, down, img_batch_stride);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_gather_patches_subcell_bwd_off(const float* img, const int* idx, const float* off, const float* dout, float* doff,
                                                    int B, int C, int fh, int fw, int hk, int wk, int down, long long img_batch_stride,
                                                    cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "gather_patches_subcell_bwd_off";
    if (const int rc = check_gather_warp(name, img && idx && off && dout && doff, "img, idx, off, dout, doff", B, C, fh, fw, hk, wk, down,
                                         [&] { return check_subcell_sides(name, fh, fw, hk, wk, down); }, img_batch_stride, nullptr))
        return rc;
    const long long cells = (long long)B * fh * fw, blocks = (cells + GSB_WAVES - 1) / GSB_WAVES;      // one wave per cell
    COCOS_REQUIRE(blocks < 0x7fffffffll && (long long)C * down * down < 0x7fffffffll, COCOS_ERR_UNSUPPORTED,
                  "%s: %lld cells of %lld pixels", name, cells, (long long)C * down * down);
    hipLaunchKernelGGL(gather_patches_subcell_bwd_off_kernel, dim3((unsigned)blocks), dim3(GSB_THREADS), 0, as_stream(stream), img, idx, off,
                       dout, doff, cells, C, fh, fw, hk, wk, down, img_batch_stride);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
