// K36c: the winner-takes-all warp at full resolution (the hard counterpart of correspondence.py:318's averaged warp_out):
//   out[b,c,y*down+dy,x*down+dx] = img[b_e,c,(j/w)*down+dy,(j%w)*down+dx],  j = idx[b, y*w + x],  b_e = b or 0.
#include "sparse_row.h"      // wave_sum (the K46 reduction); common.h

namespace cocos {

// Every content cell receives the down x down exemplar patch of its match, a bitwise copy.  One thread per output element (a 3-channel image: nothing to tune).
__global__ __launch_bounds__(256) void gather_patches_kernel(const float* __restrict__ img, const int* __restrict__ idx,
                                                             float* __restrict__ out, long long total, int C, int H, int W,
                                                             int down, long long img_bstride) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int X = (int)(e % W), Y = (int)((e / W) % H);
    const long long bc = e / ((long long)W * H);
    const int c = (int)(bc % C);
    const long long b = bc / C;
    const int w = W / down, h = H / down;
    const int x = X / down, y = Y / down;
    int j = idx[b * ((long long)h * w) + (long long)y * w + x];
    j = min(max(j, 0), h * w - 1);                             // an index outside the grid reads the nearest valid cell
    const int sy = (j / w) * down + (Y - y * down), sx = (j % w) * down + (X - x * down);
    out[e] = img[b * img_bstride + ((long long)c * H + sy) * W + sx];
}

// K44: the same warp at a SUB-CELL position — cell (y, x) of the fh x fw content grid samples the exemplar (an hk x wk grid of
// down x down cells) bilinearly around its match moved by off[b, y*fw + x] = (off_x, off_y) cells.  For pixel (Y, X), r = (Y % down, X % down):
//   sx = (xk + off_x) * down + rx, clamped into [0, Wr - 1];  x0 = floor(sx), fx = sx - x0, x1 = min(x0 + 1, Wr - 1);  y likewise
//   out = top + fy * (bottom - top),  top = v00 + fx * (v01 - v00),  bottom = v10 + fx * (v11 - v10)
// Contraction is off: with off == 0 both weights are 0 and the result is v00, gather_patches_kernel's copy (bit for bit for finite
// pixels other than -0).  A non-finite offset makes the pixel NaN (the address then falls back to column / row 0: it stays in the image).
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

__device__ __forceinline__ float subcell_split(float off, int base, int down, int side, int& p0) {
    bool clamped;
    return subcell_split(off, base, down, side, p0, clamped);
}

__global__ __launch_bounds__(256) void gather_patches_subcell_kernel(const float* __restrict__ img, const int* __restrict__ idx,
                                                                     const float* __restrict__ off, float* __restrict__ out,
                                                                     long long total, int C, int fh, int fw, int hk, int wk, int down,
                                                                     long long img_bstride) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int H = fh * down, W = fw * down, Hr = hk * down, Wr = wk * down;
    const int X = (int)(e % W), Y = (int)((e / W) % H);
    const long long bc = e / ((long long)W * H);
    const int c = (int)(bc % C);
    const long long b = bc / C;
    const int x = X / down, y = Y / down;
    const long long cell = b * ((long long)fh * fw) + (long long)y * fw + x;
    int j = idx[cell];
    j = min(max(j, 0), hk * wk - 1);                           // an index outside the grid reads the nearest valid cell
    const float ox = off[cell * 2], oy = off[cell * 2 + 1];
    int x0, y0;
    const float fx = subcell_split(ox, (j % wk) * down + (X - x * down), down, Wr, x0);
    const float fy = subcell_split(oy, (j / wk) * down + (Y - y * down), down, Hr, y0);
    const int x1 = min(x0 + 1, Wr - 1), y1 = min(y0 + 1, Hr - 1);
    const float* plane = img + b * img_bstride + (long long)c * Hr * Wr;
    const float v00 = plane[(long long)y0 * Wr + x0], v01 = plane[(long long)y0 * Wr + x1];
    const float v10 = plane[(long long)y1 * Wr + x0], v11 = plane[(long long)y1 * Wr + x1];
    const float top = v00 + fx * (v01 - v00), bottom = v10 + fx * (v11 - v10);
    out[e] = top + fy * (bottom - top);
}

// K46: the gradient of gather_patches_subcell_kernel's output to the offset, doff[b, cell] = sum over the cell's C down^2 pixels of
// dout * d out / d off.  The integer pixel and the fraction are formed exactly as the forward forms them (subcell_split), and
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
    const int H = fh * down, W = fw * down, Hr = hk * down, Wr = wk * down;
    const long long b = cell / ((long long)fh * fw);
    const int pos = (int)(cell - b * ((long long)fh * fw));
    const int y = pos / fw, x = pos - y * fw;
    int j = idx[cell];
    j = min(max(j, 0), hk * wk - 1);                           // an index outside the grid reads the nearest valid cell
    const float ox = off[cell * 2], oy = off[cell * 2 + 1];
    const int per = down * down, n = C * per;
    float ax = 0.f, ay = 0.f;
    for (int t = lane; t < n; t += kWave) {
        const int c = t / per, ry = (t - c * per) / down, rx = t - c * per - ry * down;
        int x0, y0;
        bool xc, yc;
        const float fx = subcell_split(ox, (j % wk) * down + rx, down, Wr, x0, xc);
        const float fy = subcell_split(oy, (j / wk) * down + ry, down, Hr, y0, yc);
        const int x1 = min(x0 + 1, Wr - 1), y1 = min(y0 + 1, Hr - 1);
        const float* plane = img + b * img_bstride + (long long)c * Hr * Wr;
        const float v00 = plane[(long long)y0 * Wr + x0], v01 = plane[(long long)y0 * Wr + x1];
        const float v10 = plane[(long long)y1 * Wr + x0], v11 = plane[(long long)y1 * Wr + x1];
        const float top = v00 + fx * (v01 - v00), bottom = v10 + fx * (v11 - v10);
        // (a clamped axis contributes its fraction: 0, or the NaN of a non-finite offset)
        const float sx = xc ? fx : (1.f - fy) * (v01 - v00) + fy * (v11 - v10);
        const float sy = yc ? fy : bottom - top;
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

}  // namespace cocos

extern "C" int cocos_gather_patches_subcell_bwd_off(const float* img, const int* idx, const float* off, const float* dout, float* doff,
                                                    int B, int C, int fh, int fw, int hk, int wk, int down, long long img_batch_stride,
                                                    cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "gather_patches_subcell_bwd_off";
    COCOS_REQUIRE(img && idx && off && dout && doff, COCOS_ERR_INVALID, "%s: null pointer (img, idx, off, dout, doff)", name);
    COCOS_REQUIRE(B >= 1 && C >= 1 && fh >= 1 && fw >= 1 && hk >= 1 && wk >= 1 && down >= 1, COCOS_ERR_INVALID,
                  "%s: non-positive size: B=%d C=%d fh=%d fw=%d hk=%d wk=%d down=%d", name, B, C, fh, fw, hk, wk, down);
    const long long Hr = (long long)hk * down, Wr = (long long)wk * down, H = (long long)fh * down, W = (long long)fw * down;
    COCOS_REQUIRE(Hr < (1 << 24) && Wr < (1 << 24) && H < (1 << 24) && W < (1 << 24) && (long long)hk * wk < 0x7fffffffll &&
                      (long long)fh * fw < 0x7fffffffll,
                  COCOS_ERR_UNSUPPORTED, "%s: an image side of 2^24 pixels or more (fp32 sample positions are exact below it)", name);
    const long long per = (long long)C * Hr * Wr;
    COCOS_REQUIRE(img_batch_stride == 0 || img_batch_stride == per, COCOS_ERR_INVALID,
                  "%s: img_batch_stride %lld: expected 0 (one exemplar for all samples) or the dense %lld", name, img_batch_stride, per);
    const long long cells = (long long)B * fh * fw, blocks = (cells + GSB_WAVES - 1) / GSB_WAVES;
    COCOS_REQUIRE(blocks < 0x7fffffffll && (long long)C * down * down < 0x7fffffffll, COCOS_ERR_UNSUPPORTED,
                  "%s: %lld cells of %lld pixels", name, cells, (long long)C * down * down);
    hipLaunchKernelGGL(gather_patches_subcell_bwd_off_kernel, dim3((unsigned)blocks), dim3(GSB_THREADS), 0, as_stream(stream), img, idx, off,
                       dout, doff, cells, C, fh, fw, hk, wk, down, img_batch_stride);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_gather_patches_subcell(const float* img, const int* idx, const float* off, float* out, int B, int C, int fh, int fw,
                                            int hk, int wk, int down, long long img_batch_stride, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "gather_patches_subcell";
    COCOS_REQUIRE(img && idx && off && out, COCOS_ERR_INVALID, "%s: null pointer (img, idx, off, out)", name);
    COCOS_REQUIRE(B >= 1 && C >= 1 && fh >= 1 && fw >= 1 && hk >= 1 && wk >= 1 && down >= 1, COCOS_ERR_INVALID,
                  "%s: non-positive size: B=%d C=%d fh=%d fw=%d hk=%d wk=%d down=%d", name, B, C, fh, fw, hk, wk, down);
    const long long Hr = (long long)hk * down, Wr = (long long)wk * down, H = (long long)fh * down, W = (long long)fw * down;
    COCOS_REQUIRE(Hr < (1 << 24) && Wr < (1 << 24) && H < (1 << 24) && W < (1 << 24) && (long long)hk * wk < 0x7fffffffll &&
                      (long long)fh * fw < 0x7fffffffll,
                  COCOS_ERR_UNSUPPORTED, "%s: an image side of 2^24 pixels or more (fp32 sample positions are exact below it)", name);
    const long long per = (long long)C * Hr * Wr;
    COCOS_REQUIRE(img_batch_stride == 0 || img_batch_stride == per, COCOS_ERR_INVALID,
                  "%s: img_batch_stride %lld: expected 0 (one exemplar for all samples) or the dense %lld", name, img_batch_stride, per);
    const long long total = (long long)B * C * H * W, blocks = (total + 255) / 256;
    COCOS_REQUIRE(blocks < 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "%s: %lld elements", name, total);
    hipLaunchKernelGGL(gather_patches_subcell_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), img, idx, off, out, total, C,
                       fh, fw, hk, wk, down, img_batch_stride);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_gather_patches(const float* img, const int* idx, float* out, int B, int C, int H, int W, int down,
                                    long long img_batch_stride, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(img && idx && out, COCOS_ERR_INVALID, "gather_patches: null pointer");
    COCOS_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1 && down >= 1, COCOS_ERR_INVALID,
                  "gather_patches: bad dims B=%d C=%d H=%d W=%d down=%d", B, C, H, W, down);
    COCOS_REQUIRE(H % down == 0 && W % down == 0, COCOS_ERR_UNSUPPORTED,
                  "gather_patches: H=%d and W=%d must be multiples of down=%d (the match grid is (H / down) x (W / down))", H, W, down);
    const long long per = (long long)C * H * W;
    COCOS_REQUIRE(img_batch_stride == 0 || img_batch_stride == per, COCOS_ERR_INVALID,
                  "gather_patches: img_batch_stride %lld: expected 0 (one exemplar for all samples) or the dense %lld", img_batch_stride, per);
    const long long total = per * B, blocks = (total + 255) / 256;
    COCOS_REQUIRE(blocks < 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "gather_patches: %lld elements", total);
    hipLaunchKernelGGL(gather_patches_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), img, idx, out, total, C, H, W,
                       down, img_batch_stride);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
