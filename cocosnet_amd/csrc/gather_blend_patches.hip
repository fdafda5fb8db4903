// K39c: the k-sparse warp at full resolution — between K36c's winner-takes-all copy and correspondence.py:318's averaged warp_out:
//   out[b,c,y*down+dy,x*down+dx] = sum_r w[b,r,y,x] * img[b_e,c,(j_r/wg)*down+dy,(j_r%wg)*down+dx],  j_r = idx[b,r,y,x],  b_e = b or 0.
#include "common.h"

namespace cocos {

// One thread per output element, as K36c (a 3-channel image and k <= 8 taps: nothing to tune).  fp32, fixed order: acc = w_0 p_0, then
// acc = fma(w_r, p_r, acc); k = 1 with w = 1 is K36c's copy bit for bit (1 * p is p).
__global__ __launch_bounds__(256) void gather_blend_patches_kernel(const float* __restrict__ img, const int* __restrict__ idx,
                                                                   const float* __restrict__ wgt, float* __restrict__ out,
                                                                   long long total, int C, int H, int W, int down, int k,
                                                                   long long img_bstride) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int X = (int)(e % W), Y = (int)((e / W) % H);
    const long long bc = e / ((long long)W * H);
    const int c = (int)(bc % C);
    const long long b = bc / C;
    const int w = W / down, h = H / down;
    const int x = X / down, y = Y / down;
    const long long cells = (long long)h * w;
    const long long cell = b * k * cells + (long long)y * w + x;            // rank r of this cell: + r * cells
    const float* const plane = img + b * img_bstride + (long long)c * H * W;
    float acc = 0.f;
    for (int r = 0; r < k; ++r) {
        int j = idx[cell + r * cells];
        j = min(max(j, 0), h * w - 1);                         // an index outside the grid reads the nearest valid cell
        const int sy = (j / w) * down + (Y - y * down), sx = (j % w) * down + (X - x * down);
        const float p = plane[(long long)sy * W + sx], wr = wgt[cell + r * cells];
        acc = r == 0 ? wr * p : __builtin_fmaf(wr, p, acc);
    }
    out[e] = acc;
}

}  // namespace cocos

extern "C" int cocos_gather_blend_patches(const float* img, const int* idx, const float* w, float* out, int B, int C, int H, int W,
                                          int down, int k, long long img_batch_stride, cocos_stream_t stream) {
    using namespace cocos;
    COCOS_REQUIRE(img && idx && w && out, COCOS_ERR_INVALID, "gather_blend_patches: null pointer");
    COCOS_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1 && down >= 1, COCOS_ERR_INVALID,
                  "gather_blend_patches: bad dims B=%d C=%d H=%d W=%d down=%d", B, C, H, W, down);
    COCOS_REQUIRE(k >= 1 && k <= COCOS_MATCH_TOPK_MAX, COCOS_ERR_INVALID, "gather_blend_patches: k=%d: expected 1 <= k <= %d", k,
                  COCOS_MATCH_TOPK_MAX);
    COCOS_REQUIRE(H % down == 0 && W % down == 0, COCOS_ERR_UNSUPPORTED,
                  "gather_blend_patches: H=%d and W=%d must be multiples of down=%d (the match grid is (H / down) x (W / down))", H, W, down);
    const long long per = (long long)C * H * W;
    COCOS_REQUIRE(img_batch_stride == 0 || img_batch_stride == per, COCOS_ERR_INVALID,
                  "gather_blend_patches: img_batch_stride %lld: expected 0 (one exemplar for all samples) or the dense %lld",
                  img_batch_stride, per);
    const long long total = per * B, blocks = (total + 255) / 256;
    COCOS_REQUIRE(blocks < 0x7fffffffll, COCOS_ERR_UNSUPPORTED, "gather_blend_patches: %lld elements", total);
    hipLaunchKernelGGL(gather_blend_patches_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), img, idx, w, out, total, C, H,
                       W, down, k, img_batch_stride);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
