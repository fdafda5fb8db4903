// K36c: the winner-takes-all warp at full resolution (the hard counterpart of correspondence.py:318's averaged warp_out):
//   out[b,c,y*down+dy,x*down+dx] = img[b_e,c,(j/w)*down+dy,(j%w)*down+dx],  j = idx[b, y*w + x],  b_e = b or 0.
#include "common.h"

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

}  // namespace cocos

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
