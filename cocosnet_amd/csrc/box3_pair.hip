// K51 / K52: the trainable sparse kernels of the match_kernel-3 route — a softmax over a few CANDIDATE keys per query, on the logit of
// the 3x3-unfolded, centred, normalised vectors taken for ONE pair (box3_rows.h: the pair core):
//   R[p,q] = sum over the taps d in {-1,0,1}^2 of [p+d inside the content grid] [q+d inside the exemplar grid] <theta[:,p+d], phi[:,q+d]>
//   c[p,q] = R[p,q] - kc mu_p nu_q,   z[p,q] = inv_t a_p b_q c[p,q],   kc = 9 * 256,   (mu, a), (nu, b) the K12 statistics
// Whether a tap is inside a grid is decided on the 2-D coordinates (y, x), never on the flat index: a key in the last column does not
// pick up the first cell of the next row.  Nothing here has an Nq x Nk extent.  What a candidate is, is a policy (`Set`, below):
//   K51  TopkSet    the k keys idx[b,p,:] (clamped into [0, Nk)) that the top-k readout (K41) selected; w = softmax over them,
//                   out[b,:,p] = sum_r w_r v[b,:,j_r] — the k-sparse correspondence warp.  State: w, c, g, hb, each [B,Nq,k].
//   K52  WindowSet  the keys INSIDE the exemplar grid of the (2 r + 1)^2 window around the centre idx[b,p] (one outside is left out:
//                   neither clamped nor wrapped); slot s = (dy + r) W1 + (dx + r), W1 = 2 r + 1, W = W1^2, visited dy ascending
//                   outside, dx ascending inside; the window soft-argmax (K44 / K46) — the sub-cell refinement.  State: c, g, hb,
//                   each [B,Nq,W].
// Operands are fp32 position-major rows [B,N,256] (cocos_transpose_f32 of the channel-major tensors).  One wave per row, four per
// workgroup; every sum has a fixed order, no atomics, no LDS: the results are bitwise reproducible.
//
//   forward, pair backward   one wave per query; K51 keeps per-candidate arrays and blends v, K52 keeps slot s in lane s (W <= 49 < 64)
//                    and reads the sums over the window through v_readlane, in visiting order: two kernels each, that difference is real
//   theta gradient   box3_pair_bwd_theta_kernel<Set>: one wave per content position m, a GATHER over the taps and that query's candidates
//   key gradient     one wave per exemplar position n, a GATHER over the inverse table of idx (K42's); two bodies on the shared accessors
// K52's kernels and the gathers are compiled with contraction off and every fused multiply-add written out; K51's forward and pair
// backward are not, and keep their x * y + z expressions in their own bodies (box3_rows.h has the rule).
#include "box3_rows.h"

namespace cocos {

constexpr int BP_MAXK = COCOS_MATCH_TOPK_MAX;

// ---- the candidate policies: which keys are the candidates of a query, in the route's order, and where each one's g lies; for the
// host, the route's own requirements (own) and the width of its tables ------------------------------------------------------------
// K51: the candidates of query prow are idx[prow k + r], r ascending, g at prow k + r.
struct TopkSet {
    const int* idx;
    int k;
    static constexpr int kTapUnroll = 9;      // (the tap loops' code shape, as each route always had it)
    static constexpr const char* kWidthName = "k";
    static constexpr const char* kWidthNoun = "entries";
    int width() const { return k; }             // g / hb entries per query
    template <class F>
    __device__ __forceinline__ void each_candidate(long long prow, int gh, int gw, F&& f) const {      // f(ky, kx, position in g)
        for (int r = 0; r < k; ++r) {
            const int j = clamp_key(idx[prow * k + r], gh * gw), ky = j / gw;
            f(ky, j - ky * gw, prow * k + r);
        }
    }
    // sizes, Cv and the temperature in one refusal, then k (the words and the order the K51 entry points always had)
    int own(const char* name, int B, int fh, int fw, int gh, int gw, int Cv, float inv_temperature) const {
        COCOS_REQUIRE(B >= 1 && fh >= 1 && fw >= 1 && gh >= 1 && gw >= 1 && Cv >= 1 && inv_temperature > 0.f, COCOS_ERR_INVALID,
                      "%s: bad dims B=%d content grid %dx%d exemplar grid %dx%d Cv=%d", name, B, fh, fw, gh, gw, Cv);
        const long long Nk = (long long)gh * gw;
        COCOS_REQUIRE(k >= 1 && k <= COCOS_MATCH_TOPK_MAX && k <= Nk, COCOS_ERR_INVALID, "%s: k=%d: expected 1 <= k <= min(%d, Nk=%lld)", name,
                      k, COCOS_MATCH_TOPK_MAX, Nk);
        return COCOS_OK;
    }
};

// K52: the candidates of query prow are the in-grid keys of the window around idx[prow], in visiting order, g at prow W + slot.
struct WindowSet {
    const int* idx;
    int r;
    static constexpr int kTapUnroll = 1;
    static constexpr const char* kWidthName = "W";
    static constexpr const char* kWidthNoun = "window slots";
    int width() const { return (2 * r + 1) * (2 * r + 1); }
    template <class F>
    __device__ __forceinline__ void each_candidate(long long prow, int gh, int gw, F&& f) const {
        const int W1 = 2 * r + 1, j = clamp_key(__builtin_amdgcn_readfirstlane(idx[prow]), gh * gw), yk = j / gw, xk = j - yk * gw;
        for (int wy = 0; wy < W1; ++wy) {
            const int ky = yk + wy - r;
            if (ky < 0 || ky >= gh) continue;
            for (int wx = 0; wx < W1; ++wx) {
                const int kx = xk + wx - r;
                if (kx < 0 || kx >= gw) continue;
                f(ky, kx, prow * (W1 * W1) + (wy * W1 + wx));
            }
        }
    }
    // sizes, the radius, the temperature: three refusals (the words and the order the K52 entry points always had)
    int own(const char* name, int B, int fh, int fw, int gh, int gw, int, float inv_temperature) const {
        COCOS_REQUIRE(B >= 1 && fh >= 1 && fw >= 1 && gh >= 1 && gw >= 1, COCOS_ERR_INVALID,
                      "%s: non-positive size: B=%d content grid %dx%d exemplar grid %dx%d", name, B, fh, fw, gh, gw);
        COCOS_REQUIRE(r >= 1 && r <= COCOS_MATCH_REFINE_MAX_RADIUS, COCOS_ERR_INVALID, "%s: radius=%d: expected 1 .. %d", name, r,
                      COCOS_MATCH_REFINE_MAX_RADIUS);
        COCOS_REQUIRE(inv_temperature > 0.f, COCOS_ERR_INVALID, "%s: inv_temperature must be positive", name);
        return COCOS_OK;
    }
};

// ---- K51: forward and pair backward -------------------------------------------------------------------------------------------------
//   w = softmax over r of z[p, j_r],   out^T[p] = sum_r w_r v^T[j_r];   c_r is kept: the backward's state
// BIAS (K54): w = softmax over r of z[p, j_r] + k_bias[b, j_r] — a flag on this one body, not a second unit; the bias is a constant of the
// softmax, so c, the saved w and the three backward entries serve both flavours.  A bias of zeros adds 0 to a rounded product: the bits
// of the unbiased forward.
template <bool BIAS>
__global__ __launch_bounds__(BOX3_THREADS) void box3_sparse_fwd_kernel(const float* __restrict__ th_t, const float* __restrict__ ph_t,
                                                                       const float* __restrict__ mu, const float* __restrict__ a,
                                                                       const float* __restrict__ nu, const float* __restrict__ b,
                                                                       const float* __restrict__ vt, const int* __restrict__ idx,
                                                                       float* __restrict__ out_t, float* __restrict__ w_out,
                                                                       float* __restrict__ c_out, long long rows, int fh, int fw, int gh,
                                                                       int gw, int Cv, int k, float inv_t, float kc,
                                                                       const float* __restrict__ k_bias) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * BOX3_WAVES + (threadIdx.x >> 6);    // b * Nq + p
    if (row >= rows) return;                                                          // (whole waves; the kernel has no barrier)
    const int Nq = fh * fw, Nk = gh * gw;
    const long long bq = row / Nq;
    const int p = (int)(row - bq * Nq), py = p / fw, px = p - py * fw;
    const long long kbase = bq * Nk;
    const QueryTaps taps = load_query_taps(th_t, row, py, px, fh, fw, lane);
    const float kmu = kc * mu[row], za = inv_t * a[row];
    long long key[BP_MAXK];
    float s[BP_MAXK];
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < BP_MAXK; ++r) {
        key[r] = kbase;
        s[r] = -INFINITY;
        if (r < k) {
            const int j = clamp_key(idx[row * k + r], Nk), qy = j / gw, qx = j - qy * gw;
            key[r] = kbase + j;
            const float c = pair_R(taps, ph_t, key[r], qy, qx, gh, gw, lane) - kmu * nu[key[r]];
            if (lane == r) c_out[row * k + r] = c;
            s[r] = za * b[key[r]] * c;
            if constexpr (BIAS) s[r] = s[r] + k_bias[key[r]];
            m = fmaxf(m, s[r]);
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < BP_MAXK; ++r) {
        s[r] = r < k ? expf(s[r] - m) : 0.f;
        sum += s[r];
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int r = 0; r < BP_MAXK; ++r) {
        s[r] *= inv;
        if (r < k && lane == r) w_out[row * k + r] = s[r];
    }
    for (int ch = lane; ch < Cv; ch += kWave) {
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < BP_MAXK; ++r)
            if (r < k) acc = __builtin_fmaf(s[r], vt[key[r] * Cv + ch], acc);
        out_t[row * Cv + ch] = acc;
    }
}

// dw_r = <dout^T[p], v^T[j_r]>, dz_r = w_r (dw_r - sum w dw).  hb_out, dmu_out, da_out may be null.
__global__ __launch_bounds__(BOX3_THREADS) void box3_sparse_bwd_pair_kernel(const float* __restrict__ vt, const float* __restrict__ dout_t,
                                                                            const int* __restrict__ idx, const float* __restrict__ w,
                                                                            const float* __restrict__ c, const float* __restrict__ a,
                                                                            const float* __restrict__ nu, const float* __restrict__ b,
                                                                            float* __restrict__ g_out, float* __restrict__ hb_out,
                                                                            float* __restrict__ dmu_out, float* __restrict__ da_out,
                                                                            long long rows, int Nq, int Nk, int Cv, int k, float inv_t,
                                                                            float kc) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * BOX3_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long long kbase = (row / Nq) * Nk;
    long long key[BP_MAXK];
    float wr[BP_MAXK], dw[BP_MAXK];
#pragma unroll
    for (int r = 0; r < BP_MAXK; ++r) {
        key[r] = kbase + (r < k ? clamp_key(idx[row * k + r], Nk) : 0);
        wr[r] = r < k ? w[row * k + r] : 0.f;
        dw[r] = 0.f;
    }
    for (int ch = lane; ch < Cv; ch += kWave) {
        const float go = dout_t[row * Cv + ch];
#pragma unroll
        for (int r = 0; r < BP_MAXK; ++r)
            if (r < k) dw[r] = __builtin_fmaf(go, vt[key[r] * Cv + ch], dw[r]);
    }
    float dot = 0.f;
#pragma unroll
    for (int r = 0; r < BP_MAXK; ++r) {
        if (r < k) dw[r] = wave_sum(dw[r]);
        dot = __builtin_fmaf(wr[r], dw[r], dot);
    }
    const float a_p = a[row];
    float gnu = 0.f, da = 0.f;
#pragma unroll
    for (int r = 0; r < BP_MAXK; ++r) {
        if (r < k) {
            const float c_r = c[row * k + r];
            const PairGrad pg = pair_grad(wr[r] * (dw[r] - dot) * inv_t, a_p, b[key[r]], c_r);
            gnu = __builtin_fmaf(pg.g, nu[key[r]], gnu);
            da = __builtin_fmaf(pg.ab, c_r, da);
            if (lane == r) {
                g_out[row * k + r] = pg.g;
                if (hb_out) hb_out[row * k + r] = pg.hb;
            }
        }
    }
    if (lane == 0) {
        if (dmu_out) dmu_out[row] = -kc * gnu;
        if (da_out) da_out[row] = da;
    }
}

// ---- K53: the logit head — TopkSet at k = 1 with the pair's logit itself as the output instead of a blend --------------------------
//   z[b,p] = inv_t a_p b_j (R[p,j] - kc mu_p nu_j),  j = idx[b,p];  a NEGATIVE idx (an unsupervised cell) gives z = 0 and c = 0, and the
//   pair backward gives it g = hb = dmu = da = 0.  c is kept: the backward's state.  The gathers are K51's (TopkSet{idx, 1}, the
//   inverse table of the clamped idx): a negative entry rides along as key 0 with a zero coefficient.
__global__ __launch_bounds__(BOX3_THREADS) void box3_pair_logit_fwd_kernel(const float* __restrict__ th_t, const float* __restrict__ ph_t,
                                                                           const float* __restrict__ mu, const float* __restrict__ a,
                                                                           const float* __restrict__ nu, const float* __restrict__ b,
                                                                           const int* __restrict__ idx, float* __restrict__ z_out,
                                                                           float* __restrict__ c_out, long long rows, int fh, int fw, int gh,
                                                                           int gw, float inv_t, float kc) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = wave_row();                                                 // b * Nq + p
    if (row >= rows) return;                                                          // (whole waves; the kernel has no barrier)
    const int Nq = fh * fw, Nk = gh * gw;
    const long long bq = row / Nq;
    const int p = (int)(row - bq * Nq), py = p / fw, px = p - py * fw;
    const int t = __builtin_amdgcn_readfirstlane(idx[row]);
    float c = 0.f, z = 0.f;
    if (t >= 0) {
        const int j = clamp_key(t, Nk), ky = j / gw, kx = j - ky * gw;
        const long long key = bq * Nk + j;
        const QueryTaps taps = load_query_taps(th_t, row, py, px, fh, fw, lane);
        c = pair_R(taps, ph_t, key, ky, kx, gh, gw, lane) - (kc * mu[row]) * nu[key];
        z = (inv_t * a[row]) * b[key] * c;
    }
    if (lane == 0) {
        z_out[row] = z;
        c_out[row] = c;
    }
}

// one THREAD per query: g = dz inv_t a_p b_j, hb = dz inv_t a_p c, dmu_p = -kc g nu_j, da_p = dz inv_t b_j c (pair_grad).  hb_out,
// dmu_out, da_out may be null.
__global__ __launch_bounds__(BOX3_THREADS) void box3_pair_logit_bwd_pair_kernel(const int* __restrict__ idx, const float* __restrict__ c,
                                                                                const float* __restrict__ a, const float* __restrict__ nu,
                                                                                const float* __restrict__ b, const float* __restrict__ dz,
                                                                                float* __restrict__ g_out, float* __restrict__ hb_out,
                                                                                float* __restrict__ dmu_out, float* __restrict__ da_out,
                                                                                long long rows, int Nq, int Nk, float inv_t, float kc) {
#pragma clang fp contract(off)
    const long long row = (long long)blockIdx.x * BOX3_THREADS + threadIdx.x;
    if (row >= rows) return;
    const int t = idx[row];
    const long long key = (row / Nq) * Nk + clamp_key(t, Nk);
    const float c_r = c[row];
    const PairGrad pg = pair_grad(t >= 0 ? dz[row] * inv_t : 0.f, a[row], b[key], c_r);
    g_out[row] = pg.g;
    if (hb_out) hb_out[row] = pg.hb;
    if (dmu_out) dmu_out[row] = -kc * (pg.g * nu[key]);
    if (da_out) da_out[row] = pg.ab * c_r;
}

// ---- K52: forward and pair backward -------------------------------------------------------------------------------------------------
//   m = max z;  lse_win = m + log sum exp(z - m);  p = exp(z - lse_win);  off = (sum p dx, sum p dy) in visiting order, limited to
//   [-r, r];  c is kept per slot (0 outside the grid): the backward's state
__global__ __launch_bounds__(BOX3_THREADS) void box3_refine_fwd_kernel(const float* __restrict__ th_t, const float* __restrict__ ph_t,
                                                                       const float* __restrict__ mu, const float* __restrict__ a,
                                                                       const float* __restrict__ nu, const float* __restrict__ b,
                                                                       const int* __restrict__ idx, float* __restrict__ off,
                                                                       float* __restrict__ lse_win, float* __restrict__ c_out,
                                                                       long long rows, int fh, int fw, int gh, int gw, int r, float inv_t,
                                                                       float kc) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = wave_row();                                                 // b * Nq + p
    if (row >= rows) return;                                                          // (whole waves; the kernel has no barrier)
    const int Nq = fh * fw, Nk = gh * gw, W1 = 2 * r + 1;
    const long long bq = row / Nq;
    const int p = (int)(row - bq * Nq), py = p / fw, px = p - py * fw;
    const long long kbase = bq * Nk;
    const QueryTaps taps = load_query_taps(th_t, row, py, px, fh, fw, lane);
    const float kmu = kc * mu[row], za = inv_t * a[row];
    const int j = clamp_key(__builtin_amdgcn_readfirstlane(idx[row]), Nk), yk = j / gw, xk = j - yk * gw;
    float c_mine = 0.f, z_mine = -INFINITY;      // lane s: slot s (outside the grid: c = 0, no score)
    for (int wy = 0; wy < W1; ++wy) {
        const int ky = yk + wy - r;
        if (ky < 0 || ky >= gh) continue;
        for (int wx = 0; wx < W1; ++wx) {
            const int kx = xk + wx - r;
            if (kx < 0 || kx >= gw) continue;
            const long long key = kbase + (long long)ky * gw + kx;
            const float c = pair_R(taps, ph_t, key, ky, kx, gh, gw, lane) - kmu * nu[key];
            const float z = za * b[key] * c;
            const int s = wy * W1 + wx;
            c_mine = lane == s ? c : c_mine;
            z_mine = lane == s ? z : z_mine;
        }
    }
    // the centre is always inside: the window is never empty.  A slot outside the grid adds exp(-inf) = 0, which changes no bit
    const float m = wave_max(z_mine);
    const float e = expf(z_mine - m);
    float sum = 0.f;
    for (int s = 0; s < W1 * W1; ++s) sum = sum + lane_value(e, s);
    const float lse = m + logf(sum);
    const float pr = expf(z_mine - lse);
    float ox = 0.f, oy = 0.f;
    for (int wy = 0; wy < W1; ++wy) {
        for (int wx = 0; wx < W1; ++wx) {
            const float ps = lane_value(pr, wy * W1 + wx);
            ox = __builtin_fmaf(ps, (float)(wx - r), ox);
            oy = __builtin_fmaf(ps, (float)(wy - r), oy);
        }
    }
    // the rounded weights may sum to an ulp above 1: |off| <= r is kept exactly (comparisons, not fmin / fmax: a NaN stays a NaN)
    const float top = (float)r;
    ox = ox > top ? top : (ox < -top ? -top : ox);
    oy = oy > top ? top : (oy < -top ? -top : oy);
    if (lane == 0) {
        off[row * 2] = ox;
        off[row * 2 + 1] = oy;
        lse_win[row] = lse;
    }
    if (lane < W1 * W1) c_out[row * (W1 * W1) + lane] = c_mine;
}

//   p = exp(z - m) / sum exp(z - m) from the saved c (z in the forward's arithmetic), o not limited,
//   dz_s = p_s ((dx_s - o_x) doff_x + (dy_s - o_y) doff_y), 0 outside the grid.  hb_out, dmu_out, da_out may be null.
__global__ __launch_bounds__(BOX3_THREADS) void box3_refine_bwd_pair_kernel(const int* __restrict__ idx, const float* __restrict__ c,
                                                                            const float* __restrict__ a, const float* __restrict__ nu,
                                                                            const float* __restrict__ b, const float* __restrict__ doff,
                                                                            float* __restrict__ g_out, float* __restrict__ hb_out,
                                                                            float* __restrict__ dmu_out, float* __restrict__ da_out,
                                                                            long long rows, int Nq, int gh, int gw, int r, float inv_t,
                                                                            float kc) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = wave_row();
    if (row >= rows) return;
    const int Nk = gh * gw, W1 = 2 * r + 1, W = W1 * W1;
    const long long kbase = (row / Nq) * Nk;
    const int j = clamp_key(__builtin_amdgcn_readfirstlane(idx[row]), Nk), yk = j / gw, xk = j - yk * gw;
    // lane s owns slot s; a lane without a slot in the grid reads the centre's statistics (in the buffers) and contributes exact zeros
    const int wy = lane / W1, wx = lane - wy * W1, dy = wy - r, dx = wx - r;
    const bool mine = lane < W && in_grid(yk + dy, xk + dx, gh, gw);
    const long long key = kbase + (mine ? (yk + dy) * gw + (xk + dx) : j);
    const float c_s = lane < W ? c[row * W + lane] : 0.f, b_s = b[key], nu_s = nu[key];
    const float a_p = a[row], za = inv_t * a_p;
    const float z = mine ? za * b_s * c_s : -INFINITY;      // the forward's score, bit for bit
    const float m = wave_max(z);
    const float e = expf(z - m);
    float sum = 0.f;
    for (int s = 0; s < W; ++s) sum = sum + lane_value(e, s);
    // p = exp(z - m) / sum: exp(z - lse_win) without the rounding of lse_win (K46)
    const float pr = e * (1.0f / sum);
    float ox = 0.f, oy = 0.f;
    for (int sy = 0; sy < W1; ++sy) {
        for (int sx = 0; sx < W1; ++sx) {
            const float ps = lane_value(pr, sy * W1 + sx);
            ox = __builtin_fmaf(ps, (float)(sx - r), ox);
            oy = __builtin_fmaf(ps, (float)(sy - r), oy);
        }
    }
    const float gx = doff[row * 2], gy = doff[row * 2 + 1];
    const float dz = mine ? pr * (((float)dx - ox) * gx + ((float)dy - oy) * gy) : 0.f;
    const PairGrad pg = pair_grad(dz * inv_t, a_p, b_s, c_s);
    float gnu = 0.f, da = 0.f;
    for (int s = 0; s < W; ++s) {
        gnu = __builtin_fmaf(lane_value(pg.g, s), lane_value(nu_s, s), gnu);
        da = __builtin_fmaf(lane_value(pg.ab, s), lane_value(c_s, s), da);
    }
    if (lane < W) {
        g_out[row * W + lane] = pg.g;
        if (hb_out) hb_out[row * W + lane] = pg.hb;
    }
    if (lane == 0) {
        if (dmu_out) dmu_out[row] = -kc * gnu;
        if (da_out) da_out[row] = da;
    }
}

// ---- the gathers (explicit fused multiply-adds, multiplies and adds only: nothing in them depends on the contraction regime) ------------
// dtheta^T[m] = sum over the taps d (raster order) with p = m - d inside the content grid, over p's candidates q in the policy's
//               order, of g[p,q] [q + d inside the exemplar grid] phi^T[q + d];  a position nobody reaches writes its own zeros
template <class Set>
__global__ __launch_bounds__(BOX3_THREADS) void box3_pair_bwd_theta_kernel(const float* __restrict__ ph_t, const float* __restrict__ g,
                                                                           float* __restrict__ dth_t, long long rows, int fh, int fw, int gh,
                                                                           int gw, const Set set) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = wave_row();                                                 // b * Nq + m
    if (row >= rows) return;
    const int Nq = fh * fw, Nk = gh * gw;
    const long long bq = row / Nq;
    const int m = (int)(row - bq * Nq), my = m / fw, mx = m - my * fw;
    const long long kbase = bq * Nk;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll Set::kTapUnroll
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        if (!in_grid(my - dy, mx - dx, fh, fw)) continue;
        set.each_candidate(row - (dy * fw + dx), gh, gw, [&](int ky, int kx, long long at) {
            if (in_grid(ky + dy, kx + dx, gh, gw)) acc = fma4(g[at], row4(ph_t, kbase + (long long)(ky + dy) * gw + (kx + dx), lane), acc);
        });
    }
    *reinterpret_cast<f32x4*>(dth_t + row * BOX3_ROW_C + lane * 4) = acc;
}

// The key gather is two bodies on the shared core, not a template: as one template the K52 instantiation measured 0.2 - 0.9 % above the
// parent's range (profiles/box3_pair_refactor.txt).  entries / offsets are the inverse table of the clamped idx
// (ops._inverse_index_table; K52: of the centres, k = 1), read through list_begin / list_end / list_entry, and a tap is taken only where
// the entry's own (py, px) + d lies inside the content grid: a malformed table cannot send a read outside g / hb / w / mu / the rows.
// Every output may be null; a key nobody names gets zeros, written here.
// K51: an entry is the flat position pos = (b Nq + p) k + r of an idx entry that names the key.
//   dphi^T[n] = sum over the taps d (raster order) with q = n - d inside the exemplar grid, over list(q) in table order, of
//               g[pos] [p + d inside the content grid] theta^T[p + d]
//   from list(n) alone: dv^T[n] = sum w[pos] dout^T[p],  dnu_n = -kc sum g[pos] mu_p,  db_n = sum hb[pos]
__global__ __launch_bounds__(BOX3_THREADS) void box3_sparse_bwd_key_kernel(const float* __restrict__ th_t, const float* __restrict__ dout_t,
                                                                           const float* __restrict__ g, const float* __restrict__ hb,
                                                                           const float* __restrict__ w, const float* __restrict__ mu,
                                                                           const int* __restrict__ entries, const int* __restrict__ offsets,
                                                                           float* __restrict__ dph_t, float* __restrict__ dv_t,
                                                                           float* __restrict__ dnu, float* __restrict__ db, long long keys,
                                                                           int total, int fh, int fw, int gh, int gw, int Cv, int k, float kc) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const long long key = wave_row();                                                 // b * Nk + n
    if (key >= keys) return;
    const int Nq = fh * fw, Nk = gh * gw;
    const int n = (int)(key % Nk), ny = n / gw, nx = n - ny * gw;
    if (dph_t) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3 - 1, dx = t % 3 - 1;
            if (!in_grid(ny - dy, nx - dx, gh, gw)) continue;
            const long long qkey = key - (dy * gw + dx);
            for (int e = list_begin(offsets, qkey, total), end = list_end(offsets, qkey, total); e < end; ++e) {
                const int pos = list_entry(entries, e, total), prow = pos / k, p = prow % Nq, py = p / fw, px = p - py * fw;
                if (in_grid(py + dy, px + dx, fh, fw)) acc = fma4(g[pos], row4(th_t, (long long)prow + dy * fw + dx, lane), acc);
            }
        }
        *reinterpret_cast<f32x4*>(dph_t + key * BOX3_ROW_C + lane * 4) = acc;
    }
    const int beg = list_begin(offsets, key, total), end = list_end(offsets, key, total);
    if (dv_t) {
        for (int c0 = 0; c0 < Cv; c0 += 4 * kWave) {          // four channels per lane and walk of the list
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int e = beg; e < end; ++e) {
                const int pos = list_entry(entries, e, total);
                const float wp = w[pos];
                const float* const go = dout_t + (long long)(pos / k) * Cv;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int ch = c0 + u * kWave + lane;
                    if (ch < Cv) acc[u] = __builtin_fmaf(wp, go[ch], acc[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ch = c0 + u * kWave + lane;
                if (ch < Cv) dv_t[key * Cv + ch] = acc[u];
            }
        }
    }
    if (dnu || db) {                     // scalars: every lane forms the same two sums in table order, lane 0 writes them
        float sn = 0.f, sb = 0.f;
        for (int e = beg; e < end; ++e) {
            const int pos = list_entry(entries, e, total);
            if (dnu) sn = __builtin_fmaf(g[pos], mu[pos / k], sn);
            if (db) sb = sb + hb[pos];
        }
        if (lane == 0) {
            if (dnu) dnu[key] = -kc * sn;
            if (db) db[key] = sb;
        }
    }
}

// K52: an entry is the row pos = b Nq + p of a query whose (clamped) centre is the list's key.
//   dphi^T[n] = sum over the taps d (raster order) with q = n - d inside the exemplar grid, over the window offsets e (visiting order)
//               with the centre q - e inside it, over list(q - e) in table order, of g[p, s(e)] [p + d inside the content grid] theta^T[p + d]
//   from d = 0 alone: dnu_n = -kc sum g[p, s(e)] mu_p,  db_n = sum hb[p, s(e)]
__global__ __launch_bounds__(BOX3_THREADS) void box3_refine_bwd_key_kernel(const float* __restrict__ th_t, const float* __restrict__ g,
                                                                           const float* __restrict__ hb, const float* __restrict__ mu,
                                                                           const int* __restrict__ entries, const int* __restrict__ offsets,
                                                                           float* __restrict__ dph_t, float* __restrict__ dnu,
                                                                           float* __restrict__ db, long long keys, int total, int fh, int fw,
                                                                           int gh, int gw, int r, float kc) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const long long key = wave_row();                                                 // b * Nk + n
    if (key >= keys) return;
    const int Nq = fh * fw, Nk = gh * gw, W1 = 2 * r + 1, W = W1 * W1;
    const long long kbase = (key / Nk) * Nk;
    const int n = (int)(key - kbase), ny = n / gw, nx = n - ny * gw;
    if (dph_t) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3 - 1, dx = t % 3 - 1;
            const int qy = ny - dy, qx = nx - dx;
            if (!in_grid(qy, qx, gh, gw)) continue;
            for (int wy = 0; wy < W1; ++wy) {
                const int cy = qy - (wy - r);
                if (cy < 0 || cy >= gh) continue;
                for (int wx = 0; wx < W1; ++wx) {
                    const int cx = qx - (wx - r);
                    if (cx < 0 || cx >= gw) continue;
                    const long long centre = kbase + (long long)cy * gw + cx;
                    const int slot = wy * W1 + wx;
                    for (int e = list_begin(offsets, centre, total), end = list_end(offsets, centre, total); e < end; ++e) {
                        const int pos = list_entry(entries, e, total), p = pos % Nq, py = p / fw, px = p - py * fw;
                        if (in_grid(py + dy, px + dx, fh, fw))
                            acc = fma4(g[(long long)pos * W + slot], row4(th_t, (long long)pos + dy * fw + dx, lane), acc);
                    }
                }
            }
        }
        *reinterpret_cast<f32x4*>(dph_t + key * BOX3_ROW_C + lane * 4) = acc;
    }
    if (dnu || db) {                     // scalars: every lane forms the same two sums in the same order, lane 0 writes them
        float sn = 0.f, sb = 0.f;
        for (int wy = 0; wy < W1; ++wy) {
            const int cy = ny - (wy - r);
            if (cy < 0 || cy >= gh) continue;
            for (int wx = 0; wx < W1; ++wx) {
                const int cx = nx - (wx - r);
                if (cx < 0 || cx >= gw) continue;
                const long long centre = kbase + (long long)cy * gw + cx;
                const int slot = wy * W1 + wx;
                for (int e = list_begin(offsets, centre, total), end = list_end(offsets, centre, total); e < end; ++e) {
                    const int pos = list_entry(entries, e, total);
                    if (dnu) sn = __builtin_fmaf(g[(long long)pos * W + slot], mu[pos], sn);
                    if (db) sb = sb + hb[(long long)pos * W + slot];
                }
            }
        }
        if (lane == 0) {
            if (dnu) dnu[key] = -kc * sn;
            if (db) db[key] = sb;
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// What the eight entry points require alike (before any HIP call), refused in the order and the words they always were: the route's
// own requirements (Set::own), the channel count, the 32-bit tables.
template <class Set>
static int box3_pair_check(const char* name, const Set& set, int B, int K, int fh, int fw, int gh, int gw, int Cv, float inv_temperature) {
    if (const int rc = set.own(name, B, fh, fw, gh, gw, Cv, inv_temperature)) return rc;
    COCOS_REQUIRE(K == BOX3_ROW_C, COCOS_ERR_UNSUPPORTED, "%s: needs K == 256 (got %d)", name, K);
    const long long Nq = (long long)fh * fw, Nk = (long long)gh * gw, state = B * Nq * set.width();
    COCOS_REQUIRE(Nq < 0x7fffffffll && Nk < 0x7fffffffll && state < 0x7fffffffll && B * Nk < 0x7fffffffll, COCOS_ERR_UNSUPPORTED,
                  "%s: B Nq %s = %lld %s / B Nk = %lld keys exceed the 32-bit tables", name, Set::kWidthName, state, Set::kWidthNoun, B * Nk);
    return COCOS_OK;
}

static unsigned box3_pair_blocks(long long rows) { return (unsigned)((rows + BOX3_WAVES - 1) / BOX3_WAVES); }

template <class Set>
static int box3_pair_bwd_theta(const char* name, const float* ph_t, const float* g, float* dth_t, int B, int K, int fh, int fw, int gh, int gw,
                               const Set& set, cocos_stream_t stream) {
    COCOS_REQUIRE(ph_t && set.idx && g && dth_t, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (const int rc = box3_pair_check(name, set, B, K, fh, fw, gh, gw, 1, 1.f)) return rc;
    for (const void* p : {(const void*)ph_t, (const void*)dth_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the phi rows and dth_t must be 16-byte aligned", name);
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_pair_bwd_theta_kernel<Set>, dim3(box3_pair_blocks(rows)), dim3(BOX3_THREADS), 0, as_stream(stream), ph_t, g, dth_t,
                       rows, fh, fw, gh, gw, set);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

// what the two key entry points require before their launch (set.idx is not read on the key side: the inverse table stands for it)
template <class Set>
static int box3_pair_key_gate(const char* name, const Set& set, const float* th_t, const float* dout_t, const float* g, const float* hb,
                              const float* w, const float* mu, const int* entries, const int* offsets, float* dph_t, float* dv_t, float* dnu,
                              float* db, int B, int K, int fh, int fw, int gh, int gw, int Cv) {
    COCOS_REQUIRE(entries && offsets && (dph_t || dv_t || dnu || db), COCOS_ERR_INVALID, "%s: null pointer", name);
    COCOS_REQUIRE(!dph_t || (th_t && g), COCOS_ERR_INVALID, "%s: null pointer (dph_t needs the theta rows and g)", name);
    COCOS_REQUIRE(!dv_t || (dout_t && w), COCOS_ERR_INVALID, "%s: null pointer (dv_t needs dout_t and w)", name);
    COCOS_REQUIRE(!dnu || (g && mu), COCOS_ERR_INVALID, "%s: null pointer (dnu needs g and mu)", name);
    COCOS_REQUIRE(!db || hb, COCOS_ERR_INVALID, "%s: null pointer (db needs hb)", name);
    if (const int rc = box3_pair_check(name, set, B, K, fh, fw, gh, gw, Cv, 1.f)) return rc;
    for (const void* p : {(const void*)th_t, (const void*)dph_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the theta rows and dph_t must be 16-byte aligned", name);
    return COCOS_OK;
}

}  // namespace cocos

extern "C" int cocos_box3_sparse_softmax_warp_fwd(const float* th_t, const float* ph_t, const float* mu, const float* a, const float* nu,
                                                  const float* b, const float* v_t, const int* idx, float* out_t, float* w, float* c, int B,
                                                  int K, int fh, int fw, int gh, int gw, int Cv, int k, float inv_temperature,
                                                  cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_sparse_softmax_warp_fwd";
    COCOS_REQUIRE(th_t && ph_t && mu && a && nu && b && v_t && idx && out_t && w && c, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (const int rc = box3_pair_check(name, TopkSet{idx, k}, B, K, fh, fw, gh, gw, Cv, inv_temperature)) return rc;
    for (const void* p : {th_t, ph_t}) COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the theta / phi rows must be 16-byte aligned", name);
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_sparse_fwd_kernel<false>, dim3(box3_pair_blocks(rows)), dim3(BOX3_THREADS), 0, as_stream(stream), th_t, ph_t, mu, a,
                       nu, b, v_t, idx, out_t, w, c, rows, fh, fw, gh, gw, Cv, k, inv_temperature, (float)(9 * BOX3_ROW_C), nullptr);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_box3_sparse_softmax_warp_bias_fwd(const float* th_t, const float* ph_t, const float* mu, const float* a, const float* nu,
                                                       const float* b, const float* v_t, const int* idx, const float* k_bias, float* out_t,
                                                       float* w, float* c, int B, int K, int fh, int fw, int gh, int gw, int Cv, int k,
                                                       float inv_temperature, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_sparse_softmax_warp_bias_fwd";
    COCOS_REQUIRE(th_t && ph_t && mu && a && nu && b && v_t && idx && k_bias && out_t && w && c, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (const int rc = box3_pair_check(name, TopkSet{idx, k}, B, K, fh, fw, gh, gw, Cv, inv_temperature)) return rc;
    for (const void* p : {th_t, ph_t}) COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the theta / phi rows must be 16-byte aligned", name);
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_sparse_fwd_kernel<true>, dim3(box3_pair_blocks(rows)), dim3(BOX3_THREADS), 0, as_stream(stream), th_t, ph_t, mu, a,
                       nu, b, v_t, idx, out_t, w, c, rows, fh, fw, gh, gw, Cv, k, inv_temperature, (float)(9 * BOX3_ROW_C), k_bias);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_box3_sparse_softmax_warp_bwd_pair(const float* v_t, const float* dout_t, const int* idx, const float* w, const float* c,
                                                       const float* a, const float* nu, const float* b, float* g, float* hb, float* dmu,
                                                       float* da, int B, int K, int fh, int fw, int gh, int gw, int Cv, int k,
                                                       float inv_temperature, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_sparse_softmax_warp_bwd_pair";
    COCOS_REQUIRE(v_t && dout_t && idx && w && c && a && nu && b && g, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (const int rc = box3_pair_check(name, TopkSet{idx, k}, B, K, fh, fw, gh, gw, Cv, inv_temperature)) return rc;
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_sparse_bwd_pair_kernel, dim3(box3_pair_blocks(rows)), dim3(BOX3_THREADS), 0, as_stream(stream), v_t, dout_t, idx,
                       w, c, a, nu, b, g, hb, dmu, da, rows, fh * fw, gh * gw, Cv, k, inv_temperature, (float)(9 * BOX3_ROW_C));
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_box3_sparse_softmax_warp_bwd_theta(const float* ph_t, const int* idx, const float* g, float* dth_t, int B, int K, int fh,
                                                        int fw, int gh, int gw, int k, cocos_stream_t stream) {
    return cocos::box3_pair_bwd_theta("box3_sparse_softmax_warp_bwd_theta", ph_t, g, dth_t, B, K, fh, fw, gh, gw, cocos::TopkSet{idx, k}, stream);
}

extern "C" int cocos_box3_sparse_softmax_warp_bwd_key(const float* th_t, const float* dout_t, const float* g, const float* hb, const float* w,
                                                      const float* mu, const int* entries, const int* offsets, float* dph_t, float* dv_t,
                                                      float* dnu, float* db, int B, int K, int fh, int fw, int gh, int gw, int Cv, int k,
                                                      cocos_stream_t stream) {
    using namespace cocos;
    if (const int rc = box3_pair_key_gate("box3_sparse_softmax_warp_bwd_key", TopkSet{nullptr, k}, th_t, dout_t, g, hb, w, mu, entries, offsets,
                                          dph_t, dv_t, dnu, db, B, K, fh, fw, gh, gw, Cv))
        return rc;
    const long long keys = (long long)B * gh * gw;
    hipLaunchKernelGGL(box3_sparse_bwd_key_kernel, dim3(box3_pair_blocks(keys)), dim3(BOX3_THREADS), 0, as_stream(stream), th_t, dout_t, g,
                       hb, w, mu, entries, offsets, dph_t, dv_t, dnu, db, keys, B * fh * fw * k, fh, fw, gh, gw, Cv, k, (float)(9 * BOX3_ROW_C));
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_box3_pair_logit_fwd(const float* th_t, const float* ph_t, const float* mu, const float* a, const float* nu, const float* b,
                                         const int* idx, float* z, float* c, int B, int K, int fh, int fw, int gh, int gw,
                                         float inv_temperature, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_pair_logit_fwd";
    COCOS_REQUIRE(th_t && ph_t && mu && a && nu && b && idx && z && c, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (const int rc = box3_pair_check(name, TopkSet{idx, 1}, B, K, fh, fw, gh, gw, 1, inv_temperature)) return rc;
    for (const void* p : {th_t, ph_t}) COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the theta / phi rows must be 16-byte aligned", name);
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_pair_logit_fwd_kernel, dim3(box3_pair_blocks(rows)), dim3(BOX3_THREADS), 0, as_stream(stream), th_t, ph_t, mu, a,
                       nu, b, idx, z, c, rows, fh, fw, gh, gw, inv_temperature, (float)(9 * BOX3_ROW_C));
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_box3_pair_logit_bwd_pair(const int* idx, const float* c, const float* a, const float* nu, const float* b, const float* dz,
                                              float* g, float* hb, float* dmu, float* da, int B, int K, int fh, int fw, int gh, int gw,
                                              float inv_temperature, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_pair_logit_bwd_pair";
    COCOS_REQUIRE(idx && c && a && nu && b && dz && g, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (const int rc = box3_pair_check(name, TopkSet{idx, 1}, B, K, fh, fw, gh, gw, 1, inv_temperature)) return rc;
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_pair_logit_bwd_pair_kernel, dim3((unsigned)((rows + BOX3_THREADS - 1) / BOX3_THREADS)), dim3(BOX3_THREADS), 0,
                       as_stream(stream), idx, c, a, nu, b, dz, g, hb, dmu, da, rows, fh * fw, gh * gw, inv_temperature,
                       (float)(9 * BOX3_ROW_C));
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_box3_match_refine_fwd(const float* th_t, const float* ph_t, const float* mu, const float* a, const float* nu,
                                           const float* b, const int* idx, float* off, float* lse_win, float* c, int B, int K, int fh, int fw,
                                           int gh, int gw, int radius, float inv_temperature, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_match_refine_fwd";
    COCOS_REQUIRE(th_t && ph_t && mu && a && nu && b && idx && off && lse_win && c, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (const int rc = box3_pair_check(name, WindowSet{idx, radius}, B, K, fh, fw, gh, gw, 1, inv_temperature)) return rc;
    for (const void* p : {th_t, ph_t}) COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the theta / phi rows must be 16-byte aligned", name);
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_refine_fwd_kernel, dim3(box3_pair_blocks(rows)), dim3(BOX3_THREADS), 0, as_stream(stream), th_t, ph_t, mu, a, nu,
                       b, idx, off, lse_win, c, rows, fh, fw, gh, gw, radius, inv_temperature, (float)(9 * BOX3_ROW_C));
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_box3_match_refine_bwd_pair(const int* idx, const float* c, const float* a, const float* nu, const float* b,
                                                const float* doff, float* g, float* hb, float* dmu, float* da, int B, int K, int fh, int fw,
                                                int gh, int gw, int radius, float inv_temperature, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_match_refine_bwd_pair";
    COCOS_REQUIRE(idx && c && a && nu && b && doff && g, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (const int rc = box3_pair_check(name, WindowSet{idx, radius}, B, K, fh, fw, gh, gw, 1, inv_temperature)) return rc;
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_refine_bwd_pair_kernel, dim3(box3_pair_blocks(rows)), dim3(BOX3_THREADS), 0, as_stream(stream), idx, c, a, nu, b,
                       doff, g, hb, dmu, da, rows, fh * fw, gh, gw, radius, inv_temperature, (float)(9 * BOX3_ROW_C));
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_box3_match_refine_bwd_theta(const float* ph_t, const int* idx, const float* g, float* dth_t, int B, int K, int fh, int fw,
                                                 int gh, int gw, int radius, cocos_stream_t stream) {
    return cocos::box3_pair_bwd_theta("box3_match_refine_bwd_theta", ph_t, g, dth_t, B, K, fh, fw, gh, gw, cocos::WindowSet{idx, radius}, stream);
}

extern "C" int cocos_box3_match_refine_bwd_key(const float* th_t, const float* g, const float* hb, const float* mu, const int* entries,
                                               const int* offsets, float* dph_t, float* dnu, float* db, int B, int K, int fh, int fw, int gh,
                                               int gw, int radius, cocos_stream_t stream) {
    using namespace cocos;
    if (const int rc = box3_pair_key_gate("box3_match_refine_bwd_key", WindowSet{nullptr, radius}, th_t, nullptr, g, hb, nullptr, mu, entries,
                                          offsets, dph_t, nullptr, dnu, db, B, K, fh, fw, gh, gw, 1))
        return rc;
    const long long keys = (long long)B * gh * gw;
    hipLaunchKernelGGL(box3_refine_bwd_key_kernel, dim3(box3_pair_blocks(keys)), dim3(BOX3_THREADS), 0, as_stream(stream), th_t, g, hb, mu,
                       entries, offsets, dph_t, dnu, db, keys, B * fh * fw, fh, fw, gh, gw, radius, (float)(9 * BOX3_ROW_C));
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
