// K52: the trainable sub-cell refinement on the match_kernel-3 route — K44 / K46's window soft-argmax on K51's logit of the 3x3-unfolded,
// centred, normalised vectors, taken for ONE pair:
//   R[p,q] = sum over the taps d in {-1,0,1}^2 of [p+d inside the content grid] [q+d inside the exemplar grid] <theta[:,p+d], phi[:,q+d]>
//   c[p,q] = R[p,q] - kc mu_p nu_q,   z[p,q] = inv_t a_p b_q c[p,q],   kc = 9 * 256,   (mu, a), (nu, b) the K12 statistics
// Query (b, p) has the centre idx[b,p] (clamped into [0, Nk)) at (yk, xk); with W1 = 2 r + 1 the window has W = W1^2 slots,
// slot s = (dy + r) W1 + (dx + r), and holds the keys (yk + dy, xk + dx) INSIDE the exemplar grid (one outside is left out: neither
// clamped nor wrapped), visited dy ascending outside, dx ascending inside.  Inside is decided on 2-D coordinates, for the window and
// for the taps: a key in the last column never picks up the first cell of the next row.
//   forward    m = max z;  lse_win = m + log sum exp(z - m);  p = exp(z - lse_win);  off = (sum p dx, sum p dy) in visiting order,
//              limited to [-r, r];  c is kept per slot (0 outside the grid): the backward's state, [B,Nq,W]
//   backward   p = exp(z - m) / sum exp(z - m) from the saved c (z in the forward's arithmetic), o not limited,
//              dz_s = p_s ((dx_s - o_x) doff_x + (dy_s - o_y) doff_y), 0 outside the grid;  g = dz inv_t a_p b_q (the coefficient on R),
//              hb = dz inv_t a_p c (the pair's share of db_q), dmu_p = -kc sum_s g_s nu_q, da_p = sum_s dz_s inv_t b_q c_s
// Operands are fp32 position-major rows [B,N,256] (box3_rows.h); a window's slot s lives in lane s (W <= 49 < 64), so no kernel
// keeps a per-slot array: the sums over the window read lane s through v_readlane, in visiting order.  One wave per row, four per
// workgroup, no LDS, no atomics, contraction off and every fused multiply-add written out: the results are bitwise reproducible.
// The W x 9 row loads of a window touch (2 r + 3)^2 distinct phi rows; the kernels do not stage them, the cache serves the repeats.
//
//   forward          one wave per query: the nine theta neighbour rows stay in registers; per in-grid slot the taps' products, one butterfly
//   pair backward    one wave per query, lane s owns slot s: g, hb [B,Nq,W], dmu, da
//   theta gradient   one wave per content position m, a GATHER: the taps d with p = m - d in the grid, that query's window
//   key gradient     one wave per exemplar position n, a GATHER over the inverse table of the clamped centres (K42's, k = 1): per tap d
//                    the key q = n - d, per window offset e the centre q - e and its list.  A centre every query names is a serial
//                    list of Nq entries, walked for up to 9 W (tap, offset) pairs.
#include "box3_rows.h"       // row4, in_grid, lane_fma4; wave_sum, clamp_key

namespace cocos {

constexpr int BR_WAVES = 4;              // rows (queries, content positions or keys) per workgroup, one per wave
constexpr int BR_THREADS = BR_WAVES * kWave;

// (the wave index is the same in all 64 lanes: saying so keeps the row, its coordinates and the window walk on the scalar side)
__device__ __forceinline__ long long wave_row() {
    return (long long)blockIdx.x * BR_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// lane s's value in every lane; s is wave-uniform
__device__ __forceinline__ float lane_value(float v, int s) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), s));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, kWave));
    return v;
}

__device__ __forceinline__ f32x4 fma4(float s, const f32x4& v, const f32x4& acc) {
    return f32x4{__builtin_fmaf(s, v[0], acc[0]), __builtin_fmaf(s, v[1], acc[1]), __builtin_fmaf(s, v[2], acc[2]),
                 __builtin_fmaf(s, v[3], acc[3])};
}

__global__ __launch_bounds__(BR_THREADS) void box3_refine_fwd_kernel(const float* __restrict__ th_t, const float* __restrict__ ph_t,
                                                                     const float* __restrict__ mu, const float* __restrict__ a,
                                                                     const float* __restrict__ nu, const float* __restrict__ b,
                                                                     const int* __restrict__ idx, float* __restrict__ off,
                                                                     float* __restrict__ lse_win, float* __restrict__ c_out, long long rows,
                                                                     int fh, int fw, int gh, int gw, int r, float inv_t, float kc) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = wave_row();                                                 // b * Nq + p
    if (row >= rows) return;                                                          // (whole waves; the kernel has no barrier)
    const int Nq = fh * fw, Nk = gh * gw, W1 = 2 * r + 1;
    const long long bq = row / Nq;
    const int p = (int)(row - bq * Nq), py = p / fw, px = p - py * fw;
    const long long kbase = bq * Nk;
    f32x4 q[9];
    unsigned qmask = 0;                  // bit t: tap t of the query lies inside the content grid
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        q[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (in_grid(py + dy, px + dx, fh, fw)) {
            qmask |= 1u << t;
            q[t] = row4(th_t, row + dy * fw + dx, lane);
        }
    }
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
            float acc = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int dy = t / 3 - 1, dx = t % 3 - 1;
                if (((qmask >> t) & 1u) && in_grid(ky + dy, kx + dx, gh, gw)) acc = lane_fma4(q[t], row4(ph_t, key + dy * gw + dx, lane), acc);
            }
            const float c = wave_sum(acc) - kmu * nu[key];
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

// hb_out, dmu_out, da_out may be null
__global__ __launch_bounds__(BR_THREADS) void box3_refine_bwd_pair_kernel(const int* __restrict__ idx, const float* __restrict__ c,
                                                                          const float* __restrict__ a, const float* __restrict__ nu,
                                                                          const float* __restrict__ b, const float* __restrict__ doff,
                                                                          float* __restrict__ g_out, float* __restrict__ hb_out,
                                                                          float* __restrict__ dmu_out, float* __restrict__ da_out,
                                                                          long long rows, int Nq, int gh, int gw, int r, float inv_t, float kc) {
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
    const float dzt = dz * inv_t;
    const float g_s = dzt * a_p * b_s, da_s = dzt * b_s;
    float gnu = 0.f, da = 0.f;
    for (int s = 0; s < W; ++s) {
        gnu = __builtin_fmaf(lane_value(g_s, s), lane_value(nu_s, s), gnu);
        da = __builtin_fmaf(lane_value(da_s, s), lane_value(c_s, s), da);
    }
    if (lane < W) {
        g_out[row * W + lane] = g_s;
        if (hb_out) hb_out[row * W + lane] = dzt * a_p * c_s;
    }
    if (lane == 0) {
        if (dmu_out) dmu_out[row] = -kc * gnu;
        if (da_out) da_out[row] = da;
    }
}

// dtheta^T[m] = sum over the taps d (raster order) with p = m - d inside the content grid, over the slots s of p's window ascending, of
//               g[p,s] [q_s + d inside the exemplar grid] phi^T[q_s + d];  a position nobody reaches writes its own zeros
__global__ __launch_bounds__(BR_THREADS) void box3_refine_bwd_theta_kernel(const float* __restrict__ ph_t, const int* __restrict__ idx,
                                                                           const float* __restrict__ g, float* __restrict__ dth_t,
                                                                           long long rows, int fh, int fw, int gh, int gw, int r) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = wave_row();                                                 // b * Nq + m
    if (row >= rows) return;
    const int Nq = fh * fw, Nk = gh * gw, W1 = 2 * r + 1;
    const long long bq = row / Nq;
    const int m = (int)(row - bq * Nq), my = m / fw, mx = m - my * fw;
    const long long kbase = bq * Nk;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        if (!in_grid(my - dy, mx - dx, fh, fw)) continue;
        const long long prow = row - (dy * fw + dx);
        const int j = clamp_key(__builtin_amdgcn_readfirstlane(idx[prow]), Nk), yk = j / gw, xk = j - yk * gw;
        const float* const gp = g + prow * (W1 * W1);
        for (int wy = 0; wy < W1; ++wy) {
            const int ky = yk + wy - r;
            if (ky < 0 || ky >= gh || ky + dy < 0 || ky + dy >= gh) continue;
            for (int wx = 0; wx < W1; ++wx) {
                const int kx = xk + wx - r;
                if (kx < 0 || kx >= gw || kx + dx < 0 || kx + dx >= gw) continue;
                acc = fma4(gp[wy * W1 + wx], row4(ph_t, kbase + (long long)(ky + dy) * gw + (kx + dx), lane), acc);
            }
        }
    }
    *reinterpret_cast<f32x4*>(dth_t + row * BOX3_ROW_C + lane * 4) = acc;
}

// entries[offsets[centre] .. offsets[centre + 1]) are the rows b Nq + p of the queries whose (clamped) centre is `centre` = b Nk + j,
// ascending (ops._inverse_index_table with k = 1).  Positions and ranges are clamped into the tables, and a tap is taken only where
// the entry's own (py, px) + d lies inside the content grid: a malformed table cannot send a read outside g / hb / mu / the rows.
//   dphi^T[n] = sum over the taps d (raster order) with q = n - d inside the exemplar grid, over the window offsets e (visiting order)
//               with the centre q - e inside it, over list(q - e) in table order, of g[p, s(e)] [p + d inside the content grid] theta^T[p + d]
//   from d = 0 alone: dnu_n = -kc sum g[p, s(e)] mu_p,  db_n = sum hb[p, s(e)]
// Every output may be null; a key in nobody's window gets zeros, written here.
__global__ __launch_bounds__(BR_THREADS) void box3_refine_bwd_key_kernel(const float* __restrict__ th_t, const float* __restrict__ g,
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
                    const int beg = min(max(offsets[centre], 0), total), end = min(max(offsets[centre + 1], beg), total);
                    for (int e = beg; e < end; ++e) {
                        const int pos = min(max(entries[e], 0), total - 1), p = pos % Nq, py = p / fw, px = p - py * fw;
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
                const int beg = min(max(offsets[centre], 0), total), end = min(max(offsets[centre + 1], beg), total);
                for (int e = beg; e < end; ++e) {
                    const int pos = min(max(entries[e], 0), total - 1);
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

// the checks the four entry points share (before any HIP call)
static int box3_refine_check(const char* name, int B, int K, int fh, int fw, int gh, int gw, int radius, float inv_temperature) {
    COCOS_REQUIRE(B >= 1 && fh >= 1 && fw >= 1 && gh >= 1 && gw >= 1, COCOS_ERR_INVALID,
                  "%s: non-positive size: B=%d content grid %dx%d exemplar grid %dx%d", name, B, fh, fw, gh, gw);
    COCOS_REQUIRE(radius >= 1 && radius <= COCOS_MATCH_REFINE_MAX_RADIUS, COCOS_ERR_INVALID, "%s: radius=%d: expected 1 .. %d", name, radius,
                  COCOS_MATCH_REFINE_MAX_RADIUS);
    COCOS_REQUIRE(inv_temperature > 0.f, COCOS_ERR_INVALID, "%s: inv_temperature must be positive", name);
    COCOS_REQUIRE(K == BOX3_ROW_C, COCOS_ERR_UNSUPPORTED, "%s: needs K == 256 (got %d)", name, K);
    const long long Nq = (long long)fh * fw, Nk = (long long)gh * gw, slots = (long long)(2 * radius + 1) * (2 * radius + 1);
    COCOS_REQUIRE(Nq < 0x7fffffffll && Nk < 0x7fffffffll && B * Nq * slots < 0x7fffffffll && B * Nk < 0x7fffffffll, COCOS_ERR_UNSUPPORTED,
                  "%s: B Nq W = %lld window slots / B Nk = %lld keys exceed the 32-bit tables", name, B * Nq * slots, B * Nk);
    return COCOS_OK;
}

static unsigned box3_refine_blocks(long long rows) { return (unsigned)((rows + BR_WAVES - 1) / BR_WAVES); }

}  // namespace cocos

extern "C" int cocos_box3_match_refine_fwd(const float* th_t, const float* ph_t, const float* mu, const float* a, const float* nu,
                                           const float* b, const int* idx, float* off, float* lse_win, float* c, int B, int K, int fh, int fw,
                                           int gh, int gw, int radius, float inv_temperature, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_match_refine_fwd";
    COCOS_REQUIRE(th_t && ph_t && mu && a && nu && b && idx && off && lse_win && c, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (int rc = box3_refine_check(name, B, K, fh, fw, gh, gw, radius, inv_temperature)) return rc;
    for (const void* p : {th_t, ph_t}) COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the theta / phi rows must be 16-byte aligned", name);
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_refine_fwd_kernel, dim3(box3_refine_blocks(rows)), dim3(BR_THREADS), 0, as_stream(stream), th_t, ph_t, mu, a, nu,
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
    if (int rc = box3_refine_check(name, B, K, fh, fw, gh, gw, radius, inv_temperature)) return rc;
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_refine_bwd_pair_kernel, dim3(box3_refine_blocks(rows)), dim3(BR_THREADS), 0, as_stream(stream), idx, c, a, nu, b,
                       doff, g, hb, dmu, da, rows, fh * fw, gh, gw, radius, inv_temperature, (float)(9 * BOX3_ROW_C));
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_box3_match_refine_bwd_theta(const float* ph_t, const int* idx, const float* g, float* dth_t, int B, int K, int fh, int fw,
                                                 int gh, int gw, int radius, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_match_refine_bwd_theta";
    COCOS_REQUIRE(ph_t && idx && g && dth_t, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (int rc = box3_refine_check(name, B, K, fh, fw, gh, gw, radius, 1.f)) return rc;
    for (const void* p : {(const void*)ph_t, (const void*)dth_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the phi rows and dth_t must be 16-byte aligned", name);
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_refine_bwd_theta_kernel, dim3(box3_refine_blocks(rows)), dim3(BR_THREADS), 0, as_stream(stream), ph_t, idx, g,
                       dth_t, rows, fh, fw, gh, gw, radius);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_box3_match_refine_bwd_key(const float* th_t, const float* g, const float* hb, const float* mu, const int* entries,
                                               const int* offsets, float* dph_t, float* dnu, float* db, int B, int K, int fh, int fw, int gh,
                                               int gw, int radius, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_match_refine_bwd_key";
    COCOS_REQUIRE(entries && offsets && (dph_t || dnu || db), COCOS_ERR_INVALID, "%s: null pointer", name);
    COCOS_REQUIRE(!dph_t || (th_t && g), COCOS_ERR_INVALID, "%s: null pointer (dph_t needs the theta rows and g)", name);
    COCOS_REQUIRE(!dnu || (g && mu), COCOS_ERR_INVALID, "%s: null pointer (dnu needs g and mu)", name);
    COCOS_REQUIRE(!db || hb, COCOS_ERR_INVALID, "%s: null pointer (db needs hb)", name);
    if (int rc = box3_refine_check(name, B, K, fh, fw, gh, gw, radius, 1.f)) return rc;
    for (const void* p : {(const void*)th_t, (const void*)dph_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the theta rows and dph_t must be 16-byte aligned", name);
    const long long keys = (long long)B * gh * gw;
    hipLaunchKernelGGL(box3_refine_bwd_key_kernel, dim3(box3_refine_blocks(keys)), dim3(BR_THREADS), 0, as_stream(stream), th_t, g, hb, mu,
                       entries, offsets, dph_t, dnu, db, keys, B * fh * fw, fh, fw, gh, gw, radius, (float)(9 * BOX3_ROW_C));
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
