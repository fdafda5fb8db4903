// K51: the k-sparse correspondence warp with gradients on the match_kernel-3 route — attention over the k keys per query that the
// top-k readout of the x-box tensor (K41) selected, on the logit of the 3x3-unfolded, centred, normalised vectors taken for ONE pair:
//   R[p,q] = sum over the taps d in {-1,0,1}^2 of [p+d inside the content grid] [q+d inside the exemplar grid] <theta[:,p+d], phi[:,q+d]>
//   z[p,q] = inv_t a_p b_q (R[p,q] - kc mu_p nu_q),   kc = 9 * 256,   (mu, a), (nu, b) the K12 statistics of theta and phi
//   w = softmax over r of z[p, j_r],  j_r = idx[b,p,r] (clamped into [0, Nk)),   out[b,:,p] = sum_r w_r v[b,:,j_r]
// and its gradients.  Whether a tap is inside a grid is decided on the 2-D coordinates (y, x), never on the flat index: a candidate in
// the last column does not pick up the first cell of the next row.  Nothing here has an Nq x Nk extent: the state is idx, w, c, g and
// hb, each [B,Nq,k].
//
// Operands are fp32 position-major rows [B,N,256] (cocos_transpose_f32 of the channel-major tensors), read as whole 1 KiB rows: lane l
// of a wave holds channels 4 l .. 4 l + 3.  A dot product is fp32 FMAs per lane over the taps in raster order and ONE butterfly over
// the 64 lanes per pair (wave_sum: every lane ends with the same sum); every sum below has a fixed order, no atomics, no LDS.
//
//   forward          one wave per query: the query's (up to) nine neighbour rows stay in registers, per candidate the in-grid taps'
//                    products, c_r = R - kc mu_p nu_j, the softmax over k in registers, out^T row, w, c
//   pair backward    one wave per query: dw_r = <dout^T[p], v^T[j_r]>, dz_r = w_r (dw_r - sum w dw), g_r = dz_r inv_t a_p b_j (the
//                    coefficient on R), hb_r = dz_r inv_t a_p c_r (the pair's share of db_j), dmu_p, da_p
//   theta gradient   one wave per content position m, a GATHER: the taps d with p = m - d in the grid, that query's k candidates
//   key gradient     one wave per exemplar position n, a GATHER over the inverse table of idx (K42's): per tap d the list of the key
//                    q = n - d; from the d = 0 list alone dv^T[n], dnu_n, db_n.  A key every query names is a serial list of Nq
//                    entries, walked for up to nine taps.
#include "box3_rows.h"       // row4, in_grid, lane_fma4; wave_sum, clamp_key

namespace cocos {

constexpr int BS_WAVES = 4;              // rows (queries, content positions or keys) per workgroup, one per wave
constexpr int BS_THREADS = BS_WAVES * kWave;
constexpr int BS_MAXK = COCOS_MATCH_TOPK_MAX;
constexpr int BS_C = BOX3_ROW_C;         // channels of theta / phi

__global__ __launch_bounds__(BS_THREADS) void box3_sparse_fwd_kernel(const float* __restrict__ th_t, const float* __restrict__ ph_t,
                                                                     const float* __restrict__ mu, const float* __restrict__ a,
                                                                     const float* __restrict__ nu, const float* __restrict__ b,
                                                                     const float* __restrict__ vt, const int* __restrict__ idx,
                                                                     float* __restrict__ out_t, float* __restrict__ w_out,
                                                                     float* __restrict__ c_out, long long rows, int fh, int fw, int gh,
                                                                     int gw, int Cv, int k, float inv_t, float kc) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * BS_WAVES + (threadIdx.x >> 6);      // b * Nq + p
    if (row >= rows) return;                                                          // (whole waves; the kernel has no barrier)
    const int Nq = fh * fw, Nk = gh * gw;
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
    long long key[BS_MAXK];
    float s[BS_MAXK];
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < BS_MAXK; ++r) {
        key[r] = kbase;
        s[r] = -INFINITY;
        if (r < k) {
            const int j = clamp_key(idx[row * k + r], Nk), qy = j / gw, qx = j - qy * gw;
            key[r] = kbase + j;
            float acc = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int dy = t / 3 - 1, dx = t % 3 - 1;
                if (((qmask >> t) & 1u) && in_grid(qy + dy, qx + dx, gh, gw)) acc = lane_fma4(q[t], row4(ph_t, key[r] + dy * gw + dx, lane), acc);
            }
            const float c = wave_sum(acc) - kmu * nu[key[r]];
            if (lane == r) c_out[row * k + r] = c;
            s[r] = za * b[key[r]] * c;
            m = fmaxf(m, s[r]);
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < BS_MAXK; ++r) {
        s[r] = r < k ? expf(s[r] - m) : 0.f;
        sum += s[r];
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int r = 0; r < BS_MAXK; ++r) {
        s[r] *= inv;
        if (r < k && lane == r) w_out[row * k + r] = s[r];
    }
    for (int ch = lane; ch < Cv; ch += kWave) {
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < BS_MAXK; ++r)
            if (r < k) acc = __builtin_fmaf(s[r], vt[key[r] * Cv + ch], acc);
        out_t[row * Cv + ch] = acc;
    }
}

// g [B,Nq,k] = dz inv_t a_p b_j: dloss / dR of the pair.  hb [B,Nq,k] = dz inv_t a_p c: the pair's share of db_j (the key kernel sums
// it over the key's list); dmu_p = -kc sum_r g_r nu_j, da_p = sum_r dz_r inv_t b_j c_r.  hb_out, dmu_out, da_out may be null.
__global__ __launch_bounds__(BS_THREADS) void box3_sparse_bwd_pair_kernel(const float* __restrict__ vt, const float* __restrict__ dout_t,
                                                                          const int* __restrict__ idx, const float* __restrict__ w,
                                                                          const float* __restrict__ c, const float* __restrict__ a,
                                                                          const float* __restrict__ nu, const float* __restrict__ b,
                                                                          float* __restrict__ g_out, float* __restrict__ hb_out,
                                                                          float* __restrict__ dmu_out, float* __restrict__ da_out,
                                                                          long long rows, int Nq, int Nk, int Cv, int k, float inv_t, float kc) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * BS_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long long kbase = (row / Nq) * Nk;
    long long key[BS_MAXK];
    float wr[BS_MAXK], dw[BS_MAXK];
#pragma unroll
    for (int r = 0; r < BS_MAXK; ++r) {
        key[r] = kbase + (r < k ? clamp_key(idx[row * k + r], Nk) : 0);
        wr[r] = r < k ? w[row * k + r] : 0.f;
        dw[r] = 0.f;
    }
    for (int ch = lane; ch < Cv; ch += kWave) {
        const float go = dout_t[row * Cv + ch];
#pragma unroll
        for (int r = 0; r < BS_MAXK; ++r)
            if (r < k) dw[r] = __builtin_fmaf(go, vt[key[r] * Cv + ch], dw[r]);
    }
    float dot = 0.f;
#pragma unroll
    for (int r = 0; r < BS_MAXK; ++r) {
        if (r < k) dw[r] = wave_sum(dw[r]);
        dot = __builtin_fmaf(wr[r], dw[r], dot);
    }
    const float a_p = a[row];
    float gnu = 0.f, da = 0.f;
#pragma unroll
    for (int r = 0; r < BS_MAXK; ++r) {
        if (r < k) {
            const float dzt = wr[r] * (dw[r] - dot) * inv_t, b_j = b[key[r]], c_r = c[row * k + r];
            const float g = dzt * a_p * b_j;
            gnu = __builtin_fmaf(g, nu[key[r]], gnu);
            da = __builtin_fmaf(dzt * b_j, c_r, da);
            if (lane == r) {
                g_out[row * k + r] = g;
                if (hb_out) hb_out[row * k + r] = dzt * a_p * c_r;
            }
        }
    }
    if (lane == 0) {
        if (dmu_out) dmu_out[row] = -kc * gnu;
        if (da_out) da_out[row] = da;
    }
}

// dtheta^T[m] = sum over the taps d (raster order) with p = m - d inside the content grid, over r ascending, of
//               g[p,r] [j_{p,r} + d inside the exemplar grid] phi^T[j_{p,r} + d];  a position nobody reaches writes its own zeros
__global__ __launch_bounds__(BS_THREADS) void box3_sparse_bwd_theta_kernel(const float* __restrict__ ph_t, const int* __restrict__ idx,
                                                                           const float* __restrict__ g, float* __restrict__ dth_t,
                                                                           long long rows, int fh, int fw, int gh, int gw, int k) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * BS_WAVES + (threadIdx.x >> 6);      // b * Nq + m
    if (row >= rows) return;
    const int Nq = fh * fw, Nk = gh * gw;
    const long long bq = row / Nq;
    const int m = (int)(row - bq * Nq), my = m / fw, mx = m - my * fw;
    const long long kbase = bq * Nk;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        if (!in_grid(my - dy, mx - dx, fh, fw)) continue;
        const long long prow = row - (dy * fw + dx);
        for (int r = 0; r < k; ++r) {
            const int j = clamp_key(idx[prow * k + r], Nk), qy = j / gw, qx = j - qy * gw;
            if (in_grid(qy + dy, qx + dx, gh, gw)) acc += g[prow * k + r] * row4(ph_t, kbase + j + dy * gw + dx, lane);
        }
    }
    *reinterpret_cast<f32x4*>(dth_t + row * BS_C + lane * 4) = acc;
}

// entries[offsets[key] .. offsets[key + 1]) are the flat positions e = (b Nq + p) k + r of the idx entries that name `key` = b Nk + q,
// ascending (ops._inverse_index_table, K42's).  Positions and ranges are clamped into the tables, and a tap is taken only where the
// entry's own (py, px) + d lies inside the content grid: a malformed table cannot send a read outside g / hb / w / mu / the rows.
//   dphi^T[n] = sum over the taps d (raster order) with q = n - d inside the exemplar grid, over list(q) in table order, of
//               g[e] [p + d inside the content grid] theta^T[p + d]
//   from list(n) alone: dv^T[n] = sum w[e] dout^T[p],  dnu_n = -kc sum g[e] mu_p,  db_n = sum hb[e]
// Every output may be null; a key nobody names gets zeros, written here.
__global__ __launch_bounds__(BS_THREADS) void box3_sparse_bwd_key_kernel(const float* __restrict__ th_t, const float* __restrict__ dout_t,
                                                                         const float* __restrict__ g, const float* __restrict__ hb,
                                                                         const float* __restrict__ w, const float* __restrict__ mu,
                                                                         const int* __restrict__ entries, const int* __restrict__ offsets,
                                                                         float* __restrict__ dph_t, float* __restrict__ dv_t,
                                                                         float* __restrict__ dnu, float* __restrict__ db, long long keys,
                                                                         int total, int fh, int fw, int gh, int gw, int Cv, int k, float kc) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long key = (long long)blockIdx.x * BS_WAVES + (threadIdx.x >> 6);      // b * Nk + n
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
            const int qbeg = min(max(offsets[qkey], 0), total), qend = min(max(offsets[qkey + 1], qbeg), total);
            for (int e = qbeg; e < qend; ++e) {
                const int pos = min(max(entries[e], 0), total - 1), prow = pos / k, p = prow % Nq, py = p / fw, px = p - py * fw;
                if (in_grid(py + dy, px + dx, fh, fw)) acc += g[pos] * row4(th_t, (long long)prow + dy * fw + dx, lane);
            }
        }
        *reinterpret_cast<f32x4*>(dph_t + key * BS_C + lane * 4) = acc;
    }
    const int beg = min(max(offsets[key], 0), total), end = min(max(offsets[key + 1], beg), total);
    if (dv_t) {
        for (int c0 = 0; c0 < Cv; c0 += 4 * kWave) {          // four channels per lane and walk of the list
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int e = beg; e < end; ++e) {
                const int pos = min(max(entries[e], 0), total - 1);
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
            const int pos = min(max(entries[e], 0), total - 1);
            if (dnu) sn = __builtin_fmaf(g[pos], mu[pos / k], sn);
            if (db) sb += hb[pos];
        }
        if (lane == 0) {
            if (dnu) dnu[key] = -kc * sn;
            if (db) db[key] = sb;
        }
    }
}

static int box3_sparse_check(const char* name, int B, int K, int fh, int fw, int gh, int gw, int Cv, int k, float inv_temperature) {
    COCOS_REQUIRE(B >= 1 && fh >= 1 && fw >= 1 && gh >= 1 && gw >= 1 && Cv >= 1 && inv_temperature > 0.f, COCOS_ERR_INVALID,
                  "%s: bad dims B=%d content grid %dx%d exemplar grid %dx%d Cv=%d", name, B, fh, fw, gh, gw, Cv);
    const long long Nq = (long long)fh * fw, Nk = (long long)gh * gw;
    COCOS_REQUIRE(k >= 1 && k <= COCOS_MATCH_TOPK_MAX && k <= Nk, COCOS_ERR_INVALID, "%s: k=%d: expected 1 <= k <= min(%d, Nk=%lld)", name, k,
                  COCOS_MATCH_TOPK_MAX, Nk);
    COCOS_REQUIRE(K == BS_C, COCOS_ERR_UNSUPPORTED, "%s: needs K == 256 (got %d)", name, K);
    COCOS_REQUIRE(Nq < 0x7fffffffll && Nk < 0x7fffffffll && B * Nq * k < 0x7fffffffll && B * Nk < 0x7fffffffll, COCOS_ERR_UNSUPPORTED,
                  "%s: B Nq k = %lld entries / B Nk = %lld keys exceed the 32-bit tables", name, B * Nq * k, B * Nk);
    return COCOS_OK;
}

static unsigned box3_sparse_blocks(long long rows) { return (unsigned)((rows + BS_WAVES - 1) / BS_WAVES); }

}  // namespace cocos

extern "C" int cocos_box3_sparse_softmax_warp_fwd(const float* th_t, const float* ph_t, const float* mu, const float* a, const float* nu,
                                                  const float* b, const float* v_t, const int* idx, float* out_t, float* w, float* c, int B,
                                                  int K, int fh, int fw, int gh, int gw, int Cv, int k, float inv_temperature,
                                                  cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_sparse_softmax_warp_fwd";
    COCOS_REQUIRE(th_t && ph_t && mu && a && nu && b && v_t && idx && out_t && w && c, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (int rc = box3_sparse_check(name, B, K, fh, fw, gh, gw, Cv, k, inv_temperature)) return rc;
    for (const void* p : {th_t, ph_t}) COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the theta / phi rows must be 16-byte aligned", name);
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_sparse_fwd_kernel, dim3(box3_sparse_blocks(rows)), dim3(BS_THREADS), 0, as_stream(stream), th_t, ph_t, mu, a, nu,
                       b, v_t, idx, out_t, w, c, rows, fh, fw, gh, gw, Cv, k, inv_temperature, (float)(9 * BS_C));
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
    if (int rc = box3_sparse_check(name, B, K, fh, fw, gh, gw, Cv, k, inv_temperature)) return rc;
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_sparse_bwd_pair_kernel, dim3(box3_sparse_blocks(rows)), dim3(BS_THREADS), 0, as_stream(stream), v_t, dout_t, idx,
                       w, c, a, nu, b, g, hb, dmu, da, rows, fh * fw, gh * gw, Cv, k, inv_temperature, (float)(9 * BS_C));
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_box3_sparse_softmax_warp_bwd_theta(const float* ph_t, const int* idx, const float* g, float* dth_t, int B, int K, int fh,
                                                        int fw, int gh, int gw, int k, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_sparse_softmax_warp_bwd_theta";
    COCOS_REQUIRE(ph_t && idx && g && dth_t, COCOS_ERR_INVALID, "%s: null pointer", name);
    if (int rc = box3_sparse_check(name, B, K, fh, fw, gh, gw, 1, k, 1.f)) return rc;
    for (const void* p : {(const void*)ph_t, (const void*)dth_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the phi rows and dth_t must be 16-byte aligned", name);
    const long long rows = (long long)B * fh * fw;
    hipLaunchKernelGGL(box3_sparse_bwd_theta_kernel, dim3(box3_sparse_blocks(rows)), dim3(BS_THREADS), 0, as_stream(stream), ph_t, idx, g,
                       dth_t, rows, fh, fw, gh, gw, k);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}

extern "C" int cocos_box3_sparse_softmax_warp_bwd_key(const float* th_t, const float* dout_t, const float* g, const float* hb, const float* w,
                                                      const float* mu, const int* entries, const int* offsets, float* dph_t, float* dv_t,
                                                      float* dnu, float* db, int B, int K, int fh, int fw, int gh, int gw, int Cv, int k,
                                                      cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_sparse_softmax_warp_bwd_key";
    COCOS_REQUIRE(entries && offsets && (dph_t || dv_t || dnu || db), COCOS_ERR_INVALID, "%s: null pointer", name);
    COCOS_REQUIRE(!dph_t || (th_t && g), COCOS_ERR_INVALID, "%s: null pointer (dph_t needs the theta rows and g)", name);
    COCOS_REQUIRE(!dv_t || (dout_t && w), COCOS_ERR_INVALID, "%s: null pointer (dv_t needs dout_t and w)", name);
    COCOS_REQUIRE(!dnu || (g && mu), COCOS_ERR_INVALID, "%s: null pointer (dnu needs g and mu)", name);
    COCOS_REQUIRE(!db || hb, COCOS_ERR_INVALID, "%s: null pointer (db needs hb)", name);
    if (int rc = box3_sparse_check(name, B, K, fh, fw, gh, gw, Cv, k, 1.f)) return rc;
    for (const void* p : {(const void*)th_t, (const void*)dph_t})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: the theta rows and dph_t must be 16-byte aligned", name);
    const long long keys = (long long)B * gh * gw;
    hipLaunchKernelGGL(box3_sparse_bwd_key_kernel, dim3(box3_sparse_blocks(keys)), dim3(BS_THREADS), 0, as_stream(stream), th_t, dout_t, g,
                       hb, w, mu, entries, offsets, dph_t, dv_t, dnu, db, keys, B * fh * fw * k, fh, fw, gh, gw, Cv, k, (float)(9 * BS_C));
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
