// K53: the adjoint of the row log-sum-exp of the match_kernel-3 logits — what turns a gradient on the lse of cocos_box3_match_f16x3
// into the family's G, so that the supervised match loss (row and column NLL) trains on the one x-box tensor T.
//
//   z[p,q]  = scale a_p b_q (ybox(T)[p,q] - kc mu_p nu_q)                    (box3_fused_f16x3.hip: K19 / K37 form it from T)
//   lse[p]  = log sum_q exp z[p,q]                                           (cocos_box3_match_f16x3's third output)
//   w[p,q]  = d loss / d z[p,q] = g_lse[p] exp(z[p,q] - lse[p])              (g_lse: the upstream gradient on lse, any magnitude)
//
// CONVENTION of g_blocked — that of cocos_box3_softmax_warp_bwd_f16x3, whose L = P (V.dO - D) is this kernel's w: what is written is
//   G[p,q] = w[p,q] scale a_p b_q = d loss / d ybox(T)[p,q]      — NOT d loss / dT (K20 applies the y box of the adjoint with the x box)
// in fp32, unscaled (K20 derives its power-of-two plane scale from *gmax_dev = max|G|), tile-blocked like the STORED T: [B][Nk/32]
// [Nq/32] blocks of 4 KB = [g][lane][4], registers 4g..4g+3 of a lane = keys 8g + 4 (lane >> 5) + 0..3, lane & 31 = query.  With
// COCOS_BOX3_T_TRANSPOSED the tile is transposed back in LDS and lands in block (qb, kt): the layout of the stored T.  With
// COCOS_BOX3_G_ACCUMULATE the block is read, added to and written back, and max|G| is that of the sum.  The statistics terms are the
// existing backward's with La = w scale a_p:  da_p = sum_q La tt / a_p,  dmu_p = -sum_q La kn_q,  db_q = sum_p La tt / b_q,
// dnu_q = -kc b_q sum_p La mu_p   (tt = b_q ybox(T) - mu_p kn_q,  kn_q = kc nu_q b_q).
//
// The T walk is K37's and K19's: one workgroup per 128 queries, wave = 32-query block, 32-key tiles in ascending order, three 4 KB
// blocks of T per tile two tiles ahead, the per-key statistics in LDS (a ring of 2048-key chunks above 4096 keys), the transposed read
// through a per-wave LDS image.  The statements that form tt are bx_logits' of box3_fused_f16x3.hip, in its order (that file is not
// touched: its helpers have internal shape there, so the skeleton is restated below, inside an unnamed namespace): z is the readout's
// bit for bit.  Exponent (K49's rule): the difference is rounded ONCE, fma(tt, scale a_p, -lse), and clamped at 0 from above before
// the exp2, so |w| <= |g_lse| whatever the lse holds.
// No MFMA, no atomics: a streaming pass, 4 B read (each T block three times, two of them cache hits) and 4 B written per logit (8 + 4
// under ACCUMULATE).  Row sums live in registers in key order; column sums go through the existing backward's colpart scheme (four
// waves' images in LDS, a fixed DPP fold, one partial per workgroup, folded in workgroup order by the second launch); max|G| leaves
// as one value per wave and is folded by the second launch's first workgroup — every reduction has a fixed order: bitwise reproducible.
#include "box3_common.h"

namespace cocos {
namespace {

constexpr int LB3_KCH = 2048, LB3_TCH = LB3_KCH / 32;      // the statistics ring (BX_KCH / BX_TCH)
constexpr int LB3_XT_ROW = 36, LB3_XT_FLOATS = 32 * LB3_XT_ROW;
constexpr int LB3_FLAG_TRANSPOSED = 1, LB3_FLAG_ACCUMULATE = 2;

struct BxTile {
    f32x4 s[3][4];      // [dy + 1][g]: accumulator registers 4g..4g+3
};

struct BxGeom {
    __amdgpu_buffer_rsrc_t t_rs;
    int qblk, py, tpr, tpr_log2, himg, nqblk;
    unsigned lane_off;      // lane * 16
    const float* kstat;     // LDS: [b_q | kc nu_q b_q] of this sample's keys (x 2 buffers when chunked)
    int nk;                 // keys per LDS buffer
    float* xt;              // transposed T: this wave's [32][LB3_XT_ROW] floats of LDS; nullptr = T as stored
};

// x[4g + e] of lane (h, c) = element (8g + 4h + e, c) of a 32 x 32 matrix  ->  the same registers of the TRANSPOSED matrix
__device__ __forceinline__ void bx_transpose32(float (&x)[16], float* xt, int h, int c) {
    float* row = xt + c * LB3_XT_ROW + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(row + 8 * g) = f32x4{x[4 * g], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3]};
    __builtin_amdgcn_wave_barrier();      // one wave's LDS instructions execute in order: no workgroup barrier
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) x[4 * g + e] = xt[(8 * g + 4 * h + e) * LB3_XT_ROW + c];
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void bx_fetch(BxTile& tl, const BxGeom& gm, int t, int ntiles) {
    const int tc = min(t, ntiles - 1);                  // look-ahead past the end re-reads the last tile
    const int ky = tc >> gm.tpr_log2;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int dy = d - 1;
        const bool ok = (unsigned)(gm.py + dy) < (unsigned)gm.himg && (unsigned)(ky + dy) < (unsigned)gm.himg;
        const int kb = tc + dy * gm.tpr, qb = gm.qblk + dy * gm.tpr;
        const int blk = ok ? (gm.xt ? qb * gm.nqblk + kb : kb * gm.nqblk + qb) : 0;
        const unsigned voff = ok ? gm.lane_off : kBufOob;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            tl.s[d][g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                gm.t_rs, (int)voff, (int)((unsigned)blk * 4096u + (unsigned)g * 1024u), 0));
    }
}

__device__ __forceinline__ void bx_stage_stats(float* kstat, const float* __restrict__ b_k, const float* __restrict__ nu_k,
                                               int cap, int n, float kc, int tid) {
    for (int i = tid; i < n; i += 256) {
        const float bq = b_k[i];
        kstat[i] = bq;
        kstat[cap + i] = kc * nu_k[i] * bq;
    }
}
template <bool CHUNKED>
__device__ __forceinline__ void bx_stage_next_chunk(float* kstat, const float* __restrict__ b_k, const float* __restrict__ nu_k,
                                                    int t, int ntiles, float kc, int tid) {
    if (CHUNKED && (t & (LB3_TCH - 1)) == 0 && t + LB3_TCH < ntiles) {
        const int c1 = t / LB3_TCH + 1;
        bx_stage_stats(kstat + (c1 & 1) * 2 * LB3_KCH, b_k + c1 * LB3_KCH, nu_k + c1 * LB3_KCH, LB3_KCH,
                       min(LB3_KCH, ntiles * 32 - c1 * LB3_KCH), kc, tid);
    }
}

// tt[r] = b_q * (T_sum) - mu_p * kc * nu_q * b_q  (the logit without its per-query factor scale * a_p), b_q and kn_q per register
template <bool CHUNKED>
__device__ __forceinline__ void bx_logits(const BxTile& tl, const BxGeom& gm, int t, int h, float mu_p, float (&tt)[16],
                                          float (&bq)[16], float (&kn)[16], int lane_c) {
    const float* ks = gm.kstat + (CHUNKED ? ((t / LB3_TCH) & 1) * 2 * LB3_KCH + (t & (LB3_TCH - 1)) * 32 : t * 32);
    float ts[16];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            ts[4 * g + e] = (tl.s[0][g][e] + tl.s[2][g][e]) + tl.s[1][g][e];
    if (gm.xt) bx_transpose32(ts, gm.xt, h, lane_c);      // (workgroup-uniform: one branch per tile)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(ks + 8 * g + 4 * h);
        const f32x4 k4 = *reinterpret_cast<const f32x4*>(ks + gm.nk + 8 * g + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 4 * g + e;
            bq[r] = b4[e];
            kn[r] = k4[e];
            tt[r] = __builtin_fmaf(bq[r], ts[r], -(mu_p * kn[r]));
        }
    }
}

// exchange with lane c ^ MASK inside a row of 16 lanes, on the DPP path
template <int MASK>
__device__ __forceinline__ float bx_xchg(float v) {
    const int x = __builtin_bit_cast(int, v);
    int r;
    if (MASK == 1) r = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, false);            // quad_perm [1,0,3,2]
    else if (MASK == 2) r = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, false);       // quad_perm [2,3,0,1]
    else if (MASK == 4)
        r = __builtin_amdgcn_update_dpp(0, __builtin_amdgcn_update_dpp(0, x, 0x141, 0xf, 0xf, false), 0x1B, 0xf, 0xf, false);
    else r = __builtin_amdgcn_update_dpp(0, x, 0x128, 0xf, 0xf, false);                     // row_ror:8
    return __builtin_bit_cast(float, r);
}
// x[0..3] = registers 4w..4w+3 of the summed image -> the column sum of register 4w + 2*b0 + b1 (b_k = bit k of the lane)
__device__ __forceinline__ float bx_colsum4(const float (&x)[4], int c) {
    const bool up0 = (c & 1) != 0, up1 = (c & 2) != 0;
    const float y0 = (up0 ? x[2] : x[0]) + bx_xchg<1>(up0 ? x[0] : x[2]);
    const float y1 = (up0 ? x[3] : x[1]) + bx_xchg<1>(up0 ? x[1] : x[3]);
    float z = (up1 ? y1 : y0) + bx_xchg<2>(up1 ? y0 : y1);
    z += bx_xchg<4>(z);
    z += bx_xchg<8>(z);
    return z + __shfl_xor(z, 16, 64);
}

// LDS: [2 buf][4 waves][2 quantities][4 groups][64 lanes][4] column images | [b | kn] statistics | (transposed) 4 x-pose images
template <bool CHUNKED>
__global__ __launch_bounds__(256, 1) void box3_lse_bwd_kernel(
    const float* __restrict__ T, const float* __restrict__ mu_q, const float* __restrict__ a_q, const float* __restrict__ nu_k,
    const float* __restrict__ b_k, const float* __restrict__ lse, const float* __restrict__ g_lse, float* __restrict__ G,
    float* __restrict__ dmu, float* __restrict__ da, float* __restrict__ colpart, float* __restrict__ wavemax, int B, int Nq, int Nk,
    int himg, int wimg, float kc, float scale, int flags) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bx_smem[];
    float* const colacc = reinterpret_cast<float*>(bx_smem);
    float* const kstat = colacc + 2 * 4 * 2048;

    const int tid = threadIdx.x, lane = tid & 63;
    // wave-uniform BY CONSTRUCTION for the compiler too: derived from threadIdx alone it lives in a VGPR and every block load / store that
    // depends on it sits in a waterfall loop
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, c = lane & 31;
    const int nqb = Nq / 128;
    const int vb = xcd_remap(blockIdx.x, gridDim.x);
    const int b = vb / nqb, wg = vb % nqb, q0 = wg * 128;
    const int i_lane = q0 + wave * 32 + c;
    const float* const bk_b = b_k + (size_t)b * Nk;
    const float* const nu_b = nu_k + (size_t)b * Nk;
    bx_stage_stats(kstat, bk_b, nu_b, CHUNKED ? LB3_KCH : Nk, CHUNKED ? LB3_KCH : Nk, kc, tid);

    const __amdgpu_buffer_rsrc_t G_rs = make_rsrc(G + (size_t)b * Nk * Nq, (size_t)Nk * Nq * 4);
    BxGeom gm;
    gm.t_rs = make_rsrc(T + (size_t)b * Nk * Nq, (size_t)Nk * Nq * 4);
    gm.kstat = kstat;
    gm.nk = CHUNKED ? LB3_KCH : Nk;
    gm.tpr = wimg / 32;
    gm.tpr_log2 = gm.tpr == 4 ? 2 : 1;          // (64- or 128-wide grids: cocos_box3_fused_supported)
    gm.qblk = (q0 >> 5) + wave;
    gm.py = gm.qblk >> gm.tpr_log2;
    gm.himg = himg;
    gm.nqblk = Nq >> 5;
    gm.lane_off = (unsigned)lane * 16u;
    gm.xt = (flags & LB3_FLAG_TRANSPOSED) ? kstat + (CHUNKED ? 4 * LB3_KCH : 2 * Nk) + wave * LB3_XT_FLOATS : nullptr;
    const bool accumulate = (flags & LB3_FLAG_ACCUMULATE) != 0;

    const size_t at = (size_t)b * Nq + i_lane;
    const float mu_p = mu_q[at];
    const float a_p = a_q[at];
    const float a_n = a_p * scale;                     // natural-domain factor: z = tt * a_n
    const float lse_p = lse[at];
    const float ga = (g_lse ? g_lse[at] : 0.f) * a_n;  // La = w a_n = (g a_n) e,  e = exp(z - lse) in [0, 1]

    float* const cp_b = colpart + ((size_t)b * nqb + wg) * 2 * Nk;
    // behind the barrier that ended tile t: register group `wave` of the four waves' images, summed -> column sums -> colpart
    auto reduce_cols = [&](int t) {
        const float* a = colacc + (t & 1) * 4 * 2048 + wave * 256 + lane * 4;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            f32x4 acc = *reinterpret_cast<const f32x4*>(a + q * 1024);
#pragma unroll
            for (int w = 1; w < 4; ++w) acc += *reinterpret_cast<const f32x4*>(a + w * 2048 + q * 1024);
            const float x[4] = {acc[0], acc[1], acc[2], acc[3]};
            const float z = bx_colsum4(x, c);
            if (c < 4) cp_b[(size_t)q * Nk + t * 32 + 8 * wave + 4 * h + 2 * (c & 1) + ((c >> 1) & 1)] = z;
        }
    };

    const int ntiles = Nk / 32;
    BxTile tl0, tl1;        // tiles t and t + 1 in flight
    bx_fetch(tl0, gm, 0, ntiles);
    bx_fetch(tl1, gm, 1, ntiles);
    __syncthreads();

    float r2 = 0.f, rm = 0.f, gabs = 0.f;
    auto do_tile = [&](int t, BxTile& tl) __attribute__((always_inline)) {
        const int buf = t & 1;
        if (t > 0) reduce_cols(t - 1);
        bx_stage_next_chunk<CHUNKED>(kstat, bk_b, nu_b, t, ntiles, kc, tid);
        float tt[16], bq[16], kn[16];
        bx_logits<CHUNKED>(tl, gm, t, h, mu_p, tt, bq, kn, c);
        bx_fetch(tl, gm, t + 2, ntiles);
        float x1[16], x2[16], gv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // the difference rounded once, clamped at 0 from above: e <= 1 whatever lse holds (fminf drops a NaN)
            const float e = fast_exp2(fminf(__builtin_fmaf(tt[r], a_n, -lse_p) * kLog2e, 0.f));
            const float La = ga * e;
            gv[r] = La * bq[r];
            x1[r] = La * tt[r];
            x2[r] = La * mu_p;
            r2 += x1[r];
            rm = __builtin_fmaf(La, kn[r], rm);
        }
        if (gm.xt) bx_transpose32(gv, gm.xt, h, c);
        const unsigned blk = (unsigned)((gm.xt ? gm.qblk * gm.nqblk + t : t * gm.nqblk + gm.qblk) * 4096);
        if (accumulate) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 old = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(G_rs, (int)gm.lane_off,
                                                                                                 (int)(blk + (unsigned)g * 1024u), 0));
#pragma unroll
                for (int e = 0; e < 4; ++e) gv[4 * g + e] += old[e];
            }
        }
        f32x4 gout[4];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            gout[r >> 2][r & 3] = gv[r];
            gabs = fmaxf(gabs, fabsf(gv[r]));
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, gout[g]), G_rs, (int)gm.lane_off,
                                                   (int)(blk + (unsigned)g * 1024u), 2);      // nt: a stream for K20
        // (a 16-byte store whose soffset is a REGISTER: LLVM models no write-after-read hazard on its data registers, gfx950 has one —
        //  box3_fused_f16x3.hip.  Keep the four quads untouched for a few cycles.)
        asm volatile("s_nop 4" : : "v"(gout[0]), "v"(gout[1]), "v"(gout[2]), "v"(gout[3]));
        // (slot of tile t - 2 was read by every wave before it passed the barrier of tile t - 1)
        float* a = colacc + buf * 4 * 2048 + wave * 2048 + lane * 4;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            *reinterpret_cast<f32x4*>(a + g * 256) = f32x4{x1[4 * g], x1[4 * g + 1], x1[4 * g + 2], x1[4 * g + 3]};
            *reinterpret_cast<f32x4*>(a + 1024 + g * 256) = f32x4{x2[4 * g], x2[4 * g + 1], x2[4 * g + 2], x2[4 * g + 3]};
        }
        __syncthreads();      // (also the chunk ring's barrier: every wave is past chunk c - 1 before chunk c + 1 is staged over it)
    };
    {
        int t = 0;
        for (; t + 1 < ntiles; t += 2) {
            do_tile(t, tl0);
            do_tile(t + 1, tl1);
        }
        if (t < ntiles) do_tile(t, tl0);
    }
    reduce_cols(ntiles - 1);

    r2 += swap_half(r2);
    rm += swap_half(rm);
    if (h == 0) {
        da[at] = r2 / a_p;
        dmu[at] = -rm;          // (rm carries the factor a_n already)
    }
    gabs = wave_max_dpp(gabs);
    if (lane == 0) wavemax[(size_t)vb * 4 + wave] = gabs;
}

// d nu[b,q] = -kc * b_q * sum_wg colpart[b,wg,1,q];   d b[b,q] = sum_wg colpart[b,wg,0,q] / b_q   (workgroup order);  the first
// workgroup also folds the per-wave maxima into *gmax (a maximum: the order does not matter, and no atomic is needed)
__global__ __launch_bounds__(256) void box3_lse_col_reduce_kernel(const float* __restrict__ colpart, const float* __restrict__ wavemax,
                                                                  const float* __restrict__ b_k, float* __restrict__ dnu,
                                                                  float* __restrict__ db, float* __restrict__ gmax, int B, int nwg, int Nk,
                                                                  float kc) {
    __shared__ float red[4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * Nk) {
        const int b = i / Nk, q = i % Nk;
        float c2 = 0.f, cm = 0.f;
        for (int w = 0; w < nwg; ++w) {
            const float* p = colpart + ((size_t)b * nwg + w) * 2 * Nk;
            c2 += p[q];
            cm += p[Nk + q];
        }
        const float bq = b_k[i];
        dnu[i] = -kc * bq * cm;
        db[i] = c2 / bq;
    }
    if (blockIdx.x == 0) {
        float m = 0.f;
        for (int j = threadIdx.x; j < B * nwg * 4; j += 256) m = fmaxf(m, wavemax[j]);
        m = wave_max_dpp(m);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) *gmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    }
}

}  // namespace
}  // namespace cocos

extern "C" size_t cocos_box3_lse_bwd_colpart_bytes(int B, int Nq, int Nk) {
    if (B < 1 || Nq < 128 || Nk < 1) return 0;
    return ((size_t)B * (Nq / 128) * 2 * Nk + (size_t)B * (Nq / 128) * 4) * sizeof(float);      // column partials, then one max|G| per wave
}

extern "C" int cocos_box3_lse_bwd_f16x3(const float* t_blocked, const float* mu_q, const float* a_q, const float* nu_k, const float* b_k,
                                        const float* lse, const float* g_lse, float* g_blocked, float* dmu, float* da, float* dnu,
                                        float* db, void* colpart, float* gmax_dev, int B, int Nq, int Nk, int grid_h, int grid_w,
                                        float k_unfolded, float scale, int flags, cocos_stream_t stream) {
    using namespace cocos;
    const char* name = "box3_lse_bwd_f16x3";
    COCOS_REQUIRE((flags & ~(LB3_FLAG_TRANSPOSED | LB3_FLAG_ACCUMULATE)) == 0, COCOS_ERR_INVALID,
                  "%s: flags=%d (bit 0: T transposed, bit 1: add G to g_blocked)", name, flags);
    COCOS_REQUIRE(t_blocked && mu_q && a_q && nu_k && b_k && lse && g_blocked && dmu && da && dnu && db && colpart && gmax_dev,
                  COCOS_ERR_INVALID, "%s: null pointer (g_lse alone may be null: zeros)", name);
    COCOS_REQUIRE(B >= 1 && scale > 0.f, COCOS_ERR_INVALID, "%s: bad B=%d / scale", name, B);
    COCOS_REQUIRE(cocos_box3_fused_supported(Nq, Nk, 1, grid_h, grid_w), COCOS_ERR_UNSUPPORTED,
                  "%s: needs a 64- or 128-wide grid with Nq == Nk == h*w, Nq %% 256 == 0 (Nq=%d Nk=%d grid %dx%d)", name, Nq, Nk, grid_h,
                  grid_w);
    for (const void* p : {(const void*)t_blocked, (const void*)g_blocked, (const void*)nu_k, (const void*)b_k, (const void*)colpart})
        COCOS_REQUIRE(aligned16(p), COCOS_ERR_INVALID, "%s: T, G, nu, b and colpart must be 16-byte aligned", name);
    COCOS_REQUIRE((long long)B * (Nq / 128) < 0x7fffffffll / 4, COCOS_ERR_UNSUPPORTED, "%s: grid too large", name);
    const bool chunked = Nk > 2 * LB3_KCH;
    const size_t smem = (size_t)(2 * 4 * 2048 + (chunked ? 4 * LB3_KCH : 2 * Nk)) * sizeof(float) +
                        ((flags & LB3_FLAG_TRANSPOSED) ? (size_t)4 * LB3_XT_FLOATS * sizeof(float) : 0);
    float* const cp = static_cast<float*>(colpart);
    float* const wavemax = cp + (size_t)B * (Nq / 128) * 2 * Nk;
    hipStream_t s = as_stream(stream);
    auto kern = chunked ? box3_lse_bwd_kernel<true> : box3_lse_bwd_kernel<false>;
    COCOS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kern, dim3(B * (Nq / 128)), dim3(256), smem, s, t_blocked, mu_q, a_q, nu_k, b_k, lse, g_lse, g_blocked, dmu, da, cp,
                       wavemax, B, Nq, Nk, grid_h, grid_w, k_unfolded, scale, flags);
    COCOS_HIP_CHECK(hipGetLastError());
    const int n = B * Nk;
    hipLaunchKernelGGL(box3_lse_col_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, s, cp, wavemax, b_k, dnu, db, gmax_dev, B, Nq / 128,
                       Nk, k_unfolded);
    COCOS_HIP_CHECK(hipGetLastError());
    return COCOS_OK;
}
