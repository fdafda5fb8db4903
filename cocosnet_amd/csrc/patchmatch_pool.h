// The integer side of a PatchMatch step, shared by K43 (patchmatch_f16x3.hip: the plane logit) and K57 (patchmatch_box3.hip: the box
// logit): the hash, the candidate pool of a query source by source, the wave-uniform candidate list.  Everything
// here is 32-bit integer arithmetic on wave-uniform values (the callers make the query row uniform with readfirstlane), so it stays on
// the scalar side, and a host restatement reproduces every pool exactly (tests/patchmatch_case.py).  What a SCORE is belongs to the
// kernel that includes this header; nothing below reads an operand.
//   own           idx_in[b,i,r], r < k (clamped into [0, Nk)); with idx_in == null the hashed positions pm_init_list makes
//   propagation   for the neighbours n = (y -+ d, x), (y, x -+ d) inside the query grid and r < k: the key position of idx_in[b,n,r]
//                 minus the offset (n - i); a candidate outside the key grid is skipped
//   random search for s < S and r < k: the own key position + (oy, ox), clamped into the key grid, oy / ox = hash mod (2 rho + 1) - rho,
//                 rho = max(1, R >> s)
#pragma once
#include "sparse_row.h"
#include "topk_list.h"

namespace cocos {

constexpr int PM_WAVES = 4;              // queries per workgroup, one per wave
constexpr int PM_THREADS = PM_WAVES * kWave;

__host__ __device__ __forceinline__ unsigned pm_fmix32(unsigned h) {      // the 32-bit murmur3 finaliser
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// the hash of (seed, iteration, query row b Nq + i, word): word = (r << 8) | (s << 1) | axis for the search, (r << 8) | 0xff for
// the random initialisation
__host__ __device__ __forceinline__ unsigned pm_hash(int seed, int iteration, int row, unsigned word) {
    unsigned h = pm_fmix32((unsigned)seed ^ 0x9e3779b9u);
    h = pm_fmix32(h ^ (unsigned)iteration);
    h = pm_fmix32(h ^ (unsigned)row);
    return pm_fmix32(h ^ word);
}

// The candidate list: K (score, key) pairs in the order of topk_before, empty slots (-inf, -1).  Unlike TopkList::push_ascending
// the keys arrive in ANY order and may repeat: a key already in the list is refused, the place of a new one is found by topk_before
// itself.  A NaN score never enters.  All loops are unrolled: the arrays stay in registers.
template <int K>
struct PoolList {
    float v[K];
    int i[K];

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int p = 0; p < K; ++p) { v[p] = -INFINITY; i[p] = -1; }
    }

    __device__ __forceinline__ void insert(float x, int j) {      // j >= 0
        bool fresh = true;
#pragma unroll
        for (int p = 0; p < K; ++p) fresh = fresh && i[p] != j;
#pragma unroll
        for (int p = K - 1; p >= 1; --p) {
            const bool up = fresh && topk_before(x, j, v[p - 1], i[p - 1]), here = fresh && topk_before(x, j, v[p], i[p]);
            v[p] = up ? v[p - 1] : (here ? x : v[p]);
            i[p] = up ? i[p - 1] : (here ? j : i[p]);
        }
        const bool first = fresh && topk_before(x, j, v[0], i[0]);
        v[0] = first ? x : v[0];
        i[0] = first ? j : i[0];
    }
};

// the k own candidates of query row `row` when there is no idx_in: hashed key positions, made pairwise distinct by linear probing
// (k <= Nk: the probe ends)
template <int K>
__device__ __forceinline__ void pm_init_list(int (&own)[K], int row, int k, int Nk, int seed, int iteration) {
#pragma unroll
    for (int r = 0; r < K; ++r) {
        own[r] = 0;
        if (r < k) {
            int p = (int)(pm_hash(seed, iteration, row, ((unsigned)r << 8) | 0xffu) % (unsigned)Nk);
            for (int tries = 0; tries < K; ++tries) {      // at most r earlier entries can collide, each at most once
                bool taken = false;
#pragma unroll
                for (int e = 0; e < K; ++e) taken = taken || (e < r && own[e] == p);
                if (!taken) break;
                p = p + 1 == Nk ? 0 : p + 1;
            }
            own[r] = p;
        }
    }
}

// the list of query row `row`: idx_in clamped into the key grid, or the random initialisation
template <int K>
__device__ __forceinline__ void pm_list(int (&out)[K], const int* __restrict__ idx_in, int row, int k, int Nk, int seed, int iteration) {
    if (idx_in) {
#pragma unroll
        for (int r = 0; r < K; ++r) out[r] = r < k ? clamp_key(idx_in[(long long)row * k + r], Nk) : 0;
    } else {
        pm_init_list<K>(out, row, k, Nk, seed, iteration);
    }
}

// what a step draws from: the two grids and the schedule of this launch
struct PmStep {
    int hq, wq, hk, wk;      // query grid, key grid
    int Nq, Nk;              // hq wq, hk wk
    int k, stride, S, R;     // candidates per query, propagation distance, search radii and the first radius
    int seed, iteration;
};

// the number of sources of a query: 0 the own list, 1 .. 4 the neighbours (y - d, x), (y + d, x), (y, x - d), (y, x + d), 5 + s the
// search at radius s
__device__ __forceinline__ int pm_sources(const PmStep& st) { return 5 + st.S; }

// the candidates of source `src` of query row `row` = b Nq + y wq + x, whose own list is `own`: key index, or -1: no candidate
template <int K>
__device__ __forceinline__ void pm_source(int (&cand)[K], int src, const int (&own)[K], const int* __restrict__ idx_in, int row, int b,
                                          int y, int x, const PmStep& st) {
    const int k = st.k, hq = st.hq, wq = st.wq, hk = st.hk, wk = st.wk;
    if (src == 0) {
#pragma unroll
        for (int r = 0; r < K; ++r) cand[r] = r < k ? own[r] : -1;
    } else if (src < 5) {
        const int stride = st.stride;
        const int dy = src == 1 ? -stride : (src == 2 ? stride : 0), dx = src == 3 ? -stride : (src == 4 ? stride : 0);
        const int ny = y + dy, nx = x + dx;
#pragma unroll
        for (int r = 0; r < K; ++r) cand[r] = -1;
        if (ny >= 0 && ny < hq && nx >= 0 && nx < wq) {
            int theirs[K];
            pm_list<K>(theirs, idx_in, b * st.Nq + ny * wq + nx, k, st.Nk, st.seed, st.iteration);
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int ky = theirs[r] / wk - dy, kx = theirs[r] % wk - dx;
                if (r < k && ky >= 0 && ky < hk && kx >= 0 && kx < wk) cand[r] = ky * wk + kx;
            }
        }
    } else {
        const int s = src - 5;
        const int rho = max(1, st.R >> s);
        const unsigned span = 2u * (unsigned)rho + 1u;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            cand[r] = -1;
            if (r < k) {
                const unsigned word = ((unsigned)r << 8) | ((unsigned)s << 1);
                const int oy = (int)(pm_hash(st.seed, st.iteration, row, word) % span) - rho;
                const int ox = (int)(pm_hash(st.seed, st.iteration, row, word | 1u) % span) - rho;
                const int ky = min(max(own[r] / wk + oy, 0), hk - 1), kx = min(max(own[r] % wk + ox, 0), wk - 1);
                cand[r] = ky * wk + kx;
            }
        }
    }
}

// What the two entry points require of the schedule alike (before any HIP call), in the order and the words K43 always had; Nk = hk wk
inline int pm_check_schedule(const char* name, int k, long long Nk, int stride, int radii, int radius0) {
    COCOS_REQUIRE(k >= 1 && k <= COCOS_MATCH_TOPK_MAX && k <= Nk, COCOS_ERR_UNSUPPORTED, "%s: k=%d: expected 1 <= k <= min(%d, Nk=%lld)",
                  name, k, COCOS_MATCH_TOPK_MAX, Nk);
    COCOS_REQUIRE(stride >= 1 && stride <= (1 << 20), COCOS_ERR_UNSUPPORTED, "%s: stride=%d: expected 1 .. 2^20", name, stride);
    COCOS_REQUIRE(radii >= 0 && radii <= COCOS_PATCHMATCH_MAX_RADII, COCOS_ERR_UNSUPPORTED, "%s: radii=%d: expected 0 .. %d", name, radii,
                  COCOS_PATCHMATCH_MAX_RADII);
    COCOS_REQUIRE(radius0 >= 0 && radius0 <= (1 << 20), COCOS_ERR_UNSUPPORTED, "%s: radius0=%d: expected 0 .. 2^20", name, radius0);
    return COCOS_OK;
}

// the 32-bit tables of a step: rows b Nq + i, entries (b Nq + i) k + r, keys b Nk + j
inline int pm_check_tables(const char* name, long long B, long long Nq, long long Nk, int k) {
    COCOS_REQUIRE(B * Nq < 0x7ffffff0ll && B * Nq * k < 0x7fffffffll && B * Nk < 0x7fffffffll, COCOS_ERR_UNSUPPORTED,
                  "%s: B Nq k = %lld entries / B Nk = %lld keys exceed the 32-bit tables", name, B * Nq * k, B * Nk);
    return COCOS_OK;
}

}  // namespace cocos
