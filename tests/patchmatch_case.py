"""A numpy restatement of one PatchMatch step (K43, cocosnet_amd/csrc/patchmatch_f16x3.hip) for the tests: the integer hash, the
candidate pool of every query (own, propagated, random search; the random initialisation when there is no table) and fp64 scores from
the operand-plane values.  Everything that chooses a candidate is integer arithmetic, so the pools are the kernel's exactly.

    H(seed, iteration, row, word) = f(f(f(f(seed ^ 0x9e3779b9) ^ iteration) ^ row) ^ word)   on uint32, row = b Nq + i,
    f(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16         (murmur3's finaliser)
    search:  word = (r << 8) | (s << 1) | axis (0: y, 1: x), offset = H mod (2 rho + 1) - rho, rho = max(1, R >> s)
    init:    word = (r << 8) | 0xff, p_r = H mod Nk, stepped by +1 mod Nk while it equals an earlier p_e (e < r)
"""
import numpy as np

_M = np.uint64(0xFFFFFFFF)


def _u(x):
    return np.asarray(x).astype(np.int64).astype(np.uint64) & _M      # (two's complement for negative seeds)


def fmix32(h):
    h = _u(h)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & _M
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & _M
    h ^= h >> np.uint64(16)
    return h


def pm_hash(seed, iteration, row, word):
    h = fmix32(_u(seed) ^ np.uint64(0x9E3779B9))
    h = fmix32(h ^ _u(iteration))
    h = fmix32(h ^ _u(row))
    return fmix32(h ^ _u(word))


def init_table(seed, iteration, B, Nq, Nk, k):
    """[B,Nq,k] int64: the random initialisation of every query"""
    rows = np.arange(B * Nq, dtype=np.int64)
    own = np.zeros((B * Nq, k), dtype=np.int64)
    for r in range(k):
        p = (pm_hash(seed, iteration, rows, (r << 8) | 0xFF) % np.uint64(Nk)).astype(np.int64)
        while True:
            taken = (own[:, :r] == p[:, None]).any(axis=1)
            if not taken.any():
                break
            p = np.where(taken, (p + 1) % Nk, p)
        own[:, r] = p
    return own.reshape(B, Nq, k)


def pool(idx_in, B, grids, k, stride, S, R, seed, iteration):
    """[B,Nq,k (5 + S)] int64: every candidate of every query, -1 where there is none (a neighbour outside the query grid, a
    propagated key outside the key grid).  idx_in [B,Nq,k] (any integers: clamped into the key grid) or None (random initialisation).
    Order: own, the neighbours (y - d, x), (y + d, x), (y, x - d), (y, x + d), then the search radius by radius."""
    (hq, wq), (hk, wk) = grids
    Nq, Nk = hq * wq, hk * wk
    table = init_table(seed, iteration, B, Nq, Nk, k) if idx_in is None else np.clip(np.asarray(idx_in, dtype=np.int64), 0, Nk - 1)
    grid = table.reshape(B, hq, wq, k)
    ys, xs = np.arange(hq).reshape(1, hq, 1, 1), np.arange(wq).reshape(1, 1, wq, 1)
    parts = [grid]
    for dy, dx in ((-stride, 0), (stride, 0), (0, -stride), (0, stride)):
        ny, nx = ys + dy, xs + dx
        inside = (ny >= 0) & (ny < hq) & (nx >= 0) & (nx < wq)
        theirs = grid[:, np.clip(ny, 0, hq - 1).reshape(-1)][:, :, np.clip(nx, 0, wq - 1).reshape(-1)]
        ky, kx = theirs // wk - dy, theirs % wk - dx
        ok = inside & (ky >= 0) & (ky < hk) & (kx >= 0) & (kx < wk)
        parts.append(np.where(ok, ky * wk + kx, -1))
    rows = np.arange(B * Nq, dtype=np.int64).reshape(B, hq, wq, 1)
    rs = np.arange(k, dtype=np.int64).reshape(1, 1, 1, k)
    for s in range(S):
        rho = max(1, R >> s)
        word = (rs << 8) | (s << 1)
        oy = (pm_hash(seed, iteration, rows, word) % np.uint64(2 * rho + 1)).astype(np.int64) - rho
        ox = (pm_hash(seed, iteration, rows, word | 1) % np.uint64(2 * rho + 1)).astype(np.int64) - rho
        parts.append(np.clip(grid // wk + oy, 0, hk - 1) * wk + np.clip(grid % wk + ox, 0, wk - 1))
    return np.concatenate(parts, axis=3).reshape(B, Nq, k * (5 + S))


def plane_values(hi, lo, scale):
    """fp64 [B,N,256]: what the kernels read from a position-major f16 hi / lo plane pair (torch tensors, any device)"""
    return (hi.double().cpu().numpy() + lo.double().cpu().numpy()) / scale


def scores(qv, kv, cand, inv_t):
    """fp64 [B,Nq,P]: inv_t <q_i, k_j> for the candidates `cand` [B,Nq,P] (-inf where cand is -1)"""
    B = qv.shape[0]
    out = np.stack([np.einsum("ic,ipc->ip", qv[b], kv[b][np.maximum(cand[b], 0)]) for b in range(B)]) * inv_t
    return np.where(cand >= 0, out, -np.inf)


def kth_best_distinct(cand, sc, k):
    """fp64 [B,Nq]: the k-th largest score over the DISTINCT keys of every pool (-inf where a pool holds fewer than k), and the number
    of distinct keys [B,Nq]"""
    B, Nq, _ = cand.shape
    kth, count = np.full((B, Nq), -np.inf), np.zeros((B, Nq), dtype=np.int64)
    for b in range(B):
        for i in range(Nq):
            keys, first = np.unique(cand[b, i][cand[b, i] >= 0], return_index=True)
            vals = np.sort(sc[b, i][cand[b, i] >= 0][first])[::-1]
            count[b, i] = len(keys)
            if len(keys) >= k:
                kth[b, i] = vals[k - 1]
    return kth, count
