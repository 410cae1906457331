"""The order vg_clip_topk / vg_clip_topk_host must return, in numpy, and the crafted tables both test files run it on.

`order(probs, k)`: one lexsort per row on (class index, -p) with the NaN rule in front -- probability descending, class index
ascending, -0.0 == +0.0, a NaN behind every number and NaNs among themselves by index.  `reference_vote` restates the reference's
vote (lidar_frame.py:269-285) entry by entry with numpy's own np.unique / np.mean."""
import ctypes

import numpy as np

SENTINEL_I, SENTINEL_F = np.int32(-77), np.float32(-5.5)
MAX_TOPK = 32
SIZES_K = (1, 2, 63, 64, 65, 127, 128, 129, 257, 1203, 4096)


def order(probs, k):
    """-> (idx [n, k] int32, score [n, k] float32: the table's own bits)"""
    probs = np.ascontiguousarray(probs, np.float32)
    n, K = probs.shape
    idx = np.zeros((n, k), np.int32)
    for i in range(n):
        nan = np.isnan(probs[i])
        neg = np.where(nan, np.float32(0), -probs[i])
        idx[i] = np.lexsort((np.arange(K), neg, nan))[:k]          # last key first: NaN flag, then -p, then the index
    return idx, np.take_along_axis(probs, idx.astype(np.int64), axis=1) if n else np.zeros((0, k), np.float32)


def ks_for(K):
    return sorted({k for k in (1, 2, 5, 32, K) if k <= min(K, MAX_TOPK)})


def crafted(K, seed=0):
    """{name: row [K] float32}: the tie and special-value patterns, placed where the kernel's lane / stride layout has its seams."""
    rng = np.random.default_rng(1000 * K + seed)
    base = (rng.random(K, dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    rows = {'distinct': base.copy(), 'softmax': None}
    z = rng.normal(size=K).astype(np.float32) * np.float32(3)
    e = np.exp(z - z.max())
    rows['softmax'] = (e / e.sum()).astype(np.float32)
    rows['all_equal'] = np.full(K, np.float32(1.0 / K), np.float32)

    def top_at(cols, value=0.75):
        r = base.copy()
        r[[c for c in cols if c < K]] = np.float32(value)
        return r
    c = 5 % K
    rows['one_stride'] = top_at((c, c + 64, c + 128))                          # one lane's classes
    rows['one_stride_far'] = top_at((c + 64 * 17, c + 64 * 3, c + 64 * 63))
    rows['neighbours'] = top_at((c, c + 1, c + 2))                             # neighbouring lanes
    rows['seam_63_64_65'] = top_at((63, 64, 65))
    rows['cut_group'] = top_at(tuple(int(x) for x in rng.choice(K, size=min(K, 9), replace=False)))    # 9 equal: k = 2, 5 cut it
    r = top_at((K - 1, K // 2, 0), 0.6)
    r[rng.choice(K, size=min(K, 40), replace=False)] = np.float32(0.25)      # a second tie group further down (k = 32 cuts it)
    rows['two_groups'] = r
    rows['levels'] = (rng.integers(0, 4, size=K) / 4).astype(np.float32)       # four levels: ties everywhere
    r = np.zeros(K, np.float32)
    sub = np.array([1e-45, 1e-40, 3e-39, 1e-45], np.float32)                   # denormals (two equal)
    pos = rng.choice(K, size=min(K, 4), replace=False)
    r[pos] = sub[:len(pos)]
    rows['zeros_denormals'] = r
    r = np.zeros(K, np.float32)
    r[::2] = np.float32(-0.0)                                                  # -0.0 beside +0.0: the index decides
    rows['signed_zeros'] = r
    r = base.copy() - np.float32(0.25)                                         # negative numbers, -0.0 and +0.0 among them
    r[c] = np.float32(-0.0)
    r[(c + 1) % K] = np.float32(0.0)
    rows['signed'] = r
    rows['all_nan'] = np.full(K, np.nan, np.float32)
    r = base.copy()
    r[(7 * K) // 11] = np.nan
    rows['one_nan'] = r
    r = np.full(K, np.nan, np.float32)                                          # numbers only in a few places: NaNs fill the top k
    r[rng.choice(K, size=min(K, 3), replace=False)] = np.float32([0.5, 0.5, -np.inf][:min(K, 3)])
    rows['mostly_nan'] = r
    r = base.copy()
    r[0 % K] = np.inf
    r[K - 1] = np.inf
    rows['infinities'] = r
    return rows


def crafted_table(K, seed=0):
    rows = crafted(K, seed)
    return list(rows), np.ascontiguousarray(np.stack(list(rows.values())), np.float32)


def host(lib, probs, k, n=None, n_classes=None, null=()):
    """vg_clip_topk_host on sentinel-filled outputs with one guard row behind them -> (status, idx, score, guard untouched)"""
    probs = np.ascontiguousarray(probs, np.float32)
    n = probs.shape[0] if n is None else n
    K = probs.shape[1] if n_classes is None else n_classes
    rows = max(n, 0) + 1
    kk = max(k, 1)
    idx = np.full((rows, kk), SENTINEL_I, np.int32)
    score = np.full((rows, kk), SENTINEL_F, np.float32)
    p = lambda a, name: None if name in null else a.ctypes.data_as(ctypes.c_void_p)
    st = lib.vg_clip_topk_host(p(probs, 'probs'), n, K, k, p(idx, 'idx'), p(score, 'score'))
    return st, idx, score


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def reference_vote(names, scores):
    """lidar_frame.py:269-285 for one detection: names [E] mapped names, scores [E] float32 -> (name, float32 score)"""
    names, scores = np.asarray(names), np.asarray(scores, np.float32)
    uniq, counts = np.unique(names, return_counts=True)
    if np.sum(counts[np.argmax(counts)] == counts) > 1:
        best, best_s = None, 0
        for nm in uniq:
            s = np.mean(scores[names == nm])
            if s > best_s:
                best, best_s = nm, s
        return best, best_s
    nm = uniq[np.argmax(counts)]
    return nm, np.mean(scores[names == nm])
