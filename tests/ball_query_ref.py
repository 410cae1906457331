"""Dense reference and scenes for the ball query (csrc/cluster_ball_query.inc: k_cl_ball_query, vg_ball_query_host).  TEST INFRASTRUCTURE ONLY.

The reference is numpy over ALL query x target pairs: `neighbors_ref.d2_f32`, then `np.flatnonzero(d2 < r2)[:nsample]` per query, padded
with the first hit (an empty ball: zeros).  No cells, no buffer, no sort: nothing the kernel's selection can get wrong exists here.
The scenes of tests/neighbors_ref.py are used as they are; the ones built here aim at the kernel's own constants.
"""
import functools

import numpy as np

import neighbors_ref as nr

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------ the reference
def d2_matrix(query, target):
    """float32 d2 of every pair [nq, nt] (rows with a coordinate that is not finite give NaN / inf: no hit)"""
    q, t = nr._xyz(query), nr._xyz(target)
    out = np.empty((len(q), len(t)), F32)
    rows = max(1, (1 << 22) // max(len(t), 1))
    with np.errstate(all='ignore'):
        for a in range(0, len(q), rows):
            out[a:a + rows] = nr.d2_f32(q[a:a + rows, None, :], t[None, :, :])
    return out


def from_d2(d2, r2, nsample, inclusive=False):
    """-> (idx int32 [nq, nsample], cnt int32 [nq]) from the pair distances (`inclusive`: <=, the WRONG rule, for the fault checks)"""
    r2 = F32(r2)
    with np.errstate(invalid='ignore'):
        hit = d2 <= r2 if inclusive else d2 < r2
    idx, cnt = np.zeros((len(d2), nsample), np.int32), np.zeros(len(d2), np.int32)
    for i in range(len(d2)):
        h = np.flatnonzero(hit[i])[:nsample]
        if len(h):
            idx[i] = h[0]
            idx[i, :len(h)] = h
            cnt[i] = len(h)
    return idx, cnt


def ball_query(query, target, r2, nsample, inclusive=False):
    return from_d2(d2_matrix(query, target), r2, nsample, inclusive)


def count_from_idx(idx):
    """the count the reference project derives from the table (pointcloud_utils.py:86-87), for rows whose ball is not empty"""
    return np.count_nonzero(idx != idx[:, :1], axis=1) + 1


def same(got_idx, got_cnt, want_idx, want_cnt):
    """'' or one line about the first query whose row or count differs (exact equality, every entry, the padding included)"""
    got_idx, want_idx = np.asarray(got_idx), np.asarray(want_idx)
    if got_idx.shape != want_idx.shape:
        return f'idx shape {got_idx.shape}, want {want_idx.shape}'
    bad = (got_idx != want_idx).any(1)
    if got_cnt is not None:
        got_cnt = np.asarray(got_cnt)
        if got_cnt.shape != np.asarray(want_cnt).shape:
            return f'cnt shape {got_cnt.shape}, want {np.asarray(want_cnt).shape}'
        bad = bad | (got_cnt != want_cnt)
    if not bad.any():
        return ''
    i = int(np.flatnonzero(bad)[0])
    k = np.flatnonzero(got_idx[i] != want_idx[i])
    at = f'first at column {int(k[0])}: got {int(got_idx[i, k[0]])} want {int(want_idx[i, k[0]])}' if len(k) else 'rows equal'
    gc = '-' if got_cnt is None else int(got_cnt[i])
    return f'{int(bad.sum())} of {len(bad)} queries differ; first: query {i} cnt got {gc} want {int(want_cnt[i])}, {at}'


# ------------------------------------------------------------------------------------------------------------ the host form
def _p(a):
    import ctypes
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


def host(query, target, r2, nsample, qstride=None, tstride=None, want_cnt=True, rc=0):
    """vg_ball_query_host on the rows as given -> (idx, cnt), both poisoned with -7 first"""
    from vilgod_amd._lib import lib
    q, t = np.ascontiguousarray(query, F32), np.ascontiguousarray(target, F32)
    idx, cnt = np.full((len(q), max(nsample, 0)), -7, np.int32), np.full(len(q), -7, np.int32)
    got = lib.vg_ball_query_host(_p(t), len(t), tstride or (t.shape[1] if t.ndim == 2 else 3), _p(q), len(q), qstride or (q.shape[1] if q.ndim == 2 else 3),
                                 float(r2), nsample, _p(idx), _p(cnt) if want_cnt else None)
    assert got == rc, (got, rc)
    return idx, cnt


# ------------------------------------------------------------------------------------------------------------ scenes
NSAMPLES = (1, 2, 63, 64, 65, 100, 1000, 1024)
DENSE_R2 = (F32(0.09), F32(0.2), F32(10.24))            # 0 .. 873, 0 .. 1 901 and 2 153 .. 3 003 hits per query of `dense_cell`


def orders(n, seed=7):
    """three target orders: as built, reversed, a seeded permutation"""
    return [np.arange(n), np.arange(n)[::-1].copy(), np.random.default_rng(seed).permutation(n)]


def cand():
    from vilgod_amd.ball_query import BALL_QUERY_CAND
    return BALL_QUERY_CAND


@functools.lru_cache(maxsize=None)
def built(hits, nlow, offset=(140.0, -90.0, 3.0)):
    """ONE query with exactly `hits` targets inside r2 = 0.09.  The query sits 0.05 m inside the upper corner of its cell.  Rows
    0 .. nlow - 1 -- the lowest -- lie in the cell diagonally above (x + 1, y + 1, z + 1), the LAST cell of the reach cube in the
    kernel's z, y, x order; the other hits lie in the query's own cell.  100 more targets share those two cells outside the radius.
    The two anchors that fix the grid come last.  -> (targets [n,4], query [1,3])"""
    rng = np.random.default_rng([37, hits, nlow])
    A, anchor = nr.anchors(offset)
    m = np.array([100, 100, 30])
    corner = A + (m + 1) * nr.CELL
    q = corner - 0.05
    nlow = min(nlow, hits)
    low = corner + rng.uniform(0.02, 0.08, size=(nlow, 3))
    own = q + rng.uniform(-0.08, 0.04, size=(hits - nlow, 3))
    miss = np.concatenate([corner + rng.uniform(0.3, 0.38, size=(50, 3)), q - rng.uniform(0.25, 0.3, size=(50, 3))])
    rest = np.concatenate([own, miss])
    rng.shuffle(rest)
    t = np.concatenate([low, rest, anchor]).astype(F32)
    return np.c_[t, np.zeros(len(t), F32)].astype(F32), q[None, :].astype(F32)


@functools.lru_cache(maxsize=None)
def coincident(interleaved, copies=40000):
    """`copies` targets on ONE point and 64 queries on it; interleaved: the copies' rows alternate with as many far points
    -> (targets [n,4], queries [64,3])"""
    p = F32([3.25, -1.5, 0.75])
    t = np.repeat(p[None, :], copies, 0)
    if interleaved:
        rng = np.random.default_rng(43)
        far = (p + rng.uniform(2.0, 30.0, size=(copies, 3)) * rng.choice([-1.0, 1.0], size=(copies, 3)) * [1, 1, 0.2]).astype(F32)
        t = np.stack([t, far], 1).reshape(-1, 3)
    return np.c_[t, np.zeros(len(t), F32)].astype(F32), np.repeat(p[None, :], 64, 0)


def nonfinite_rows(queries):
    """a copy of 24 query rows with NaN / +inf / -inf in one, two and all coordinates, between ordinary rows"""
    q = np.array(nr._xyz(queries)[:24])
    bad = [np.nan, np.inf, -np.inf]
    for i in range(0, len(q), 2):
        q[i, i % 3] = bad[(i // 2) % 3]
        if i % 4 == 0:
            q[i, (i + 1) % 3] = bad[(i // 2 + 1) % 3]
    q[-2] = np.nan
    return q
