"""Dense references and input families for the fixed-radius neighbour queries (csrc/cluster_queries.inc: k_cl_ball_count, k_cl_nearest), the
entropy score (csrc/segment.hip: k_entropy_scores) and the subsample keys (k_subsample_keys).  TEST INFRASTRUCTURE ONLY.

The references work on ALL query x target pairs in chunks: no KD-tree, no cells, no pruning, so nothing a pruning rule can get wrong
exists here.  `grid_origin` / `cell_of` / `cell_lb` restate the kernels' documented cell rules; they only PLACE points (so that a pair
sits across a face, an edge, a corner, or outside the grid) and DESCRIBE a failing pair -- no expected count or index depends on them.
"""
import functools
import itertools
import math

import numpy as np

F32 = np.float32
CELL = 0.4
NB = (512, 512, 64)                                   # cells per axis: 204.8 m x 204.8 m x 25.6 m
EXT = tuple(n * CELL for n in NB)
OFFSETS = ((0.0, 0.0, 0.0), (140.0, -90.0, 3.0), (-480.0, 510.0, -20.0), (1000.0, 1000.0, 0.0))
R2_ENTROPY = F32(0.3) * F32(0.3)                      # count_neighbors: max_neighbor_point_dist ** 2 in float32
R2_INTER = F32(0.2) * F32(0.2)                        # count_neighbors_inter_frame(points, 0.2)
R2_MOVING = F32(0.1)                                  # dists < 0.1 on squared distances
R2_GATE = F32(0.2)                                    # float32(0.2), and ...
R2_KNN = np.nextafter(F32(0.2), F32(0))               # ... the gate of knn_labels itself: `dists > 0.2` in float64, and float32(0.2) > 0.2
RADII = (R2_ENTROPY, R2_INTER, R2_MOVING, R2_GATE)
R2_REACH1, R2_REACH2, R2_REACH8 = F32(0.16), F32(0.64), F32(10.24)      # sqrt(r2) / 0.4 sits at 1, 2 and 8


# ------------------------------------------------------------------------------------------------------------ distances
def _xyz(a):
    return np.ascontiguousarray(np.asarray(a, F32)[..., :3])


def d2_f32(q, t):
    """float32 fma(dz, dz, fma(dy, dy, dx * dx)) of broadcastable [..., 3] float32 arrays.  Every step is formed in float64, where
    the product of two float32 values is exact, and rounded to float32.  The float64 SUM is itself rounded (a 48-bit product under a
    24-bit addend can need more than 53 bits), so `_round_sum` repairs the one case where two roundings differ from one."""
    q, t = np.asarray(q, F32), np.asarray(t, F32)
    d = (q - t).astype(np.float64)                                   # the float32 subtraction, widened
    p = (d[..., 0] * d[..., 0]).astype(F32).astype(np.float64)
    p = _round_sum(d[..., 1] * d[..., 1], p).astype(np.float64)
    return _round_sum(d[..., 2] * d[..., 2], p)


def _round_sum(prod, acc):
    """float32(prod + acc) rounded ONCE.  prod: exact float64 product, acc: a float32 value as float64 (same shape)."""
    s = prod + acc                                                   # rounded to float64
    r = s.astype(F32)
    r64 = r.astype(np.float64)
    diff = s - r64
    sp = np.spacing(np.abs(r)).astype(np.float64)
    cand = np.flatnonzero((diff != 0) & ((np.abs(diff) * 2 == sp) | (np.abs(diff) * 4 == sp)))      # s (maybe) half-way between two float32
    if len(cand):
        p_, a_, s_ = prod.reshape(-1)[cand], np.broadcast_to(acc, prod.shape).reshape(-1)[cand], s.reshape(-1)[cand]
        bv = s_ - a_
        err = (a_ - (s_ - bv)) + (p_ - bv)                           # TwoSum: s + err is the exact sum
        r_ = r.reshape(-1)[cand]
        other = np.nextafter(r_, np.where(s_ > r_, F32(np.inf), F32(-np.inf)).astype(F32))
        tie = ((r_.astype(np.float64) + other.astype(np.float64)) * 0.5 == s_) & (err != 0)
        fixed = np.where(tie, np.where(err > 0, np.maximum(r_, other), np.minimum(r_, other)), r_)
        r = r.copy().reshape(-1)
        r[cand] = fixed
        r = r.reshape(s.shape)
    return r


def d2_exact(q, t):
    """float64 squared distance of the same float32 points."""
    d = np.asarray(q, F32).astype(np.float64) - np.asarray(t, F32).astype(np.float64)
    return (d * d).sum(-1)


def ulps_from(d2, r2):
    """signed distance of float32 d2 (>= 0) from r2 in float32 steps (positive floats order like their bit patterns)."""
    return np.asarray(d2, F32).view(np.int32).astype(np.int64) - int(F32(r2).view(np.int32))


def _chunks(q, t, rows=None):
    rows = rows or max(1, (1 << 22) // max(len(t), 1))
    for a in range(0, len(q), rows):
        yield a, d2_f32(q[a:a + rows, None, :], t[None, :, :])


def ball_count(query, target, r2, cap, inclusive=False):
    """min(cap, #{t : d2 < r2}) per query (`inclusive`: <=, the WRONG rule, for the family checks)."""
    q, t = _xyz(query), _xyz(target)
    out = np.zeros(len(q), np.int32)
    if len(t) == 0:
        return out
    r2 = F32(r2)
    for a, d2 in _chunks(q, t):
        out[a:a + len(d2)] = np.minimum((d2 <= r2 if inclusive else d2 < r2).sum(1), cap)
    return out


def nearest(query, target, max_d2):
    """(lowest row of the minimum among d2 <= max_d2, that d2) per query; (-1, +inf) when there is none."""
    q, t = _xyz(query), _xyz(target)
    idx, best = np.full(len(q), -1, np.int64), np.full(len(q), np.inf, F32)
    if len(t) == 0:
        return idx, best
    for a, d2 in _chunks(q, t):
        d2 = np.where(d2 <= F32(max_d2), d2, F32(np.inf))
        j = d2.argmin(1)                                              # the first (= lowest row) of the minima
        m = d2[np.arange(len(j)), j]
        idx[a:a + len(j)] = np.where(np.isinf(m), -1, j)
        best[a:a + len(j)] = m
    return idx, best


def threshold_pairs_of(query, target, r2, ulps=2):
    """-> (qi, ti, step) of the pairs whose float32 d2 is within `ulps` float32 steps of r2."""
    q, t = _xyz(query), _xyz(target)
    qi, ti, st = [], [], []
    for a, d2 in _chunks(q, t):
        u = ulps_from(d2, r2)
        i, j = np.nonzero(np.abs(u) <= ulps)
        qi.append(i + a); ti.append(j); st.append(u[i, j])
    return np.concatenate(qi), np.concatenate(ti), np.concatenate(st)


# ------------------------------------------------------------------------------------------------------------ the grid (placing, describing)
def grid_origin(targets):
    """k_cl_grid: per axis the data is centred in the grid when its span fits, otherwise the grid is anchored at the minimum; the
    start is floored to a multiple of 0.4 (all in float64 from the float32 extremes)."""
    t = _xyz(targets).astype(np.float64)
    o = np.empty(3)
    for a in range(3):
        lo, hi = t[:, a].min(), t[:, a].max()
        span = hi - lo
        start = lo - 0.5 * (EXT[a] - span) if span < EXT[a] else lo
        o[a] = math.floor(start / CELL) * CELL
    return o


def cell_unclamped(p, origin):
    return np.floor((_xyz(p).astype(np.float64) - origin) * (1.0 / CELL)).astype(np.int64)


def cell_of(p, origin):
    """cl_cell_of: floor((x - o) * (1 / 0.4)) in float64, clamped into the grid."""
    return np.clip(cell_unclamped(p, origin), 0, np.array(NB) - 1)


def cell_lb(origin, q, cell):
    """cl_cell_d2_lb restated (float32, sources compiled without contraction) -- for failure reports only."""
    q = _xyz(q)
    d2 = F32(0)
    for a in range(3):
        lo, hi = F32(origin[a] + cell[a] * CELL), F32(origin[a] + (cell[a] + 1) * CELL)
        d = F32(0)
        if q[a] < lo and cell[a] > 0:
            d = F32(lo - q[a])
        elif q[a] > hi and cell[a] < NB[a] - 1:
            d = F32(q[a] - hi)
        d2 = F32(d2 + F32(d * d))
    return F32(F32(d2 * F32(0.9999)) - F32(1e-6))


def describe(query, target, r2, qi, ti=None):
    """One line about query row qi (and target row ti): positions, cells, d2, r2, the cell lower bound."""
    q, t = _xyz(query), _xyz(target)
    o = grid_origin(t)
    s = f'query {qi} {q[qi].tolist()} cell {cell_of(q[qi], o).tolist()} (unclamped {cell_unclamped(q[qi], o).tolist()}) r2 {F32(r2)!r} origin {o.tolist()}'
    if ti is not None and ti >= 0:
        c = cell_of(t[ti], o)
        s += (f' | target {ti} {t[ti].tolist()} cell {c.tolist()} d2 {d2_f32(q[qi], t[ti])!r} ({int(ulps_from(d2_f32(q[qi], t[ti]), r2))} steps from r2)'
              f' exact {d2_exact(q[qi], t[ti])!r} lb {cell_lb(o, q[qi], c)!r}')
    return s


def explain_counts(query, target, r2, cap, got):
    """Message for a count mismatch: the first wrong query and every target of it within 4 steps of r2 (or all hits if none)."""
    want = ball_count(query, target, r2, cap)
    bad = np.flatnonzero(want != np.asarray(got))
    if len(bad) == 0:
        return ''
    i = int(bad[0])
    d2 = d2_f32(_xyz(query)[i][None, :], _xyz(target))
    near = np.flatnonzero(np.abs(ulps_from(d2, r2)) <= 4)
    if len(near) == 0:
        near = np.flatnonzero(d2 < F32(r2))[:8]
    lines = [f'{len(bad)} of {len(want)} counts differ (cap {cap}); first: query {i} got {int(np.asarray(got)[i])} want {int(want[i])}']
    lines += [describe(query, target, r2, i, int(j)) for j in near[:8]] or [describe(query, target, r2, i)]
    return '\n'.join(lines)


def explain_nearest(query, target, max_d2, got_idx, got_d2):
    widx, wd2 = nearest(query, target, max_d2)
    bad = np.flatnonzero((widx != np.asarray(got_idx)) | (wd2.view(np.int32) != np.asarray(got_d2, F32).view(np.int32)))
    if len(bad) == 0:
        return ''
    i = int(bad[0])
    return '\n'.join([f'{len(bad)} of {len(widx)} nearest results differ; first: query {i} got ({int(got_idx[i])}, {got_d2[i]!r}) want ({int(widx[i])}, {wd2[i]!r})',
                      'want: ' + describe(query, target, max_d2, i, int(widx[i])), 'got:  ' + describe(query, target, max_d2, i, int(got_idx[i]))])


# ------------------------------------------------------------------------------------------------------------ entropy, keys
def ephe_score(counts, seek=-1):
    """PP score of counts [nq, n_frames] (1 is subtracted from column `seek` first): -sum P log(P + 1e-8) / log N with
    P = c / (sum c + 1e-8), in np.longdouble; the sum is compensated (Neumaier), so no summation order shows in the result."""
    c = np.array(counts, dtype=np.longdouble)
    if seek >= 0:
        c[:, seek] -= 1
    eps = np.longdouble(1e-8)                      # the double constant 1e-8, widened (what the kernel and numpy add)
    P = c / (c.sum(1, keepdims=True) + eps)
    with np.errstate(invalid='ignore', divide='ignore'):
        terms = -P * np.log(P + eps)
    s = np.zeros(len(c), np.longdouble); comp = np.zeros(len(c), np.longdouble)
    for f in range(terms.shape[1]):
        v = terms[:, f]
        t = s + v
        with np.errstate(invalid='ignore'):
            comp += np.where(np.abs(s) >= np.abs(v), (s - t) + v, (v - t) + s)
        s = t
    return (s + comp) / np.log(np.longdouble(c.shape[1]))


def subsample_keys(seed, tag, n):
    """k_subsample_keys: mix64(seed * 0x100000001B3 + (tag << 32) + i) >> 1 in wrapping 64-bit arithmetic (splitmix64 finaliser)."""
    M = (1 << 64) - 1
    base = np.uint64((int(seed) * 0x100000001B3 + ((int(tag) << 32) & M)) & M)
    with np.errstate(over='ignore'):
        z = base + np.arange(n, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(1)).astype(np.int64)


def count_matrices(n_frames, nq, seed=0, cap=1000):
    """[nq, n_frames] int32 counts drawn from {0 .. cap} with, in the first rows: all zeros, one non-zero frame (first, middle, last),
    the cap in every frame, one everywhere, the cap in one frame only."""
    rng = np.random.default_rng([seed, n_frames, nq])
    c = rng.integers(0, cap + 1, size=(nq, n_frames)).astype(np.int32)
    small = rng.random(nq) < 0.3
    c[small] = rng.integers(0, 4, size=(int(small.sum()), n_frames))             # mostly-empty rows: P = 0 terms
    special = [np.zeros(n_frames, np.int32), np.full(n_frames, cap, np.int32), np.ones(n_frames, np.int32)]
    for f in (0, n_frames // 2, n_frames - 1):
        one = np.zeros(n_frames, np.int32); one[f] = 7
        top = np.zeros(n_frames, np.int32); top[f] = cap
        special += [one, top]
    for k, row in enumerate(special[:nq]):
        c[k] = row
    return c


# ------------------------------------------------------------------------------------------------------------ placing queries at the radius
DIRS = [d for d in itertools.product((0, 1), repeat=3) if any(d)]               # x, y, z, the face diagonals, the body diagonal
DIRS.sort(key=lambda d: (sum(d), d[::-1]))


def _ulp(x):
    x = np.abs(np.asarray(x, F32))
    return (np.nextafter(x, F32(np.inf)) - x).astype(np.float64)


def shell_queries(targets, units, r2, rng, tries=96, steps=(-2, -1, 0, 1, 2)):
    """For target i and unit vector units[i]: queries near t + r * u whose float32 d2 to the target is r2 moved by each of `steps`
    float32 steps (where the float32 lattice at that place holds such a point), else the plain rounded t + (r - k ulp(r)) u.

    The float32 spacing of a coordinate at 1000 m is 6e-5 m, which moves d2 by thousands of its own steps, so rounding t + r u hits
    the threshold only near the origin.  Each try therefore leaves the shell point a little sideways (|e| <= sqrt(3 r ulp)), rounds
    it, and then solves ONE coordinate for d2 = r2 given the other two; the five neighbours of that solution are evaluated with the
    real float32 d2.  -> (queries [n, len(steps), 3] float32, hit [n, len(steps)] bool)."""
    t = _xyz(targets)
    n = len(t)
    u = np.asarray(units, np.float64)
    r2 = F32(r2)
    r = math.sqrt(float(r2))
    t64 = t.astype(np.float64)
    ur = float(np.nextafter(F32(r), F32(np.inf)) - F32(r))
    out = np.stack([(t64 + u * (r - k * ur)).astype(F32) for k in steps], 1)                 # the fallback: plain rounding
    hit = np.zeros((n, len(steps)), bool)
    want = np.array(steps)
    coarse = _ulp(t64 + u * r).max(1)                                                          # largest coordinate spacing at the query
    side = np.sqrt(3 * r * coarse)[:, None, None]
    e = rng.normal(size=(n, tries, 3))
    e -= (e * u[:, None, :]).sum(-1, keepdims=True) * u[:, None, :]                            # sideways only
    e *= side * rng.random((n, tries, 1)) / np.maximum(np.linalg.norm(e, axis=-1, keepdims=True), 1e-30)
    base = (t64[:, None, :] + u[:, None, :] * (r - 1.5 * coarse[:, None, None] * rng.random((n, tries, 1))) + e).astype(F32)
    tt = np.broadcast_to(t[:, None, :], base.shape)
    for w in range(3):                                                                         # the coordinate that is solved for
        d = base.astype(np.float64) - tt
        rest = (np.delete(d, w, axis=-1) ** 2).sum(-1)
        ok = rest < float(r2)
        dw = np.sqrt(np.where(ok, float(r2) - rest, 0.0)) * np.where(d[..., w] < 0, -1.0, 1.0)
        sol = (tt[..., w].astype(np.float64) + dw).astype(F32)
        for nudge in range(-2, 3):
            cand = base.copy()
            v = sol
            for _ in range(abs(nudge)):
                v = np.nextafter(v, F32(np.inf) if nudge > 0 else F32(-np.inf))
            cand[..., w] = v
            st = ulps_from(d2_f32(cand, tt), r2)
            for k, s in enumerate(want):
                m = ok & (st == s)
                first = m.argmax(1)
                take = m.any(1) & ~hit[:, k]
                out[take, k] = cand[take, first[take]]
                hit[take, k] = True
    return out, hit


def _seed(tag, offset, r2=0.0):
    return [tag] + [int(v) + 100000 for v in offset] + [int(float(F32(r2)) * 1e6)]


def _unit(d, sign=1.0):
    v = np.asarray(d, np.float64)
    return sign * v / np.linalg.norm(v)


@functools.lru_cache(maxsize=None)
def threshold_pairs(offset, r2):
    """~600 targets in a 12 m cube centred at `offset`; for target i the queries at t + s (r - k ulp) u, k = -2 .. 2, with (u, s) the
    i-th of the 7 directions x 2 signs, placed by `shell_queries`.  -> (targets [n,4], queries [m,3])."""
    rng = np.random.default_rng(_seed(11, offset, r2))
    n = 600
    t = (np.asarray(offset) + rng.uniform(-6, 6, size=(n, 3))).astype(F32)
    units = np.array([_unit(DIRS[i % 7], 1.0 if (i // 7) % 2 == 0 else -1.0) for i in range(n)])
    q, _ = shell_queries(t, units, r2, rng)
    targets = np.c_[t, rng.random(n).astype(F32)].astype(F32)
    return targets, np.ascontiguousarray(q.reshape(-1, 3))


def anchors(offset):
    """Two points that fix the grid origin whatever lies between them: they span more than the grid on every axis, so the grid is
    anchored at the minimum, A = floor(lo / 0.4) * 0.4, with lo in the middle of its cell.  -> (A [3] float64, points [2,3] float32)."""
    k = np.floor(np.asarray(offset, np.float64) / CELL) - 40
    lo = (k * CELL + 0.2).astype(F32)
    hi = (lo.astype(np.float64) + np.array(EXT) + (60.0, 57.0, 59.0)).astype(F32)
    return k * CELL, np.stack([lo, hi])


@functools.lru_cache(maxsize=None)
def face_lattice(offset, r2=R2_ENTROPY):
    """Targets ON the cell faces A + m * 0.4, moved by -1, 0, +1 float32 step, in one, two and three axes at once (the other axes sit
    inside the cell); for each target queries at the radius (`shell_queries`) along the diagonal of those axes, in both senses -- for
    r = reach * 0.4 that is the far side of the farthest reachable cell.  -> (targets [n,4], queries [m,3], A)."""
    rng = np.random.default_rng(_seed(13, offset, r2))
    A, anchor = anchors(offset)
    T, U = [], []
    for site in range(9):
        m = np.array([60 + 9 * site, 55 + 11 * site, 8 + 5 * site]) + rng.integers(0, 3, 3)
        for axes in DIRS:
            on = np.flatnonzero(axes)
            for shift in itertools.product((-1, 0, 1), repeat=len(on)):
                p = (A + (m + 0.5 + rng.uniform(-0.3, 0.3, 3)) * CELL).astype(F32)               # inside cell m ...
                for a, s in zip(on, shift):                                                      # ... except on the chosen faces
                    v = F32(A[a] + m[a] * CELL)
                    p[a] = v if s == 0 else np.nextafter(v, F32(np.inf) if s > 0 else F32(-np.inf))
                for sign in (1.0, -1.0):
                    T.append(p); U.append(_unit(axes, sign))
    T, U = np.array(T, F32), np.array(U)
    q, _ = shell_queries(T, U, r2, rng, steps=(-2, 0, 1))
    t = np.concatenate([anchor, T[::2]])                                                         # each target once
    targets = np.c_[t, np.zeros(len(t), F32)].astype(F32)
    return targets, np.ascontiguousarray(q.reshape(-1, 3)), A


@functools.lru_cache(maxsize=None)
def outside_grid():
    """Targets spanning 270 m x 268 m x 90 m (the grid: 204.8 x 204.8 x 25.6, anchored at the minimum), some up to 60 m beyond the
    last cell of each axis; queries beyond all six sides by less than r, about r and 50 m, next to clamped targets, and in the last
    regular cell (510 / 62) next to a clamped target of the border cell.  -> (targets [n,4], queries [m,3])."""
    rng = np.random.default_rng(17)
    lo = np.array([-115.1, -114.9, -4.1])
    span = np.array([270.0, 268.0, 90.0])
    corner = np.stack([lo, lo + span]).astype(F32)
    o = np.floor(corner[0].astype(np.float64) / CELL) * CELL
    end = o + np.array(EXT)
    T = [corner, lo + rng.random((900, 3)) * span]
    Q = []
    for a in range(3):
        others = [b for b in range(3) if b != a]
        for beyond in (0.1, 0.3, 50.0):
            # low side: targets in cell 0 right at the minimum, queries below the origin (clamped into cell 0)
            c = o + rng.random((24, 3)) * np.array(EXT)
            c[:, a] = corner[0, a] + rng.random(24) * 0.25
            T.append(c + rng.normal(scale=0.05, size=c.shape) * [b != a for b in range(3)])
            q = c.copy(); q[:, a] = o[a] - beyond * rng.uniform(0.8, 1.2, 24)
            Q.append(q)
            # high side: targets beyond the last cell (clamped), queries beyond the grid next to them
            c = o + rng.random((24, 3)) * np.array(EXT)
            c[:, a] = end[a] + beyond * rng.uniform(0.8, 1.2, 24)
            for k in range(3):
                T.append(c + rng.normal(scale=0.12, size=c.shape))
            Q.append(c + rng.normal(scale=0.15, size=c.shape))
            q = c.copy(); q[:, a] = end[a] + rng.random(24) * 0.3                             # just beyond, the target further out
            Q.append(q)
        # the last regular cell next to a clamped target: 0.40 .. 0.50 m apart (r2 = 0.2 gives r = 0.447)
        c = o + rng.random((40, 3)) * np.array(EXT)
        c[:, a] = end[a] + rng.uniform(0.001, 0.04, 40)
        T.append(c)
        q = c + rng.normal(scale=0.01, size=c.shape); q[:, a] = end[a] - CELL - rng.uniform(0.001, 0.06, 40)
        Q.append(q)
        # beyond TWO sides at once (a corner of the grid)
        c = o + rng.random((16, 3)) * np.array(EXT)
        c[:, a] = end[a] + rng.uniform(0.05, 30.0, 16)
        c[:, others[0]] = end[others[0]] + rng.uniform(0.05, 30.0, 16)
        T.append(c + rng.normal(scale=0.1, size=c.shape)); T.append(c + rng.normal(scale=0.1, size=c.shape))
        Q.append(c + rng.normal(scale=0.1, size=c.shape))
    t = np.concatenate(T).astype(F32)
    t = np.minimum(np.maximum(t, corner[0]), corner[1])                                       # the two corners stay the extremes
    q = np.concatenate(Q).astype(F32)
    targets = np.c_[t, rng.random(len(t)).astype(F32)].astype(F32)
    return targets, q


@functools.lru_cache(maxsize=None)
def ties(offset=(0.0, 0.0, 0.0)):
    """Queries with 2 to 6 targets at EXACTLY equal float32 d2: t = q -+ d along the axes, every coordinate a multiple of 2^-6 and
    d = 0.25, so all of it is exact.  The query sits at (0.3, 0.2, 0.2) of its 0.4 m cell: the -x target shares the query's cell,
    the other five lie in five different neighbour cells; -z is the first neighbour cell the kernel visits, +z the last.
    Within a query's group the rows are ordered by `mode`: 0 own cell lowest, 1 the -z cell lowest, 2 the +z cell lowest, 3 random.
    Some targets are duplicated at a far higher and at a lower row; some queries coincide with a target.
    -> (targets [n,4], queries [m,3], info dict of per-query arrays)."""
    rng = np.random.default_rng(_seed(19, offset))
    A, anchor = anchors(offset)
    d = 0.25
    snap = lambda v: np.round(np.asarray(v) * 64) / 64
    steps = np.array([[-d, 0, 0], [d, 0, 0], [0, -d, 0], [0, d, 0], [0, 0, -d], [0, 0, d]])
    nq = 240
    groups, Q, mode = [], [], []
    for i in range(nq):
        m = np.array([50 + 6 * (i % 20), 50 + 6 * (i // 20), 10 + (i % 7) * 5])
        q = snap(A + (m + np.array([0.75, 0.5, 0.5])) * CELL)
        md = i % 4
        k = 2 + (i // 4) % 5                                         # 2 .. 6 targets
        need = {0: [0], 1: [0, 4], 2: [0, 5], 3: [0]}[md]
        rest = [s for s in rng.permutation(6) if s not in need]
        chosen = need + rest[:k - len(need)]
        first = {0: 0, 1: 4, 2: 5}.get(md)
        order = list(rng.permutation(chosen))
        if first is not None:
            order.remove(first); order.insert(0, first)
        groups.append(q + steps[order]); Q.append(q); mode.append(md)
    perm = rng.permutation(nq)                                       # groups in a random order, each group's rows consecutive
    dup_low = np.array([groups[g][-1] for g in perm[:40]])           # a copy of a group's LAST row, placed before every group
    dup_high = np.array([groups[g][0] for g in perm[40:80]])         # a copy of a group's FIRST row, placed after every group
    t = np.concatenate([anchor, dup_low] + [groups[g] for g in perm] + [dup_high]).astype(F32)
    q = np.array(Q)
    coincide = np.concatenate([dup_low[:20], dup_high[:20], np.array([groups[g][1] for g in perm[80:120]])])
    q_all = np.concatenate([q, coincide]).astype(F32)
    assert np.array_equal(q_all.astype(np.float64), np.concatenate([q, coincide])) and np.array_equal(t[2:].astype(np.float64) * 64, np.round(t[2:].astype(np.float64) * 64))
    targets = np.c_[t, np.zeros(len(t), F32)].astype(F32)
    return targets, q_all, dict(mode=np.array(mode), n_ring=nq, r2=F32(d * d), A=A)


@functools.lru_cache(maxsize=None)
def dense_cell(offset=(140.0, -90.0, 3.0)):
    """3 000 targets in one cell and its neighbours (sigma 0.25 m) among 300 spread over 30 m; 512 queries in and around the heap."""
    rng = np.random.default_rng(23)
    c = np.asarray(offset) + 0.2
    t = np.concatenate([c + rng.normal(scale=0.25, size=(3000, 3)), c + rng.uniform(-15, 15, size=(300, 3))]).astype(F32)
    rng.shuffle(t)
    q = np.concatenate([c + rng.normal(scale=0.3, size=(384, 3)), c + rng.uniform(-2, 2, size=(128, 3))]).astype(F32)
    return np.c_[t, np.zeros(len(t), F32)].astype(F32), q


@functools.lru_cache(maxsize=None)
def reach_limits(offset=(-480.0, 510.0, -20.0)):
    """2 500 targets in a 9 m cube and 64 queries inside it: r2 = 10.24 (reach 8) looks at 17^3 cells per query."""
    rng = np.random.default_rng(29)
    t = (np.asarray(offset) + rng.uniform(-4.5, 4.5, size=(2500, 3))).astype(F32)
    q = (np.asarray(offset) + rng.uniform(-4.0, 4.0, size=(64, 3))).astype(F32)
    return np.c_[t, np.zeros(len(t), F32)].astype(F32), q
