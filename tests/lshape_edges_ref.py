"""What csrc/lshape.hip computes, stated so that every check of tests/test_lshape_edges.py has one right answer.

Three things live here, none of which takes anything from the kernel's output:

  pick_box     the restatement of k_lshape_pick from (cluster, table row): the projection of ls_proj (first product rounded, second
               added by one FMA; float32 for closeness, float64 for variance -- `fma32`, `fma64` round once, by the round-to-odd
               trick), plain min / max, the flip tested in the criterion's dtype, the second projection with table columns 2, 3, the
               corners of ls_corner, l and w as sqrt(ax * ax + ay * ay) with every operation rounded on its own, the centre
               (c0 + c2) / 2, cz and h + 0.3 in float32, rz = column 4 + flip + 2 swap, aux[2] = column 4 + flip.  Given the row,
               every output bit is determined: minima and maxima do not depend on order, the rest is one sequence of operations.
  exact        the criteria as exact numbers.  The distances Dx, Dy are order-free too (projection, extent, two subtractions, one
               minimum), so they are restated in bits.  Closeness: beta = max(float64(min(Dx, Dy)), delta_zero), 1 / beta rounded
               once, math.fsum of the terms.  Variance: the counts, sums and sums of squares of the two sides as integers (every
               distance scaled by one power of two), so -var = -(n S2 - S1^2) / n^2 is a rational number, rounded once to float64;
               comparisons between two angles use the rationals themselves (`Exact.cmp`).
  emulate      a numpy emulation of both kernels in the kernel's own order: lane-strided partial sums (lane l adds points l, l + 64,
               ...), then the xor butterfly 32, 16, ..., 1; the argmax by 256 threads striding the angles, merged by 'larger
               criterion, then lower index'.  `fault=` turns one operation into a plausible wrong one (FAULTS).

The bounds (u = 2^-53; n the cluster's size, n_x / n_y the points of the variance sides, mu_x / mu_y their exact means):

  closeness    |work - exact| <= (n + 1) u exact.  The n terms are the same correctly rounded numbers on both sides; the kernel adds
               n positive float64 terms in some order: (n - 1) u relative to first order (each of the n - 1 additions rounds once and
               every partial sum is below the total).  fsum's own rounding is one more u, and the last u covers the second-order
               part (n u < 2^-38 for n < 2^15).
  variance     per side the kernel computes m = fl(fl-sum(D) / n_s): |m - mu| <= n_s u mu (n_s - 1 additions of non-negative
               terms, one division), then sum fl(fl(D - m)^2): three roundings per term, n_s - 1 additions, one division by n_s, and
               sum (D - m)^2 = sum (D - mu)^2 + n_s (m - mu)^2 exactly, because the deviations from the exact mean sum to zero.  The
               two sides are added to 0.0: one more rounding; the exact value is rounded once to float64: one more; one u is spare
               for the second-order part.  So
                   |work - exact| <= (max(n_x, n_y) + 6) u |exact| + (1 + 2^-20) u^2 (n_x^2 mu_x^2 + n_y^2 mu_y^2).
               The second term is tiny (1e-28 for 100 points at 1 m) but it is what is left when the variance itself is tiny next to
               the mean; where the sums are exact (the designed equality cases) the kernel is expected to beat it by giving the exact
               value, and does.
  index        eps = the bound above at each angle.  Angles whose exact criterion is below the maximum by more than
               eps(a) + eps(max) + 2 u |max| (the 2 u: both are known rounded once) cannot win.  If every other angle is that far
               below or exactly equal (compared as rationals / by an fsum of the difference), the kernel must report the FIRST angle
               of the exact maximum; otherwise the cluster counts as ambiguous and the kernel's angle must be one of the close ones.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
CLOSENESS, VARIANCE = 0, 1
NAMES = {CLOSENESS: 'closeness_rectangle', VARIANCE: 'variance_rectangle'}
FAULTS = ('zero_start_score', 'zero_start_pick', 'flip_le', 'swap_ge', 'side_le', 'clamp_dropped', 'clamp_f32', 'acc_f32', 'last_max',
          'wave_tie_high', 'loop_256', 'rz_unflipped', 'f64_lw', 'f64_centre', 'index_ignored', 'stride3')


# ----------------------------------------------------------------------------------------------------- fused multiply-add, rounded once
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    h = c - (c - a)
    return h, a - h


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_odd(a, b):
    """a + b rounded to odd (float64 arrays): an inexact sum whose last bit is even moves one ulp towards the exact value."""
    s, e = _two_sum(a, b)
    bits = np.ascontiguousarray(s).view(np.int64)
    toward = np.where((e > 0) == (s > 0), 1, -1)
    return np.where((e != 0) & ((bits & 1) == 0), bits + toward, bits).view(np.float64)


def fma32(a, b, c):
    """float32 fma(a, b, c), rounded once: the product is exact in float64, its sum with c is rounded to odd (53 >= 24 + 2 bits)."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c)))
    return _add_odd(a * b, c).astype(np.float32)


def fma64(a, b, c):
    """float64 fma(a, b, c), rounded once (Boldo & Melquiond 2008): a b = uh + ul exactly, c + ul = th + tl, uh + th = vh + vl,
    result = RN(vh + RO(tl + vl)).  No overflow or underflow at the magnitudes of point clouds."""
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))         # (not broadcast yet: the splits run on the operands' shapes)
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    return vh + _add_odd(tl, vl)


def fma_exact(a, b, c, dtype):
    """one fma by rational arithmetic, rounded once to `dtype` (the yardstick of fma32 / fma64)"""
    f = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    r = dtype(float(f))                                  # for float32 this may have rounded twice: look at the neighbours too
    it = {np.float32: np.int32, np.float64: np.int64}[dtype]
    near = [r, np.nextafter(r, dtype(-np.inf)), np.nextafter(r, dtype(np.inf))]
    return min(near, key=lambda v: (abs(Fraction(float(v)) - f), int(np.array(v).view(it)) & 1))


def _fma(a, b, c):
    return fma32(a, b, c) if np.asarray(a).dtype == np.float32 else fma64(a, b, c)


def project(x, y, cs, sn):
    """ls_proj: u = fma(y, s, x * c), v = fma(y, c, x * -s) in the operands' dtype"""
    return _fma(y, sn, x * cs), _fma(y, cs, x * -sn)


def corner(u, v, cs, sn):
    """ls_corner: x = fma(v, -s, u * c), y = fma(v, c, u * s)"""
    return _fma(v, -sn, u * cs), _fma(v, cs, u * sn)


def dtype_of(crit):
    return np.float32 if crit == CLOSENESS else np.float64


# ----------------------------------------------------------------------------------------------------- the distances, in bits
_DIST = {}


def distances(xy, rows, crit, zero_start=False):
    """Dx, Dy [n, R] in the criterion's dtype for the table rows `rows` [R, >= 2]: the distance of every projected point to the nearer
    end of the extent.  zero_start: the extents started from 0 (a fault).  The latest results are kept (up to 512 MB): the exact
    criteria and the emulation of one case ask for the same ones."""
    key = (xy.tobytes(), rows[:, :2].tobytes(), crit, zero_start)
    if key not in _DIST:
        out = _distances(xy, rows, crit, zero_start)
        size = out[0].nbytes * 2
        while _DIST and sum(v[0].nbytes * 2 for v in _DIST.values()) + size > 2 ** 29:
            _DIST.pop(next(iter(_DIST)))
        if size <= 2 ** 29:
            _DIST[key] = out
        return out
    return _DIST[key]


def _distances(xy, rows, crit, zero_start):
    T = dtype_of(crit)
    x, y = xy[:, :1].astype(T), xy[:, 1:2].astype(T)
    with np.errstate(invalid='ignore'):
        u, v = project(x, y, rows[:, 0].astype(T)[None], rows[:, 1].astype(T)[None])
        out = []
        for p in (u, v):
            lo, hi = p.min(axis=0), p.max(axis=0)
            if zero_start:
                lo, hi = np.minimum(lo, T(0)), np.maximum(hi, T(0))
            out.append(np.minimum(p - lo, hi - p))
    return out


def closeness_terms(dx, dy, delta_zero, fault=None):
    b32 = np.minimum(dx, dy)
    if fault == 'clamp_f32':
        return 1.0 / np.maximum(b32, np.float32(delta_zero)).astype(np.float64)
    beta = b32.astype(np.float64)
    with np.errstate(divide='ignore'):
        return 1.0 / (beta if fault == 'clamp_dropped' else np.maximum(beta, delta_zero))


# ----------------------------------------------------------------------------------------------------- exact criteria
def _to_int(D, E):
    """float64 D -> object array of the Python ints D / 2^E (exact: 2^E divides every D); the slow yardstick of colsum_int"""
    m, e = np.frexp(D)
    mi = np.ldexp(m, 53).astype(np.int64)
    sh = np.where(D != 0, e.astype(np.int64) - 53 - E, 0)
    return mi.astype(object) << sh.astype(object)


def _low_bit(D):
    nz = D[D != 0]
    return int(np.frexp(nz)[1].min()) - 53 if nz.size else 0


def colsum_int(X, E):
    """Exact column sums of float64 X [n, r] as Python ints in units of 2^E (2^E divides every X) -> object array [r].
    Each pass rounds every entry to a grid coarse enough for the column's float64 sum to be exact (sigma = 2^M times a power of two
    above the column's largest magnitude, n <= 2^M: q = (sigma + x) - sigma is a multiple of ulp(sigma) / 2, |q| <= sigma / 2^M, so
    every partial sum of the q is a multiple of that grid below 2^53 grid steps), takes the exact remainder x - q, and repeats on the
    remainders, which shrink by 2^(52 - M) per pass, until none is left."""
    X = np.array(X, np.float64)
    n, r = X.shape
    assert -E < 900, 'distances this small are outside the conversion below'
    M = int(np.ceil(np.log2(n + 2)))
    out = np.zeros(r, object)
    while True:
        mu = np.abs(X).max(axis=0) if n else np.zeros(r)
        if not mu.any():
            return out
        sigma = np.ldexp(1.0, np.frexp(mu)[1] + M)
        q = (sigma + X) - sigma
        X -= q
        out = out + np.array([int(v) for v in np.ldexp(q.sum(axis=0), -E).tolist()], object)


class Exact:
    """Exact criteria of one cluster at R distinct rows.  vals: the exact value rounded once to float64; eps: the kernel's bound;
    cmp(a, b): the sign of exact[a] - exact[b], decided without rounding."""

    def __init__(self, xy, rows, crit, delta_zero):
        n, R = len(xy), len(rows)
        self.crit, self.n = crit, n
        if crit == CLOSENESS:
            self.terms = closeness_terms(*distances(xy, rows, crit), delta_zero)
            self.vals = np.array([math.fsum(col) for col in self.terms.T.tolist()])
            self.eps = (n + 1) * U * self.vals
            return
        self.N = np.empty((2, R), object)                       # n_s S2 - S1^2 of each side, in units of 2^(2 E) of its column
        self.cnt = np.empty((2, R), np.int64)
        E = np.zeros(R, np.int64)
        mu = np.zeros((2, R))
        step = max(1, 2_000_000 // max(n, 1))                   # (the 20 000-point cluster goes through in slices of 100 angles)
        for r0 in range(0, R, step):
            sl = slice(r0, r0 + step)
            dx, dy = distances(xy, rows[sl], crit)
            E[sl] = e = min(_low_bit(dx), _low_bit(dy))
            for s, (d, o) in enumerate(((dx, dy), (dy, dx))):
                m = d < o
                d = np.where(m, d, 0.0)
                cnt = m.sum(axis=0)
                hi, lo = _split(d)                               # 26 bits each: the three products below are exact
                S1 = colsum_int(d, e)
                S2 = colsum_int(hi * hi, 2 * e) + 2 * colsum_int(hi * lo, 2 * e) + colsum_int(lo * lo, 2 * e)
                self.cnt[s, sl] = cnt
                self.N[s, sl] = cnt.astype(object) * S2 - S1 * S1
                mu[s, sl] = [a / max(int(c), 1) for a, c in zip(S1, cnt)]          # (int / int is rounded once)
        self.E = E
        mu = np.ldexp(mu, E)
        c0, c1 = (np.maximum(self.cnt[s], 1).astype(object) ** 2 for s in (0, 1))
        self.num, self.den = -(self.N[0] * c1 + self.N[1] * c0), c0 * c1         # exact = num / den 2^(2 E); an empty side has N = 0
        self.vals = np.array([math.ldexp(a / b, 2 * int(e)) for a, b, e in zip(self.num, self.den, E)])
        nmax = self.cnt.max(axis=0)
        self.eps = (nmax + 6) * U * np.abs(self.vals) + (1 + 2.0 ** -20) * U * U * ((self.cnt * mu) ** 2).sum(axis=0)

    def cmp(self, a, b):
        if self.crit == CLOSENESS:
            d = math.fsum(self.terms[:, a].tolist() + (-self.terms[:, b]).tolist())     # fsum rounds correctly: 0 only if equal
        else:
            ea, eb = 2 * int(self.E[a]), 2 * int(self.E[b])
            d = (self.num[a] * self.den[b] << ea - min(ea, eb)) - (self.num[b] * self.den[a] << eb - min(ea, eb))
        return (d > 0) - (d < 0)


# ----------------------------------------------------------------------------------------------------- the restated pick
def pick_box(xyz, row, crit, fault=None):
    """k_lshape_pick from (cluster [n, 3] float32, table row [8]) -> (box [7] float64, aux[2], corners [4, 2] float64)."""
    T = dtype_of(crit)
    x, y = xyz[:, 0].astype(T), xyz[:, 1].astype(T)
    zero = fault == 'zero_start_pick'

    def extent(cs, sn):
        u, v = project(x, y, np.full(1, cs, T), np.full(1, sn, T))
        if zero:
            u, v = np.append(u, T(0)), np.append(v, T(0))
        return u.min(), u.max(), v.min(), v.max()
    with np.errstate(invalid='ignore'):
        cs, sn = T(row[0]), T(row[1])
        mnx, mxx, mny, mxy = extent(cs, sn)
        flip = bool(T(mxx - mnx) <= T(mxy - mny)) if fault == 'flip_le' else bool(T(mxx - mnx) < T(mxy - mny))
        if flip:
            cs, sn = T(row[2]), T(row[3])
            mnx, mxx, mny, mxy = extent(cs, sn)
        cx, cy = corner(np.array([mxx, mnx, mnx, mxx], T), np.array([mny, mny, mxy, mxy], T), np.full(1, cs, T), np.full(1, sn, T))
        wide = (lambda v: v.astype(np.float64)) if fault == 'f64_lw' else (lambda v: v)
        ax, ay, bx, by = wide(cx[0]) - wide(cx[1]), wide(cy[0]) - wide(cy[1]), wide(cx[0]) - wide(cx[3]), wide(cy[0]) - wide(cy[3])
        l, w = np.sqrt(ax * ax + ay * ay), np.sqrt(bx * bx + by * by)
        swap = bool(w >= l) if fault == 'swap_ge' else bool(w > l)
        z = xyz[:, 2].astype(np.float32)
        zmin, height = z.min(), z.max() - z.min()
        col = 4 + (0 if fault == 'rz_unflipped' else int(flip))
        mid = (lambda a, b: (np.float64(a) + np.float64(b)) / 2) if fault == 'f64_centre' else (lambda a, b: (a + b) / T(2))
        box = np.array([mid(cx[0], cx[2]), mid(cy[0], cy[2]), zmin + height / np.float32(2),
                        w if swap else l, l if swap else w, height + np.float32(0.3), row[col + 2 * int(swap)]], np.float64)
    return box, float(row[col]), np.stack([cx, cy], 1).astype(np.float64)


# ----------------------------------------------------------------------------------------------------- the emulated kernels
_LANES = np.arange(64)


def lane_sum(t, dtype=np.float64):
    """[n, R] -> [R]: vg_wave_sum of the lane-strided partial sums, in `dtype` (a lane without a point adds nothing: + 0.0)"""
    n, R = t.shape
    t = np.concatenate([t.astype(dtype), np.zeros(((-n) % 64, R), dtype)]).reshape(-1, 64, R)
    acc = np.zeros((64, R), dtype)
    for blk in t:
        acc = acc + blk
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[_LANES ^ o]
    return acc[0].astype(np.float64)


def emulate_score(xy, rows, crit, delta_zero, fault=None):
    """k_lshape_score of one cluster at the rows -> [R] float64"""
    R = len(rows)
    if len(xy) == 0:
        return np.zeros(R)
    step = max(1, 2_000_000 // len(xy))
    if R > step:
        return np.concatenate([emulate_score(xy, rows[r0:r0 + step], crit, delta_zero, fault) for r0 in range(0, R, step)])
    acc_t = np.float32 if fault == 'acc_f32' else np.float64
    dx, dy = distances(xy, rows, crit, zero_start=fault == 'zero_start_score')
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        if crit == CLOSENESS:
            return lane_sum(closeness_terms(dx, dy, delta_zero, fault), acc_t)
        out = np.zeros(R)
        for d, o in ((dx, dy), (dy, dx)):
            m = (d <= o) if fault == 'side_le' else (d < o)
            cnt = m.sum(axis=0)
            mean = np.where(cnt > 0, lane_sum(np.where(m, d, 0), acc_t) / np.maximum(cnt, 1), 0.0)
            e = d - mean
            q = lane_sum(np.where(m, e * e, 0), acc_t)
            out = np.where(cnt > 0, out + -(q / np.maximum(cnt, 1)), out)
    return out


def emulate_pick_index(w, fault=None):
    """the argmax of k_lshape_pick over one work row"""
    A = len(w)
    if fault == 'last_max':
        return A - 1 - int(np.argmax(w[::-1]))
    if fault == 'loop_256':
        return int(np.argmax(w[:256]))
    if fault != 'wave_tie_high':
        return int(np.argmax(w))                     # threads, lanes and waves all keep the lower index of equal values
    best = []
    for wave in range(4):                            # every thread starts from angle 0; the wave's threads own a % 256 in its 64
        own = np.flatnonzero((np.arange(A) % 256) // 64 == wave)
        own = own if wave == 0 else np.r_[0, own]
        best.append(int(own[np.argmax(w[own])]))
    top = max(w[b] for b in best)
    return max(b for b in best if w[b] == top)


def unique_rows(table):
    """(indices of the first occurrence of each distinct row's columns 0..3, the id of every row's distinct row)"""
    _, first, inv = np.unique(np.ascontiguousarray(table[:, :4]).view(np.uint64), axis=0, return_index=True, return_inverse=True)
    return first, inv.reshape(-1)


def gather(case, c, fault=None):
    """the [n, 3] float32 points of cluster c as the kernel reads them"""
    pts, seg = case['pts'], case['seg']
    idx = np.arange(seg[c], seg[c + 1]) if fault == 'index_ignored' else case['index'][seg[c]:seg[c + 1]].astype(np.int64)
    stride = 3 if fault == 'stride3' else pts.shape[1]
    flat = pts.reshape(-1)
    return flat[idx[:, None] * stride + np.arange(3)[None]]


def emulate(case, fault=None):
    """vg_cluster_lshape on a case -> (box [C, 7], aux [C, 3], work [C, A])"""
    table, crit = case['table'], case['crit']
    first, inv = unique_rows(table)
    C, A = len(case['seg']) - 1, len(table)
    box, aux, work = np.full((C, 7), np.nan), np.full((C, 3), np.nan), np.zeros((C, A))
    for c in range(C):
        xyz = gather(case, c, fault)
        work[c] = emulate_score(xyz[:, :2], table[first], crit, case['dz'], fault)[inv]
        k = emulate_pick_index(work[c], fault)
        aux[c, :2] = k, work[c, k]
        if len(xyz):
            box[c], aux[c, 2], _ = pick_box(xyz, table[k], crit, fault)
    return box, aux, work


# ----------------------------------------------------------------------------------------------------- the checker
_REF = {}


def reference(case):
    """per cluster: (xyz, Exact at the distinct rows, row ids) -- computed once per case name"""
    if case['name'] not in _REF:
        first, inv = unique_rows(case['table'])
        out = []
        for c in range(len(case['seg']) - 1):
            xyz = gather(case, c)
            out.append((xyz, Exact(xyz[:, :2], case['table'][first], case['crit'], case['dz']) if len(xyz) else None, inv))
        _REF[case['name']] = out
    return _REF[case['name']]


def decide(ex, inv):
    """-> (the index a correct kernel must report, or None when ambiguous; the set of acceptable indices)"""
    vals, eps = ex.vals[inv], ex.eps[inv]
    m = vals.max()
    top = np.flatnonzero(vals == m)
    ids = list(dict.fromkeys(inv[top].tolist()))                 # distinct rows whose rounded value is the maximum
    best = ids[0]
    for i in ids[1:]:
        if ex.cmp(i, best) > 0:
            best = i
    winners = {i for i in ids if i == best or ex.cmp(i, best) == 0}
    is_win = np.isin(inv, list(winners)) & (vals == m)
    a_star = int(np.flatnonzero(is_win)[0])
    close = (m - vals <= eps + eps[a_star] + 2 * U * abs(m))
    if np.array_equal(close, is_win):
        return a_star, {a_star}
    return None, set(np.flatnonzero(close).tolist())


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def check(case, box, aux, work):
    """Every bar of the module docstring on one run of a case.  -> {'share': worst |work - exact| / eps, 'ambiguous': clusters
    without a decided index, 'clusters': non-empty clusters}"""
    name, table, crit = case['name'], case['table'], case['crit']
    C, A = len(case['seg']) - 1, len(table)
    assert box.shape == (C, 7) and aux.shape == (C, 3) and work.shape == (C, A), name
    share, ambiguous, full = 0.0, 0, 0
    for c, (xyz, ex, inv) in enumerate(reference(case)):
        at = f'{name} cluster {c} (n={len(xyz)})'
        if ex is None:                                           # the empty cluster
            assert np.isnan(box[c]).all(), at
            assert np.array_equal(_bits(work[c]), np.zeros(A, np.uint64)), at
            assert aux[c, 0] == 0 and _bits(aux[c, 1]) == 0 and np.isnan(aux[c, 2]), at
            continue
        full += 1
        vals, eps = ex.vals[inv], ex.eps[inv]
        err = np.abs(work[c] - vals)
        assert (err <= eps).all(), f'{at}: criterion off by {np.nanmax(err / np.maximum(eps, 1e-300)):.3g} of the bound at angle ' \
                                   f'{int(np.argmax(~(err <= eps)))}'
        share = max(share, float((err[eps > 0] / eps[eps > 0]).max()) if (eps > 0).any() else 0.0)
        k = int(aux[c, 0])
        assert aux[c, 0] == k and 0 <= k < A, at
        assert _bits(aux[c, 1]) == _bits(work[c, k]), at
        assert k == int(np.argmax(work[c])), f'{at}: index {k}, the first maximum of its own criteria is {int(np.argmax(work[c]))}'
        want, ok = decide(ex, inv)
        if want is None:
            ambiguous += 1
            assert k in ok, f'{at}: index {k} is not among the angles within 2 eps of the maximum {sorted(ok)[:8]}'
        else:
            assert k == want, f'{at}: index {k}, the exact maximum is first at {want}'
        wbox, waux, _ = pick_box(xyz, table[k], crit)
        assert np.array_equal(_bits(box[c]), _bits(wbox)), f'{at}: box {box[c].tolist()} != {wbox.tolist()} at index {k}'
        assert _bits(aux[c, 2]) == _bits(waux), at
        for key, v in case.get('expect', {}).get(c, {}).items():
            got = {'index': k, 'rz_col': int(np.flatnonzero(_bits(table[k, 4:8]) == _bits(box[c, 6]))[0]),
                   'crit0': float(work[c, 0])}[key]
            assert got == v, f'{at}: {key} = {got}, designed {v}'
    return {'share': share, 'ambiguous': ambiguous, 'clusters': full}


def rejected(case, out):
    try:
        check(case, *out)
    except AssertionError:
        return True
    return False


# ----------------------------------------------------------------------------------------------------- the cases
def angle_table(crit, **args):
    from vilgod_amd import boxes as vb
    return vb.lshape_angle_table(*vb.box_method({'name': NAMES[crit], 'args': args}))


def make_case(name, clusters, crit, table, dz=1e-2, expect=None):
    """packed: identity index, stride 3"""
    seg = np.r_[0, np.cumsum([len(p) for p in clusters])].astype(np.int32)
    pts = np.concatenate([np.asarray(p, np.float32).reshape(-1, 3) for p in clusters] + [np.zeros((1, 3), np.float32)])
    return dict(name=name, pts=np.ascontiguousarray(pts), index=np.arange(seg[-1], dtype=np.int32), seg=seg, crit=crit,
                table=np.ascontiguousarray(table, np.float64), dz=float(dz), expect=expect or {})


def gathered(case, stride, seed):
    """the same lists through a permutation into a larger array of row stride `stride`; unreferenced rows and unused columns NaN"""
    rng = np.random.default_rng(seed)
    n = len(case['pts'])
    rows = rng.permutation(2 * n + 7)[:n]
    big = np.full((2 * n + 7, stride), np.nan, np.float32)
    big[rows, :3] = case['pts']
    return dict(case, name=f"{case['name']}/stride{stride}", pts=big, index=rows[case['index']].astype(np.int32))


def shared_case(name, clusters, crit, table, dz=1e-2):
    """clusters whose index lists overlap: cluster c reads the points of `clusters[c]` and the first half of cluster c - 1's rows"""
    base = make_case(name, clusters, crit, table, dz)
    lists, seg = [], base['seg']
    for c in range(len(clusters)):
        own = np.arange(seg[c], seg[c + 1])
        prev = np.arange(seg[c - 1], seg[c - 1] + (seg[c] - seg[c - 1]) // 2) if c else own[:0]
        lists.append(np.r_[own, prev])
    base['index'] = np.concatenate(lists).astype(np.int32)
    base['seg'] = np.r_[0, np.cumsum([len(i) for i in lists])].astype(np.int32)
    return base


def packed(case):
    """the packed form of a gathered case: every cluster's points copied out in list order"""
    cl = [gather(case, c) for c in range(len(case['seg']) - 1)]
    return make_case(case['name'] + '/packed', cl, case['crit'], case['table'], case['dz'], case.get('expect'))


def l_cluster(rng, n, yaw_deg, centre=(31.5, -17.25)):
    """n points on the two visible sides of a 4.5 x 1.8 m box turned by yaw, with 2 cm of noise"""
    t = rng.uniform(-0.5, 0.5, n)
    side = rng.integers(2, size=n)
    xy = np.where(side[:, None] == 0, np.stack([t * 4.5, np.full(n, -0.9)], 1), np.stack([np.full(n, 2.25), t * 1.8], 1))
    xy = xy + rng.normal(0, 0.02, (n, 2))
    a = np.deg2rad(yaw_deg)
    xy = xy @ np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]]) + np.asarray(centre)
    return np.concatenate([xy, rng.uniform(-1, 1, (n, 1))], 1).astype(np.float32)


TIE_A = (1, 2, 3, 4, 5, 255, 256, 257, 513, 9001)


def tie_ks(A):
    return sorted({k for k in (0, 63, 64, 255, 256, A - 1) if k < A})


def tie_case(crit, A, k, identical=False):
    """rows [0, k) hold a poor angle (good + 45 degrees), rows [k, A) the good one (30 degrees, the clusters' yaw), each with its own
    columns 4..7; `identical`: A equal rows.  The kernel must report k (0 when identical)."""
    T = dtype_of(crit)
    good, poor = np.deg2rad(30.0), np.deg2rad(75.0)
    tab = np.empty((A, 8))
    for r in range(A):
        a = poor if r < k else good
        f = a + np.pi / 2
        tag = 0.0 if identical else r * 2.0 ** -20
        tab[r] = (T(np.cos(a)), T(np.sin(a)), T(np.cos(f)), T(np.sin(f)), a + tag, f + tag, a + np.pi / 2 + tag, f + np.pi / 2 + tag)
    rng = np.random.default_rng(1000 + A)
    cl = [l_cluster(rng, n, 30.0) for n in (40, 7, 130)]
    return make_case(f'tie/{NAMES[crit]}/A{A}/' + ('identical' if identical else f'k{k}'), cl, crit, tab,
                     expect={c: {'index': 0 if identical else k} for c in range(3)})


SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
POSITIONS = ('first', 'last', 63, 64, 255, 256)
EXTREMES = ((-10.0, 0.25), (10.0, -0.5), (0.5, -10.0), (-0.25, 10.0))         # the x-min, x-max, y-min, y-max points (centre at 0)


def size_clusters():
    """(label, [n, 3]) for every size; from 3 points on, every extreme point at every position that fits.  The four extreme points
    lie 10 m out on the axes and the rest within 1 m of the centre, so at every angle of the quadrant each of them alone decides
    one end of one extent.  The centre is (31.5, -17.25): an extent started from 0 would be wrong."""
    rng = np.random.default_rng(5)
    centre = np.array([31.5, -17.25])
    out = []
    for n in SIZES:
        if n < 5:
            out.append((f'n{n}', np.concatenate([rng.uniform(-1, 1, (n, 2)) + centre, rng.uniform(-1, 1, (n, 1))], 1)))
            continue
        for pos in POSITIONS:
            p = {'first': 0, 'last': n - 1}.get(pos, pos)
            if not 0 <= p < n or (pos not in ('first', 'last') and p in (0, n - 1)):
                continue
            for e in range(4):
                xy = rng.uniform(-1, 1, (n, 2))
                others = rng.choice(np.setdiff1d(np.arange(n), [p]), 3, replace=False)
                where = np.insert(others, e, p)
                xy[where] = EXTREMES
                out.append((f'n{n}/extreme{e}@{pos}', np.concatenate([xy + centre, rng.uniform(-1, 1, (n, 1))], 1)))
    return out


def size_case(crit):
    """all sizes in one call; the empty cluster sits between non-empty ones"""
    cl = size_clusters()
    cl = cl[1:4] + cl[:1] + cl[4:]
    assert len(cl[3][1]) == 0
    table = angle_table(crit, delta=2)
    return make_case(f'sizes/{NAMES[crit]}', [p for _, p in cl], crit, table), [label for label, _ in cl]


def axis_table(honest=True, extra=None):
    """row 0: exactly cos 1, sin 0; its flipped axes exactly (0, 1) -- or, `honest=False`, (1, 0) again, so that a flip keeps the
    projection and the longer side lands on w: the only way to a swap with exact axes.  Columns 4..7 name themselves."""
    t = np.array([[1.0, 0.0, 0.0 if honest else 1.0, 1.0 if honest else 0.0, 4.0, 5.0, 6.0, 7.0]])
    return t if extra is None else np.concatenate([t, extra])


def rect(w, h, z=(0.0, 1.0)):
    """corners and edge midpoints of [0, w] x [0, h] (float32 values) plus an inner point"""
    w, h = np.float32(w), np.float32(h)
    xy = [(0, 0), (w, 0), (0, h), (w, h), (w / 2, 0), (0, h / 2), (w / 2, h / 2)]
    return np.array([(x, y, z[i % 2]) for i, (x, y) in enumerate(xy)], np.float32)


def equality_cases(crit):
    """single-row tables; expect names the rz column (4 + flip + 2 swap)"""
    up = np.nextafter(np.float32(2), np.float32(3))
    sq, tall = rect(2, 2), rect(2, up)
    wide = rect(up, 2)
    same = np.tile(np.array([[1.25, -3.5, 0.75]], np.float32), (5, 1))
    one = same[:1]
    cases = [make_case(f'equal/{NAMES[crit]}/honest', [sq, tall, wide, same, one], crit, axis_table(True),
                       expect={0: {'rz_col': 0}, 1: {'rz_col': 1}, 2: {'rz_col': 0}, 3: {'rz_col': 0}, 4: {'rz_col': 0}}),
             make_case(f'equal/{NAMES[crit]}/same-axes', [sq, tall, wide], crit, axis_table(False),
                       expect={0: {'rz_col': 0}, 1: {'rz_col': 3}, 2: {'rz_col': 0}})]
    if crit == VARIANCE:
        # points on the diagonals of a 4 x 4 square have Dx == Dy: neither side.  + (1, 2): one point on the x side (Dx 1 < Dy 2);
        # + (2.25, 0.5): one on the y side; + both x-side points (1, 2), (0.5, 1.5): variance of {1, 0.5} = 0.0625
        diag = np.array([(0, 0), (4, 0), (0, 4), (4, 4), (1, 1), (3, 1), (2, 2), (1.5, 2.5)], np.float32)
        def with_(*extra):
            xy = np.concatenate([diag, np.array(extra, np.float32).reshape(-1, 2)])
            return np.concatenate([xy, np.linspace(0, 1, len(xy), dtype=np.float32)[:, None]], 1)
        multi = angle_table(VARIANCE, delta=15)
        cl = [with_(), with_((1, 2)), with_((2.25, 0.5)), with_((1, 2), (0.5, 1.5)), same, one]
        cases.append(make_case('equal/variance_rectangle/sides', cl, crit, axis_table(True),
                               expect={0: {'crit0': 0.0}, 1: {'crit0': 0.0}, 2: {'crit0': 0.0}, 3: {'crit0': -0.0625}}))
        cases.append(make_case('equal/variance_rectangle/zero', [same, one, with_()[:2]], crit, axis_table(True, multi),
                               expect={c: {'index': 0, 'crit0': 0.0} for c in range(3)}))
    else:
        cases.append(make_case('equal/closeness_rectangle/zero', [same, one], crit, axis_table(True, angle_table(CLOSENESS)),
                               expect={0: {'index': 0, 'crit0': 500.0}, 1: {'index': 0, 'crit0': 100.0}}))
    return cases


CLAMP_DZ = (1e-6, 1e-2, 0.05, 10.0)


def clamp_cases():
    """A 64 x 64 m frame and points at distance b from its left edge, b = float32(delta_zero) and its two float32 neighbours; with
    delta_zero as given and with delta_zero = float32(delta_zero), where beta == delta_zero is reachable (10 is both)."""
    out = []
    for dz in CLAMP_DZ:
        b = np.float32(dz)
        steps = [np.nextafter(b, np.float32(0)), b, np.nextafter(b, np.float32(100))]
        frame = [(0, 0), (64, 0), (0, 64), (64, 64)]
        cl = [np.array(frame + [(s, 32)] + [(s, 30), (s, 31)][:i], np.float32) for i, s in enumerate(steps)]
        cl.append(np.array(frame + [(s, 32) for s in steps], np.float32))
        cl = [np.concatenate([p, np.linspace(0, 1, len(p), dtype=np.float32)[:, None]], 1) for p in cl]
        table = axis_table(True, angle_table(CLOSENESS))
        for passed in sorted({float(dz), float(b)}):
            out.append(make_case(f'clamp/dz{dz:g}/passed{passed!r}', cl, CLOSENESS, table, dz=passed))
    return out


def seeded_clusters(count, seed, nmax=200):
    """the three kinds tests/test_lshape.py draws: a blob, an L, a coarse grid with many exact ties; turned and moved"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(1, nmax))
        kind = i % 3
        if kind == 0:
            xy = rng.normal(0, rng.uniform(0.05, 3), (n, 2)) * rng.uniform(0.2, 1, 2)
        elif kind == 1:
            t = rng.uniform(-0.5, 0.5, n)
            side = rng.integers(2, size=n)
            xy = np.where(side[:, None] == 0, np.stack([t * 4.5, np.full(n, -0.9)], 1), np.stack([np.full(n, 2.25), t * 1.8], 1))
            xy = xy + rng.normal(0, 0.03, (n, 2))
        else:
            xy = np.round(rng.uniform(-2, 2, (n, 2)), 1)
        yaw = rng.uniform(-np.pi, np.pi)
        xy = xy @ np.array([[np.cos(yaw), np.sin(yaw)], [-np.sin(yaw), np.cos(yaw)]]) + rng.uniform(-50, 50, 2)
        out.append(np.concatenate([xy, rng.uniform(-1, 2, (n, 1))], 1).astype(np.float32))
    return out


def fixture_clusters(golden_dir):
    g = np.load(f'{golden_dir}/lshape_golden.npz')
    return [g['points'][g['seg'][c]:g['seg'][c + 1]] for c in range(len(g['seg']) - 1)]


def real_clusters(golden_dir):
    import pickle
    with open(f'{golden_dir}/detect_golden.pkl', 'rb') as f:
        g = pickle.load(f)
    gm = np.zeros(len(g['points']), bool)
    gm[g['ground_idx']] = True
    X = g['points_ref'][~gm][:, :3].astype(np.float32)
    return [X[np.asarray(i)] for i in g['det_index']]


FAMILIES = ('fixture', 'real', 'seeded', 'delta_a', 'delta_b')


def family_case(family, crit, golden_dir):
    """fixture / real / seeded at the default table; delta_a: closeness delta 1, variance delta 0.5; delta_b: closeness delta 0.5,
    variance delta 0.01 (9001 angles; clusters under 100 points)"""
    name = f'family/{family}/{NAMES[crit]}'
    if family == 'fixture':
        return make_case(name, fixture_clusters(golden_dir), crit, angle_table(crit))
    if family == 'real':
        return make_case(name, real_clusters(golden_dir), crit, angle_table(crit))
    if family == 'seeded':
        return make_case(name, seeded_clusters(210, 7), crit, angle_table(crit))
    if family == 'delta_a':
        return make_case(name, seeded_clusters(60, 11), crit, angle_table(crit, delta=1 if crit == CLOSENESS else 0.5))
    if crit == CLOSENESS:
        return make_case(name, seeded_clusters(60, 13), crit, angle_table(crit, delta=0.5))
    return make_case(name, seeded_clusters(12, 17, nmax=100), crit, angle_table(crit, delta=0.01))


GROUPS = ('tie', 'sizes', 'index', 'equal', 'clamp') + tuple(f'family/{f}' for f in FAMILIES)
_CASES = {}


def cases(group, crit, golden_dir=None):
    """the cases of a group for one criterion (built once)"""
    key = (group, crit)
    if key not in _CASES:
        if group == 'tie':
            out = [tie_case(crit, A, k) for A in TIE_A for k in tie_ks(A)] + [tie_case(crit, A, 0, identical=True) for A in TIE_A]
        elif group == 'sizes':
            out = [size_case(crit)[0]]
        elif group == 'index':
            cl = [p for label, p in size_clusters() if label in ('n1', 'n2', 'n3', 'n0', 'n65/extreme0@last', 'n257/extreme3@first')]
            cl = cl[1:] + cl[:1] + seeded_clusters(9, 3)                # (the empty one fourth; every cluster also reads half of the
            base = shared_case(f'index/{NAMES[crit]}', cl, crit, angle_table(crit, delta=2))          # one before it)
            out = [gathered(base, s, 40 + s) for s in (3, 4, 5, 7)]
        elif group == 'equal':
            out = equality_cases(crit)
        elif group == 'clamp':
            out = clamp_cases() if crit == CLOSENESS else []
        else:
            out = [family_case(group.split('/')[1], crit, golden_dir)]
        _CASES[key] = out
    return _CASES[key]
