"""Plain high-precision references and checkers of the box, plane and filter kernels of csrc/segment.hip (vg_cluster_boxes,
vg_plane_ransac, vg_cluster_filter), shared by tests/test_segment_edges.py and its CPU tests of the checkers themselves.
numpy and python integers only: no torch, no GPU.

Boxes.  The hull is exact (integer arithmetic on the float32 values).  The rectangle of every hull edge is evaluated with the
reference's expressions (pointcloud_utils.py:331-357) in float64 and once more in extended precision, which gives the float64
evaluation's own error `K_REF`, in units of 2^-53 * S * P (S = largest |coordinate|, P = the rectangle's perimeter).  A kernel's
box may deviate from the float64 reference by K = 8 * K_REF of those units in an area and by K * 2^-53 * S in a length: the factor
8 covers a device libm whose atan2 / cos differ from the host's by a few ulp.  `check_box` checks properties, not one expected box:
where several edges give equally small rectangles (a square, an octagon, a lattice) libm's last bit decides between them.

Every checker raises AssertionError on a mismatch and returns what it measured (for the test log)."""
import math

import numpy as np

PI2 = np.pi / 2.
U53 = 2.0 ** -53
K_REF = 2.66       # the float64 rectangle's own error over all clusters of test_segment_edges.py: measured 2.657 (test_box_bound_k_ref)
K_BOX = 8 * K_REF
ANGLE_MATCH = 2.0 ** -48       # identifies the hull edge a box was built on: 8 ulp of an atan2 result (<= pi), nothing else uses it

if np.finfo(np.longdouble).eps < 2.0 ** -60:
    _EXT = np.longdouble
else:                                                      # platforms whose long double is a double
    try:
        import mpmath as _mp
    except ImportError as e:                               # pragma: no cover
        raise ImportError('segment_ref needs an extended precision: np.longdouble is a double here and mpmath does not import') from e
    _mp.mp.prec = 113
    _EXT = None


# ---------------------------------------------------------------------------------------------------------------- hull
def _as_ints(xy):
    """float32 coordinates -> python ints on one common power-of-two scale (exact)."""
    vals = [[float(v) for v in p] for p in np.asarray(xy, dtype=np.float32)]
    den = 1
    for p in vals:
        for v in p:
            den = max(den, v.as_integer_ratio()[1])
    out = []
    for p in vals:
        row = []
        for v in p:
            n, d = v.as_integer_ratio()
            row.append(n * (den // d))
        out.append(tuple(row))
    return out


def exact_hull(xy_f32):
    """Strict convex hull vertices of float32 points, counter-clockwise, as a float64 [H, 2] array: collinear points dropped,
    duplicates merged.  1 vertex for identical points, 2 for collinear ones.  Monotone chain on exact integers."""
    xy = np.asarray(xy_f32, dtype=np.float32).reshape(-1, 2)
    ints = _as_ints(xy)
    first = {}
    for k, p in enumerate(ints):
        first.setdefault(p, k)
    pts = sorted(first)
    if len(pts) <= 2:
        return xy[[first[p] for p in pts]].astype(np.float64)

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    def chain(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and cross(h[-2], h[-1], p) <= 0:
                h.pop()
            h.append(p)
        return h
    lower, upper = chain(pts), chain(pts[::-1])
    hull = lower[:-1] + upper[:-1]
    return xy[[first[p] for p in hull]].astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- rectangles
def _rectangles(hull, dt):
    h = np.asarray(hull, dtype=dt)
    pi2 = dt(PI2)                                          # the reference's float64 constant in either precision: the same function
    e = np.roll(h, -1, axis=0) - h                         # every edge, the closing one included
    ang = np.abs(np.mod(np.arctan2(e[:, 1], e[:, 0]), pi2))
    r00, r01, r10 = np.cos(ang), np.cos(ang - pi2), np.cos(ang + pi2)
    x = r00[:, None] * h[None, :, 0] + r01[:, None] * h[None, :, 1]
    y = r10[:, None] * h[None, :, 0] + r00[:, None] * h[None, :, 1]
    mnx, mxx, mny, mxy = x.min(1), x.max(1), y.min(1), y.max(1)
    return {'angle': ang, 'r': (r00, r01, r10), 'mnx': mnx, 'mxx': mxx, 'mny': mny, 'mxy': mxy, 'wx': mxx - mnx, 'wy': mxy - mny,
            'area': (mxx - mnx) * (mxy - mny)}


def _rectangles_mp(hull):                                  # pragma: no cover  (only where long double is a double)
    mp = _mp
    pi2 = mp.mpf(PI2)
    H = [(mp.mpf(float(x)), mp.mpf(float(y))) for x, y in hull]
    out = {k: [] for k in ('angle', 'wx', 'wy', 'area')}
    for i, (x0, y0) in enumerate(H):
        x1, y1 = H[(i + 1) % len(H)]
        a = mp.atan2(y1 - y0, x1 - x0)
        a = abs(a - pi2 * mp.floor(a / pi2))
        c, s, m = mp.cos(a), mp.cos(a - pi2), mp.cos(a + pi2)
        xs = [c * x + s * y for x, y in H]
        ys = [m * x + c * y for x, y in H]
        wx, wy = max(xs) - min(xs), max(ys) - min(ys)
        for k, v in zip(('angle', 'wx', 'wy', 'area'), (a, wx, wy, wx * wy)):
            out[k].append(float(v))
    return {k: np.array(v) for k, v in out.items()}


def min_area_rectangles(hull, extended=False):
    """pointcloud_utils.py:329-357 for EVERY edge of the hull cycle: angle = abs(mod(atan2(dy, dx), pi/2)), rotation
    [[cos a, cos(a - pi/2)], [cos(a + pi/2), cos a]] (cosines, as the reference writes them), extents of the rotated hull, area.
    float64, or extended precision (`extended=True`).  -> dict of per-edge arrays: angle, mnx, mxx, mny, mxy, wx, wy, area."""
    if not extended:
        return _rectangles(hull, np.float64)
    return _rectangles(hull, _EXT) if _EXT is not None else _rectangles_mp(hull)


def scale_of(points):
    """S: the largest absolute xy coordinate."""
    return float(np.abs(np.asarray(points, dtype=np.float64)[:, :2]).max())


def measure_k_ref(points):
    """Largest deviation of the float64 rectangles of `points`' exact hull from the extended-precision ones: areas in units of
    2^-53 * S * P, side lengths in units of 2^-53 * S (sides compared as an unordered pair: an angle a hair below pi/2 in one
    precision and 0 in the other names the same rectangle with its sides exchanged).  0 for a degenerate hull."""
    hull = exact_hull(np.asarray(points)[:, :2])
    if len(hull) < 3:
        return 0.0
    S = scale_of(points)
    lo, hi = min_area_rectangles(hull), min_area_rectangles(hull, extended=True)
    P = 2 * (lo['wx'] + lo['wy'])
    d_area = np.abs(hi['area'] - lo['area']).astype(np.float64) / (U53 * S * P)
    a64 = np.sort(np.stack([lo['wx'], lo['wy']]), axis=0)
    aext = np.sort(np.stack([hi['wx'], hi['wy']]), axis=0)
    d_len = np.abs(aext - a64).astype(np.float64).max(0) / (U53 * S)
    return float(max(d_area.max(), d_len.max()))


def z_box(points):
    """(cz, h) of zero_shot_detector.py:459-461: the height is a float32 difference, cz = zmin + h / 2 and h + 0.3 in float64."""
    z = np.asarray(points, dtype=np.float32)[:, 2]
    zmin, zmax = z.min(), z.max()
    h32 = np.float32(zmax - zmin)
    assert h32.dtype == np.float32
    return float(zmin) + float(h32) / 2, float(h32) + 0.3


def emulate_box(points, hull=None, edges=None, swap_rz=True, z64=False):
    """What a correct kernel writes, in float64 with the host's libm: (box7, aux3).  The switches synthesise wrong kernels:
    `hull` = the vertices it wrapped (default: the exact hull), `edges` = the hull edges it tries (default: all),
    swap_rz=False exchanges l and w without adding pi/2, z64 computes the height in float64."""
    pts = np.asarray(points, dtype=np.float32)
    full = exact_hull(pts[:, :2])
    hull = full if hull is None else np.asarray(hull, dtype=np.float64)
    cz, h = z_box(pts)
    if z64:
        z = pts[:, 2].astype(np.float64)
        cz, h = z.min() + (z.max() - z.min()) / 2, (z.max() - z.min()) + 0.3
    if len(hull) < 3:
        m = pts[:, :2].astype(np.float64).mean(0)
        return np.array([m[0], m[1], cz, 0.1, 0.1, h, 0.0]), np.array([len(hull), 0.0, 1.0], dtype=np.float32)
    R = min_area_rectangles(hull)
    cand = np.arange(len(hull)) if edges is None else np.asarray(edges)
    order = sorted(cand, key=lambda i: (R['area'][i], R['angle'][i]))
    b = order[0]
    r00, r01, r10 = (v[b] for v in R['r'])
    mnx, mxx, mny, mxy = R['mnx'][b], R['mxx'][b], R['mny'][b], R['mxy'][b]
    c0 = np.array([mxx * r00 + mny * r10, mxx * r01 + mny * r00])
    c1 = np.array([mnx * r00 + mny * r10, mnx * r01 + mny * r00])
    c2 = np.array([mnx * r00 + mxy * r10, mnx * r01 + mxy * r00])
    c3 = np.array([mxx * r00 + mxy * r10, mxx * r01 + mxy * r00])
    l, w, rz = np.linalg.norm(c0 - c1), np.linalg.norm(c0 - c3), R['angle'][b]
    if w > l:
        l, w = w, l
        if swap_rz:
            rz = rz + np.pi / 2
    c = (c0 + c2) / 2
    return np.array([c[0], c[1], cz, l, w, h, rz]), np.array([len(hull), R['area'][b], 0.0], dtype=np.float32)


def check_box(points_f32, box7, aux3, k=K_BOX):
    """Properties of one cluster's box (see the module text).  -> the largest share of the bound k * 2^-53 * S * P (areas) or
    k * 2^-53 * S (lengths) that the box uses; 0.0 for a degenerate cluster."""
    pts = np.asarray(points_f32, dtype=np.float32)
    box, aux = np.asarray(box7, dtype=np.float64), np.asarray(aux3, dtype=np.float32)
    hull = exact_hull(pts[:, :2])
    cz, h = z_box(pts)
    assert box[2] == cz and box[5] == h, ('cz, h are float32(zmax - zmin) arithmetic', box[[2, 5]], (cz, h))
    assert aux[0] == len(hull), ('hull vertices', float(aux[0]), len(hull))
    S = scale_of(pts)
    if len(hull) < 3:
        assert aux[2] == 1 and aux[1] == 0, ('degenerate flag', aux)
        n = len(pts)
        mean = np.array([math.fsum(pts[:, 0].astype(np.float64)), math.fsum(pts[:, 1].astype(np.float64))]) / n
        # a float64 sum of n values of magnitude <= S in any order, then one division: (n - 1) + 1 roundings of at most 2^-53 * n * S / n
        assert np.abs(box[:2] - mean).max() <= n * U53 * S, ('0.1 m square at the float64 mean', box[:2], mean)
        assert box[3] == 0.1 and box[4] == 0.1 and box[6] == 0.0, box
        return 0.0
    assert aux[2] == 0, ('degenerate flag on a hull with area', aux)
    R = min_area_rectangles(hull)
    l, w, rz = box[3], box[4], box[6]
    assert l >= w, ('l >= w', l, w)
    used_best, why = None, []
    for swapped in (False, True):
        for i in np.flatnonzero(np.abs(R['angle'] + (PI2 if swapped else 0.0) - rz) <= ANGLE_MATCH):
            a_len, a_wid = (R['wy'][i], R['wx'][i]) if swapped else (R['wx'][i], R['wy'][i])
            P = 2 * (R['wx'][i] + R['wy'][i])
            b_area, b_len = k * U53 * S * P, k * U53 * S
            r00, r01, r10 = (v[i] for v in R['r'])
            u, v = (R['mxx'][i] + R['mnx'][i]) / 2, (R['mxy'][i] + R['mny'][i]) / 2
            centre = np.array([u * r00 + v * r10, u * r01 + v * r00])
            used = {'sides': max(abs(l - a_len), abs(w - a_wid)) / b_len,
                    'area': abs(l * w - R['area'][i]) / b_area,
                    'aux area': max(0.0, abs(float(aux[1]) - R['area'][i]) - float(np.spacing(np.float32(R['area'][i]))) / 2) / b_area,
                    'minimum over all edges': (R['area'][i] - R['area'].min()) / b_area,
                    'centre': np.abs(box[:2] - centre).max() / b_len}
            # every input point inside the rectangle: l lies along the direction rz (either way round)
            E = np.longdouble
            d = pts[:, :2].astype(E) - box[:2].astype(E)
            cr, sr = np.cos(E(rz)), np.sin(E(rz))
            along, across = np.abs(d[:, 0] * cr + d[:, 1] * sr), np.abs(-d[:, 0] * sr + d[:, 1] * cr)
            used['inside'] = float(max((along - l / 2).max(), (across - w / 2).max(), 0)) / b_len
            worst = max(used.values())
            if worst <= 1.0:
                used_best = worst if used_best is None else min(used_best, worst)
            else:
                why.append((int(i), swapped, {n_: float(v_) for n_, v_ in used.items() if v_ > 1.0}))
    assert used_best is not None, ('no hull edge explains the box within the bound (edge, swapped, shares of the bound above 1)',
                                   why or 'rz mod pi/2 is no edge angle', box)
    return float(used_best)


# ---------------------------------------------------------------------------------------------------------------- plane
def _sample3(seed, it, n):
    from oracle import segment_oracle as so
    return so.sample3(seed, it, n)


def _distances(P, plane):
    a, b, c, d = (float(v) for v in plane)
    with np.errstate(all='ignore'):
        return (((a * P[:, 0] + b * P[:, 1]) + c * P[:, 2]) + d) / np.sqrt((a * a + b * b) + c * c)


def plane_reference(points, idx, thresh, iters, seed):
    """The bit-exact target of vg_plane_ransac: oracle.segment_oracle.plane_ransac on points[idx] (idx None = all rows).
    -> (plane4 float64, flags uint8 [n], count)."""
    from oracle import segment_oracle as so
    P = np.asarray(points)[:, :3] if idx is None else np.asarray(points)[np.asarray(idx), :3]
    eq, inl = so.plane_ransac(P, thresh, iters, seed)
    flags = np.zeros(len(P), np.uint8)
    flags[inl] = 1
    return eq, flags, len(inl)


def check_plane(points, idx, thresh, iters, seed, plane, flags, count):
    """Cross-check that shares no code with the oracle's loop: every hypothesis is rebuilt with np.cross in extended precision and
    its inliers counted by brute force; the returned plane must pass through the three sampled points of the FIRST iteration with
    the largest count, and flags / count must be the brute-force ones of the returned plane.  -> it_best (-1: no hypothesis has
    an inlier, e.g. all points collinear: the plane is then all zeros, never NaN)."""
    P32 = np.asarray(points)[:, :3] if idx is None else np.asarray(points)[np.asarray(idx), :3]
    P = P32.astype(np.float64)
    n = len(P)
    plane, flags = np.asarray(plane, dtype=np.float64), np.asarray(flags)
    assert np.isfinite(plane).all(), ('NaN plane', plane)
    E = np.longdouble
    counts, samples = np.zeros(iters, np.int64), []
    for it in range(iters):
        s = _sample3(seed, it, n)
        samples.append(s)
        nrm = np.cross(P[s[1]].astype(E) - P[s[0]].astype(E), P[s[2]].astype(E) - P[s[0]].astype(E))
        ln = np.sqrt((nrm * nrm).sum())
        if not ln > 0:
            continue                                        # a degenerate triple: NaN distances, no inlier
        dist = np.abs((P.astype(E) - P[s[1]].astype(E)) @ (nrm / ln))
        near = np.abs(dist - thresh) <= 2.0 ** -40 * max(1.0, float(np.abs(P).max()))
        if near.any():                                      # within rounding of the threshold: the float64 expression decides
            pl = np.r_[(nrm / ln).astype(np.float64), 0.0]
            pl[3] = -((pl[0] * P[s[1], 0] + pl[1] * P[s[1], 1]) + pl[2] * P[s[1], 2])
            counts[it] = int((np.abs(_distances(P, pl)) <= thresh).sum())
        else:
            counts[it] = int((dist <= thresh).sum())
    best = int(counts.max())
    if best == 0:
        assert not plane.any() and count == 0 and not flags.any(), ('no hypothesis has inliers: zero plane, no flags', plane, count)
        return -1
    it_best = int(np.flatnonzero(counts == best)[0])
    want = (np.abs(_distances(P, plane)) <= thresh)
    assert count == int(want.sum()), ('count is the brute-force count of the returned plane', count, int(want.sum()))
    assert np.array_equal(flags.astype(bool), want), 'inlier flags (<= thresh, inclusive)'
    assert count == best, ('the largest count over all hypotheses', count, best)
    assert abs(math.sqrt(float((plane[:3] ** 2).sum())) - 1) <= 4 * U53, ('unit normal', plane)
    S = max(1.0, float(np.abs(P).max()))
    through = np.abs(_distances(P[samples[it_best]], plane))
    # the normal carries the relative error of a float64 cross product of differences: a few 2^-53 of |A||B| / |A x B| ...
    A, B = P[samples[it_best][1]] - P[samples[it_best][0]], P[samples[it_best][2]] - P[samples[it_best][0]]
    cond = np.linalg.norm(A) * np.linalg.norm(B) / np.linalg.norm(np.cross(A, B))
    assert through.max() <= 16 * U53 * S * cond, ('the plane passes through the sample of the first best iteration', it_best, through)
    return it_best


# ---------------------------------------------------------------------------------------------------------------- filter
def filter_reference(points, plane, min_points=10, max_points=999999, max_min_height=1.0, min_max_height=0.5, min_height=0.3,
                     max_height=6.0):
    """vg_cluster_filter of ONE cluster: (stats float32 [6] = {n, zmin, zmax, dmin, dmax, height}, valid).  The plane distance is
    the kernel's expression order in float64, (((a x + b y) + c z) + d) / sqrt((a^2 + b^2) + c^2): + - * / sqrt are correctly
    rounded on both sides, so float32() of the extremes is the exact target.  An empty cluster keeps the reductions' identities
    (zmin = dmin = +inf, zmax = dmax = -inf, height = -inf) and is invalid unless no filter can fail."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, np.asarray(points).shape[-1])
    n = len(p)
    a, b, c, d = (float(v) for v in plane)
    inv = math.sqrt((a * a + b * b) + c * c)
    if n:
        x, y, z = (p[:, k].astype(np.float64) for k in range(3))
        with np.errstate(all='ignore'):
            dist = (((a * x + b * y) + c * z) + d) / inv
        zmin, zmax, dmin, dmax = p[:, 2].min(), p[:, 2].max(), dist.min(), dist.max()
    else:
        zmin, zmax, dmin, dmax = np.float32(np.inf), np.float32(-np.inf), np.inf, -np.inf
    with np.errstate(all='ignore'):
        height = np.float32(zmax - zmin)
    ok = (min_points <= n <= max_points) and (dmin <= max_min_height and dmax >= min_max_height) \
        and (float(height) >= min_height and float(height) <= max_height)
    with np.errstate(over='ignore'):
        stats = np.array([np.float32(n), zmin, zmax, np.float32(dmin), np.float32(dmax), height], dtype=np.float32)
    return stats, bool(ok)


def check_filter(points, plane, stats, valid, **thresholds):
    want, ok = filter_reference(points, plane, **thresholds)
    got = np.asarray(stats, dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ('stats bit for bit', got, want)
    assert bool(valid) == ok, ('valid', bool(valid), ok, want)
