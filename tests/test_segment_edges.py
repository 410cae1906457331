"""The box, plane and filter kernels of csrc/segment.hip (vg_cluster_boxes, vg_plane_ransac, vg_cluster_filter) at the shapes where
kernels go wrong: block-stride boundaries, tie rules, inclusive thresholds, degenerate input, the hull capacity.

CPU: the references and checkers of tests/segment_ref.py against scipy / the oracle, and against synthesised wrong kernels.
GPU: the kernels through the C ABI -- every cluster of a group in ONE ragged launch, the clusters' rows scattered over the point array.
"""
import ctypes

import numpy as np
import pytest

import segment_ref as sr
from oracle import segment_oracle as so

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------ box clusters
def _rot(p, yaw):
    yaw = float(F32(yaw))
    R = np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
    q = np.array(p, dtype=np.float64, copy=True)
    q[:, :2] = q[:, :2] @ R.T
    return q


def _cloud(rng, n, centre, yaw=0.6, half=(2.2, 0.9, 0.8)):
    p = rng.uniform(-1, 1, size=(n, 3)) * half
    return (_rot(p, yaw) + [centre[0], centre[1], 0.4]).astype(F32)


def circle(n, r=3.0, centre=(20.0, -10.0)):
    """float32 circle of n points: n strict hull vertices (checked by test_capacity_circles_have_the_stated_hulls)."""
    t = 2 * np.pi * np.arange(n) / n
    z = np.where(np.arange(n) % 2 == 0, 0.25, 1.5)
    return np.stack([centre[0] + r * np.cos(t), centre[1] + r * np.sin(t), z], 1).astype(F32)


def _winner_cluster(rng, n, which, pos):
    """n points whose start vertex (lowest y), next hull vertex, lowest z and highest z are four known points; `which` of them sits
    at position `pos` of the cluster's index list."""
    p = _cloud(rng, n, (20.0, -10.0))
    w = {'start': 1 % n, 'next': 2 % n, 'zmin': 3 % n, 'zmax': 4 % n}
    p[w['start'], :2] = (20.0, -15.0)
    p[w['next'], :2] = (26.0, -14.875)
    p[w['zmin'], 2] = -5.0
    p[w['zmax'], 2] = 7.0
    j = w[which]
    p[[j, pos]] = p[[pos, j]]
    return p


# Triples (a, b, c) inside 2^-20 .. 2^2 whose orientation the rounded float64 expression gets wrong (it returns 0: the line through b and
# c passes a at 2^-52 of the size of the products).  Found by a seeded search over lines through a point near the origin.
SLIVERS = [((-1.213900645780086e-06, -1.340969333796238e-06), (1.6394978761672974, 1.282660722732544), (2.0569822788238525, 1.6092796325683594)),
           ((-1.6518041547897155e-06, 3.212169303878909e-06), (1.4059200286865234, 1.7803527116775513), (1.806897521018982, 2.288119316101074)),
           ((9.665805009717587e-07, 1.348856017102662e-06), (1.0425288677215576, 1.170340657234192), (1.8912845849990845, 2.1231517791748047)),
           ((-2.4792934709694237e-06, 1.7649724668444833e-06), (1.833655595779419, 0.56951504945755), (2.5073866844177246, 0.7787682414054871))]


def _straddle():
    """Coordinates from 2^-20 to 2^2 on both sides of both axes; on every edge of the outline three more points, each one float32
    ulp off the line through the edge's ends (alternately outside = a vertex, inside = none): orientation products of ~70 bits."""
    V = np.array([[2.0 ** -20, -2.0 ** -18], [4.0, -2.0 ** -19], [3.0, 4.0], [-2.0 ** -19, 3.5], [-1.5 * 2.0 ** -20, 2.0 ** -20]])
    pts, k = [tuple(v) for v in V.astype(F32)], 0
    for i in range(len(V)):
        A, B = V[i].astype(F32).astype(np.float64), V[(i + 1) % len(V)].astype(F32).astype(np.float64)
        for t in (0.25, 0.5, 0.75, 2.0 ** -12):
            m = (A + t * (B - A)).astype(F32)
            ax = 1 if abs(B[0] - A[0]) >= abs(B[1] - A[1]) else 0          # nudge across the edge
            m[ax] = np.nextafter(m[ax], F32(np.inf) if k % 2 else F32(-np.inf))
            pts.append((m[0], m[1]))
            k += 1
    pts += [q for tri in SLIVERS for q in tri]
    xy = np.array(pts, dtype=F32)
    assert 2.0 ** -23 <= np.abs(xy).min() and np.abs(xy).max() == 4.0         # (no point of an edge falls on an axis)
    return np.c_[xy, np.linspace(0, 1, len(xy)).astype(F32)].astype(F32)


def box_cases():
    """name -> [n, 3] float32 points, in the order of the cluster's index list."""
    rng = np.random.default_rng(11)
    c = {}
    c['one'] = np.array([[3.5, -2.0, 0.7]], F32)
    c['two'] = np.array([[3.5, -2.0, 0.7], [4.5, -1.0, 0.1]], F32)
    c['two_identical'] = np.array([[3.5, -2.0, 0.7], [3.5, -2.0, 0.1]], F32)
    c['triangle'] = np.array([[3.5, -2.0, 0.7], [4.5, -1.0, 0.1], [3.0, 1.0, 0.3]], F32)
    c['collinear3'] = np.array([[1.0, 2.0, 0.7], [2.0, 4.0, 0.1], [1.5, 3.0, 0.3]], F32)
    c['four_two_coincide'] = np.array([[3.5, -2.0, 0.7], [4.5, -1.0, 0.1], [3.5, -2.0, 0.2], [3.0, 1.0, 0.3]], F32)
    c['identical'] = np.tile(np.array([[1.5, -2.0, 0.3]], F32), (7, 1))
    c['hline'] = np.c_[rng.permutation(9) * 0.5 + 3, np.full(9, -7.25), rng.uniform(0, 1, 9)].astype(F32)
    c['vline'] = np.c_[np.full(9, -7.25), rng.permutation(9) * 0.5 + 3, rng.uniform(0, 1, 9)].astype(F32)
    k = np.array([3, 0, 5, 5, 1, 0, 7, 3, 7, 2], np.float64)
    c['diag_dups'] = np.c_[1 + 0.25 * k, -2 + 0.5 * k, 0.125 * k].astype(F32)
    for n in (255, 256, 257, 1023):
        for which in ('start', 'next', 'zmin', 'zmax'):
            c[f'n{n}_{which}_first'] = _winner_cluster(rng, n, which, 0)
            c[f'n{n}_{which}_last'] = _winner_cluster(rng, n, which, n - 1)
    p = _cloud(rng, 40, (5.0, 5.0), yaw=0.0)
    p[:5, 0], p[:5, 1] = [7.0, 3.0, 5.0, 6.0, 4.0], 2.0                     # several points on the lowest y
    c['min_y_ties'] = p
    p = _cloud(rng, 300, (5.0, 5.0))
    p[17, :2] = (5.0, -1.0)
    p[[0, 150, 299], :2] = p[17, :2]                                        # the start vertex three more times
    c['start_dup3'] = p
    gx, gy = np.meshgrid(np.arange(17.0), np.arange(9.0))
    lat = np.c_[gx.ravel() / 16 + 20, gy.ravel() / 16 - 10, (gx.ravel() % 3) / 4]
    c['lattice'] = lat[rng.permutation(len(lat))].astype(F32)
    lat0 = np.c_[gx.ravel() / 16, gy.ravel() / 16, (gx.ravel() % 3) / 4]
    c['lattice_rotated'] = (_rot(lat0, 0.4) + [20, -10, 0])[rng.permutation(len(lat0))].astype(F32)
    sq = np.array([[0, 0], [2, 0], [2, 2], [0, 2], [1, 1], [0.5, 1.5], [1, 0], [2, 1]], np.float64) + [10, 4]
    c['square'] = np.c_[sq, np.linspace(0, 1, len(sq))].astype(F32)
    tall = np.array([[0, 0], [1, 0], [1, 3], [0, 3], [0.5, 1.5], [0.25, 2.5]], np.float64) + [-6, 2]
    c['tall_rectangle'] = np.c_[tall, np.linspace(0, 1, len(tall))].astype(F32)      # w > l before the swap
    t = np.pi / 4 * np.arange(8) + 0.2
    c['octagon'] = np.c_[12 + 2 * np.cos(t), -3 + 2 * np.sin(t), np.linspace(0, 2, 8)].astype(F32)
    c['far_rectangle'] = _cloud(rng, 400, (70.0, -55.0), yaw=1.1)
    c['near_rectangle'] = _cloud(rng, 400, (-0.4, 0.3), yaw=2.0, half=(1.5, 0.6, 0.5))
    c['straddle'] = _straddle()
    for k, tri in enumerate(SLIVERS):                                       # three vertices each: a triangle some 1e-16 m wide
        c[f'sliver{k}'] = np.c_[np.array(tri, dtype=F32), [0.5, 0.25, 1.0]].astype(F32)
    for n in (511, 512, 513, 1000):
        c[f'circle{n}'] = circle(n)
    return c


OVER_CAPACITY = ('circle513', 'circle1000')
# the float64 emulation of a correct kernel (segment_ref.emulate_box) may use 1 / 8 of the bound for the rectangle itself (k = 8 k_ref)
# and as much again for the corners, their centre and the side lengths computed from them (a rotation back and a norm)
EMULATION_SHARE = 0.25


def pack(clusters, seed=5):
    """Clusters -> (X [M, 5] float32 with the rows of all clusters scattered among filler rows, index, seg)."""
    rng = np.random.default_rng(seed)
    total = sum(len(c) for c in clusters)
    rows = rng.permutation(total + 37)
    X = rng.uniform(-50, 50, size=(total + 37, 5)).astype(F32)
    index, seg, o = [], [0], 0
    for c in clusters:
        r = rows[o:o + len(c)]
        X[r, :3] = c[:, :3]
        index.append(r)
        o += len(c)
        seg.append(o)
    return X, np.concatenate(index).astype(np.int32) if index else np.zeros(0, np.int32), np.array(seg, np.int32)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_exact_hull_equals_scipy_in_general_position():
    from scipy import spatial
    rng = np.random.default_rng(0)
    for n in (3, 4, 10, 100, 2000):
        p = (rng.normal(size=(n, 2)) * [3, 1] + [20, -10]).astype(F32)
        h = sr.exact_hull(p)
        want = p[spatial.ConvexHull(p.astype(np.float64)).vertices].astype(np.float64)
        assert {tuple(v) for v in h} == {tuple(v) for v in want}
        k = int(np.flatnonzero((want == h[0]).all(1))[0])                  # both counter-clockwise: equal up to the start
        assert np.array_equal(np.roll(want, -k, axis=0), h)
    assert len(sr.exact_hull(np.array([[1, 1], [1, 1], [1, 1]], F32))) == 1
    assert len(sr.exact_hull(np.array([[1, 2], [3, 6], [2, 4], [2, 4]], F32))) == 2
    assert len(sr.exact_hull(box_cases()['lattice'][:, :2])) == 4


def test_capacity_circles_have_the_stated_hulls():
    for n in (511, 512, 513, 1000):
        assert len(sr.exact_hull(circle(n)[:, :2])) == n


RING_SIZES = (512, 513, 1024, 1025)          # VG_BOX_MAX_HULL and the filter's hull capacity (filters_ref.HULL_CAPACITY), and one more


def ring(n, start_first):
    """circle(n) with its start vertex (lowest y, then lowest x) at the first or the last position of the index list"""
    p = circle(n)
    s = int(np.lexsort((p[:, 0], p[:, 1]))[0])
    rest = np.delete(np.arange(n), s)
    return p[np.r_[s, rest] if start_first else np.r_[rest, s]]


def hull_cases():
    """The clusters both hull callers (vg_cluster_boxes, vg_cluster_filter_ex) are run on: box_cases() from 3 points up and the rings."""
    c = {name: p for name, p in box_cases().items() if len(p) >= 3}
    for n in RING_SIZES:
        c[f'ring{n}_start_first'], c[f'ring{n}_start_last'] = ring(n, True), ring(n, False)
    return c


def test_capacity_rings_have_the_stated_hulls():
    for n in RING_SIZES:
        for first in (True, False):
            p = ring(n, first)
            assert len(sr.exact_hull(p[:, :2])) == n
            low = p[:, 1] == p[:, 1].min()
            assert low.sum() == 1 and low[0 if first else n - 1]


def test_rectangle_reference_agrees_with_the_oracle_on_tie_free_shapes():
    """so.fit_box(all_edges=True) evaluates the reference's float32 expression sequence on qhull's vertices: its box is the float64
    all-edges box within float32 resolution of the coordinates."""
    rng = np.random.default_rng(3)
    for centre in ((20.0, -10.0), (70.0, -55.0), (-0.4, 0.3)):
        for n in (12, 60, 500):
            p = _cloud(rng, n, centre, yaw=rng.uniform(0.1, 1.4))
            box, aux = sr.emulate_box(p)
            want = so.fit_box(p, all_edges=True)
            tol = 64 * 2.0 ** -24 * sr.scale_of(p)
            ca, cb = so.box_corners_bev(box), so.box_corners_bev(want)
            assert np.abs(ca[:, None, :] - cb[None]).sum(-1).min(1).max() <= tol, (centre, n)
            assert abs(box[3] * box[4] - want[3] * want[4]) <= tol * 2 * (box[3] + box[4])
            # (cz, h: the oracle's numpy 2 keeps float32 scalars through `+ height / 2` and `+ 0.3`, numpy 1 -- and the kernel -- float64)
            assert np.abs(box[[2, 5]] - want[[2, 5]]).max() <= 2.0 ** -23 * max(1.0, np.abs(want[[2, 5]]).max())
            assert sr.check_box(p, box, aux) <= EMULATION_SHARE


def test_box_bound_k_ref():
    """k_ref: the float64 rectangles' deviation from the extended-precision ones over every cluster of this file, in units of
    2^-53 S P (areas) / 2^-53 S (sides).  segment_ref.K_REF is that measurement rounded up; the kernels get 8 x."""
    worst = {name: sr.measure_k_ref(p) for name, p in box_cases().items()}
    top = max(worst, key=worst.get)
    print(f'box bound: k_ref = {worst[top]:.3f} (cluster {top}); K_REF = {sr.K_REF}, kernels are held to k = {sr.K_BOX}')
    assert 0 < worst[top] <= sr.K_REF
    assert sr.K_BOX == 8 * sr.K_REF


def test_emulated_correct_boxes_pass():
    for name, p in box_cases().items():
        box, aux = sr.emulate_box(p)
        assert sr.check_box(p, box, aux) <= EMULATION_SHARE, name


def _rejects(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


def test_box_checker_rejects_synthesised_faults():
    cases = box_cases()
    # the parent commit's kernel on the 1000-vertex circle: a rectangle over the first 512 vertices counter-clockwise from the lowest
    p = cases['circle1000']
    hull = sr.exact_hull(p[:, :2])
    start = int(np.lexsort((hull[:, 0], hull[:, 1]))[0])
    part = np.roll(hull, -start, axis=0)[:512]
    box, aux = sr.emulate_box(p, hull=part)
    assert _rejects(sr.check_box, p, box, aux)
    aux_lie = aux.copy()
    aux_lie[0] = 1000
    assert _rejects(sr.check_box, p, box, aux_lie)                          # the box alone is wrong too: points outside, no such edge
    # the closing edge dropped where it is the best one
    rng = np.random.default_rng(8)
    p = _cloud(rng, 200, (20.0, -10.0), yaw=0.7)
    hull = sr.exact_hull(p[:, :2])
    R = sr.min_area_rectangles(hull)
    b = int(np.argmin(R['area']))
    rolled = np.roll(hull, -(b + 1), axis=0)                                 # the best edge is now the closing one
    assert int(np.argmin(sr.min_area_rectangles(rolled)['area'])) == len(hull) - 1
    box, aux = sr.emulate_box(p, hull=rolled, edges=np.arange(len(hull) - 1))
    assert _rejects(sr.check_box, p, box, aux)
    good, gaux = sr.emulate_box(p)
    assert sr.check_box(p, good, gaux) <= EMULATION_SHARE
    # l / w swapped without the +pi/2
    p = cases['tall_rectangle']
    box, aux = sr.emulate_box(p, swap_rz=False)
    assert _rejects(sr.check_box, p, box, aux)
    box, aux = sr.emulate_box(p)
    assert box[6] >= np.pi / 2 and sr.check_box(p, box, aux) <= EMULATION_SHARE
    bad = box.copy()
    bad[3], bad[4] = box[4], box[3]
    assert _rejects(sr.check_box, p, bad, aux)                              # l < w
    # the height in float64
    p = cases['far_rectangle'].copy()
    p[0, 2], p[1, 2] = F32(0.1), F32(1.7000001)
    p[2:, 2] = np.clip(p[2:, 2], 0.2, 1.6)
    box, aux = sr.emulate_box(p, z64=True)
    good, _ = sr.emulate_box(p)
    assert (box[5] != good[5] or box[2] != good[2]) and _rejects(sr.check_box, p, box, aux)
    # the centre off by one float32 ulp of S
    bad = good.copy()
    bad[0] += float(np.spacing(F32(sr.scale_of(p))))
    assert _rejects(sr.check_box, p, bad, aux)
    # flags and counts
    for name in ('collinear3', 'identical', 'two'):
        box, aux = sr.emulate_box(cases[name])
        assert sr.check_box(cases[name], box, aux) == 0.0
        for k, v in ((0, aux[0] + 1), (2, 0.0)):
            lie = aux.copy()
            lie[k] = v
            assert _rejects(sr.check_box, cases[name], box, lie), (name, k)
    box, aux = sr.emulate_box(cases['octagon'])
    lie = aux.copy()
    lie[2] = 1
    assert _rejects(sr.check_box, cases['octagon'], box, lie)


def test_naive_float64_orientation_is_wrong_on_the_straddling_cluster():
    """Why vg_orient splits its products: the rounded float64 expression gives a wrong sign for triples of the straddling cluster
    (a wrapping that trusts it takes each sliver for a line: 2 vertices, degenerate)."""
    p = box_cases()['straddle'][:, :2].astype(np.float64)
    ints = sr._as_ints(p.astype(F32))
    wrong = n = 0
    for a in range(len(p)):
        for b in range(len(p)):
            for c in range(b + 1, len(p)):
                if a in (b, c):
                    continue
                naive = (p[b, 0] - p[a, 0]) * (p[c, 1] - p[a, 1]) - (p[b, 1] - p[a, 1]) * (p[c, 0] - p[a, 0])
                exact = (ints[b][0] - ints[a][0]) * (ints[c][1] - ints[a][1]) - (ints[b][1] - ints[a][1]) * (ints[c][0] - ints[a][0])
                n += 1
                wrong += int(np.sign(naive) != (exact > 0) - (exact < 0))
    print(f'straddling cluster: the rounded float64 orientation has the wrong sign in {wrong} of {n} triples')
    assert wrong > 0
    for tri in SLIVERS:
        assert np.array_equal(np.array(tri, dtype=F32).astype(np.float64), np.array(tri)) and len(sr.exact_hull(np.array(tri, dtype=F32))) == 3


def _plane_cases():
    """name -> (P [m, stride] float32, idx or None, thresh, iters, seed)."""
    rng = np.random.default_rng(21)

    def ground(n, stride=5):
        P = np.zeros((n, stride), F32)
        P[:, 0], P[:, 1] = rng.uniform(-60, 60, n), rng.uniform(-60, 60, n)
        P[:, 2] = 0.01 * P[:, 0] + 0.004 * P[:, 1] + 0.03 + rng.normal(0, 0.03, n)
        P[: n // 10, 2] += rng.uniform(0.3, 2, n // 10).astype(F32)
        return P
    c = {}
    for n in (3, 4, 255, 256, 257, 1023, 1024, 1025):
        c[f'n{n}'] = (ground(n), None, 0.1, 20, 666)
    c['stride3'] = (ground(257, 3), None, 0.1, 20, 666)
    c['iters1'] = (ground(300), None, 0.1, 1, 666)
    for s in (0, 666, 2 ** 32 + 1, 2 ** 63 + 5):
        c[f'seed{s}'] = (ground(257), None, 0.1, 20, s)
    gx, gy = np.meshgrid(np.arange(16.0), np.arange(16.0))
    lat = np.c_[gx.ravel(), gy.ravel(), (gx.ravel() + 2 * gy.ravel()) / 4, np.zeros(256), np.zeros(256)].astype(F32)
    c['planar_lattice'] = (lat[rng.permutation(256)], None, 0.1, 30, 666)
    k = rng.permutation(50).astype(np.float64)
    c['collinear'] = (np.c_[0.25 * k, 0.5 * k, 0.75 * k, k, k].astype(F32), None, 0.1, 30, 666)
    four = ground(4)
    dup = np.r_[four[rng.integers(0, 4, 290)], ground(10)]
    c['duplicates'] = (dup[rng.permutation(300)], None, 0.1, 40, 666)
    flat = np.zeros((200, 5), F32)
    flat[:, 0], flat[:, 1] = rng.integers(-30, 30, 200), rng.integers(-30, 30, 200)
    edge = np.zeros((50, 5), F32)
    edge[:, 0], edge[:, 1] = rng.integers(-30, 30, 50), rng.integers(-30, 30, 50)
    edge[:20, 2], edge[20:40, 2] = 0.125, -0.125                                  # exactly at the threshold: inliers
    edge[40:45, 2], edge[45:, 2] = np.nextafter(F32(0.125), F32(1)), -np.nextafter(F32(0.125), F32(1))      # one ulp beyond
    c['at_threshold'] = (np.r_[flat, edge][rng.permutation(250)], None, 0.125, 100, 666)
    return c


def test_plane_checker_passes_the_oracle_and_rejects_synthesised_faults():
    cases = _plane_cases()
    for name, (P, idx, thresh, iters, seed) in cases.items():
        plane, flags, count = sr.plane_reference(P, idx, thresh, iters, seed)
        it = sr.check_plane(P, idx, thresh, iters, seed, plane, flags, count)
        assert (it == -1) == (name == 'collinear'), name
    P, idx, thresh, iters, seed = cases['at_threshold']
    plane, flags, count = sr.plane_reference(P, idx, thresh, iters, seed)
    assert count == 240 and np.array_equal(np.abs(plane), [0, 0, 1, 0])
    # `<` instead of `<=` at the threshold
    strict = (np.abs(P[:, 2].astype(np.float64)) < thresh).astype(np.uint8)
    assert strict.sum() == 200 and _rejects(sr.check_plane, P, idx, thresh, iters, seed, plane, strict, 200)
    assert _rejects(sr.check_plane, P, idx, thresh, iters, seed, plane, strict, count)
    # the plane of the second-best hypothesis
    done = 0
    for name in ('n1025', 'n1024', 'n257', 'seed0', 'seed666'):
        P, idx, thresh, iters, seed = cases[name]
        plane, flags, count = sr.plane_reference(P, idx, thresh, iters, seed)
        it_best = sr.check_plane(P, idx, thresh, iters, seed, plane, flags, count)
        if it_best == 0:
            continue
        eq2, inl2 = so.plane_ransac(P, thresh, it_best, seed)                  # the best of the iterations before the best one
        f2 = np.zeros(len(P), np.uint8)
        f2[inl2] = 1
        assert 0 < len(inl2) < count and _rejects(sr.check_plane, P, idx, thresh, iters, seed, eq2, f2, len(inl2)), name
        done += 1
    assert done >= 2
    # a NaN plane with flags set for collinear input
    P, idx, thresh, iters, seed = cases['collinear']
    assert _rejects(sr.check_plane, P, idx, thresh, iters, seed, np.full(4, np.nan), np.ones(len(P), np.uint8), len(P))


FILTER_PLANE = np.array([0.02, -0.04, 2.0, -1.5])          # not unit length
EXACT_PLANE = np.array([0.0, 0.0, 2.0, -1.0])              # distance = z - 0.5 exactly
THRESHOLDS = dict(min_points=8, max_points=1025, max_min_height=1.0, min_max_height=0.25, min_height=0.5, max_height=4.0)


def _filter_size_clusters():
    rng = np.random.default_rng(31)
    out = []
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        for pos in sorted({0, n - 1, min(63, n - 1), min(64, n - 1)}):
            p = (rng.uniform(-1, 1, size=(n, 3)) * [2, 1, 0.8] + [20, -10, 1.2]).astype(F32)
            p[pos] = (21.0, -10.5, 9.0)                                            # highest z and largest plane distance
            if n > 1:
                p[n - 1 - pos if n - 1 - pos != pos else (pos + 1) % n] = (19.0, -9.5, -4.0)     # lowest of both
            out.append(p)
    out.append((rng.uniform(-1, 1, size=(70, 3)) * [2, 1, 0.8] + [20, -10, -3.0]).astype(F32))     # wholly below the plane
    out.insert(5, np.zeros((0, 3), F32))                                                        # a zero-length segment
    return out


def _filter_threshold_clusters():
    """(points, expected verdict) under EXACT_PLANE and THRESHOLDS: every threshold hit exactly (valid), and one float32 ulp beyond."""
    up, dn = (lambda v: np.nextafter(F32(v), F32(np.inf))), (lambda v: np.nextafter(F32(v), F32(-np.inf)))

    def cl(n, zlo, zhi):
        p = np.zeros((n, 3), F32)
        p[:, 0], p[:, 1] = np.arange(n) % 7, np.arange(n) % 5
        p[:, 2] = np.linspace(zlo, zhi, n).astype(F32)
        p[0, 2], p[-1, 2] = zlo, zhi
        return p
    return [(cl(8, 0.5, 2.0), True), (cl(7, 0.5, 2.0), False),                  # n == min_points
            (cl(1025, 0.5, 2.0), True), (cl(1026, 0.5, 2.0), False),            # n == max_points
            (cl(20, 1.0, 1.5), True), (cl(20, 1.0, dn(1.5)), False),            # height == min_height
            (cl(20, -1.0, 3.0), True), (cl(20, -1.0, up(up(3.0))), False),      # height == max_height (4 + 2^-21: the next float32)
            (cl(20, 1.5, 3.0), True), (cl(20, up(1.5), 3.0), False),            # dmin == max_min_height
            (cl(20, 0.25, 0.75), True), (cl(20, 0.25, dn(0.75)), False)]        # dmax == min_max_height


def test_filter_reference_agrees_with_the_oracle_and_rejects_synthesised_faults():
    for p in _filter_size_clusters():
        if len(p) == 0:
            continue
        st, ok = sr.filter_reference(p, FILTER_PLANE, **THRESHOLDS)
        ok2, st2 = so.filter_cluster(p, FILTER_PLANE, **THRESHOLDS)
        assert ok == ok2 and st[0] == st2[0] and st[1] == F32(st2[1]) and st[2] == F32(st2[2]) and st[5] == F32(st2[5])
        assert np.allclose(st[3:5], st2[3:5], rtol=0, atol=1e-5)
        sr.check_filter(p, FILTER_PLANE, st, ok, **THRESHOLDS)
    for p, want in _filter_threshold_clusters():
        st, ok = sr.filter_reference(p, EXACT_PLANE, **THRESHOLDS)
        assert ok == want and so.filter_cluster(p, EXACT_PLANE, **THRESHOLDS)[0] == want
    # dmin / zmin over all but the last point
    p = [c for c in _filter_size_clusters() if len(c) == 257][0]              # (pos = 0: the lowest point is the last one)
    assert p[-1, 2] == -4.0
    st, ok = sr.filter_reference(p, FILTER_PLANE, **THRESHOLDS)
    st_bad, ok_bad = sr.filter_reference(p[:-1], FILTER_PLANE, **THRESHOLDS)
    st_bad[0] = st[0]
    assert _rejects(sr.check_filter, p, FILTER_PLANE, st_bad, ok, **THRESHOLDS)
    only_d = st.copy()
    only_d[3] = st_bad[3]
    assert _rejects(sr.check_filter, p, FILTER_PLANE, only_d, ok, **THRESHOLDS)
    one_ulp = st.copy()
    one_ulp[4] = np.nextafter(st[4], F32(np.inf))
    assert _rejects(sr.check_filter, p, FILTER_PLANE, one_ulp, ok, **THRESHOLDS)
    # an exclusive comparison at a threshold
    p, want = _filter_threshold_clusters()[8]
    st, ok = sr.filter_reference(p, EXACT_PLANE, **THRESHOLDS)
    assert want and _rejects(sr.check_filter, p, EXACT_PLANE, st, False, **THRESHOLDS)


def test_host_fallback_box_passes_the_checker():
    """vilgod_amd.boxes.all_edges_box: what fast mode fits on the host for a hull beyond the kernel's capacity."""
    from vilgod_amd import boxes as vb
    cases = box_cases()
    for name in ('circle513', 'circle1000', 'straddle', 'lattice', 'collinear3', 'identical', 'octagon', 'tall_rectangle', 'far_rectangle'):
        p = cases[name]
        h = vb.exact_hull_xy(p[:, :2])
        assert len(h) == len(sr.exact_hull(p[:, :2])), name
        box = vb.all_edges_box(p)
        n_h = len(h)
        aux = np.array([n_h, 0 if n_h < 3 else box[3] * box[4], n_h < 3], F32)
        assert sr.check_box(p, box, aux) <= EMULATION_SHARE, name


# ------------------------------------------------------------------------------------------------------------ GPU
def _run_boxes(cuda, clusters):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    X, index, seg = pack(clusters)
    d_X, d_index, d_seg = (torch.from_numpy(v).to(cuda) for v in (X, index, seg))
    C = len(clusters)
    box = torch.full((C, 7), -7.0, dtype=torch.float64, device=cuda)
    aux = torch.full((C, 3), -7.0, dtype=torch.float32, device=cuda)
    check(lib.vg_cluster_boxes(ptr(d_X), d_X.stride(0), ptr(d_index), ptr(d_seg), C, ptr(box), ptr(aux), stream_ptr()))
    return box.cpu().numpy(), aux.cpu().numpy(), (d_X, index, seg)


@pytest.mark.gpu
def test_hip_cluster_boxes_pass_the_property_check(cuda):
    """Every cluster of box_cases() in one launch.  Within capacity: check_box (exact hull count, an edge angle of the exact hull, its
    area, the smallest area, l >= w and the swap, all points inside, centre, float32 height arithmetic, flags) under k = 8 k_ref.
    Beyond capacity (513, 1000 vertices): the overflow flag and no rectangle -- never a box over part of the outline."""
    from vilgod_amd._lib import BOX_FLAG_HULL_OVERFLOW, BOX_MAX_HULL
    cases = box_cases()
    names = list(cases)
    box, aux, _ = _run_boxes(cuda, [cases[n] for n in names])
    used = {}
    for c, name in enumerate(names):
        if name in OVER_CAPACITY:
            assert aux[c, 2] == BOX_FLAG_HULL_OVERFLOW and aux[c, 0] == BOX_MAX_HULL and aux[c, 1] == 0, (name, aux[c])
            assert np.isnan(box[c, [0, 1, 3, 4, 6]]).all(), (name, box[c])
            assert (box[c, 2], box[c, 5]) == sr.z_box(cases[name]), name
            continue
        try:
            used[name] = sr.check_box(cases[name], box[c], aux[c])
        except AssertionError as e:
            raise AssertionError(f'cluster {name}: {e}') from e
    top = max(used, key=used.get)
    print(f'vg_cluster_boxes: {len(used)} clusters pass; largest share of the bound k = {sr.K_BOX} (8 x k_ref = {sr.K_REF}): '
          f'{used[top]:.3f} (cluster {top}); straddling cluster: {int(aux[names.index("straddle"), 0])} hull vertices')
    assert aux[names.index('lattice'), 0] == 4


def _run_area_filter(cuda, clusters):
    """vg_cluster_filter_ex with only the area filter active (every threshold open) -> stats [C, 16]"""
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr, check, FilterParams, FILTER_NAMES, FILTER_AND, FILTER_NSTATS
    X, index, seg = pack(clusters)
    d_X, d_index, d_seg = (torch.from_numpy(v).to(cuda) for v in (X, index, seg))
    C = len(clusters)
    p = FilterParams()
    p.active[FILTER_NAMES.index('filter_by_area')], p.logic[FILTER_NAMES.index('filter_by_area')] = 1, FILTER_AND
    stats = torch.full((C, FILTER_NSTATS), -7.0, dtype=torch.float64, device=cuda)
    verdict = torch.zeros((C, len(FILTER_NAMES)), dtype=torch.uint8, device=cuda)
    valid = torch.zeros(C, dtype=torch.uint8, device=cuda)
    check(lib.vg_cluster_filter_ex(ptr(d_X), d_X.stride(0), ptr(d_index), ptr(d_seg), C, ptr(torch.from_numpy(FILTER_PLANE).to(cuda)), None,
                                   ctypes.byref(p), ptr(stats), ptr(verdict), ptr(valid), stream_ptr()))
    return stats.cpu().numpy()


@pytest.mark.gpu
def test_hip_box_and_filter_hulls_agree(cuda):
    """The two callers of vg_hull_wrap (csrc/segment.hip) on the same clusters: where neither overflows, both report the exact hull's
    vertex count and the same degenerate flag.  Rings at both capacities, start vertex first and last in the index list: a hull of
    exactly the capacity closes unflagged, one more vertex is flagged and reports the capacity."""
    from vilgod_amd._lib import (BOX_FLAG_DEGENERATE, BOX_FLAG_HULL_OVERFLOW, BOX_MAX_HULL, FILTER_FLAG_DEGENERATE,
                                 FILTER_FLAG_HULL_OVERFLOW)
    import filters_ref as fr
    cases = hull_cases()
    names = list(cases)
    _, aux, _ = _run_boxes(cuda, [cases[n] for n in names])
    stats = _run_area_filter(cuda, [cases[n] for n in names])
    seen = set()
    for c, name in enumerate(names):
        nh = len(sr.exact_hull(cases[name][:, :2]))
        flags = int(stats[c, 12])
        box_over, fil_over = aux[c, 2] == BOX_FLAG_HULL_OVERFLOW, bool(flags & FILTER_FLAG_HULL_OVERFLOW)
        assert box_over == (nh > BOX_MAX_HULL) and fil_over == (nh > fr.HULL_CAPACITY), (name, nh, aux[c], stats[c, 11:13])
        assert aux[c, 0] == (BOX_MAX_HULL if box_over else nh), (name, nh, aux[c])
        assert stats[c, 11] == (fr.HULL_CAPACITY if fil_over else nh), (name, nh, stats[c, 11:13])
        if not box_over and not fil_over:
            assert aux[c, 0] == stats[c, 11] == nh, (name, nh, aux[c], stats[c, 11])
            assert (aux[c, 2] == BOX_FLAG_DEGENERATE) == bool(flags & FILTER_FLAG_DEGENERATE), (name, aux[c], flags)
        seen.add((nh, bool(box_over), fil_over))
    assert {(512, False, False), (513, True, False), (1024, True, False), (1025, True, True)} <= seen


@pytest.mark.gpu
def test_hip_fast_boxes_refit_hulls_beyond_capacity(cuda):
    """PseudoLabelPipeline.fit_boxes in fast mode (also what the tracker's static_box_of reads): one 1000-vertex ring among ordinary
    clusters -- every final box passes check_box, the ring's through the host refit."""
    import torch
    from vilgod_amd.pipeline import PseudoLabelPipeline
    cases = box_cases()
    names = ['far_rectangle', 'circle1000', 'octagon', 'circle513', 'n257_start_last', 'collinear3']
    X, index, seg = pack([cases[n] for n in names])
    pipe = PseudoLabelPipeline(device=cuda, max_points=len(X) + 16, clip_model_path='/nonexistent', box_mode='fast', box_workers=0)
    d_X = torch.from_numpy(X).to(cuda)
    got = pipe.fit_boxes(d_X, index, seg)
    assert got.shape == (len(names), 7) and np.isfinite(got).all()
    # pack='device' frames keep the lists on the device only (process_frame passes index = None): the refit gathers through those
    dev = pipe.fit_boxes(d_X, None, seg, torch.from_numpy(index).to(cuda), torch.from_numpy(seg).to(cuda))
    assert np.array_equal(dev, got)
    for c, name in enumerate(names):
        nh = len(sr.exact_hull(cases[name][:, :2]))
        aux = np.array([nh, 0 if nh < 3 else got[c, 3] * got[c, 4], nh < 3], F32)
        try:
            sr.check_box(cases[name], got[c], aux)
        except AssertionError as e:
            raise AssertionError(f'cluster {name}: {e}') from e


def _run_plane(cuda, P, idx, thresh, iters, seed):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    d_P = torch.from_numpy(np.ascontiguousarray(P)).to(cuda)
    n = len(P) if idx is None else len(idx)
    d_idx = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(cuda)
    work = torch.zeros(iters * 36 + 64, dtype=torch.uint8, device=cuda)
    plane = torch.full((4,), -7.0, dtype=torch.float64, device=cuda)
    flags = torch.full((n,), 7, dtype=torch.uint8, device=cuda)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=cuda)
    check(lib.vg_plane_ransac(ptr(d_P), P.shape[1], ptr(d_idx) if d_idx is not None else None, n, thresh, iters, ctypes.c_uint64(seed),
                              ptr(work), ptr(plane), ptr(flags), ptr(cnt), stream_ptr()))
    return plane.cpu().numpy(), flags.cpu().numpy(), int(cnt.item())


@pytest.mark.gpu
def test_hip_plane_ransac_edges_equal_oracle_and_cross_check(cuda):
    """Plane, flags and count bit-equal to the oracle AND consistent with the independent cross-check, at n = 3 .. 1025 (the count is
    split over 4 blocks of 256), stride 3 / 5, one iteration, 64-bit seeds, tied hypotheses (first wins), all-degenerate hypotheses
    (zero plane, never NaN), duplicate samples, points exactly at +-thresh (inclusive).  The same points through an index list."""
    rng = np.random.default_rng(2)
    for name, (P, _, thresh, iters, seed) in _plane_cases().items():
        want_plane, want_flags, want_count = sr.plane_reference(P, None, thresh, iters, seed)
        big = rng.uniform(-50, 50, size=(len(P) + 23, P.shape[1])).astype(F32)
        idx = rng.permutation(len(big))[:len(P)].astype(np.int32)
        big[idx] = P
        for pts, ix in ((P, None), (big, idx)):
            plane, flags, count = _run_plane(cuda, pts, ix, thresh, iters, seed)
            assert np.array_equal(plane, want_plane) and not np.isnan(plane).any(), (name, ix is None, plane, want_plane)
            assert np.array_equal(flags, want_flags) and count == want_count, (name, ix is None, count, want_count)
            try:
                sr.check_plane(pts, ix, thresh, iters, seed, plane, flags, count)
            except AssertionError as e:
                raise AssertionError(f'case {name}: {e}') from e
        if name == 'at_threshold':
            assert count == 240
        if name == 'planar_lattice':
            assert count == len(P)
        if name == 'collinear':
            assert count == 0 and not plane.any() and not flags.any()


def _run_filter(cuda, clusters, plane, th):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    X, index, seg = pack(clusters, seed=9)
    d_X, d_index, d_seg = (torch.from_numpy(v).to(cuda) for v in (X, index, seg))
    if len(index) == 0:
        d_index = torch.zeros(1, dtype=torch.int32, device=cuda)
    C = len(clusters)
    stats = torch.full((C, 6), -7.0, dtype=torch.float32, device=cuda)
    valid = torch.full((C,), 7, dtype=torch.uint8, device=cuda)
    d_plane = torch.from_numpy(plane).to(cuda)
    check(lib.vg_cluster_filter(ptr(d_X), d_X.stride(0), ptr(d_index), ptr(d_seg), C, ptr(d_plane), th['min_points'], th['max_points'],
                                th['max_min_height'], th['min_max_height'], th['min_height'], th['max_height'], ptr(stats), ptr(valid),
                                stream_ptr()))
    return stats.cpu().numpy(), valid.cpu().numpy()


@pytest.mark.gpu
def test_hip_cluster_filter_edges_equal_reference(cuda):
    """stats bit-equal to filter_reference and valid equal to its verdict: sizes 1 .. 1025 with the extremes at the first index, the
    last index and a wave boundary, a plane that is not unit length, a cluster below the plane, every threshold hit exactly
    (inclusive) and one float32 ulp beyond.  The zero-length segment: the oracle (so.filter_cluster) does not define it (np.max of
    nothing raises); the expectation is the behaviour include/vilgod_hip.h documents for vg_cluster_filter and vg_cluster_filter_ex:
    the reductions' identities (zmin = dmin = +inf, zmax = dmax = -inf, height = -inf), n = 0, invalid."""
    clusters = _filter_size_clusters()
    stats, valid = _run_filter(cuda, clusters, FILTER_PLANE, THRESHOLDS)
    for c, p in enumerate(clusters):
        try:
            sr.check_filter(p, FILTER_PLANE, stats[c], valid[c], **THRESHOLDS)
        except AssertionError as e:
            raise AssertionError(f'cluster {c} (n = {len(p)}): {e}') from e
    empty = [c for c, p in enumerate(clusters) if len(p) == 0][0]
    assert stats[empty, 0] == 0 and stats[empty, 5] == -np.inf and not valid[empty]
    hits = _filter_threshold_clusters()
    stats, valid = _run_filter(cuda, [p for p, _ in hits], EXACT_PLANE, THRESHOLDS)
    for c, (p, want) in enumerate(hits):
        sr.check_filter(p, EXACT_PLANE, stats[c], valid[c], **THRESHOLDS)
        assert bool(valid[c]) == want, c
