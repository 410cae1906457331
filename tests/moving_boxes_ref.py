"""Exact reference and shared fixtures for the oriented extents (csrc/oriented_extent.hip, vg_cluster_oriented_extents[_host]).

`ref_extents` evaluates the chain include/vilgod_hip.h states with fractions.Fraction: every float64 step -- the rounded product with
row 0 of the rotation, the fused product-and-sum with row 1 -- is ONE correctly rounded float(Fraction); the float32 subtraction in
front of it is numpy's float32 `-` (an IEEE basic operation: correctly rounded on every machine).  Minimum and maximum are taken in
Python.  No BLAS, nothing that depends on the machine.

`kernel_cases(B)` builds the shapes at which the kernel can go wrong (B = VG_OEXT_BLOCK); the host tests compare the host entry point
with `ref_extents` on them, the GPU tests compare the kernel with the host entry point on the same ones.
"""
from fractions import Fraction

import numpy as np

NAN6 = [float('nan')] * 6


def bits(a):
    """float64 array -> its bit patterns: `bit for bit` comparisons go through this (NaN payloads and the sign of zero count)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rot4_of_angles(angles):
    """float32 angles -> [n,4] float64 {r00, r01, r10, r11} of scipy's rotation about z, as tracking.moving_boxes builds it"""
    from scipy.spatial.transform import Rotation as R
    angles = np.asarray(angles, dtype=np.float32)
    return np.ascontiguousarray(R.from_euler('z', angles, degrees=False).as_matrix()[:, :2, :2].reshape(-1, 4))


def ref_extents(points, index, seg, pair_cluster, center3, rot4):
    points, center3, rot4 = np.asarray(points, np.float32), np.asarray(center3, np.float32).reshape(-1, 3), np.asarray(rot4, np.float64).reshape(-1, 4)
    C = len(seg) - 1
    pair_cluster = np.arange(C) if pair_cluster is None else np.asarray(pair_cluster)
    out = np.empty((len(pair_cluster), 6))
    for p, c in enumerate(pair_cluster):
        if not 0 <= c < C or seg[c + 1] <= seg[c] or not np.isfinite(center3[p]).all():
            out[p] = NAN6
            continue
        rows = points[np.asarray(index[seg[c]:seg[c + 1]]), :3]
        if not np.isfinite(rows).all():
            out[p] = NAN6
            continue
        cx, cy = center3[p, 0], center3[p, 1]
        r00, r01, r10, r11 = (Fraction(float(v)) for v in rot4[p])
        px, py = [], []
        for x, y in rows[:, :2]:
            dx, dy = Fraction(float(np.float32(x - cx))), Fraction(float(np.float32(y - cy)))       # float32 subtraction, rounded once
            px.append(float(dy * r10 + Fraction(float(dx * r00))))                                  # fma(dy, r10, fl(dx * r00))
            py.append(float(dy * r11 + Fraction(float(dx * r01))))
        z = [float(v) + 0.0 for v in rows[:, 2]]                                                    # (-0 is written as +0)
        out[p] = (min(px), max(px), min(py), max(py), min(z), max(z))
    return out


def float32_safe(v):
    """The fixture precondition of the final-box comparisons: the float32 a host BLAS's np.dot result rounds to does not depend on the
    summation order it used (any order stays within a few float64 ulps of `v`)."""
    return np.float32(v * (1 - 2.0 ** -50)) == np.float32(v) == np.float32(v * (1 + 2.0 ** -50))


def assert_float32_safe(ext, what=''):
    for e in np.asarray(ext).reshape(-1, 6):
        for v in e[:4]:
            assert float32_safe(v), (what, v)


class _Scene:
    """clusters of float32 points stored in shuffled order (the index lists are not monotonic), five columns per point"""

    def __init__(self, rng):
        self.rng, self.xyz, self.lists = rng, [], []
        self.n = 0

    def add(self, xyz, repeat=False):
        xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        ids = np.arange(self.n, self.n + len(xyz))
        if repeat and len(ids):                               # a list that names some of its points several times, in no order
            ids = np.r_[ids, self.rng.choice(ids, len(ids))]
            self.rng.shuffle(ids)
        self.xyz.append(xyz)
        self.lists.append(ids)
        self.n += len(xyz)
        return len(self.lists) - 1

    def far(self):
        """a neighbour whose points lie far outside every cluster's extents: a list read one element too far shows"""
        sign = 1.0 if len(self.lists) % 2 else -1.0
        return self.add(self.rng.uniform(-1, 1, (3, 3)) + sign * np.array([5e4, -7e4, 9e3]))

    def finish(self, pair_cluster, center3, rot4):
        xyz = np.concatenate(self.xyz) if self.xyz else np.zeros((0, 3), np.float32)
        perm = self.rng.permutation(len(xyz))
        where = np.empty(len(xyz), np.int64)
        where[perm] = np.arange(len(xyz))
        pts = np.concatenate([xyz[perm], self.rng.normal(size=(len(xyz), 2)).astype(np.float32)], axis=1)
        index = where[np.concatenate(self.lists)] if self.lists else np.zeros(0, np.int64)
        seg = np.r_[0, np.cumsum([len(i) for i in self.lists])]
        return dict(points=np.ascontiguousarray(pts, np.float32), index=index.astype(np.int32), seg=seg.astype(np.int32),
                    pair_cluster=None if pair_cluster is None else np.asarray(pair_cluster, np.int32),
                    center3=np.asarray(center3, np.float32).reshape(-1, 3), rot4=np.asarray(rot4, np.float64).reshape(-1, 4))


ORIGINS = [(0.0, 0.0, 0.0), (140.0, -90.0, 3.0), (-480.0, 510.0, -20.0), (1000.0, 1000.0, 0.0)]
FIXED_ANGLES = np.array([0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi], dtype=np.float32)


def _cluster(rng, n, origin, angle, place, B):
    """n points within +-1 m of `origin`, and two points far out along the direction `angle` -- one holds the maximum of x', y' and z,
    the other the minimum -- placed first, last, or at positions B - 1 and B of the list (the last lane of a trip and the first lane
    of the next; clamped to the list)."""
    xyz = rng.uniform(-1, 1, (n, 3)) + origin
    if n:
        c, s = np.cos(float(angle)), np.sin(float(angle))
        far = np.array([6 * c - 7 * s, 6 * s + 7 * c, 3.0])            # x' = 6, y' = 7 under a rotation by `angle` (either sense: far outside +-1.5)
        a, b = {'first': (0, 1), 'last': (n - 1, n - 2), 'block': (B - 1, B)}[place]
        a, b = min(max(a, 0), n - 1), min(max(b, 0), n - 1)
        xyz[a] = origin + far
        if b != a:
            xyz[b] = origin - far
    return xyz.astype(np.float32)


def kernel_cases(B):
    """-> [(name, case)], case = dict(points [N,5] f32, index, seg, pair_cluster (or None), center3, rot4)."""
    cases = []
    # ---- every size, the extremes at every place, each cluster between two far neighbours, two rotations per cluster ----
    rng = np.random.default_rng(2024)
    sc, pc, c3, ang = _Scene(rng), [], [], []
    k = 0
    for n in (1, 2, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, 0):
        for place in ('first', 'last', 'block'):
            origin = np.array(ORIGINS[k % 4])
            angles = np.array([FIXED_ANGLES[k % 5], rng.uniform(-np.pi, np.pi)], dtype=np.float32)
            k += 1
            sc.far()
            xyz = _cluster(rng, n, origin, angles[0], place, B)
            c = sc.add(xyz)
            med = np.median(xyz, axis=0) if n else origin.astype(np.float32)
            for a in angles:
                pc.append(c); c3.append(med); ang.append(a)
    sc.far()
    cases.append(('sizes', sc.finish(pc, c3, rot4_of_angles(ang))))
    # ---- one cluster of 20 001 points per place of the extremes ----
    rng = np.random.default_rng(2025)
    sc, pc, c3, ang = _Scene(rng), [], [], []
    for j, place in enumerate(('first', 'last', 'block')):
        origin, a = np.array(ORIGINS[1 + j]), np.float32(rng.uniform(-np.pi, np.pi))
        sc.far()
        xyz = _cluster(rng, 20001, origin, a, place, B)
        pc.append(sc.add(xyz)); c3.append(np.median(xyz, axis=0)); ang.append(a)
    sc.far()
    cases.append(('large', sc.finish(pc, c3, rot4_of_angles(ang))))
    # ---- 300 pairs over 40 clusters: clusters repeated under different rotations, in shuffled order; lists with repeated indices ----
    rng = np.random.default_rng(2026)
    sc, meds = _Scene(rng), []
    for c in range(40):
        xyz = (rng.normal(size=(int(rng.integers(1, 90)), 3)) * [1.5, 0.7, 0.6] + ORIGINS[c % 4]).astype(np.float32)
        sc.add(xyz, repeat=c % 3 == 0)
        meds.append(np.median(xyz, axis=0))
    pc = rng.integers(0, 40, 300)
    ang = np.r_[FIXED_ANGLES, rng.uniform(-np.pi, np.pi, 295).astype(np.float32)]
    many = sc.finish(pc, [meds[c] for c in pc], rot4_of_angles(ang))
    cases.append(('pairs300', many))
    cases.append(('pairs1', dict(many, pair_cluster=many['pair_cluster'][:1], center3=many['center3'][:1], rot4=many['rot4'][:1])))
    cases.append(('pairs0', dict(many, pair_cluster=many['pair_cluster'][:0], center3=many['center3'][:0], rot4=many['rot4'][:0])))
    cases.append(('identity', dict(many, pair_cluster=None, center3=np.array(meds, np.float32), rot4=many['rot4'][:40])))
    out_of_range = many['pair_cluster'][:6].copy()
    out_of_range[1], out_of_range[4] = 40, -1
    cases.append(('out_of_range', dict(many, pair_cluster=out_of_range, center3=many['center3'][:6], rot4=many['rot4'][:6])))
    # ---- geometry: projections all negative, all positive, straddling zero (the centre need not be the median); identical points ----
    rng = np.random.default_rng(2027)
    sc, pc, c3, ang = _Scene(rng), [], [], []
    for j, origin in enumerate(ORIGINS):
        xyz = (rng.uniform(-2, 2, (70, 3)) + origin).astype(np.float32)
        c = sc.add(xyz)
        same = sc.add(np.tile(xyz[:1], (70, 1)))
        for shift in (0.0, 20.0, -20.0):
            for a in (FIXED_ANGLES[j], np.float32(rng.uniform(-np.pi, np.pi))):
                cs, sn = np.cos(float(a)), np.sin(float(a))
                off = np.array([shift * (cs - sn), shift * (sn + cs), 0.0])            # the centre at x' = y' = shift: everything on one side of it
                pc.append(c); c3.append((np.median(xyz, axis=0) + off).astype(np.float32)); ang.append(a)
        pc.append(same); c3.append(xyz[0]); ang.append(FIXED_ANGLES[j])
        pc.append(same); c3.append(xyz[0] + np.float32(0.5)); ang.append(np.float32(rng.uniform(-np.pi, np.pi)))
    cases.append(('geometry', sc.finish(pc, c3, rot4_of_angles(ang))))
    # ---- non-finite input: a NaN in one point, an infinite coordinate, a NaN in one centre; the clusters around them are untouched ----
    rng = np.random.default_rng(2028)
    sc, pc, c3, ang = _Scene(rng), [], [], []
    for j in range(6):
        xyz = (rng.uniform(-2, 2, (B + 40, 3)) + ORIGINS[j % 4]).astype(np.float32)
        med = np.median(xyz, axis=0)
        if j == 1:
            xyz[B + 7, 1] = np.nan
        if j == 3:
            xyz[5, 2] = np.inf
        if j == 4:
            xyz[B - 1, 0] = -np.inf
        c = sc.add(xyz)
        for rep in range(2):
            pc.append(c); c3.append(med.copy()); ang.append(np.float32(rng.uniform(-np.pi, np.pi)))
    c3[10][1] = np.nan                                                                 # cluster 5, first of its two pairs
    cases.append(('nonfinite', sc.finish(pc, c3, rot4_of_angles(ang))))
    return cases


def with_stride(case, stride):
    """the same case over point rows of `stride` floats (3: x, y, z alone; 5: as built)"""
    return dict(case, points=np.ascontiguousarray(case['points'][:, :stride]))


def seeded_tracks():
    """The 200 seeded tracks of tests/test_tracking.py::test_array_form_of_the_track_boxes_equals_the_line_by_line_form (the same
    generator, the same draws in the same order) that have motion vectors -> (trial, directions, points per entry, to_ego per entry)."""
    from oracle import tracking_oracle as to
    from vilgod_amd import synthetic
    rng = np.random.default_rng(0)
    for trial in range(200):
        n = int(rng.integers(1, 40))
        speed = rng.choice([0.0, 0.02, 0.2, 0.6, 1.5])
        head = rng.uniform(0, 6.28)
        c = np.cumsum(np.c_[np.cos(head + rng.normal(0, 0.3, n)), np.sin(head + rng.normal(0, 0.3, n))] * speed * rng.uniform(0.5, 1.5, (n, 1)), axis=0)
        c = (c + rng.normal(0, 0.05, (n, 2)) + rng.uniform(-50, 50, 2)).astype(np.float32)
        a = to.motion_vectors(c)
        if not a:
            continue
        pts = [(rng.normal(size=(int(rng.integers(12, 300)), 5)) * [1.5, 0.7, 0.6, 1, 1] + [c[i, 0], c[i, 1], 0.8, 0, 0]).astype(np.float32) for i in range(n)]
        T = [np.linalg.inv(p) for p in synthetic.make_poses(n, seed=trial)]
        yield trial, a, pts, T
