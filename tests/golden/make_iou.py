"""Generates tests/golden/iou_golden.npz: rotated-box pairs and their IoU from 60-digit arithmetic, for tests/test_iou_host.py and
tests/test_iou_device.py (csrc/iou.hip, csrc/iou_pair.inc).  Needs mpmath; the tests only read the file.

    python tests/golden/make_iou.py

Reference value of a pair: the eight corners from the float64 box parameters [x, y, z, dx, dy, dz, heading] in mpmath at 60
digits (the parameters are exact inputs: a heading of float64(2 pi) means that number, not 2 pi), A's rectangle clipped by B's four
edges (Sutherland-Hodgman, closed tests) and the shoelace area in the same precision, rounded to float64 at the end:
    mode 0  3-D IoU   area * z overlap / (vol_a + vol_b - that), 0 for an extent <= 0 or no z overlap
    mode 1  BEV IoU   area / (area_a + area_b - area), 0 for dx or dy <= 0 (z and dz are not read)
    mode 2  area
Stored per pair: a, b [P,7]; ref [P,3]; n_vert [P] distinct vertices of the BEV intersection; family [P] (0..4 = A..E); twin [P]
(family C: index of the origin-centred pair it was translated from, else -1).  e_host [5]: per family max |iou3d_matrix - ref|
(mode 0) of the host function vilgod_amd.evaluation.iou3d_matrix, the bar's yardstick; family C stores the value of its twins.

Families
  A  closed forms and exact zeros: the five geometries of test_evaluation.py::test_iou_of_the_golden_geometry, identical boxes on a
     yaw grid, containment, zeros with integer coordinates and yaw 0 (touching along an edge, at a corner, in z), disjoint boxes (beyond
     the half-diagonals, and inside them), a zero or negative extent
  B  near-parallel and wrapped headings: yaw differences +-1e-1 .. 1e-16, +-1 and +-2 ulp of yaw, yaw + pi/2, pi, 2 pi, -7 pi, negative
     headings; on boxes that share a centre and on offset ones
  C  all of B and the first 300 of E translated to centres (1000.3, -999.7), (-480, 510), (140, -90)
  D  intersections with 3, 4, 5, 6, 7 and 8 vertices (asserted: every count occurs)
  E  2000 seeded random pairs, extents 0.01 .. 20 (aspect up to 2000 : 1), centres within reach (asserted: at least half intersect)
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 60
FAMILIES = 'ABCDE'
CENTRES = ((1000.3, -999.7), (-480.0, 510.0), (140.0, -90.0))


# ---- the reference -------------------------------------------------------------------------------------------------------------
def _corners(b):
    x, y, dx, dy, h = (mp.mpf(float(b[k])) for k in (0, 1, 3, 4, 6))
    c, s = mp.cos(h), mp.sin(h)
    return [(x + lx * c - ly * s, y + lx * s + ly * c) for lx, ly in ((dx / 2, dy / 2), (-dx / 2, dy / 2), (-dx / 2, -dy / 2), (dx / 2, -dy / 2))]


def _clip(poly, p0, p1):
    """the part of the convex polygon on the left of p0 -> p1 (closed)"""
    ex, ey = p1[0] - p0[0], p1[1] - p0[1]
    side = [ex * (v[1] - p0[1]) - ey * (v[0] - p0[0]) for v in poly]
    out = []
    for i, v in enumerate(poly):
        j = (i + 1) % len(poly)
        if side[i] >= 0:
            out.append(v)
        if (side[i] >= 0) != (side[j] >= 0):
            t = side[i] / (side[i] - side[j])
            out.append((v[0] + t * (poly[j][0] - v[0]), v[1] + t * (poly[j][1] - v[1])))
    return out


def _distinct(poly, tol=mp.mpf(10) ** -40):
    out = []
    for v in poly:
        if not any(abs(v[0] - u[0]) <= tol and abs(v[1] - u[1]) <= tol for u in out):
            out.append(v)
    return out


def reference(a, b):
    """-> ([3-D IoU, BEV IoU, BEV area] float64, distinct vertices of the BEV intersection)"""
    if not (a[3] > 0 and a[4] > 0 and b[3] > 0 and b[4] > 0):
        return [0.0, 0.0, 0.0], 0
    poly = _corners(a)
    cb = _corners(b)
    for k in range(4):
        if len(poly) < 3:
            break
        poly = _clip(poly, cb[k], cb[(k + 1) % 4])
    poly = _distinct(poly)
    area = mp.mpf(0)
    if len(poly) >= 3:
        area = abs(sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1] for i in range(len(poly)))) / 2
    n_vert = len(poly) if area > 0 else 0
    A = [mp.mpf(float(v)) for v in a]
    B = [mp.mpf(float(v)) for v in b]
    fa, fb = A[3] * A[4], B[3] * B[4]
    bev = area / (fa + fb - area) if fa + fb - area > 0 else mp.mpf(0)
    iou = mp.mpf(0)
    if a[5] > 0 and b[5] > 0:
        zov = min(A[2] + A[5] / 2, B[2] + B[5] / 2) - max(A[2] - A[5] / 2, B[2] - B[5] / 2)
        if zov > 0:
            inter = area * zov
            uni = fa * A[5] + fb * B[5] - inter
            iou = inter / uni if uni > 0 else mp.mpf(0)
    return [float(iou), float(bev), float(area)], n_vert


# ---- the pairs -----------------------------------------------------------------------------------------------------------------
def box(x=0.0, y=0.0, z=0.0, dx=4.0, dy=2.0, dz=1.5, yaw=0.0):
    return np.array([x, y, z, dx, dy, dz, yaw], np.float64)


def family_a():
    pairs = []
    # the five geometries of test_iou_of_the_golden_geometry
    pairs += [(box(1.70), box()), (box(1.73), box()), (box(2.1, dx=6.0), box()), (box(2.1, dx=6.0), box(4.0)),
              (box(dx=1, dy=1, yaw=0.3), box(dx=1, dy=1))]
    for k in range(-16, 17):                                        # identical boxes
        b = box(3.7, -1.2, 0.4, 4.3, 1.9, 1.6, k * np.pi / 16)
        pairs.append((b, b.copy()))
    for k in range(12):                                             # containment, either way round
        big = box(0.5, -0.25, 0.1, 8.0, 6.0, 3.0, 0.37 * k)
        small = box(0.9, 0.1, 0.2, 1.7, 0.9, 1.1, -0.81 * k + 0.2)
        pairs.append((small, big) if k % 2 else (big, small))
    # exact zeros: integer coordinates, yaw 0 -- touching along an edge, at a corner, in z
    u = box(0, 0, 0, 2, 2, 2, 0)
    for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        pairs += [(u, box(2 * sx, 2 * sy, 0, 2, 2, 2, 0)), (box(3 * sx, 3 * sy, 1, 4, 4, 2, 0), u), (u, box(4 * sx + sy, 4 * sy + sx, 0, 6, 6, 4, 0))]
    for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
        pairs += [(u, box(2 * sx, 2 * sy, 0, 2, 2, 2, 0)), (box(3 * sx, 2 * sy, 0, 4, 2, 2, 0), u)]
    pairs += [(u, box(0, 0, 2, 2, 2, 2, 0)), (u, box(1, 0, -2, 2, 2, 2, 0)), (box(0, 1, 3, 2, 2, 4, 0), u)]
    # disjoint: beyond the half-diagonals, and within them
    pairs += [(box(0, 0, 0), box(30, 0, 0)), (box(0, 0, 0), box(0, -7, 0, yaw=1.0)), (box(-200.5, 300.25, 0), box(200, -300, 0, yaw=2.0)),
              (box(0, 0, 0, 10, 0.5, 1.5, 0.0), box(0, 1.0, 0, 10, 0.5, 1.5, 0.01)), (box(0, 0, 0, 6, 1, 1.5, 0.6), box(2.5, -2.5, 0, 6, 1, 1.5, 0.6)),
              (box(0, 0, 0, 4, 4, 1, 0.0), box(3.6, 3.6, 0, 2, 2, 1, np.pi / 4)), (box(0, 0, 0), box(0.5, 0.2, 5.0, yaw=0.3))]
    # a zero or negative extent (both ways round)
    for k, v in ((3, 0.0), (4, 0.0), (5, 0.0), (5, -1.5), (3, -4.0), (4, -2.0)):
        d = box(0.3, 0.1, 0.0, yaw=0.2)
        d[k] = v
        pairs += [(d, box(yaw=-0.1)), (box(yaw=-0.1), d)]
    return pairs


def family_b():
    pairs = []
    shapes = [(box(0, 0, 0, 4.2, 1.8, 1.5), box(0, 0, 0, 4.2, 1.8, 1.5)),                    # same centre and size: every edge nearly shared
              (box(0.3, -0.2, 0.1, 4.2, 1.8, 1.5), box(0.9, 0.3, 0.0, 3.9, 2.1, 1.7)),
              (box(0, 0, 0, 12.0, 0.4, 2.0), box(1.5, 0.05, 0.3, 9.0, 0.6, 1.0))]
    yaws = (0.0, 0.7, -2.1, float(np.pi / 2), -0.3)
    for si, (a0, b0) in enumerate(shapes):
        for yi, yaw in enumerate(yaws):
            if (si + yi) % 2 and si:                                  # thin the offset shapes
                continue
            deltas = [sg * 10.0 ** -k for k in range(1, 17) for sg in (1, -1)]
            for d in deltas:
                a, b = a0.copy(), b0.copy()
                a[6], b[6] = yaw, yaw + d
                pairs.append((a, b))
            for steps in (1, 2, -1, -2):                              # +-1, +-2 ulp
                y2 = yaw
                for _ in range(abs(steps)):
                    y2 = np.nextafter(y2, np.inf * np.sign(steps))
                a, b = a0.copy(), b0.copy()
                a[6], b[6] = yaw, y2
                pairs.append((a, b))
            for wrap in (np.pi / 2, np.pi, 2 * np.pi, -7 * np.pi):
                a, b = a0.copy(), b0.copy()
                a[6], b[6] = yaw, yaw + wrap
                pairs += [(a, b), (b.copy(), a.copy())]
    return pairs


def family_d(rng):
    sq = box(0, 0, 0, 2, 2, 1, 0)
    pairs = [(sq, box(0, 0, 0, 2, 2, 1, np.pi / 4)), (box(0.3, -0.2, 0, 3, 3, 1, 0.2), box(0.3, -0.2, 0.1, 3, 3, 2, 0.2 + np.pi / 4))]
    want = {n: 12 for n in range(3, 9)}
    want[8] -= 2
    while any(want.values()):
        a = box(*rng.uniform(-1, 1, 3), *rng.uniform(1.0, 4.0, 2), rng.uniform(1, 2), rng.uniform(-np.pi, np.pi))
        b = box(*rng.uniform(-1.5, 1.5, 2), rng.uniform(-0.5, 0.5), *rng.uniform(1.0, 4.0, 2), rng.uniform(1, 2), rng.uniform(-np.pi, np.pi))
        if rng.random() < 0.3:                                        # near-equal squares near 45 degrees: 7 and 8 vertices
            s = rng.uniform(1.5, 3.0)
            a[3:5] = s
            b[3:5] = s * rng.uniform(0.9, 1.1, 2)
            b[:2] = a[:2] + rng.uniform(-0.15, 0.15, 2)
            b[6] = a[6] + np.pi / 4 + rng.uniform(-0.2, 0.2)
        _, n = reference(a, b)
        if want.get(n, 0) > 0:
            want[n] -= 1
            pairs.append((a, b))
    return pairs


def family_e(rng, n=2000):
    pairs = []
    for i in range(n):
        ea, eb = np.exp(rng.uniform(np.log(0.01), np.log(20.0), 2)), np.exp(rng.uniform(np.log(0.01), np.log(20.0), 2))
        ha, hb = np.exp(rng.uniform(np.log(0.1), np.log(5.0), 2))
        ca = rng.uniform(-60, 60, 2)
        reach = 0.5 * (np.hypot(*ea) + np.hypot(*eb))
        r, phi = reach * 0.55 * np.sqrt(rng.random()), rng.uniform(0, 2 * np.pi)
        span = np.pi if i % 5 else 4 * np.pi
        a = box(ca[0], ca[1], rng.uniform(-2, 2), ea[0], ea[1], ha, rng.uniform(-span, span))
        b = box(ca[0] + r * np.cos(phi), ca[1] + r * np.sin(phi), a[2] + rng.uniform(-0.4, 0.4) * (ha + hb), eb[0], eb[1], hb, rng.uniform(-span, span))
        pairs.append((a, b))
    return pairs


def main():
    from vilgod_amd.evaluation import iou3d_matrix
    rng = np.random.default_rng(20260)
    fam = {'A': family_a(), 'B': family_b(), 'D': family_d(rng), 'E': family_e(rng)}
    a_rows, b_rows, family, twin = [], [], [], []
    start = {}
    for f in 'ABDE':
        start[f] = len(a_rows)
        for a, b in fam[f]:
            a_rows.append(a); b_rows.append(b); family.append(FAMILIES.index(f)); twin.append(-1)
    origin = [start['B'] + i for i in range(len(fam['B']))] + [start['E'] + i for i in range(300)]
    for cx, cy in CENTRES:
        for i in origin:
            a, b = a_rows[i].copy(), b_rows[i].copy()
            a[0] += cx; a[1] += cy; b[0] += cx; b[1] += cy
            a_rows.append(a); b_rows.append(b); family.append(FAMILIES.index('C')); twin.append(i)
    a_rows, b_rows, family, twin = np.array(a_rows), np.array(b_rows), np.array(family, np.int32), np.array(twin, np.int64)
    ref = np.zeros((len(a_rows), 3))
    n_vert = np.zeros(len(a_rows), np.int32)
    host = np.zeros(len(a_rows))
    for i in range(len(a_rows)):
        ref[i], n_vert[i] = reference(a_rows[i], b_rows[i])
        host[i] = iou3d_matrix(a_rows[i][None], b_rows[i][None])[0, 0]
    fD = family == FAMILIES.index('D')
    assert set(n_vert[fD].tolist()) >= {3, 4, 5, 6, 7, 8}, sorted(set(n_vert[fD].tolist()))
    fE = family == FAMILIES.index('E')
    share = np.mean(ref[fE, 2] > 0)
    assert share >= 0.5, share
    err = np.abs(host - ref[:, 0])
    e_host = np.zeros(5)
    for k, f in enumerate(FAMILIES):
        sel = family == k
        e_host[k] = err[twin[sel]].max() if f == 'C' else err[sel].max()
        print(f'family {f}: {int(sel.sum()):5d} pairs, host error {err[sel].max():.3e}, stored E_host {e_host[k]:.3e}, '
              f'intersecting {np.mean(ref[sel, 2] > 0):.2f}')
    np.savez_compressed(os.path.join(OUT, 'iou_golden.npz'), a=a_rows, b=b_rows, ref=ref, n_vert=n_vert, family=family, twin=twin, e_host=e_host)
    print('pairs', len(a_rows), 'E share intersecting', share)


if __name__ == '__main__':
    main()
