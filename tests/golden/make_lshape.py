"""Generates tests/golden/lshape_golden.npz: the reference's closeness_rectangle and variance_rectangle
(src/utils/pointcloud_utils.py:170-288) and its box assembly (src/vilgod/zero_shot_detector.py:452-461) on 64 seeded clusters.
Run only in the build container:

    python tests/golden/make_lshape.py

The reference's module is imported with the stand-ins of oracle/refstubs.py.  numba is not installed there: `numba.jit` is an
identity decorator, so this runs the reference's function bodies as plain numpy (closeness then accumulates 1 / beta in float32,
where numba would use float64: tests/lshape_ref.py).  The functions return only the chosen angle; the criterion of every angle
is read from the running function by a line tracer on its `if beta > max_beta:` / `if var > max_var:` line.
The fixture holds data only: the clusters and the reference's outputs.
"""
import inspect
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import refstubs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def _q(a, step=1e-3):
    """coordinates on a 1 mm grid (LiDAR precision; keeps the fixture small), float32"""
    return (np.round(np.asarray(a, np.float64) / step) * step).astype(np.float32)


def _rect_outline(rng, n, length, width, yaw, centre, sides=(0, 1, 2, 3), noise=0.02):
    """n points on the chosen sides of a length x width rectangle (side k: 0 +x, 1 +y, 2 -x, 3 -y), rotated by yaw"""
    pts = []
    per = np.array_split(np.arange(n), len(sides))
    for k, idx in zip(sides, per):
        t = rng.uniform(-0.5, 0.5, len(idx))
        if k in (0, 2):
            p = np.stack([np.full_like(t, (0.5 if k == 0 else -0.5) * length), t * width], 1)
        else:
            p = np.stack([t * length, np.full_like(t, (0.5 if k == 1 else -0.5) * width)], 1)
        pts.append(p)
    p = np.concatenate(pts) + rng.normal(0, noise, (n, 2))
    c, s = np.cos(yaw), np.sin(yaw)
    return p @ np.array([[c, s], [-s, c]]) + centre


def clusters(seed=2026):
    rng = np.random.default_rng(seed)
    out = []

    def add(kind, xy, z0=None, h=None):
        z0 = rng.uniform(-1.0, 0.5) if z0 is None else z0
        h = rng.uniform(0.3, 2.0) if h is None else h
        z = z0 + rng.uniform(0, h, len(xy))
        out.append((kind, np.concatenate([_q(xy), _q(z, 1e-2)[:, None]], 1)))

    for _ in range(18):                                            # cars: the two sides facing the sensor, noisy, partly occluded
        n = int(rng.integers(40, 400))
        yaw = rng.uniform(-np.pi, np.pi)
        centre = rng.uniform(-40, 40, 2)
        xy = _rect_outline(rng, n, rng.uniform(3.8, 5.2), rng.uniform(1.6, 2.1), yaw, centre, sides=(0, 1))
        keep = rng.uniform(size=n) > 0.2 * (np.abs(xy[:, 0] - centre[0]) < 0.5)   # an occluding pole's shadow
        add('car', xy[keep])
    for _ in range(8):                                             # pedestrians
        add('pedestrian', rng.normal(0, 0.2, (int(rng.integers(15, 80)), 2)) + rng.uniform(-30, 30, 2))
    for _ in range(6):                                             # thin walls
        n = int(rng.integers(150, 600))
        t = rng.uniform(-0.5, 0.5, n) * rng.uniform(8, 25)
        yaw = rng.uniform(-np.pi, np.pi)
        p = np.stack([t, rng.normal(0, 0.03, n)], 1)
        add('wall', p @ np.array([[np.cos(yaw), np.sin(yaw)], [-np.sin(yaw), np.cos(yaw)]]) + rng.uniform(-40, 40, 2))
    for k in range(4):                                             # axis-aligned rectangles (0 and 90 degrees tie)
        add('axis_rect', _rect_outline(rng, 80, 4.0 + k, 4.0 + k if k % 2 == 0 else 2.0, 0.0, rng.uniform(-20, 20, 2), noise=0.0))
    for k in range(4):                                             # exactly 45 degrees
        add('rect_45', _rect_outline(rng, 80, 4.0, 2.0 + k * 0.5, np.pi / 4, rng.uniform(-20, 20, 2), noise=0.0))
    add('one_point', rng.uniform(-10, 10, (1, 2)))
    add('two_points', rng.uniform(-10, 10, (2, 2)))
    t = rng.uniform(0, 1, 30)
    add('collinear_x', np.stack([t * 5 + 3, np.full(30, 2.5)], 1))
    add('collinear_diag', np.stack([t * 3, t * 3], 1) + 7.0)
    add('collinear_skew', np.stack([t * 4, t * 1.3], 1) - 5.0)
    base = rng.normal(0, 0.5, (25, 2)) + 12.0
    add('duplicated', np.concatenate([base, base, base[:7]]))
    add('same_point', np.repeat(rng.uniform(-5, 5, (1, 2)), 12, axis=0))
    # one cluster of 20 000 points: a building corner (two long walls) with clutter
    n = 20000
    a = _rect_outline(rng, 16000, 30.0, 12.0, 0.37, np.array([25.0, -18.0]), sides=(0, 1), noise=0.03)
    b = rng.normal(0, 1.5, (n - 16000, 2)) + np.array([25.0, -18.0])
    add('wall_20k', np.concatenate([a, b]), z0=-0.5, h=3.0)
    while len(out) < 64:                                           # mixed: random outlines of any aspect, 2-4 sides
        n = int(rng.integers(10, 250))
        sides = tuple(sorted(rng.choice(4, int(rng.integers(1, 5)), replace=False)))
        add('mixed', _rect_outline(rng, n, rng.uniform(0.5, 8), rng.uniform(0.3, 4), rng.uniform(-np.pi, np.pi),
                                   rng.uniform(-40, 40, 2), sides=sides, noise=rng.uniform(0, 0.1)))
    return out


def _criteria_by_trace(fn, marker, var, *call_args, **call_kw):
    """Run fn and record local `var` each time the line containing `marker` runs (the reference computes every criterion and keeps
    only the best one)."""
    code = inspect.unwrap(fn).__code__
    lines, first = inspect.getsourcelines(inspect.unwrap(fn))
    target = first + next(i for i, l in enumerate(lines) if marker in l)
    seen = []

    def local(frame, event, arg):
        if event == 'line' and frame.f_lineno == target:
            seen.append(float(frame.f_locals[var]))
        return local

    def glob(frame, event, arg):
        return local if frame.f_code is code else None
    sys.settrace(glob)
    try:
        res = fn(*call_args, **call_kw)
    finally:
        sys.settrace(None)
    return res, np.array(seen)


def make():
    refstubs.install()
    from src.utils import pointcloud_utils as pu
    cl = clusters()
    pts = np.concatenate([p for _, p in cl]).astype(np.float32)
    seg = np.r_[0, np.cumsum([len(p) for _, p in cl])].astype(np.int64)
    out = dict(points=pts, seg=seg, kind=np.array([k for k, _ in cl]))
    for name, traced, marker, var in (('closeness_rectangle', pu.check_all_angles, 'if beta > max_beta', 'beta'),
                                      ('variance_rectangle', pu.variance_rectangle, 'if var > max_var', 'var')):
        idx, ang, corners, boxes, crits = [], [], [], [], []
        for _, p in cl:
            cluster_points = p
            if name == 'closeness_rectangle':
                _, crit = _criteria_by_trace(traced, marker, var, cluster_points[:, :2], 2, 1e-2)
            else:
                _, crit = _criteria_by_trace(traced, marker, var, cluster_points[:, :2])
            corners_, rz, area = getattr(pu, name)(cluster_points[:, :2])
            # zero_shot_detector.py:452-460, as written there
            l = np.linalg.norm(corners_[0] - corners_[1])
            w = np.linalg.norm(corners_[0] - corners_[-1])
            c = (corners_[0] + corners_[2]) / 2
            rz0 = rz
            if w > l:
                l, w = w, l
                rz += np.pi / 2
            height = cluster_points[:, 2].max() - cluster_points[:, 2].min()
            box = np.array([c[0], c[1], cluster_points[:, 2].min() + height / 2, l, w, height + 0.3, rz])
            k = int(np.flatnonzero(crit == crit.max())[0])
            idx.append(k)
            ang.append(rz0)
            corners.append(np.asarray(corners_, np.float64))
            boxes.append(box)
            crits.append(crit)
        key = name.split('_')[0]
        out[f'{key}_index'] = np.array(idx)
        out[f'{key}_angle'] = np.array(ang)
        out[f'{key}_corners'] = np.array(corners)
        out[f'{key}_box'] = np.array(boxes)
        out[f'{key}_crit'] = np.array(crits)
    path = os.path.join(OUT, 'lshape_golden.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(cl), 'clusters,', len(pts), 'points')


if __name__ == '__main__':
    make()
