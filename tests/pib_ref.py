"""Shared by tests/test_points_in_boxes_host.py and tests/test_points_in_boxes_device.py: the fixture of
tests/golden/make_points_in_boxes.py, the batched host entry point through ctypes, and the seeded scenes of the launch-edge tests.
TEST INFRASTRUCTURE ONLY: nothing here decides whether a point is inside a box."""
import ctypes
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FAMILIES = ('A32', 'A64', 'B32', 'B64', 'C32', 'C64', 'D32', 'D64')


def fixture():
    g = np.load(os.path.join(GOLDEN, 'points_in_boxes_golden.npz'))
    return {k: g[k] for k in g.files}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


def host_batched(points, boxes, cols=None):
    """vg_points_in_boxes_host on points [B, N, C] float32 (row stride C) and boxes [B, M, 7] float32 / float64 -> [B, N] int32"""
    from vilgod_amd._lib import lib, check
    points = np.ascontiguousarray(points, np.float32)
    boxes = np.ascontiguousarray(boxes[:, :, :7])
    assert boxes.dtype in (np.float32, np.float64)
    B, N, C = points.shape
    out = np.full((B, N), -9, np.int32)
    check(lib.vg_points_in_boxes_host(0 if boxes.dtype == np.float32 else 1, _p(points), C, N, _p(boxes), boxes.shape[1], B, _p(out)),
          'vg_points_in_boxes_host')
    return out


def scene(n_points, n_boxes, batch, seed, point_cols=3, box_cols=7, dtype=np.float32):
    """Seeded points in a square that grows with the number of boxes, boxes (1.5 .. 5 m, any heading) centred on points drawn from them:
    -> points [B, N, point_cols] float32, boxes [B, M, box_cols]; every batch element has its own points and boxes.  The columns beyond
    3 / 7 hold 1e6, which a kernel that read them would notice."""
    rng = np.random.default_rng(seed)
    half = 1.5 * np.sqrt(max(n_boxes, 1))
    points = np.full((batch, n_points, point_cols), 1e6, np.float32)
    boxes = np.full((batch, n_boxes, box_cols), 1e6, dtype)
    for b in range(batch):
        xyz = np.c_[rng.uniform(-half, half, (n_points, 2)), rng.uniform(-0.5, 0.5, n_points)]
        points[b, :, :3] = xyz
        if n_boxes and n_points:
            at = xyz[rng.integers(0, n_points, n_boxes)]
            boxes[b, :, :3] = at + rng.normal(0, 0.2, (n_boxes, 3))
            boxes[b, :, 3:5] = rng.uniform(1.5, 5.0, (n_boxes, 2))
            boxes[b, :, 5] = rng.uniform(1.0, 3.0, n_boxes)
            boxes[b, :, 6] = rng.uniform(-np.pi, np.pi, n_boxes)
    return points, boxes


def far_boxes(m, dtype=np.float64):
    """m sound boxes a long way from the origin and from each other"""
    b = np.zeros((m, 7), dtype)
    b[:, 0] = 1000.0 + 10.0 * np.arange(m)
    b[:, 3:6] = 2.0
    b[:, 6] = 0.1 * np.arange(m)
    return b
