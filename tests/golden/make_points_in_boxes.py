"""Generates tests/golden/points_in_boxes_golden.npz: float32 points, boxes and the index of the box that owns each point from 60-digit
arithmetic, for tests/test_points_in_boxes_host.py and tests/test_points_in_boxes_device.py (csrc/points_in_boxes.hip,
csrc/points_in_boxes_pair.inc).  Needs mpmath, and for family E the reference checkout (stub-imported, oracle/refstubs.py); the tests
only read the file.

    python tests/golden/make_points_in_boxes.py

The rule (include/vilgod_hip.h vg_points_in_boxes), evaluated on the STORED values -- float32 points, boxes in their family's dtype,
each widened exactly: the point (x, y, z) is inside the box {cx, cy, cz, dx, dy, dz, rz} iff
    |z - cz| <= dz / 2,   |lx| < dx / 2 + 1e-5,   |ly| < dy / 2 + 1e-5,
    lx = sx cos(rz) + sy sin(rz),  ly = -sx sin(rz) + sy cos(rz),  (sx, sy) = (x - cx, y - cy)
and no value is NaN, dx, dy, dz >= 0 and |rz| < 1.6e6.  The halves dx / 2 + 1e-5, dy / 2 + 1e-5, dz / 2 are the FLOAT64 values of these
expressions; the differences, the sine / cosine, the rotation and the comparisons are exact (mpmath, 60 digits).  A point's index is the
lowest index of a box that contains it, -1 for none.

Every family is a batch: `<F>_points` [S, N, 3] float32, `<F>_boxes` [S, M, 7], `<F>_expect` [S, N] int32 -- set s pairs its own points
with its own boxes, which is also the batched layout of the entry points.  The suffix 32 / 64 is the boxes' dtype.

  A32 A64  heading exactly 0, one box per set, centres (0,0,0), (140,-90,3), (-480,510,-20): points ON every face and 1 and 2 float32
           steps on either side of it.  x / y: the face is +-(dx / 2 + 1e-5); in A64 dx, dy are chosen so that this float64 value is a
           multiple of 2^-14, i.e. a float32 offset from the integer centres (the equality case exists); in A32 the face is no
           float32 value and the points are its float32 neighbours.  z: +-dz / 2 with dz = 1.5 (the inclusive equality exists in both).
           The kernel's arithmetic is exact here (cos = 1, sin = 0, the differences are exact), so EVERY point must match.
  B32 B64  rotated boxes, one per set: headings in all four quadrants, +-pi/2 and +-pi as float32 / float64 values, and 1000; points
           1 .. 4 float32 steps either side of each face (three places along it) and each corner, at half height and on the z faces.
           Tie zone: no point lies within 8 x TIE_UNITS x 2^-53 x (|sx| + |sy|) of an x / y face (tests/test_points_in_boxes_host.py
           derives the bound); asserted below, the smallest distance / bound ratio is stored as `B_min_clearance`.
  C32 C64  overlapping boxes: points inside two and three boxes (the lowest index wins), set 1 = set 0 with the boxes reversed.
  D32 D64  degenerate boxes side by side: extents of 0 (only the margin / only the plane z = cz contains anything), negative extents
           (-1, -1e-6), NaN in every column of a box, |rz| = 2e6, and NaN in each coordinate of a point inside a sound box.
           (n_boxes = 0 needs no fixture: every index is -1.)
  E        the reference's own LidarFrame.generate_detections(None, proposals=..., names=...) and pointcloud_utils.get_box_heights on a
           seeded 2 000-point frame with 8 proposals (its annotation boxes, two overlapping, one empty), with the rule above installed
           as roiaware_pool3d_utils.points_in_boxes_gpu: E_points, E_pose, E_ref_pose, E_proposals, E_names, per detection
           E_cluster_id / E_index + E_seg / E_box / E_object_class, and E_heights.
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 60
CENTRES = ((0.0, 0.0, 0.0), (140.0, -90.0, 3.0), (-480.0, 510.0, -20.0))
TIE_UNITS = 6          # roundings of 2^-53 (|sx| + |sy|) in the kernel's lx, ly (tests/test_points_in_boxes_host.py)
TIE_MARGIN = 8


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def inside(p, b):
    """-> (inside?, smallest |distance| of lx / ly to their faces relative to the tie bound, or inf where the rule needs no rotation)"""
    p = [float(v) for v in p]
    b = [float(v) for v in b]
    if any(np.isnan(p)) or any(np.isnan(b)):
        return False, np.inf
    if not (b[3] >= 0 and b[4] >= 0 and b[5] >= 0 and abs(b[6]) < 1.6e6):
        return False, np.inf
    hx, hy, hz = b[3] / 2 + 1e-5, b[4] / 2 + 1e-5, b[5] / 2              # float64 arithmetic: the rule's face values
    x, y, z, cx, cy, cz, rz = (mp.mpf(v) for v in (p[0], p[1], p[2], b[0], b[1], b[2], b[6]))
    sx, sy = x - cx, y - cy
    c, s = mp.cos(rz), mp.sin(rz)
    lx, ly = sx * c + sy * s, -sx * s + sy * c
    bound = TIE_MARGIN * TIE_UNITS * mp.mpf(2) ** -53 * (abs(sx) + abs(sy))
    gap = min(abs(abs(lx) - mp.mpf(hx)), abs(abs(ly) - mp.mpf(hy)))
    clear = float(gap / bound) if bound > 0 else np.inf
    return bool(abs(z - cz) <= mp.mpf(hz) and abs(lx) < mp.mpf(hx) and abs(ly) < mp.mpf(hy)), clear


def owners(points, boxes):
    """[N, 3] x [M, 7] -> (expect [N] int32, smallest clearance over all pairs)"""
    out = np.full(len(points), -1, np.int32)
    clear = np.inf
    for i, p in enumerate(points):
        for j, b in enumerate(boxes):
            hit, c = inside(p, b)
            clear = min(clear, c)
            if hit and out[i] < 0:
                out[i] = j
    return out, clear


# ---- the points ----------------------------------------------------------------------------------------------------------------
def step32(v, n):
    v = np.float32(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, np.float32(np.inf if n > 0 else -np.inf))
    return v


def half_on_grid(target):
    """a float64 extent d with fl(d / 2 + 1e-5) == target exactly (target a multiple of 2^-14)"""
    d = 2.0 * (target - 1e-5)
    for _ in range(64):
        h = d / 2 + 1e-5
        if h == target:
            return d
        d = np.nextafter(d, np.inf if h < target else -np.inf)
    raise AssertionError(target)


def family_a(dtype):
    sets = []
    for k, (cx, cy, cz) in enumerate(CENTRES):
        if dtype == np.float64:
            hx, hy = round(2.10001 * 2 ** 14) / 2 ** 14, round(0.95001 * 2 ** 14) / 2 ** 14
            dx, dy = half_on_grid(hx), half_on_grid(hy)
        else:
            dx, dy = 4.2, 1.9
        box = np.array([cx, cy, cz, dx, dy, 1.5, 0.0], dtype)
        hx, hy = float(box[3]) / 2 + 1e-5, float(box[4]) / 2 + 1e-5
        pts = []
        for sg in (1, -1):
            for n in (-2, -1, 0, 1, 2):
                for along in (0.0, 0.4, -0.7):
                    pts.append((step32(cx + sg * hx, n), np.float32(cy + along * hy), np.float32(cz + 0.25)))      # x faces
                    pts.append((np.float32(cx + along * hx), step32(cy + sg * hy, n), np.float32(cz - 0.5)))       # y faces
                    pts.append((np.float32(cx + along * hx), np.float32(cy - along * hy), step32(cz + sg * 0.75, n)))   # z faces
                pts.append((step32(cx + sg * hx, n), step32(cy - sg * hy, n), step32(cz + sg * 0.75, 0)))           # a corner, on the z face
        sets.append((np.array(pts, np.float32), box[None]))
    return sets


def headings(dtype):
    quad = [0.3, 1.2, 2.0, 2.9, -0.4, -1.3, -2.2, -3.0]
    special = [np.pi / 2, -np.pi / 2, np.pi, -np.pi]
    return [float(dtype(v)) for v in quad + special] + [1000.0]


def family_b(dtype):
    sets = []
    for k, rz in enumerate(headings(dtype)):
        cx, cy, cz = CENTRES[k % 3]
        box = np.array([cx, cy, cz, 4.2 + 0.1 * k, 1.9, 1.6, rz], dtype)
        b = [float(v) for v in box]
        hx, hy, hz = b[3] / 2 + 1e-5, b[4] / 2 + 1e-5, b[5] / 2
        c, s = np.cos(b[6]), np.sin(b[6])

        def world(lx, ly):
            return cx + lx * c - ly * s, cy + lx * s + ly * c

        pts = []
        zs = (cz, cz + hz, cz - hz)
        for n in (-4, -3, -2, -1, 1, 2, 3, 4):
            for sg in (1, -1):
                for zi, along in enumerate((0.0, 0.6, -0.8)):
                    # a face: step the coordinate the face's normal is most aligned with
                    for face in (0, 1):
                        wx, wy = world(sg * hx, along * hy) if face == 0 else world(along * hx, sg * hy)
                        nx, ny = (c, s) if face == 0 else (-s, c)
                        if abs(nx) >= abs(ny):
                            pts.append((step32(wx, n), np.float32(wy), np.float32(zs[zi])))
                        else:
                            pts.append((np.float32(wx), step32(wy, n), np.float32(zs[zi])))
                for sg2 in (1, -1):                                                       # the four corners: both coordinates move
                    wx, wy = world(sg * hx, sg2 * hy)
                    pts.append((step32(wx, n), step32(wy, n), np.float32(cz + 0.1)))
        sets.append((np.array(pts, np.float32), box[None]))
    return sets


def family_c(dtype, rng):
    boxes = np.array([[10.0, 5.0, 1.0, 6.0, 3.0, 2.0, 0.4],
                      [11.0, 5.5, 1.2, 4.0, 4.0, 2.0, -0.9],
                      [10.5, 4.5, 0.8, 8.0, 1.5, 1.8, 1.3],
                      [30.0, 5.0, 1.0, 3.0, 3.0, 2.0, 0.1]], dtype)
    pts = np.c_[rng.uniform(5.5, 15.5, 260), rng.uniform(0.5, 9.5, 260), rng.uniform(-0.3, 2.4, 260)]
    pts = np.concatenate([pts, np.c_[rng.uniform(28, 32, 20), rng.uniform(3, 7, 20), rng.uniform(-0.3, 2.4, 20)]]).astype(np.float32)
    return [(pts, boxes), (pts.copy(), boxes[::-1].copy())]


def family_d(dtype):
    nan = np.nan
    rows = [[0, 0, 0, 0.0, 0.0, 1.0, 0.3],          # 0  dx = dy = 0: the margin alone
            [0, 0, 0, 2.0, 2.0, 0.0, 0.0],          # 1  dz = 0: the plane z = cz
            [0, 0, 0, 0.0, 0.0, 0.0, 0.0],          # 2  all three
            [0, 0, 0, -1.0, 2.0, 2.0, 0.0],         # 3  negative extents
            [0, 0, 0, 2.0, -1.0, 2.0, 0.0],
            [0, 0, 0, 2.0, 2.0, -1.0, 0.0],
            [0, 0, 0, -1e-6, 2.0, 2.0, 0.0],        # 6  (the margin alone would still contain the centre)
            [0, 0, 0, 2.0, 2.0, -1e-6, 0.0],
            [0, 0, 0, 2.0, 2.0, 2.0, 2e6],          # 8  beyond the sine / cosine's domain
            [0, 0, 0, 2.0, 2.0, 2.0, -2e6]]
    for col in range(7):                             # 10 .. 16  NaN in every column
        r = [0, 0, 0, 2.0, 2.0, 2.0, 0.2]
        r[col] = nan
        rows.append(r)
    rows.append([0, 0, 0, 2.0, 2.0, 2.0, 0.2])       # 17 a sound box: NaN points around it
    boxes = np.array(rows, np.float64)
    boxes[:, 0] = 10.0 * np.arange(len(rows)) + np.where(np.isnan(boxes[:, 0]), nan, 0.0)
    boxes = boxes.astype(dtype)
    pts = []
    for k in range(len(rows)):
        cx = 10.0 * k
        for ox in (0.0, 5e-6, -5e-6, 2e-5, -2e-5, 0.5, -0.5):
            for oz in (0.0, 1e-6, -1e-6, 0.4):
                pts.append((cx + ox, ox if abs(ox) < 1e-4 else 0.0, oz))
    last = 10.0 * (len(rows) - 1)
    pts += [(nan, 0.0, 0.0), (last, nan, 0.0), (last, 0.0, nan), (nan, nan, nan), (last, 0.0, 0.0)]
    return [(np.array(pts, np.float32), boxes)]


def stack(sets):
    n = max(len(p) for p, _ in sets)
    assert all(len(p) == n for p, _ in sets), [len(p) for p, _ in sets]
    return np.stack([p for p, _ in sets]), np.stack([b for _, b in sets])


# ---- family E: the reference's own generate_detections / get_box_heights -----------------------------------------------------------
def family_e():
    import logging
    import types
    import torch
    from oracle import refstubs
    from vilgod_amd import synthetic
    refstubs.install()

    def points_in_boxes_gpu(points, boxes):          # [1, N, 3], [1, M, 7] float32 tensors -> [1, N] int32
        got, _ = owners(points[0].numpy(), boxes[0].numpy())
        return torch.from_numpy(got)[None]

    stub = types.SimpleNamespace(points_in_boxes_gpu=points_in_boxes_gpu)
    sys.modules['pcdet.ops.roiaware_pool3d'].roiaware_pool3d_utils = stub
    from src.utils import pointcloud_utils
    pointcloud_utils.roiaware_pool3d_utils = stub
    from src.vilgod.lidar_frame import LidarFrame
    pts, meta = synthetic.make_frame(31, 2000, n_objects=6, return_meta=True)
    poses = synthetic.make_poses(3, step=0.5, seed=4)
    pose, ref_pose = poses[2], poses[0]
    props = [[*o['center'], o['dims'][0] + 0.2, o['dims'][1] + 0.2, o['dims'][2] + 0.2, o['yaw']] for o in meta['objects']]
    first = props[0]
    # overlaps the first annotation box and comes BEFORE it: it takes the points they share, the annotation box keeps the rest
    props.insert(0, [first[0] + 0.4, first[1] - 0.3, first[2], first[3], first[4] + 0.5, first[5], first[6] + 0.3])
    props.insert(4, [70.0, 70.0, 30.0, 2.0, 2.0, 2.0, 0.5])                                                            # owns no point
    props = np.array(props, np.float64)
    names = np.array([f'kind_{k % 3}' for k in range(len(props))])
    frame = LidarFrame('seq', 2, pts, dict(gt_names=[], moving=[]), pose, ref_pose, None, logging.getLogger('g'))
    frame.generate_detections(None, proposals=props, names=names)
    dets = [d.serialize for d in frame.detections]
    assert len(dets) == len(props) - 1 and [int(d['cluster_id']) for d in dets] == [0, 1, 2, 3, 5, 6, 7], [d['cluster_id'] for d in dets]
    for d in dets:
        assert set(d) >= {'cluster_id', 'cluster_points_index', '_bounding_box', 'object_class'} and list(d['object_class']) == ['proposal']
        assert not any(k in d for k in ('object_class_predictions', 'object_class_score', 'object_class_predictions_score'))
    index = [np.asarray(d['cluster_points_index'], np.int64) for d in dets]
    heights = pointcloud_utils.get_box_heights(pts, props)
    return dict(E_points=pts, E_pose=pose, E_ref_pose=ref_pose, E_proposals=props, E_names=names,
                E_cluster_id=np.array([d['cluster_id'] for d in dets], np.int64), E_index=np.concatenate(index),
                E_seg=np.r_[0, np.cumsum([len(i) for i in index])].astype(np.int64),
                E_box=np.array([d['_bounding_box'] for d in dets], np.float64),
                E_object_class=np.array([str(d['object_class']['proposal']) for d in dets]), E_heights=heights)


def main():
    rng = np.random.default_rng(20261)
    out = {}
    clearance = np.inf
    for fam, make in (('A', family_a), ('B', family_b), ('C', lambda dt: family_c(dt, rng)), ('D', family_d)):
        for tag, dtype in (('32', np.float32), ('64', np.float64)):
            if fam == 'C':
                rng = np.random.default_rng(20261)                   # both dtypes see the same points
            pts, boxes = stack(make(dtype))
            expect = np.zeros(pts.shape[:2], np.int32)
            worst = np.inf
            for s in range(len(pts)):
                expect[s], c = owners(pts[s], boxes[s])
                worst = min(worst, c)
            if fam == 'B':
                assert worst > 1.0, f'B{tag}: a point inside the tie zone (clearance {worst})'
                clearance = min(clearance, worst)
            out[f'{fam}{tag}_points'], out[f'{fam}{tag}_boxes'], out[f'{fam}{tag}_expect'] = pts, boxes, expect
            inside_share = float(np.mean(expect >= 0))
            print(f'{fam}{tag}: {pts.shape[0]} sets x {pts.shape[1]} points x {boxes.shape[1]} boxes, inside {inside_share:.2f}, '
                  f'smallest clearance {worst:.3g} bounds')
            if fam in 'AB':
                assert 0.2 < inside_share < 0.8, inside_share
    # family A: the equality cases exist (a point exactly on an x / y face in A64, on a z face in both)
    for tag in ('32', '64'):
        p, b = out[f'A{tag}_points'].astype(np.float64), out[f'A{tag}_boxes'].astype(np.float64)
        assert np.any(np.abs(p[:, :, 2] - b[:, :, 2]) == b[:, :, 5] / 2)
    p, b = out['A64_points'].astype(np.float64), out['A64_boxes']
    assert np.any(np.abs(p[:, :, 0] - b[:, :, 0]) == b[:, :, 3] / 2 + 1e-5) and np.any(np.abs(p[:, :, 1] - b[:, :, 1]) == b[:, :, 4] / 2 + 1e-5)
    # family C: points inside two and three boxes
    for tag in ('32', '64'):
        pts, boxes = out[f'C{tag}_points'][0], out[f'C{tag}_boxes'][0]
        multi = np.array([sum(inside(q, bb)[0] for bb in boxes) for q in pts])
        assert np.count_nonzero(multi == 2) >= 10 and np.count_nonzero(multi == 3) >= 5, np.bincount(multi)
        assert np.any(out[f'C{tag}_expect'][0] != out[f'C{tag}_expect'][1])
    out['B_min_clearance'] = np.float64(clearance)
    out['tie_units'], out['tie_margin'] = np.int64(TIE_UNITS), np.int64(TIE_MARGIN)
    out.update(family_e())
    path = os.path.join(OUT, 'points_in_boxes_golden.npz')
    np.savez_compressed(path, **out)
    print('B smallest clearance', clearance, 'bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
