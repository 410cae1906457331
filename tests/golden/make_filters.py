"""Generates tests/golden/filters_golden.npz: the reference's seven cluster filters (src/utils/cluster_utils.py:14-64) and the
combined verdict of Detection.filter (src/dataclass/objects.py:158-181) on seeded clusters.  Run only in the build container:

    python tests/golden/make_filters.py

The reference's modules are imported with the stand-ins of oracle/refstubs.py.  The fixture holds data only: the clusters
(integer millimetres: a cluster centre plus int16 offsets; tests/filters_ref.py decode_points turns them into the float32
coordinates the reference saw here), one score per point (k / 255 as float32), a plane, and per cluster the reference's verdicts.
Clusters on which the reference raises QhullError (collinear / identical points) are not in the fixture.

Area and volume: the reference sums its shoelace in float32 on uncentred coordinates, so verdicts are only comparable outside
the band B = (H+2)/2 * 2^-24 * sum(|x_i y_j| + |x_j y_i|) around a threshold (x height for the volume).  This script asserts
what tests/test_filters.py relies on: at most 5 % of the clusters inside the band per threshold, at least 20 compared clusters
on each side of each threshold, and no differing verdict outside the band.
"""
import json
import os
import sys
from functools import partial

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import refstubs  # noqa: E402
import filters_ref as fr  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

# The score thresholds stay off the k / 255 lattice of the fixture's scores: where a percentile EQUALS float32(threshold), numpy 2
# compares the float32 percentile with the Python float in float32 and numpy 1 in float64, so the reference's verdict at such a
# tie depends on its numpy.  The kernel compares in float64, as vilgod_amd.frame_state.static_from_entropy does.
# threshold sets: 0 = tools/configs/preprocessor/waymo.yaml:20-58 as shipped; 1, 2 = other values, with the optional maxima
THRESHOLDS = [
    dict(filter_by_number_points=dict(min_points=10), filter_by_height=dict(min_height=0.3, max_height=6),
         filter_by_aspect_ratio=dict(min_aspect_ratio=1.0, max_aspect_ratio=5.0), filter_by_volume=dict(min_volume=0.5),
         filter_by_area=dict(min_area=0.35), filter_by_plane_distance=dict(max_min_height=1.0, min_max_height=0.5),
         filter_by_ephemeral_score=dict(percentile=20, min_percentile_pp_score=0.7)),
    dict(filter_by_number_points=dict(min_points=5, max_points=2000), filter_by_height=dict(min_height=0.5, max_height=2.5),
         filter_by_aspect_ratio=dict(min_aspect_ratio=1.5, max_aspect_ratio=3.0), filter_by_volume=dict(min_volume=0.2, max_volume=15.0),
         filter_by_area=dict(min_area=1.0, max_area=12.0), filter_by_plane_distance=dict(max_min_height=0.3, min_max_height=1.2),
         filter_by_ephemeral_score=dict(percentile=50, min_percentile_pp_score=0.45)),
    dict(filter_by_number_points=dict(min_points=30, max_points=60000), filter_by_height=dict(min_height=1.0, max_height=4.0),
         filter_by_aspect_ratio=dict(min_aspect_ratio=2.0, max_aspect_ratio=10.0), filter_by_volume=dict(min_volume=3.0),
         filter_by_area=dict(min_area=4.0), filter_by_plane_distance=dict(max_min_height=0.5, min_max_height=2.0),
         filter_by_ephemeral_score=dict(percentile=93.5, min_percentile_pp_score=0.9)),
]
N, H, R, V, A, P, E = fr.FILTER_NAMES
# logic assignments (name -> [logic, required]); every branch of (all(and) or any(or)) and all(required)
LOGIC = [
    {N: ['and', True], H: ['and', True], P: ['and', True]},                                   # shipped: only required
    {N: ['and', True], H: ['and', True], R: ['and', False], V: ['and', False], A: ['and', False], P: ['and', True], E: ['or', False]},
    {R: ['or', False], E: ['or', False]},                                                     # only `or`: no `and`, no required
    {V: ['and', False], A: ['and', False]},                                                   # only `and`: no `or`
    {N: ['and', True], E: ['or', True]},                                                      # `required` on an `or` filter is ignored
    {N: ['or', False], H: ['and', False], R: ['and', True], V: ['or', False], A: ['and', True], P: ['and', False], E: ['and', False]},
]


def _rot(p, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    return p @ np.array([[c, s], [-s, c]])


def _outline(rng, n, length, width, yaw, sides, noise):
    per = np.array_split(np.arange(n), len(sides))
    pts = []
    for k, idx in zip(sides, per):
        t = rng.uniform(-0.5, 0.5, len(idx))
        if k in (0, 2):
            pts.append(np.stack([np.full_like(t, (0.5 if k == 0 else -0.5) * length), t * width], 1))
        else:
            pts.append(np.stack([t * length, np.full_like(t, (0.5 if k == 1 else -0.5) * width)], 1))
    return _rot(np.concatenate(pts) + rng.normal(0, noise, (n, 2)), yaw)


def clusters(seed=20261016):
    """-> list of (kind, centre_mm int32 [3], offset_mm int16 [n,3], score_u8 [n])"""
    rng = np.random.default_rng(seed)
    out = []

    def centre():
        r, phi = rng.uniform(3.0, 75.0), rng.uniform(-np.pi, np.pi)
        return np.array([r * np.cos(phi), r * np.sin(phi)])

    def scores(n, kind):
        if kind == 'static':
            s = np.clip(rng.normal(0.85, 0.08, n), 0, 1)
        elif kind == 'moving':
            s = np.clip(rng.normal(0.3, 0.15, n), 0, 1)
        elif kind == 'unseen':
            s = np.ones(n)                                   # lidar_frame.py:111-118: 1.0 where no score was stored
        else:
            s = rng.uniform(0, 1, n)
        return np.round(s * 255).astype(np.uint8)

    def add(kind, xy, z0=None, h=None, z=None):
        n = len(xy)
        if z is None:
            z0 = rng.uniform(-1.9, -0.5) if z0 is None else z0
            h = rng.uniform(0.2, 3.0) if h is None else h
            z = z0 + rng.uniform(0, h, n)
        c = centre()
        c_mm = np.round(np.r_[c, 0.0] * 1000).astype(np.int32)
        off = np.round(np.concatenate([xy, z[:, None]], 1) * 1000)
        assert np.abs(off).max() < 32000
        out.append((kind, c_mm, off.astype(np.int16), scores(n, rng.choice(['static', 'moving', 'unseen', 'mixed'], p=[.35, .3, .1, .25]))))

    for _ in range(70):                                            # box outlines (cars, vans, trucks): 2-4 visible sides
        n = int(rng.integers(12, 500))
        sides = tuple(sorted(rng.choice(4, int(rng.integers(2, 5)), replace=False)))
        add('box', _outline(rng, n, rng.uniform(1.5, 12), rng.uniform(0.8, 2.6), rng.uniform(-np.pi, np.pi), sides, rng.uniform(0, 0.05)),
            h=rng.uniform(0.8, 3.5))
    for _ in range(50):                                            # L shapes
        n = int(rng.integers(10, 500))
        add('lshape', _outline(rng, n, rng.uniform(0.4, 6), rng.uniform(0.3, 2.2), rng.uniform(-np.pi, np.pi), (0, 1), rng.uniform(0, 0.04)))
    for _ in range(45):                                            # poles / trunks / pedestrians: small footprint
        n = int(rng.integers(5, 200))
        add('pole', rng.normal(0, rng.uniform(0.03, 0.35), (n, 2)), h=rng.uniform(0.3, 7.0))
    for _ in range(35):                                            # walls: long and thin
        n = int(rng.integers(60, 1200))
        t = rng.uniform(-0.5, 0.5, n) * rng.uniform(3, 30)
        add('wall', _rot(np.stack([t, rng.normal(0, rng.uniform(0.01, 0.15), n)], 1), rng.uniform(-np.pi, np.pi)), h=rng.uniform(0.5, 5))
    for _ in range(40):                                            # blobs around the area thresholds (0.35, 1, 4 m^2)
        n = int(rng.integers(8, 300))
        s = np.sqrt(rng.choice([0.35, 1.0, 4.0]) * rng.uniform(0.5, 2.0))
        add('blob', _rot(rng.uniform(-0.5, 0.5, (n, 2)) * [s * rng.uniform(0.6, 1.6), s], rng.uniform(-np.pi, np.pi)), h=rng.uniform(0.2, 2.5))
    for _ in range(25):                                            # 3-point clusters (proper triangles)
        while True:
            p = rng.uniform(-1.5, 1.5, (3, 2))
            q = np.round(p * 1000)
            if abs((q[1, 0] - q[0, 0]) * (q[2, 1] - q[0, 1]) - (q[1, 1] - q[0, 1]) * (q[2, 0] - q[0, 0])) > 1000:
                break
        add('three', p)
    for _ in range(10):                                            # axis-aligned / zero-height oddities: size ratios 1, extents < 1 m
        n = int(rng.integers(4, 60))
        p = rng.uniform(-0.5, 0.5, (n, 2)) * rng.uniform(0.2, 3.0, 2)
        add('flat', p, z=np.full(n, rng.uniform(-1.5, 0)))
    for n in (4000, 9000):                                  # large clusters: a building corner with clutter
        a = _outline(rng, n * 3 // 4, rng.uniform(10, 30), rng.uniform(6, 14), rng.uniform(-np.pi, np.pi), (0, 1), 0.03)
        add('corner', np.concatenate([a, rng.normal(0, 1.5, (n - len(a), 2))]), z0=-1.8, h=4.0)
    # one 50 000-point cluster on a regular scan lattice (500 columns x 100 rows of a slightly bulging facade: the rows repeat, so the
    # fixture stays small)
    t = (np.arange(500) - 250) * 0.05
    xy = _rot(np.stack([t, 0.4 * np.cos(t / 8.0)], 1), 0.6)
    add('facade_50k', np.tile(xy, (100, 1)), z=np.repeat(-1.7 + np.arange(100) * 0.05, 500))
    out[-1] = out[-1][:3] + (np.tile(np.round(np.linspace(0, 255, 500)).astype(np.uint8), 100),)
    return out


def make():
    refstubs.install()
    from scipy.spatial import QhullError
    from src.utils import cluster_utils as cu
    from src.dataclass.objects import Detection
    cl = clusters()
    seg = np.r_[0, np.cumsum([len(o) for _, _, o, _ in cl])].astype(np.int64)
    centre_mm = np.stack([c for _, c, _, _ in cl])
    offset_mm = np.concatenate([o for _, _, o, _ in cl])
    score_u8 = np.concatenate([s for _, _, _, s in cl])
    points = fr.decode_points(np.repeat(centre_mm, np.diff(seg), axis=0), offset_mm)
    scores = (score_u8.astype(np.float64) / 255.0).astype(np.float32)
    plane = np.array([0.012, -0.008, 0.9998, 1.71])              # a slightly tilted ground 1.7 m below the sensor
    C = len(cl)
    out = dict(centre_mm=centre_mm, offset_mm=offset_mm, score_u8=score_u8, seg=seg, plane=plane, kind=np.array([k for k, _, _, _ in cl]),
               meta=np.array(json.dumps(dict(thresholds=THRESHOLDS, logic=LOGIC))))
    stats = []
    for ti, T in enumerate(THRESHOLDS):
        ref = {name: np.zeros(C, bool) for name in fr.FILTER_NAMES}
        comb = np.zeros((len(LOGIC), C), bool)
        for c in range(C):
            pts, sc = points[seg[c]:seg[c + 1]], scores[seg[c]:seg[c + 1]]
            det = Detection(cluster_id=c, cluster_points=pts, cluster_points_index=np.arange(len(pts)), cluster_points_entropy=sc)
            kw = dict(ephemeral_scores=sc, height=det.height, plane_model=plane)
            try:
                for name in fr.FILTER_NAMES:
                    ref[name][c] = bool(getattr(cu, name)(points=pts, **T[name], **kw))
                for li, L in enumerate(LOGIC):
                    flt = [[partial(getattr(cu, name), **T[name]), name, lg, req] for name, (lg, req) in L.items()]
                    det.filter(flt, plane_model=plane)
                    comb[li, c] = bool(det.valid)
                    assert all(bool(det.filter_dict[name]) == ref[name][c] for name in L)
            except QhullError:
                raise SystemExit(f'cluster {c} ({cl[c][0]}): QhullError -- such clusters do not belong in the fixture')
            if ti == 0:
                stats.append(fr.cluster_stats(pts, sc, plane, T))
        for name in fr.FILTER_NAMES:
            out[f'ref_{ti}_{name}'] = ref[name]
        out[f'comb_{ti}'] = comb
        # ---- what tests/test_filters.py relies on ----
        for c in range(C):
            stats[c]['q'] = fr.percentile(scores[seg[c]:seg[c + 1]], T[E]['percentile'])
        mine = [fr.verdicts(st, T) for st in stats]
        for name in (N, H, R, P, E):
            bad = [c for c in range(C) if mine[c][name] != ref[name][c]]
            assert not bad, (ti, name, bad)
        for name, key, scale in ((A, 'area', lambda st: 1.0), (V, 'volume', lambda st: float(st['height']))):
            thr = [T[name]['min_' + key]] + ([T[name]['max_' + key]] if T[name].get('max_' + key) is not None else [])
            inside = np.array([any(abs(st[key] - t) <= fr.band_f32(st['n_hull'], st['S']) * scale(st) for t in thr) for st in stats])
            val = np.array([st[key] for st in stats])
            assert inside.mean() <= 0.05, (ti, name, inside.mean())
            for t in thr:
                assert ((val < t) & ~inside).sum() >= 20 and ((val > t) & ~inside).sum() >= 20, (ti, name, t)
            bad = [c for c in range(C) if not inside[c] and mine[c][name] != ref[name][c]]
            assert not bad, (ti, name, bad)
            print(f'set {ti} {name}: {inside.sum()} of {C} inside the band, below/above {[(int((val < t).sum()), int((val > t).sum())) for t in thr]}')
    path = os.path.join(OUT, 'filters_golden.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {C} clusters, {seg[-1]} points, {os.path.getsize(path)} bytes; hull sizes up to {max(st["n_hull"] for st in stats)}')


if __name__ == '__main__':
    make()
