"""Generates tests/golden/dbscan_golden.npz: the DBSCAN scenes with scikit-learn's `labels_` and `core_sample_indices_`, for
tests/test_dbscan_host.py and tests/test_dbscan_device.py (csrc/cluster_dbscan.inc).  Needs scikit-learn; the tests only read the file.

    python tests/golden/make_dbscan.py

Per scene `k`: X_k float32 [n, dim] (absent for the real frame: its rows are the first 20 000 of tests/golden/kitti_000000.bin),
labels_k int32 [n], core_k int32 (sklearn's core_sample_indices_), and in `meta` (JSON): name, eps, min_samples, dim, lattice.

Conditions on the INPUTS, asserted here and again by the host test (they are no measurements):
  * non-lattice scenes: no pair has |d2 - eps2| <= 1e-9 * eps2.  The float64 sum rounds below 1e-15 relative, so neither FMA
    contraction nor the order of summation inside scikit-learn can move a pair across the threshold.
  * lattice scenes: every coordinate and eps is a multiple of 2^-2 below 2^10 (or eps is the float64 just below such a value): every
    product and sum is exact.
  * `shared_border`: at least 16 border rows have core neighbours in two different clusters, and the cluster with the lower label
    comes later in Morton order (larger x, same y and z cells) -- "first found" and "smallest label" differ.
  * `numbering`: at least 8 clusters whose lowest row is a border row -- numbering by "lowest row" and by "lowest core row" differ.
Scene list: see `scenes()`; each is aimed at a way the kernels can go wrong.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from dbscan_ref import dbscan_ref, margin, margin_sparse, pair_d2     # noqa: E402

ORIGINS = ((0.0, 0.0, 0.0), (140.0, -90.0, 3.0), (-480.0, 510.0, -20.0))


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))


def cell_faces(origin, eps, seed):
    """Pairs across faces, edges and corners of the 0.4 m cells: partner = base + dir * eps * (1 -+ 2^-10), a hair inside / outside.
    The grid's origin follows the data, so the bases get random sub-cell offsets: many pairs straddle a face, an edge or a corner."""
    rng = np.random.default_rng(seed)
    dirs = []
    for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1),
              (1, 1, 1), (1, -1, 1), (1, 1, -1), (1, -1, -1)):
        v = np.array(d, dtype=np.float64)
        dirs.append(v / np.linalg.norm(v))
    pitch = 4.0 * eps + 1.0
    rows = []
    k = 0
    for rep in range(4):
        for d in dirs:
            for scale in (1.0 - 2.0 ** -10, 1.0 + 2.0 ** -10):
                base = np.array(origin) + np.array([(k % 8) * pitch, (k // 8 % 8) * pitch, (k // 64) * pitch]) + rng.uniform(0, 0.4, 3)
                rows.append(base)
                rows.append(base + d * eps * scale)
                k += 1
    return f32(rows)


def blob(rng, centre, n, sigma):
    return np.asarray(centre) + rng.normal(0, sigma, (n, 3))


def shared_border():
    """Two walls with tips, 20 sparse rows between the tips.  Array order: wall B (larger x: later in Morton order) first, so B is label 0."""
    ys, zs = np.arange(0, 81) * 0.25, np.arange(3) * 0.25      # a lattice scene: the rows between sit exactly eps from both tips
    wall = lambda x: [(x, y, z) for y in ys for z in zs]
    tips = lambda x: [(x, float(m), 0.25) for m in range(20)]
    B = wall(1.25) + tips(1.0)
    mid = tips(0.5)
    A = wall(-0.25) + tips(0.0)
    return f32(B + mid + A)


def numbering(seed):
    """40 blobs of 6 clump rows + 1 satellite (a border row at min_samples 6), rows interleaved at random; in the first 12 blobs the
    satellite is moved to the blob's lowest row."""
    rng = np.random.default_rng(seed)
    centres = []
    while len(centres) < 40:
        c = np.append(rng.uniform(-50, 50, 2), rng.uniform(-1, 1))
        if all(np.linalg.norm(c - o) > 3.0 for o in centres):
            centres.append(c)
    pts, owner, sat = [], [], []
    for b, c in enumerate(centres):
        a = rng.uniform(0, 2 * np.pi)
        u = np.array([np.cos(a), np.sin(a), 0.0])
        for t in (-0.1, -0.06, -0.02, 0.02, 0.06, 0.1):
            pts.append(c + t * u); owner.append(b); sat.append(False)
        pts.append(c + 0.45 * u); owner.append(b); sat.append(True)
    pts, owner, sat = np.array(pts), np.array(owner), np.array(sat)
    perm = rng.permutation(len(pts))
    pts, owner, sat = pts[perm], owner[perm], sat[perm]
    for b in range(12):
        rows = np.flatnonzero(owner == b)
        s = rows[sat[rows]][0]
        lo = rows[0]
        pts[[lo, s]] = pts[[s, lo]]
        sat[[lo, s]] = sat[[s, lo]]
    return f32(pts)


def serpentine(step, n):
    pts, x, y, sx = [], 0.0, 0.0, 1
    while len(pts) < n:
        for _ in range(600):
            pts.append((x, y, 0.0)); x += sx * step
        x -= sx * step
        for _ in range(10):
            y += step; pts.append((x, y, 0.0))
        y += step
        sx = -sx
    return f32(pts[:n])


def scenes():
    rng = np.random.default_rng(20261021)
    S = []
    add = lambda name, X, eps, ms, lattice=False: S.append(dict(name=name, X=f32(X).reshape(len(X), -1) if len(X) else np.zeros((0, 3), np.float32),
                                                                  eps=float(eps), min_samples=int(ms), dim=int(np.shape(X)[1]) if len(X) else 3,
                                                                  lattice=bool(lattice)))
    # 1 degenerate sizes
    add('n0', np.zeros((0, 3)), 0.5, 1)
    add('n1_ms1', [[1.0, 2.0, 3.0]], 0.5, 1)
    add('n1_ms2', [[1.0, 2.0, 3.0]], 0.5, 2)
    add('n2_ms2', [[0, 0, 0], [0.1, 0, 0]], 0.5, 2)
    add('n2_apart', [[0, 0, 0], [5.0, 0, 0]], 0.5, 1)
    add('isolated_ms1', [[5.0 * i, -3.0 * i, 0.5 * i] for i in range(10)], 0.5, 1)
    add('ms_gt_n', blob(rng, (0, 0, 0), 5, 0.05), 0.5, 6)
    for n, ms in ((64, 64), (64, 65), (65, 65), (65, 64)):
        add(f'coincident_{n}_ms{ms}', np.tile([[1.25, -2.5, 0.75]], (n, 1)), 0.5, ms, lattice=True)
    # 2 inclusive threshold
    lat = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing='ij'), -1).reshape(-1, 3) * 0.5
    for ms in (7, 8):
        add(f'lattice_ms{ms}', lat, 0.5, ms, lattice=True)
    for ms in (1, 2):
        add(f'lattice_below_ms{ms}', lat, np.nextafter(0.5, 0), ms, lattice=True)
    add('lattice_duplicates', np.concatenate([lat, lat[::3], lat[::7]]) + np.array([100.0, -200.0, 8.0]), 0.5, 9, lattice=True)
    # 3 cell faces
    for oi, o in enumerate(ORIGINS):
        for eps in (0.3, 0.4, 0.41, 3.2):
            add(f'faces_o{oi}_eps{eps}', cell_faces(o, eps, 100 * oi + int(eps * 100)), eps, 2)
    # 4 clamped rows: 600 m wide, 40 m up -- beyond the 512 x 512 x 64 cells
    add('clamped', np.concatenate([blob(rng, c, 60, 0.15) for c in ((0, 0, 0), (300, 0, 0), (-300, 10, 40), (0, 300, 40), (0, -300, -5),
                                                                      (300.3, 0.2, 0), (-300, 10, 39.6))]), 0.5, 5)
    # 5 long components: eps 0.06, spacing 0.9 eps: 3 000 rows, 162 m, 400 cells
    line = [(0.054 * i, 0.0, 0.0) for i in range(3000)]
    for ms in (2, 3):
        add(f'line_ms{ms}', line, 0.06, ms)
        add(f'serpentine_ms{ms}', serpentine(0.054, 3000), 0.06, ms)
    # 6 shared border rows
    add('shared_border', shared_border(), 0.5, 5, lattice=True)
    # 7 numbering
    add('numbering', numbering(7), 0.5, 6)
    # 8 dim 4 and 5
    g = blob(rng, (3, 4, 0.5), 30, 0.1)
    two = np.concatenate([np.column_stack([g, np.zeros(30)]), np.column_stack([g, np.full(30, 0.8)])])
    add('dim4_two_groups', two, 0.5, 5)
    add('dim3_same_groups', two[:, :3], 0.5, 5)
    m = 600
    c5 = rng.uniform(-15, 15, (12, 3)) * np.array([1, 1, 0.05])
    seq = np.column_stack([c5[rng.integers(0, 12, m)] + rng.normal(0, 0.25, (m, 3)), rng.uniform(0, 1, m), rng.integers(0, 2, m) * 0.1])
    add('dim5_points_seq', seq, 0.5, 5)
    return S


def check_inputs(s, X):
    """the conditions on the inputs (module docstring); also called by tests/test_dbscan_host.py"""
    eps, ms = s['eps'], s['min_samples']
    if s['lattice']:
        assert np.all(X * 4 == np.round(X * 4)) and np.all(np.abs(X) < 1024), s['name']
        assert eps * 4 == round(eps * 4) or np.nextafter(eps, 1) * 4 == round(np.nextafter(eps, 1) * 4), s['name']
    elif X.shape[0] > 5000:
        assert margin_sparse(X, eps) > 1e-9, (s['name'], margin_sparse(X, eps))
    else:
        assert margin(X, eps) > 1e-9, (s['name'], margin(X, eps))
    if s['name'] == 'shared_border':
        labels, core, nc = dbscan_ref(X, eps, ms)
        nb = pair_d2(X) <= eps * eps
        shared = [i for i in np.flatnonzero(~core) if len(set(labels[np.flatnonzero(nb[i] & core)])) >= 2]
        assert nc == 2 and len(shared) >= 16, (nc, len(shared))
        # label 0's rows lie at larger x, in the same y and z range: later in Morton order
        assert X[(labels == 0) & core, 0].min() > X[(labels == 1) & core, 0].max()
        assert all(labels[i] == 0 for i in shared)
    if s['name'] == 'numbering':
        labels, core, nc = dbscan_ref(X, eps, ms)
        lowest_is_border = sum(1 for c in range(nc) if not core[np.flatnonzero(labels == c)[0]])
        assert nc == 40 and lowest_is_border >= 8, (nc, lowest_is_border)


def kitti_rows():
    return np.fromfile(os.path.join(HERE, 'kitti_000000.bin'), dtype=np.float32).reshape(-1, 4)[:20000, :3].copy()


def main():
    from sklearn.cluster import DBSCAN
    out, meta = {}, []
    S = scenes() + [dict(name='kitti_20000', X=None, eps=0.5, min_samples=10, dim=3, lattice=False)]
    for k, s in enumerate(S):
        X = kitti_rows() if s['X'] is None else s['X']
        check_inputs(s, X)
        if X.shape[0]:
            m = DBSCAN(eps=s['eps'], min_samples=s['min_samples']).fit(X.astype(np.float64))
            labels, core = m.labels_.astype(np.int32), m.core_sample_indices_.astype(np.int32)
        else:
            labels, core = np.zeros(0, np.int32), np.zeros(0, np.int32)
        if X.shape[0] <= 3000:
            rl, rc, _ = dbscan_ref(X, s['eps'], s['min_samples'])
            assert np.array_equal(rl, labels) and np.array_equal(np.flatnonzero(rc), core), s['name']
        if s['X'] is not None:
            out[f'X_{k}'] = X
        out[f'labels_{k}'], out[f'core_{k}'] = labels, core
        meta.append({key: s[key] for key in ('name', 'eps', 'min_samples', 'dim', 'lattice')})
        print(f"{k:3d} {s['name']:24s} n {X.shape[0]:6d} eps {s['eps']:.4g} ms {s['min_samples']:3d} clusters {labels.max() + 1 if labels.size else 0:5d} "
              f"core {core.size:6d} noise {(labels < 0).sum():6d}")
    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, 'dbscan_golden.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
