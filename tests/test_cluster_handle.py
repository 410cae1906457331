"""The `vg_cluster` handle (csrc/cluster.hip: CL_BUFFERS, ClDbscanView) and its Python owner (vilgod_amd/cluster_handle.py).

CPU: vg_cluster_bytes, the one observable of the list of the handle's buffers, against the sizes written out here -- the per-point
bytes as the sum of the allocations the handle made before the list existed, the fixed part from the grid's constants.
GPU: one handle serving an MST, DBSCAN (which works in seven of the MST's buffers), a grid + K-nearest query and an MST again gives
what each call gives on a fresh handle.
"""
import numpy as np
import pytest

# the handle's arrays of max_points elements: 17 of four bytes (codes x 2, permutations x 2, 5th coordinate, component, hook, picked
# ends x 2, candidate end, component size, work list, far list, edge ends x 2, edge numbers x 2), 10 of eight (core distance, best
# weight / key / pair distance, candidate weight / key / pair distance, lower bound, edge weights x 2), 2 of sixteen (points, aux)
P = 17 * 4 + 10 * 8 + 2 * 16

NCODES = 1 << 24                # 512 x 512 x 64 cells
LEVELS = 7                      # cell-start tables of levels 0 .. 6, (NCODES >> 3l) + 1 entries each
PUR_LEVELS = 4                  # purity / 4th-coordinate-range tables of levels 0 .. 3, NCODES >> 3l entries each
SIZEOF_CLGRID = 3 * 8 + 6 * 4 + 8       # origin, bounding-box keys, +inf
COUNTER_BYTES = 64 + 8          # the counter words, the largest component
FIXED = (SIZEOF_CLGRID + 4 * sum((NCODES >> (3 * l)) + 1 for l in range(LEVELS))
         + 2 * 4 * sum(NCODES >> (3 * l) for l in range(PUR_LEVELS)) + COUNTER_BYTES)


def _bytes(n):
    from vilgod_amd._lib import lib
    return lib.vg_cluster_bytes(n)


def test_per_point_bytes():
    assert P == 180
    for m, n in ((1, 2), (1, 1 << 20), (1000, 160_000), (7, 400_000), (1 << 20, (1 << 20) + 1)):
        assert _bytes(n) - _bytes(m) == P * (n - m), (m, n)


def test_fixed_bytes_from_the_grid_constants():
    assert FIXED == 230_050_204             # (the figure read off the allocations, as a check of the formula above)
    assert _bytes(1) - P == FIXED


def test_no_points_no_bytes():
    assert _bytes(0) == 0 and _bytes(-5) == 0


def test_grid_queries_has_one_home_and_two_names():
    from vilgod_amd import cluster_handle, hdbscan, dbscan
    assert hdbscan.GridQueries is cluster_handle.GridQueries
    assert issubclass(hdbscan.HDBSCAN, cluster_handle.GridQueries) and issubclass(dbscan.DBSCAN, cluster_handle.GridQueries)
    assert cluster_handle.HANDLE_BYTES_PER_POINT == P and cluster_handle.HANDLE_BYTES_FIXED == FIXED


def _scene():
    """300 rows: three Gaussian blobs of 80 and 60 rows of uniform noise"""
    rng = np.random.default_rng(20240611)
    centres = np.array([[0.0, 0.0, 0.0], [3.0, 1.0, 0.5], [-2.5, 2.0, -0.5]])
    blobs = [c + 0.3 * rng.standard_normal((80, 3)) for c in centres]
    return np.concatenate(blobs + [rng.uniform(-5.0, 5.0, (60, 3))]).astype(np.float32)


def _mst(model, X):
    """the tree and the core distances as bytes.  Edges of equal weight come in the order they were emitted (vilgod_hip.h: unspecified),
    so the edges are put in (w2, lo, hi) order first; every value is compared bit for bit."""
    lo, hi, w2, core2 = (t.cpu().numpy() for t in model.mst(X, want_core=True))
    o = np.lexsort((hi, lo, w2))
    return lo[o].tobytes(), hi[o].tobytes(), w2[o].tobytes(), core2.tobytes()


@pytest.mark.gpu
def test_a_handle_carries_no_state_between_its_users(cuda):
    import torch
    from vilgod_amd.cluster_handle import GridQueries
    from vilgod_amd.dbscan import DBSCAN
    from vilgod_amd.hdbscan import HDBSCAN
    X = torch.from_numpy(_scene()).to(cuda)
    cpu = lambda ts: tuple(t.cpu().numpy().tobytes() for t in ts)

    # every call on a fresh handle (the MST's is the shared handle's own first call)
    g = GridQueries(1024, cuda)
    g.grid(X)
    knn_fresh = cpu(g.knn(X, 4))
    del g
    db = DBSCAN(eps=0.5, min_samples=5, max_points=1024, device=cuda)
    db_fresh = cpu(db.labels_device(X))
    assert np.frombuffer(db_fresh[2], np.int32)[0] >= 3            # the blobs are clusters: the borrowed buffers are in use

    hd = HDBSCAN(min_samples=5, max_points=1024, device=cuda)
    own, db._h = db._h, hd._h                                      # DBSCAN on HDBSCAN's handle
    try:
        mst_first = _mst(hd, X)
        assert cpu(db.labels_device(X)) == db_fresh
        hd.grid(X)
        assert cpu(hd.knn(X, 4)) == knn_fresh
        assert _mst(hd, X) == mst_first
    finally:
        db._h = own
