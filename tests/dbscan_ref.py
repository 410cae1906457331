"""Dense numpy statement of the DBSCAN contract (include/vilgod_hip.h, vg_cluster_dbscan), fine to about 3 000 rows.

    pair      X widened to float64; d2 = ((dx*dx + dy*dy) + dz*dz [+ d4*d4 [+ d5*d5]]), left to right; neighbours iff d2 <= eps*eps
    core      at least min_samples neighbours, the row itself counted
    clusters  connected components of the neighbour graph on core rows, numbered by their lowest core row
    border    a non-core row takes the smallest label among its core neighbours, else -1

It is what scikit-learn's dbscan_inner computes (tests/golden/make_dbscan.py holds it to scikit-learn's labels_)."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components


def pair_d2(X, dim=None):
    """float64 [n, n]: the contract's pair sum, every product and sum rounded on its own (numpy never fuses)."""
    X = np.asarray(X, dtype=np.float32)
    dim = X.shape[1] if dim is None else dim
    Xd = X[:, :dim].astype(np.float64)

    def sq(k):
        d = Xd[:, None, k] - Xd[None, :, k]
        return d * d
    d2 = (sq(0) + sq(1)) + sq(2)
    for k in range(3, dim):
        d2 = d2 + sq(k)
    return d2


def margin(X, eps, dim=None):
    """min over pairs of |d2 - eps2| / eps2 (inf for fewer than two rows): how far the nearest pair is from the threshold."""
    d2 = pair_d2(X, dim)
    if d2.shape[0] < 2:
        return np.inf
    eps2 = float(eps) * float(eps)
    iu = np.triu_indices(d2.shape[0], 1)
    return float(np.min(np.abs(d2[iu] - eps2)) / eps2)


def dbscan_ref(X, eps, min_samples, dim=None):
    """-> (labels int64 [n], core bool [n], n_clusters)"""
    X = np.asarray(X, dtype=np.float32)
    n = X.shape[0]
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, bool), 0
    nb = pair_d2(X, dim) <= float(eps) * float(eps)
    core = nb.sum(1) >= int(min_samples)
    cc = nb & core[:, None] & core[None, :]
    _, comp = connected_components(csr_matrix(cc), directed=False)
    labels = np.full(n, -1, np.int64)
    rows = np.flatnonzero(core)
    # components in ascending order of their lowest core row
    _, first = np.unique(comp[rows], return_index=True)
    order = comp[rows][np.sort(first)]
    number = {c: k for k, c in enumerate(order)}
    labels[rows] = [number[c] for c in comp[rows]]
    for i in np.flatnonzero(~core):
        js = np.flatnonzero(nb[i] & core)
        if js.size:
            labels[i] = labels[js].min()
    return labels, core, len(order)


def margin_sparse(X, eps):
    """`margin` for 3-column arrays too large for the dense matrix: a kd-tree lists the pairs within eps * (1 + 1e-6) -- every pair it
    leaves out is farther from the threshold than that -- and the contract's own sum decides among the listed ones."""
    from scipy.spatial import cKDTree
    Xd = np.asarray(X, dtype=np.float32)[:, :3].astype(np.float64)
    pairs = cKDTree(Xd).query_pairs(eps * (1 + 1e-6), output_type='ndarray')
    if len(pairs) == 0:
        return 2e-6
    d = Xd[pairs[:, 0]] - Xd[pairs[:, 1]]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    eps2 = float(eps) * float(eps)
    return min(2e-6, float(np.min(np.abs(d2 - eps2)) / eps2))


def reorder(X, order):
    """The three row orders of the tests: 'built', 'reversed', 'shuffled' (seeded)."""
    X = np.asarray(X)
    if order == 'built':
        return X
    if order == 'reversed':
        return X[::-1].copy()
    assert order == 'shuffled'
    return X[np.random.default_rng(20261021).permutation(X.shape[0])].copy()


def random_scene(seed):
    """A seeded scene of the three kinds the contract was checked on -> (X float32 [n,3], eps, min_samples, is_lattice)."""
    rng = np.random.default_rng(seed)
    kind = seed % 3
    n = int(rng.integers(1, 401))
    ms = int(rng.integers(1, 9))
    if kind == 0:
        X = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
        return X, float(rng.uniform(0.3, 1.2)), ms, False
    if kind == 1:
        c = rng.uniform(-20, 20, (int(rng.integers(1, 7)), 3))
        X = (c[rng.integers(0, len(c), n)] + rng.normal(0, 0.3, (n, 3))).astype(np.float32)
        return X, float(rng.uniform(0.2, 0.8)), ms, False
    X = (rng.integers(0, 7, (n, 3)) * 0.5).astype(np.float32)      # a 0.5-spaced lattice with duplicates, many pairs exactly at eps
    return X, 0.5, ms, True
