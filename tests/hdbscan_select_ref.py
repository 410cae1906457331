"""The reference of tests/test_hdbscan_selection.py: scikit-learn's own tree code (its port of the library the reference calls,
sklearn/cluster/_hdbscan/_tree.pyx) on one sorted minimum spanning tree -- `_linkage.make_single_linkage`, then
`_tree.tree_to_labels(single_linkage, min_cluster_size, method, allow_single_cluster, eps, max_cluster_size)`.

The tree is handed over in the strict (w2, lo, hi) order the product's hierarchy stage uses, with distance = sqrt(w2), so both sides
build the same dendrogram.  CPU only: nothing marked `gpu` imports this module."""
import numpy as np


def sorted_mst(X, min_samples):
    """-> (lo int32 [n-1], hi int32 [n-1], w2 float64 [n-1]): the oracle's mutual-reachability MST of X in (w2, lo, hi) order."""
    from oracle import hdbscan_oracle as ho
    core2 = ho.core_distances_sq(X, min_samples)
    edges, w2 = ho.mst_prim(X, core2)
    e, w2s = ho.sort_edges(edges, w2)
    return np.ascontiguousarray(e[:, 0], np.int32), np.ascontiguousarray(e[:, 1], np.int32), np.ascontiguousarray(w2s, np.float64)


def tree_to_labels(lo, hi, w2, min_cluster_size, method='eom', allow_single_cluster=False, eps=0.0, max_cluster_size=None):
    """-> (labels int64 [n], probabilities float64 [n]) of scikit-learn's tree code.  max_cluster_size: None or 0 = unlimited."""
    from sklearn.cluster._hdbscan import _linkage, _tree
    order = np.lexsort((hi, lo, w2))
    mst = np.zeros(len(w2), dtype=_linkage.MST_edge_dtype)
    mst['current_node'], mst['next_node'], mst['distance'] = lo[order], hi[order], np.sqrt(w2[order])
    sl = _linkage.make_single_linkage(mst)
    labels, probs = _tree.tree_to_labels(sl, int(min_cluster_size), method, bool(allow_single_cluster), float(eps),
                                         int(max_cluster_size) if max_cluster_size else None)
    return np.asarray(labels, np.int64), np.asarray(probs, np.float64)
