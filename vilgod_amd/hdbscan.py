"""`HDBSCAN` with the constructor and result attributes the reference uses
(tools/configs/preprocessor/waymo.yaml:10-15 -> `hdbscan.HDBSCAN(cluster_selection_epsilon=0.15,
min_cluster_size=15, metric='euclidean', core_dist_n_jobs=-1)`; `.fit(X)` then `.labels_`,
`.probabilities_`, src/vilgod/zero_shot_detector.py:248-250), running on the GPU:

    core distances + exact mutual-reachability MST + edge sort   csrc/cluster.hip: cluster_core.inc, cluster_mst.inc   (GPU)
    single linkage / condense / selection / epsilon / labels     csrc/hdbscan_tree.cpp (host, C++), or -- `hierarchy='device'` --
                                                                 csrc/hdbscan_device.hip (GPU, the same results bit for bit)

The library's cluster-selection options are taken as the library takes them (semantics of its scikit-learn port,
sklearn/cluster/_hdbscan/_tree.pyx): `cluster_selection_method` 'eom' (default) or 'leaf', `allow_single_cluster`, `max_cluster_size`
(None or 0: unlimited; excess of mass only).  Both forms of the hierarchy stage implement them.

`fit` accepts a numpy array (reference call) or a CUDA float32 tensor (fused pipeline).
"""
import ctypes

import numpy as np
import torch

from ._lib import lib, ptr, stream_ptr, check, CLUSTER_MAX_K
from .cluster_handle import GridQueries      # noqa: F401  (the base of HDBSCAN; importable from here too)


def selection_options(cluster_selection_method='eom', allow_single_cluster=False, max_cluster_size=None):
    """The library's three cluster-selection options -> (selection, allow_single_cluster, max_cluster_size) as vg_hdbscan_tree_host_ex /
    vg_hdbscan_tree_device_ex take them: 0 = 'eom' / 1 = 'leaf'; 0 / 1; 0 = unlimited (None or 0).  ValueError for anything else."""
    if cluster_selection_method not in ('eom', 'leaf'):
        raise ValueError("cluster_selection_method: 'eom' or 'leaf'")
    if max_cluster_size is not None and int(max_cluster_size) < 0:
        raise ValueError('max_cluster_size: None, 0 (both: unlimited) or a positive integer')
    return (1 if cluster_selection_method == 'leaf' else 0, int(bool(allow_single_cluster)), int(max_cluster_size) if max_cluster_size else 0)


class HDBSCAN(GridQueries):
    def __init__(self, min_cluster_size=5, min_samples=None, cluster_selection_epsilon=0.0, metric='euclidean',
                 core_dist_n_jobs=None, max_points=400_000, device='cuda', hierarchy='host', cluster_selection_method='eom',
                 allow_single_cluster=False, max_cluster_size=None, **unused):
        """max_points: the largest point set `fit` / `mst` take; the handle holds `cluster_handle.HANDLE_COST` for it."""
        if metric != 'euclidean':
            raise NotImplementedError('only the euclidean metric of the reference configuration is implemented')
        for k in unused:
            if k not in ('alpha', 'algorithm', 'leaf_size', 'approx_min_span_tree', 'gen_min_span_tree', 'prediction_data', 'memory'):
                raise TypeError(f'unexpected keyword {k}')
        # (selection, allow_single_cluster, max_cluster_size) as vg_hdbscan_tree_host_ex / _device_ex take them
        self.selection_args = selection_options(cluster_selection_method, allow_single_cluster, max_cluster_size)
        self.cluster_selection_method = cluster_selection_method
        self.allow_single_cluster = bool(allow_single_cluster)
        self.max_cluster_size = self.selection_args[2] or None
        self.min_cluster_size = int(min_cluster_size)
        self.min_samples = int(min_samples) if min_samples is not None else self.min_cluster_size
        if not 1 <= self.min_samples <= CLUSTER_MAX_K:
            raise NotImplementedError(f'min_samples must be in [1, {CLUSTER_MAX_K}] (the neighbour list of an isolated query is one '
                                      'entry per lane of a wave)')
        self.cluster_selection_epsilon = float(cluster_selection_epsilon)
        self.device = torch.device(device)
        self.max_points = int(max_points)
        # `fit`'s hierarchy stage: 'host' (csrc/hdbscan_tree.cpp) or 'device' (csrc/hdbscan_device.hip: the tree stays on the GPU);
        # identical results.  (The fused pipeline chooses for itself: PseudoLabelPipeline(hierarchy=...).)
        if hierarchy not in ('host', 'device'):
            raise ValueError("hierarchy: 'host' or 'device'")
        if self.min_cluster_size > 32 or self.max_points > (1 << 20):       # what the device stage holds (include/vilgod_hip.h)
            hierarchy = 'host'
        self.hierarchy = hierarchy
        self._hier = None
        GridQueries.__init__(self, self.max_points, self.device)
        self.labels_ = None
        self.probabilities_ = None
        self.n_rounds_ = 0

    # ---- GPU stage ---------------------------------------------------------------------------------
    def mst(self, X, want_core=False, stream=None, dim=3):
        """X: CUDA float32 [n,>=dim]; the first `dim` (3..5) columns are the clustering space.
        -> (lo int32[n-1], hi int32[n-1], w2 float64[n-1]) CUDA, sorted by w2 (+ squared core distances in input order)."""
        assert X.is_cuda and X.dtype == torch.float32 and X.stride(1) == 1 and 3 <= dim <= 5 and X.shape[1] >= dim
        n = X.shape[0]
        m = max(n - 1, 0)
        dev = X.device
        lo = torch.empty(m, dtype=torch.int32, device=dev)
        hi = torch.empty(m, dtype=torch.int32, device=dev)
        w2 = torch.empty(m, dtype=torch.float64, device=dev)
        core2 = torch.empty(n, dtype=torch.float64, device=dev) if want_core else None
        rounds = ctypes.c_int32(0)
        check(lib.vg_cluster_mst_nd(self._h, ptr(X), n, X.stride(0), int(dim), self.min_samples, ptr(core2), ptr(lo), ptr(hi),
                                    ptr(w2), ctypes.byref(rounds), stream_ptr(stream)), 'vg_cluster_mst_nd')
        self.n_rounds_ = rounds.value
        return (lo, hi, w2, core2) if want_core else (lo, hi, w2)

    # ---- host stage ----------------------------------------------------------------------------------
    def tree(self, lo, hi, w2, n):
        """numpy (host) sorted MST -> labels int32 [n], probabilities float64 [n]."""
        labels = np.empty(n, np.int32)
        probs = np.empty(n, np.float64)
        nc = ctypes.c_int32(0)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        check(lib.vg_hdbscan_tree_host_ex(p(lo), p(hi), p(w2), n, self.min_cluster_size, self.cluster_selection_epsilon,
                                          *self.selection_args, p(labels), p(probs), ctypes.byref(nc)), 'vg_hdbscan_tree_host_ex')
        return labels, probs, nc.value


    def tree_device(self, lo, hi, w2, n, stream=None):
        """CUDA sorted MST (as `mst` returns it) -> (labels int32 [n], probabilities float64 [n], n_clusters int32 [1]) CUDA tensors, queued on
        the stream, nothing waited for: the hierarchy stage as kernels (csrc/hdbscan_device.hip), the same results as `tree`."""
        if self._hier is None:
            self._hier = DeviceHierarchy(max_points=self.max_points, device=self.device)
        return self._hier.tree_async(lo, hi, w2, n, self.min_cluster_size, self.cluster_selection_epsilon, stream, *self.selection_args)

    def fit(self, X, dim=None):
        """numpy input: every column is a clustering coordinate, like the library (3 = `points_ref_wo_ground[..., :3]`,
        zero_shot_detector.py:246-248; 5 = the two-frame `points_seq`, :239-241).  CUDA tensor input (fused pipeline):
        point rows, the first `dim` (default 3) columns are used."""
        if isinstance(X, np.ndarray):
            if dim is None:
                dim = X.shape[1]
            if not 3 <= dim <= 5:
                raise NotImplementedError('3 to 5 clustering coordinates (x, y, z first)')
            Xd = torch.from_numpy(np.ascontiguousarray(X[:, :dim], dtype=np.float32)).to(self.device)
        else:
            Xd = X if (X.dtype == torch.float32 and X.stride(1) == 1) else X.float().contiguous()
            dim = 3 if dim is None else dim
        n = Xd.shape[0]
        if n < 2:
            self.labels_ = np.full(n, -1, np.int64)
            self.probabilities_ = np.zeros(n)
            return self
        lo, hi, w2 = self.mst(Xd, dim=dim)
        if self.hierarchy == 'device':
            d_labels, d_probs, _ = self.tree_device(lo, hi, w2, n)
            labels, probs = d_labels.cpu().numpy(), d_probs.cpu().numpy()
        else:
            labels, probs, _ = self.tree(lo.cpu().numpy(), hi.cpu().numpy(), w2.cpu().numpy(), n)
        self.labels_ = labels.astype(np.int64)
        self.probabilities_ = probs
        return self


class DeviceHierarchy:
    """The hierarchy stage on the device (csrc/hdbscan_device.hip): the tree `HDBSCAN.mst` returns -> labels int32 [n], probabilities
    float64 [n] (CUDA tensors) and the cluster count, equal bit for bit to `HDBSCAN.tree` on the same tree.  Holds the stage's buffers
    for trees of up to `max_points` points; one call at a time per object."""

    def __init__(self, max_points=400_000, device='cuda'):
        self.device = torch.device(device)
        self.max_points = int(max_points)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.vg_hier_create(ctypes.byref(h), self.max_points), 'vg_hier_create')
        self._h = h

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and lib is not None:
            lib.vg_hier_destroy(h)
            self._h = None

    def tree_async(self, lo, hi, w2, n, min_cluster_size, eps, stream=None, selection=0, allow_single_cluster=0, max_cluster_size=0):
        """-> (labels, probs, n_clusters) CUDA tensors, queued on `stream` (nothing waited for).  selection: 0 = excess of mass,
        1 = leaf; max_cluster_size: 0 = unlimited (`HDBSCAN.selection_args`)."""
        dev = self.device
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        probs = torch.empty(n, dtype=torch.float64, device=dev)
        nc = torch.zeros(1, dtype=torch.int32, device=dev)
        check(lib.vg_hdbscan_tree_device_ex(self._h, ptr(lo), ptr(hi), ptr(w2), int(n), int(min_cluster_size), float(eps), int(selection),
                                            int(allow_single_cluster), int(max_cluster_size or 0), ptr(labels), ptr(probs), ptr(nc),
                                            stream_ptr(stream)), 'vg_hdbscan_tree_device_ex')
        return labels, probs, nc

    def tree(self, lo, hi, w2, n, min_cluster_size, eps, stream=None, selection=0, allow_single_cluster=0, max_cluster_size=0):
        labels, probs, nc = self.tree_async(lo, hi, w2, n, min_cluster_size, eps, stream, selection, allow_single_cluster, max_cluster_size)
        return labels, probs, int(nc.item())
