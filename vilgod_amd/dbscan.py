"""`DBSCAN` with the constructor and result attributes of `sklearn.cluster.DBSCAN`, the second clustering model the reference's
`cluster_utils.py` imports (src/utils/cluster_utils.py:4-5; `hydra.utils.instantiate(cfg.preprocessor.clustering.model)`), running on
the GPU: one queued call, csrc/cluster_dbscan.inc, on the cell grid `HDBSCAN` uses.

The definition is in include/vilgod_hip.h (vg_cluster_dbscan): float64 pair distance, `d2 <= eps * eps` inclusive, a row is its own
neighbour; a core sample has at least `min_samples` neighbours; clusters are the connected components of the core samples, numbered
by their lowest core row; a border row takes the smallest label among its core neighbours.  That is what scikit-learn's
`dbscan_inner` computes: `labels_` and `core_sample_indices_` are equal to scikit-learn's.

`probabilities_` is this project's own convention: scikit-learn's class has none, and the reference reads
`cluster_info.probabilities_` after `fit` (src/vilgod/zero_shot_detector.py:248-250).  Here it is 1.0 for a labelled row, 0.0 for noise.

`eps` reaches at most 3.2 m (eight 0.4 m cells, the grid's reach limit).  `algorithm`, `leaf_size`, `p` and `n_jobs` are accepted and
ignored; other metrics and `sample_weight` are not implemented.
"""
import ctypes
import math

import numpy as np
import torch

from ._lib import lib, ptr, stream_ptr, check
from .cluster_handle import GridQueries

EPS_CELL, EPS_MAX_REACH = 0.4, 8


class DBSCAN(GridQueries):
    def __init__(self, eps=0.5, min_samples=5, metric='euclidean', metric_params=None, algorithm='auto', leaf_size=30, p=None,
                 n_jobs=None, max_points=400_000, device='cuda', **unused):
        """max_points: the largest point set `fit` / `labels_device` take; the handle holds `cluster_handle.HANDLE_COST` for it."""
        for k in unused:
            raise TypeError(f'unexpected keyword {k}')
        if metric != 'euclidean' or metric_params:
            raise NotImplementedError('only the euclidean metric is implemented')
        self.eps = float(eps)
        if not 0.0 < self.eps < math.inf or math.ceil(self.eps / EPS_CELL) > EPS_MAX_REACH:
            raise ValueError(f'eps = {eps!r}: a positive number of at most {EPS_CELL * EPS_MAX_REACH:.1f} m (the 3.2 m limit is the '
                             'reach of the 0.4 m cell grid: eight cells)')
        if int(min_samples) != min_samples or int(min_samples) < 1:
            raise ValueError(f'min_samples = {min_samples!r}: an integer >= 1')
        self.min_samples = int(min_samples)
        self.metric, self.algorithm, self.leaf_size, self.p, self.n_jobs = metric, algorithm, leaf_size, p, n_jobs
        self.device = torch.device(device)
        self.max_points = int(max_points)
        self.hierarchy = None                    # no hierarchy stage (what TwoFrameClusterer and the pipeline look at)
        GridQueries.__init__(self, self.max_points, self.device)
        self.labels_ = None
        self.core_sample_indices_ = None
        self.components_ = None
        self.probabilities_ = None
        self.n_clusters_ = 0

    def __repr__(self):
        return f'DBSCAN(eps={self.eps!r}, min_samples={self.min_samples!r})'

    def label_bound(self, n):
        """Exclusive upper bound of the labels of n rows: a cluster needs only one core row."""
        return n + 1

    def labels_device(self, X, dim=3, stream=None):
        """X: CUDA float32 [n,>=dim]; the first `dim` (3..5) columns are the clustering space.  One queued call, nothing waited for.
        -> (d_labels int32 [n], d_probs float64 [n], d_n_clusters int32 [1], d_core uint8 [n]) CUDA tensors; the handle's grid then
        holds X (`ball_count`, `nearest`, `knn`)."""
        if not 3 <= int(dim) <= 5:
            raise NotImplementedError('3 to 5 clustering coordinates (x, y, z first)')
        assert X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and X.shape[1] >= dim and (X.shape[0] == 0 or X.stride(1) == 1)
        n, dev = X.shape[0], X.device
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):      # the outputs belong to the call's stream
            d_labels = torch.empty(n, dtype=torch.int32, device=dev)
            d_probs = torch.empty(n, dtype=torch.float64, device=dev)
            d_core = torch.empty(n, dtype=torch.uint8, device=dev)
            d_nc = torch.empty(1, dtype=torch.int32, device=dev)
        check(lib.vg_cluster_dbscan(self._h, ptr(X), n, X.stride(0) if n else int(dim), int(dim), self.eps, self.min_samples,
                                    ptr(d_labels), ptr(d_core), ptr(d_probs), ptr(d_nc), stream_ptr(stream)), 'vg_cluster_dbscan')
        self._grid_ref = X
        return d_labels, d_probs, d_nc, d_core

    def fit(self, X, y=None, sample_weight=None, dim=None):
        """numpy input: every column is a clustering coordinate, like the library (3 to 5, x, y, z first); non-finite values raise
        ValueError as scikit-learn's do.  CUDA tensor input: point rows, the first `dim` (default 3) columns are used, finite by
        contract."""
        if sample_weight is not None:
            raise NotImplementedError('sample_weight is not implemented')
        if isinstance(X, np.ndarray):
            if X.ndim != 2:
                raise ValueError('X: a 2-D array')
            if dim is None:
                dim = X.shape[1]
            if not 3 <= dim <= 5:
                raise NotImplementedError('3 to 5 clustering coordinates (x, y, z first)')
            if not np.isfinite(X[:, :dim]).all():
                raise ValueError('Input X contains NaN or infinity.')
            host = np.ascontiguousarray(X[:, :dim], dtype=np.float32)
            Xd = torch.from_numpy(host).to(self.device)
        else:
            Xd = X if (X.dtype == torch.float32 and X.stride(1) == 1) else X.float().contiguous()
            dim = 3 if dim is None else dim
            host = None
        d_labels, d_probs, d_nc, d_core = self.labels_device(Xd, dim=dim)
        self.labels_ = d_labels.cpu().numpy().astype(np.int64)
        self.probabilities_ = d_probs.cpu().numpy()
        self.n_clusters_ = int(d_nc.item())
        if self.n_clusters_ < 0:
            raise RuntimeError('vg_cluster_dbscan: a bounded walk of the union-find overran (n_clusters = -1)')
        self.core_sample_indices_ = np.flatnonzero(d_core.cpu().numpy()).astype(np.int64)
        if host is not None:
            self.components_ = np.asarray(X)[self.core_sample_indices_, :dim].copy()
        else:
            self.components_ = Xd[torch.from_numpy(self.core_sample_indices_).to(Xd.device), :dim].cpu().numpy()
        return self

    def fit_predict(self, X, y=None, sample_weight=None):
        return self.fit(X, sample_weight=sample_weight).labels_


def dbscan_host(X, eps, min_samples, dim=None):
    """vg_dbscan_host on a numpy array [n,>=dim] (no GPU): -> (labels int32 [n], core uint8 [n], probs float64 [n], n_clusters).
    The definition the kernels are held to."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = X.shape[0]
    dim = X.shape[1] if dim is None else int(dim)
    labels = np.empty(n, np.int32)
    core = np.empty(n, np.uint8)
    probs = np.empty(n, np.float64)
    nc = ctypes.c_int32(-7)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    check(lib.vg_dbscan_host(p(X), n, X.shape[1] if X.ndim == 2 else dim, dim, float(eps), int(min_samples), p(labels), p(core), p(probs),
                             ctypes.byref(nc)), 'vg_dbscan_host')
    return labels, core, probs, nc.value


def is_dbscan_target(target):
    """Does a config's `clustering.model._target_` name DBSCAN (`sklearn.cluster.DBSCAN`, `vilgod_amd.dbscan.DBSCAN`)?"""
    return isinstance(target, str) and target.rsplit('.', 1)[-1] == 'DBSCAN'
