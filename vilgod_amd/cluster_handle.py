"""`GridQueries`: a `vg_cluster` handle (csrc/cluster.hip) and the queries on its cell grid.  `HDBSCAN` and `DBSCAN` derive from it;
`vilgod_amd.knn` constructs it directly for its cached handles."""
import ctypes

import numpy as np
import torch

from ._lib import lib, ptr, stream_ptr, check

# device memory of a handle, from the library's own list of its buffers (vg_cluster_bytes): bytes per point of max_points, and the part
# that does not depend on max_points (the cell-start, purity and range tables of the 0.4 m grid)
HANDLE_BYTES_PER_POINT = lib.vg_cluster_bytes(2) - lib.vg_cluster_bytes(1)
HANDLE_BYTES_FIXED = lib.vg_cluster_bytes(1) - HANDLE_BYTES_PER_POINT
HANDLE_COST = f'{HANDLE_BYTES_PER_POINT} B of device memory per point + {HANDLE_BYTES_FIXED / 1e6:.0f} MB'


class GridQueries:
    """What every clustering model of this package owns and offers besides its clustering: a `vg_cluster` handle (`self._h`, for up to
    `self.max_points` points on `self.device`) and the queries on its cell grid that `EntropyScorer`, `TwoFrameClusterer` and
    `vilgod_amd.knn` call on the pipeline's model."""

    def __init__(self, max_points, device='cuda'):
        """max_points: the largest point set any call on this handle takes; the handle holds `HANDLE_COST` for it."""
        self.max_points = int(max_points)
        self.device = torch.device(device)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.vg_cluster_create(ctypes.byref(h), self.max_points), 'vg_cluster_create')
        self._h = h

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and lib is not None:
            lib.vg_cluster_destroy(h)
            self._h = None

    # ---- fixed-radius queries on the same cell grid -----------------------------------
    def grid(self, T, stream=None):
        """Build the handle's cell grid over target points T (CUDA float32 [n,>=3]); valid until the next grid()/mst()."""
        assert T.is_cuda and T.dtype == torch.float32 and (T.shape[0] == 0 or T.stride(1) == 1)
        check(lib.vg_cluster_grid(self._h, ptr(T), T.shape[0], T.stride(0) if T.shape[0] else 3, stream_ptr(stream)),
              'vg_cluster_grid')
        self._grid_ref = T                      # the kernels read the handle's own sorted copy; kept for clarity only

    def ball_count(self, Q, r2, cap, out=None, stream=None):
        """-> int32 [nq]: min(cap, #{grid points with float32 d2 < r2}) per query row of Q (CUDA float32 [nq,>=3])."""
        assert Q.is_cuda and Q.dtype == torch.float32 and (Q.shape[0] == 0 or Q.stride(1) == 1)
        nq = Q.shape[0]
        if out is None:
            out = torch.empty(nq, dtype=torch.int32, device=Q.device)
        check(lib.vg_cluster_ball_count(self._h, ptr(Q), nq, Q.stride(0) if nq else 3, float(np.float32(r2)), int(cap), ptr(out),
                                        stream_ptr(stream)), 'vg_cluster_ball_count')
        return out

    def ball_query(self, Q, r2, nsample, out=None, stream=None):
        """-> (idx int32 [nq,nsample], cnt int32 [nq]): per query row of Q (CUDA float32 [nq,>=3]) the min(hits, nsample) LOWEST rows of
        the grid's point array with float32 d2 < r2, ascending, then the first of them repeated; a row of zeros and cnt 0 for an empty
        ball and for a query that is not finite (vg_cluster_ball_query: pcdet's ball_query, one launch).  cnt equals
        ball_count(Q, r2, nsample).  out: an (idx, cnt) pair to write."""
        assert Q.is_cuda and Q.dtype == torch.float32 and (Q.shape[0] == 0 or Q.stride(1) == 1)
        nq, nsample = Q.shape[0], int(nsample)
        if out is None:
            out = (torch.empty((nq, max(nsample, 0)), dtype=torch.int32, device=Q.device),
                   torch.empty(nq, dtype=torch.int32, device=Q.device))
        idx, cnt = out
        assert idx.dtype == cnt.dtype == torch.int32 and idx.shape == (nq, nsample) and cnt.shape == (nq,)
        assert idx.is_contiguous() and cnt.is_contiguous() and idx.device == cnt.device == Q.device
        check(lib.vg_cluster_ball_query(self._h, ptr(Q), nq, Q.stride(0) if nq else 3, float(np.float32(r2)), nsample, ptr(idx), ptr(cnt),
                                        stream_ptr(stream)), 'vg_cluster_ball_query')
        return idx, cnt

    def nearest(self, Q, max_d2, stream=None):
        """-> (idx int32 [nq] row of the grid's point array or -1, d2 float32 [nq]) of the nearest grid point with
        float32 d2 <= max_d2."""
        assert Q.is_cuda and Q.dtype == torch.float32 and (Q.shape[0] == 0 or Q.stride(1) == 1)
        nq = Q.shape[0]
        idx = torch.empty(nq, dtype=torch.int32, device=Q.device)
        d2 = torch.empty(nq, dtype=torch.float32, device=Q.device)
        check(lib.vg_cluster_nearest(self._h, ptr(Q), nq, Q.stride(0) if nq else 3, float(np.float32(max_d2)), ptr(idx), ptr(d2),
                                     stream_ptr(stream)), 'vg_cluster_nearest')
        return idx, d2

    def knn(self, Q, K, max_d2=float('inf'), out=None, stream=None):
        """-> (idx int32 [nq,K] rows of the grid's point array, d2 float32 [nq,K]): per query row of Q (CUDA float32 [nq,>=3]) the K
        grid points with the smallest (float32 d2, row) among those with d2 <= max_d2, in that order; -1 / +inf where there are fewer,
        and in a whole row whose query is not finite (vg_cluster_knn: no radius limit, one launch).  out: an (idx, d2) pair to write."""
        assert Q.is_cuda and Q.dtype == torch.float32 and (Q.shape[0] == 0 or Q.stride(1) == 1)
        nq, K = Q.shape[0], int(K)
        if out is None:
            out = (torch.empty((nq, max(K, 0)), dtype=torch.int32, device=Q.device),
                   torch.empty((nq, max(K, 0)), dtype=torch.float32, device=Q.device))
        idx, d2 = out
        assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (nq, K)
        assert idx.is_contiguous() and d2.is_contiguous() and idx.device == d2.device == Q.device
        check(lib.vg_cluster_knn(self._h, ptr(Q), nq, Q.stride(0) if nq else 3, K, float(np.float32(max_d2)), ptr(idx), ptr(d2),
                                 stream_ptr(stream)), 'vg_cluster_knn')
        return idx, d2
