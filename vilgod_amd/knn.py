"""K nearest neighbours on the GPU: pytorch3d's `knn_points` call shape over vg_cluster_grid + vg_cluster_knn (csrc/cluster_knn.inc).

    from vilgod_amd.knn import knn_points                          # instead of pytorch3d.ops.knn_points
    dists, idx, _ = knn_points(p1, p2, K=4)                        # CUDA float32 [B, P1, 3], [B, P2, 3] -> [B, P1, K] squared distances, int64 rows
    from vilgod_amd.knn import knn, knn_labels, chamfer_distance   # instead of src.utils.pointcloud_utils' (numpy in, numpy out)

The reference reaches that op in src/utils/pointcloud_utils.py:476-493 (chamfer_distance), :496-503 (knn), :505-513 (knn_labels) and
through them in src/vilgod/zero_shot_detector.py:221 (K = 4 among the moving points) and :237 (the label transfer).  The distance is
the float32 d2 = fma(dz, dz, fma(dy, dy, dx * dx)) of include/vilgod_hip.h; the K results of a query are ordered by (d2, row of p2),
strictly, so equidistant points come out lowest row first whatever K is.  `knn_host` is the same pair function over all pairs on the
CPU (vg_knn_host), bit for bit.  There is no fallback from one to the other.

Padding is this project's own: -1 / +inf beyond `lengths2` or beyond K (fewer than K points in p2), and in the rows beyond `lengths1`.
pytorch3d (a CUDA extension) was not available to run beside this, so ITS padding could not be compared; a caller that relies on
padded entries must mask by `idx >= 0`.
"""
import collections
import ctypes

import numpy as np

from ._lib import lib, check, _DEFINES

KNN_MAX_K = _DEFINES['KNN_MAX_K']
# the largest K of each instantiation of the kernel (registers: 1, 4, 8; LDS: 16, KNN_MAX_K); the tests straddle them
KNN_SWITCH_K = tuple(_DEFINES[k] for k in ('KNN_K_REG1', 'KNN_K_REG4', 'KNN_K_REG8', 'KNN_K_LDS16'))

KNN = collections.namedtuple('KNN', 'dists idx knn')       # pytorch3d.ops.knn._KNN

_MIN_HANDLE_POINTS = 1 << 16
_handles = {}                                              # device index -> GridQueries


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


def _handle(device, n_targets):
    """The cached grid handle of `device`, replaced by a larger one when `n_targets` does not fit.  A full handle, of which the search
    uses the grid buffers only: `cluster_handle.HANDLE_COST` for its max_points (at least _MIN_HANDLE_POINTS, doubled when it grows)."""
    from .cluster_handle import GridQueries
    h = _handles.get(device.index)
    if h is None or h.max_points < n_targets:
        grow = 0 if h is None else 2 * h.max_points
        _handles.pop(device.index, None)                   # (the old handle's buffers go before the new ones come)
        del h
        h = _handles[device.index] = GridQueries(max(n_targets, grow, _MIN_HANDLE_POINTS), device)
    return h


def _lengths(lengths, B, P, name):
    if lengths is None:
        return [P] * B
    ls = [int(v) for v in (lengths.tolist() if hasattr(lengths, 'tolist') else lengths)]
    if len(ls) != B or any(v < 0 or v > P for v in ls):
        raise ValueError(f'{name}: {B} values in [0, {P}], got {ls}')
    return ls


def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, norm=2, version=-1, return_nn=False, return_sorted=True, model=None):
    """p1 [B, P1, 3], p2 [B, P2, 3] CUDA float32 -> KNN(dists [B, P1, K] float32 SQUARED distances, idx [B, P1, K] int64 rows of p2,
    knn [B, P1, K, 3] or None) on the current stream: per point of p1 the K nearest points of p2, ordered by (d2, row).
    lengths1 / lengths2 ([B], tensor or list): points used per batch element.  Entries beyond lengths2 or K, and rows beyond lengths1,
    are -1 / +inf (`knn`: zeros) -- see the module docstring.  `version` and `return_sorted` are accepted and change nothing: there is
    one kernel and its output is always sorted.  One vg_cluster_grid plus one vg_cluster_knn per batch element; the queries are sent
    in `entropy.spatial_order` (neighbouring lanes walk neighbouring nodes) and put back.
    model: a `GridQueries` (an `HDBSCAN`, say) whose grid handle is used (its grid is overwritten); default: one cached handle per device."""
    import torch
    from .entropy import spatial_order
    if norm != 2:
        raise NotImplementedError(f'norm: only 2 (squared euclidean distances), got {norm}')
    both = (('p1', p1), ('p2', p2))
    for name, t in both:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'{name}: a CUDA tensor (knn takes numpy arrays)')
        if t.dim() != 3:
            raise ValueError(f'{name}: [B, P, 3], got {t.dim()} dimensions')
        if t.shape[2] != 3:
            raise NotImplementedError(f'{name}: only 3 coordinates per point, got {t.shape[2]}')
    for name, t in both:
        if t.dtype != torch.float32:
            raise ValueError(f'{name}: float32, got {t.dtype}')
    for name, t in both:
        if not t.is_cuda:
            raise ValueError(f'{name}: a CUDA tensor (knn_host is the CPU form)')
    if p1.shape[0] != p2.shape[0]:
        raise ValueError(f'p2: batch size {p2.shape[0]}, p1 has {p1.shape[0]}')
    if p2.device != p1.device:
        raise ValueError(f'p2: on {p2.device}, p1 on {p1.device}')
    K = int(K)
    if not 1 <= K <= KNN_MAX_K:
        raise ValueError(f'K: 1 .. {KNN_MAX_K}, got {K}')
    B, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    l1, l2 = _lengths(lengths1, B, P1, 'lengths1'), _lengths(lengths2, B, P2, 'lengths2')
    dev = p1.device
    with torch.cuda.device(dev):
        h = model if model is not None else _handle(dev, max(l2 + [1]))
        p1, p2 = p1.contiguous(), p2.contiguous()
        dists = torch.full((B, P1, K), float('inf'), dtype=torch.float32, device=dev)
        idx = torch.full((B, P1, K), -1, dtype=torch.int64, device=dev)
        for b in range(B):
            if l1[b] == 0:
                continue
            q = p1[b, :l1[b]]
            o = spatial_order(q)
            h.grid(p2[b, :l2[b]])
            i_s, d_s = h.knn(q.index_select(0, o), K)
            dists[b, :l1[b]].index_copy_(0, o, d_s)
            idx[b, :l1[b]].index_copy_(0, o, i_s.long())
        nn = None
        if return_nn:
            ok = (idx >= 0).unsqueeze(-1)
            g = idx.clamp_min(0).reshape(B, P1 * K, 1).expand(B, P1 * K, 3)
            nn = torch.where(ok, p2.gather(1, g).reshape(B, P1, K, 3) if P2 else p2.new_zeros((B, P1, K, 3)), p2.new_zeros(()))
    return KNN(dists, idx, nn)


def _xyz(a, name):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError(f'{name}: [N, >=3], got shape {a.shape}')
    return np.ascontiguousarray(a[..., :3], dtype=np.float32)


def knn_host(source, target, K=1):
    """The search on the CPU (vg_knn_host): float32 [N, 3], [M, 3] -> (dists float32 [N, K], idx int64 [N, K]), no GPU, the kernel's
    pair function and order over all pairs, the same bits."""
    s, t = _xyz(source, 'source'), _xyz(target, 'target')
    idx = np.empty((len(s), int(K)), np.int32)
    d2 = np.empty((len(s), int(K)), np.float32)
    check(lib.vg_knn_host(_np_ptr(s), len(s), 3, _np_ptr(t), len(t), 3, int(K), float('inf'), _np_ptr(idx), _np_ptr(d2)), 'vg_knn_host')
    return d2, idx.astype(np.int64)


def knn_gpu(source, target, K=1):
    """The search on the GPU (knn_points, B = 1): the same arguments and results as `knn_host`."""
    import torch
    s, t = _xyz(source, 'source'), _xyz(target, 'target')
    dev = torch.device('cuda', torch.cuda.current_device())
    r = knn_points(torch.from_numpy(s).to(dev).unsqueeze(0), torch.from_numpy(t).to(dev).unsqueeze(0), K=K)
    return r.dists.squeeze(0).cpu().numpy(), r.idx.squeeze(0).cpu().numpy()


def _search(search, source, target, K):
    """-> (dists [1, N, K], idx [1, N, K]) as `knn_points` returns them for a batch of one"""
    s, t = _xyz(source, 'source'), _xyz(target, 'target')
    if len(t) == 0:
        raise ValueError('target: no points to search')
    d, i = search(s, t, K)
    return d[None], i[None]


def knn(points_source, points_target, K=1, search=knn_gpu):
    """pointcloud_utils.knn (:496-503): numpy [N, >=3], [M, >=3] -> (squared distances float32, rows int64), both `.squeeze()`d as
    there: [N, K], [N] for K = 1, [K] for N = 1, a 0-d array for both.  search: `knn_host` keeps the call off the GPU."""
    dists, idx = _search(search, points_source, points_target, K)
    return dists.squeeze(), idx.squeeze()


def knn_labels(points, label_points, labels, probabilities=None, dist_threshold=0.2, K=1, search=knn_gpu):
    """pointcloud_utils.knn_labels (:505-513): the labels (and probabilities) of the nearest label points; -1 where the SQUARED
    distance exceeds dist_threshold (compared in float64, as numpy compares a float32 array with a Python float).  A single point
    takes the reference's other branch: the label becomes the plain -1."""
    dists, indices = knn(points, label_points, K=K, search=search)
    point_labels = labels[indices]
    point_probabilities = probabilities[indices] if probabilities is not None else None
    if len(points) > 1:
        point_labels[dists > dist_threshold] = -1
    else:
        point_labels = -1 if dists > dist_threshold else point_labels
    return point_labels, point_probabilities


def chamfer_distance(points_1, points_2, smallest_first=True, threshold=0.2, search=knn_gpu):
    """pointcloud_utils.chamfer_distance (:476-493): the mean squared distance from each point of the smaller set (`smallest_first`)
    to its nearest in the other, and from those nearest points back, each over the pairs with d2 < threshold, averaged; float32
    means, as numpy takes them of float32 arrays (an empty selection gives nan, as there)."""
    if len(points_1) > len(points_2) and smallest_first:
        p1, p2 = points_2[..., :3], points_1[..., :3]
    else:
        p1, p2 = points_1[..., :3], points_2[..., :3]
    x_dists, x_idx = _search(search, p1, p2, 1)
    idx_p2 = x_idx.squeeze()
    y_dists, _ = _search(search, np.asarray(p2)[np.atleast_1d(idx_p2)], p1, 1)
    cham_x = x_dists[..., 0]
    cham_x = cham_x[cham_x < threshold]
    cham_y = y_dists[..., 0]
    cham_y = cham_y[cham_y < threshold]
    return (np.mean(cham_x) + np.mean(cham_y)) / 2
