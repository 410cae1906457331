"""Ball query on the GPU: pcdet's stack `ball_query` call shape over vg_cluster_grid + vg_cluster_ball_query (csrc/cluster_ball_query.inc).

    from vilgod_amd.ball_query import ball_query      # instead of pcdet.ops.pointnet2.pointnet2_stack.pointnet2_utils.ball_query
    idx, empty_ball_mask = ball_query(0.3, 1000, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)     # CUDA float32 [N, 3], [M, 3]
    from vilgod_amd.ball_query import count_neighbors, count_neighbors_inter_frame     # instead of src.utils.pointcloud_utils'

The reference reaches that op in src/utils/pointcloud_utils.py:83 (count_neighbors) and :99 (count_neighbors_inter_frame).  A target is a
hit when the float32 d2 = fma(dz, dz, fma(dy, dy, dx * dx)) of include/vilgod_hip.h is below r2 = float32(radius) * float32(radius),
strictly; a query's row of `idx` holds its min(hits, nsample) LOWEST target rows, ascending -- pcdet's kernel walks the targets in row
order and keeps the first nsample hits -- then the first of them repeated; an empty ball is a row of zeros with its mask set.
`ball_query_host` is pcdet's loop itself on the CPU (vg_ball_query_host), the same bits.  There is no fallback from one to the other.
"""
import math

import numpy as np

from ._lib import lib, check, _DEFINES
from .knn import _handle, _np_ptr, _xyz

BALL_QUERY_MAX_NSAMPLE = _DEFINES['BALL_QUERY_MAX_NSAMPLE']
BALL_QUERY_CAND = _DEFINES['BALL_QUERY_CAND']              # rows a query's wave holds before it cuts back to nsample; the tests straddle it
MAX_RADIUS = 3.2                                           # 8 cells of 0.4 m, the reach limit of the grid's fixed-radius queries: radii BELOW it


def _r2(radius, limit=True):
    """float32(radius) * float32(radius), rounded to float32 -- what pcdet's kernel compares with"""
    r = np.float32(radius)
    if not r > 0:
        raise ValueError(f'radius: a positive number, got {radius!r}')
    r2 = np.float32(r * r)
    if not r2 > 0:
        raise ValueError(f'radius: its float32 square is {r2!r}, got {radius!r}')
    if limit and not math.ceil(math.sqrt(float(r2)) / 0.4) <= 8:
        raise ValueError(f'radius: below {MAX_RADIUS} m (sqrt(r2) within 8 cells of the 0.4 m grid), got {radius!r}; ball_query_host has no limit')
    return r2


def _nsample(nsample):
    n = int(nsample)
    if not 1 <= n <= BALL_QUERY_MAX_NSAMPLE:
        raise ValueError(f'nsample: 1 .. {BALL_QUERY_MAX_NSAMPLE}, got {nsample}')
    return n


def _batch_cnt(cnt, rows, name):
    ls = [int(v) for v in (cnt.tolist() if hasattr(cnt, 'tolist') else cnt)]
    if any(v < 0 for v in ls) or sum(ls) != rows:
        raise ValueError(f'{name}: counts >= 0 that sum to the {rows} rows, got {ls}')
    return ls


def ball_query(radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, model=None):
    """pcdet's stack ball_query: xyz [N1 + N2 + ..., 3] CUDA float32 (the targets of each batch element, back to back), xyz_batch_cnt
    [B] (tensor or list), new_xyz [M1 + M2 + ..., 3] (the queries), new_xyz_batch_cnt [B] -> (idx int32 [M, nsample], empty_ball_mask
    bool [M]) on the current stream.  The rows of `idx` count from the start of the query's batch element, as pcdet's do.
    One vg_cluster_grid plus one vg_cluster_ball_query per batch element.
    model: a `GridQueries` (an `HDBSCAN`, say) whose grid handle is used (its grid is overwritten); default: one cached handle per device."""
    import torch
    both = (('xyz', xyz), ('new_xyz', new_xyz))
    for name, t in both:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'{name}: a CUDA tensor (ball_query_host takes numpy arrays)')
        if t.dim() != 2:
            raise ValueError(f'{name}: [N, 3], got {t.dim()} dimensions')
        if t.shape[1] != 3:
            raise NotImplementedError(f'{name}: only 3 coordinates per point, got {t.shape[1]}')
    for name, t in both:
        if t.dtype != torch.float32:
            raise ValueError(f'{name}: float32, got {t.dtype}')
    for name, t in both:
        if not t.is_cuda:
            raise ValueError(f'{name}: a CUDA tensor (ball_query_host is the CPU form)')
    if new_xyz.device != xyz.device:
        raise ValueError(f'new_xyz: on {new_xyz.device}, xyz on {xyz.device}')
    nsample, r2 = _nsample(nsample), _r2(radius)
    nt = _batch_cnt(xyz_batch_cnt, xyz.shape[0], 'xyz_batch_cnt')
    nq = _batch_cnt(new_xyz_batch_cnt, new_xyz.shape[0], 'new_xyz_batch_cnt')
    if len(nq) != len(nt):
        raise ValueError(f'new_xyz_batch_cnt: {len(nq)} batch elements, xyz_batch_cnt has {len(nt)}')
    dev = xyz.device
    with torch.cuda.device(dev):
        h = model if model is not None else _handle(dev, max(nt + [1]))
        xyz, new_xyz = xyz.contiguous(), new_xyz.contiguous()
        idx = torch.empty((new_xyz.shape[0], nsample), dtype=torch.int32, device=dev)
        cnt = torch.empty(new_xyz.shape[0], dtype=torch.int32, device=dev)
        t0 = q0 = 0
        for n, m in zip(nt, nq):
            if m:
                h.grid(xyz[t0:t0 + n])
                h.ball_query(new_xyz[q0:q0 + m], r2, nsample, out=(idx[q0:q0 + m], cnt[q0:q0 + m]))
            t0, q0 = t0 + n, q0 + m
    return idx, cnt == 0


def ball_query_host(radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
    """The same call on the CPU (vg_ball_query_host), numpy in, numpy out: float32 [N, >=3], [M, >=3] and their batch counts -> (idx
    int32 [M, nsample], empty_ball_mask bool [M]).  No GPU, no grid: pcdet's loop over the targets in row order, the kernel's pair
    function, the same bits; no limit on the radius."""
    t, q = _xyz(xyz, 'xyz'), _xyz(new_xyz, 'new_xyz')
    nsample, r2 = _nsample(nsample), _r2(radius, limit=False)
    nt = _batch_cnt(xyz_batch_cnt, len(t), 'xyz_batch_cnt')
    nq = _batch_cnt(new_xyz_batch_cnt, len(q), 'new_xyz_batch_cnt')
    if len(nq) != len(nt):
        raise ValueError(f'new_xyz_batch_cnt: {len(nq)} batch elements, xyz_batch_cnt has {len(nt)}')
    idx = np.empty((len(q), nsample), np.int32)
    cnt = np.empty(len(q), np.int32)
    t0 = q0 = 0
    for n, m in zip(nt, nq):
        ts, qs, i_s, c_s = t[t0:t0 + n], q[q0:q0 + m], idx[q0:q0 + m], cnt[q0:q0 + m]
        check(lib.vg_ball_query_host(_np_ptr(ts), n, 3, _np_ptr(qs), m, 3, float(r2), nsample, _np_ptr(i_s), _np_ptr(c_s)), 'vg_ball_query_host')
        t0, q0 = t0 + n, q0 + m
    return idx, cnt == 0


def _device_points(a, name, dev):
    """[N, >=3] numpy array or CUDA float32 tensor -> CUDA float32 tensor [N, >=3] whose rows are read as x, y, z"""
    import torch
    if isinstance(a, torch.Tensor):
        if a.dim() != 2 or a.shape[1] < 3:
            raise ValueError(f'{name}: [N, >=3], got shape {tuple(a.shape)}')
        if a.dtype != torch.float32:
            raise ValueError(f'{name}: float32, got {a.dtype}')
        if not a.is_cuda:
            raise ValueError(f'{name}: a CUDA tensor or a numpy array, got a tensor on {a.device}')
        return a if a.stride(1) == 1 else a.contiguous()
    return torch.from_numpy(_xyz(a, name)).to(dev)


def _counts(query, targets, radius, cap, model, host):
    """[len(targets)] int64 arrays [nq]: min(cap, hits) of every query row against each target set -- over vg_cluster_ball_count, or
    (host) the cnt of vg_ball_query_host"""
    if host:
        q = _xyz(query.cpu().numpy() if hasattr(query, 'cpu') else query, 'query')
        cap, r2 = _nsample(cap), _r2(radius, limit=False)
        out = []
        for t in targets:
            t = _xyz(t.cpu().numpy() if hasattr(t, 'cpu') else t, 'targets')
            idx, cnt = np.empty((len(q), cap), np.int32), np.empty(len(q), np.int32)
            check(lib.vg_ball_query_host(_np_ptr(t), len(t), 3, _np_ptr(q), len(q), 3, float(r2), cap, _np_ptr(idx), _np_ptr(cnt)), 'vg_ball_query_host')
            out.append(cnt.astype(np.int64))
        return out
    import torch
    cap, r2 = _nsample(cap), _r2(radius)
    first = next((a for a in [query] + list(targets) if isinstance(a, torch.Tensor) and a.is_cuda), None)
    dev = first.device if first is not None else torch.device('cuda', torch.cuda.current_device())
    with torch.cuda.device(dev):
        q = _device_points(query, 'query', dev)
        ts = [_device_points(t, 'targets', dev) for t in targets]
        h = model if model is not None else _handle(dev, max([len(t) for t in ts] + [1]))
        out = []
        for t in ts:
            h.grid(t)
            out.append(h.ball_count(q, r2, cap))
        out = [c.cpu().numpy().astype(np.int64) for c in out]
    return out


def count_neighbors(pts_buffer, seek=0, skip_frames=1, max_neighbor_point_dist=0.3, max_neighbor_points=1000, model=None, host=False, **kwargs):
    """pointcloud_utils.count_neighbors (:74-94): pts_buffer, a list of frames (numpy arrays or CUDA float32 tensors [n_f, >=3]) ->
    numpy int64 [len(pts_buffer[seek]), frames used]: per point of frame `seek` and per every (skip_frames + 1)-th frame the number
    of that frame's points within max_neighbor_point_dist, at most max_neighbor_points; 1 is subtracted in the column of frame
    `seek` itself.  Further keyword arguments are accepted and ignored, as there.  model: as for `ball_query`.  host=True keeps the
    call off the GPU (the cnt of vg_ball_query_host: the same numbers).
    The reference derives the count from ball_query's index table (count_nonzero(idx != idx[:, :1]) + 1 on non-empty rows).  This
    runs over vg_cluster_ball_count instead, NOT over the index table: the count is cnt of ball_query by definition, and at 79k
    queries x 1000 samples that table is 316 MB per column of which the count needs nothing."""
    used = list(range(len(pts_buffer)))[::skip_frames + 1]
    cols = _counts(pts_buffer[seek], [pts_buffer[i] for i in used], max_neighbor_point_dist, max_neighbor_points, model, host)
    return np.stack([c - 1 if i == seek else c for i, c in zip(used, cols)]).T


def count_neighbors_inter_frame(points, max_neighbor_point_dist=0.1, max_neighbor_points=100, model=None, host=False):
    """pointcloud_utils.count_neighbors_inter_frame (:97-104): points (numpy array or CUDA float32 tensor [n, >=3]) -> numpy int64 [n]:
    the number of points within max_neighbor_point_dist of each point, itself included, at most max_neighbor_points.  Over
    vg_cluster_ball_count, not over the index table, as `count_neighbors`."""
    return _counts(points, [points], max_neighbor_point_dist, max_neighbor_points, model, host)[0]
