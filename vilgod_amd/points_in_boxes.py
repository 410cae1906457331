"""Points in boxes on the GPU: pcdet's `points_in_boxes_gpu` call shape over vg_points_in_boxes (csrc/points_in_boxes.hip).

    from vilgod_amd.points_in_boxes import points_in_boxes_gpu    # instead of pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils.points_in_boxes_gpu
    idx = points_in_boxes_gpu(points, boxes)                      # CUDA tensors [B, N, >=3], [B, M, >=7] -> [B, N] int32
    from vilgod_amd.points_in_boxes import points_in_boxes, get_box_heights     # instead of src.utils.pointcloud_utils' (numpy in, numpy out)

The reference reaches that op in src/utils/pointcloud_utils.py:144-158 (get_box_heights) and :516-522 (points_in_boxes), and through
the latter in src/vilgod/lidar_frame.py:154-161 (detections out of box proposals).  A box is [cx, cy, cz, dx, dy, dz, rz]; a point
gets the LOWEST index of a box that contains it, -1 when none does; the rule is spelled out in include/vilgod_hip.h, the arithmetic
is float64 whatever the input dtype.  `points_in_boxes_host` is the same per-pair code on the CPU (vg_points_in_boxes_host), bit for
bit.  There is no fallback from one to the other.
"""
import ctypes

import numpy as np

from ._lib import lib, check, ptr, stream_ptr, _DEFINES

_F32, _F64 = _DEFINES['PIB_F32'], _DEFINES['PIB_F64']
PIB_CHUNK = _DEFINES['PIB_CHUNK']           # boxes per LDS chunk of the kernel (the tests straddle it)


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


def _check_shape(shape, rank, cols, name, what):
    if len(shape) != rank:
        raise ValueError(f'{name}: {what}, got {len(shape)} dimensions')
    if shape[-1] < cols:
        raise ValueError(f'{name}: {what}, got {shape[-1]} columns')


def points_in_boxes_gpu(points, boxes):
    """points [B, N, >=3] CUDA float32, boxes [B, M, >=7] CUDA float32 or float64 -> [B, N] CUDA int32 on the current stream: per point
    the lowest index (inside its batch element) of a box that contains it, -1 for none.  The first three / seven columns are read; a
    non-contiguous view is made contiguous.  One launch, nothing read back."""
    import torch
    for name, t in (('points', points), ('boxes', boxes)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'{name}: a CUDA tensor (points_in_boxes takes numpy arrays)')
    _check_shape(points.shape, 3, 3, 'points', '[B, N, >=3]')
    _check_shape(boxes.shape, 3, 7, 'boxes', '[B, M, >=7]')
    if points.shape[0] != boxes.shape[0]:
        raise ValueError(f'boxes: batch size {boxes.shape[0]}, points have {points.shape[0]}')
    if points.dtype != torch.float32:
        raise ValueError(f'points: float32, got {points.dtype}')
    if boxes.dtype not in (torch.float32, torch.float64):
        raise ValueError(f'boxes: float32 or float64, got {boxes.dtype}')
    if not points.is_cuda:
        raise ValueError('points: a CUDA tensor (points_in_boxes_host is the CPU form)')
    if not boxes.is_cuda:
        raise ValueError('boxes: a CUDA tensor (points_in_boxes_host is the CPU form)')
    if boxes.device != points.device:
        raise ValueError(f'boxes: on {boxes.device}, points on {points.device}')
    B, N, M = points.shape[0], points.shape[1], boxes.shape[1]
    with torch.cuda.device(points.device):
        points = points.contiguous()                       # (all columns stay: the kernel steps over them by the row stride)
        boxes = boxes[:, :, :7].contiguous()
        out = torch.empty((B, N), dtype=torch.int32, device=points.device)
        check(lib.vg_points_in_boxes(_F32 if boxes.dtype == torch.float32 else _F64, ptr(points), points.shape[2], N, ptr(boxes), M, B,
                                     ptr(out), stream_ptr()), 'vg_points_in_boxes')
    return out


def _host_arrays(points, boxes):
    """-> (float32 [N, C] points, float32 [M, 7] boxes) as pointcloud_utils.py:518-520 casts them (`.float()` on both)"""
    points, boxes = np.asarray(points), np.asarray(boxes)
    _check_shape(points.shape, 2, 3, 'points', '[N, >=3]')
    _check_shape(boxes.shape, 2, 7, 'boxes', '[M, >=7]')
    return np.ascontiguousarray(points[:, :3], dtype=np.float32), np.ascontiguousarray(boxes[:, :7], dtype=np.float32)


def points_in_boxes_host(points, boxes):
    """`points_in_boxes` through the host entry point (vg_points_in_boxes_host): no GPU, the kernel's per-pair code, the same bits."""
    p, b = _host_arrays(points, boxes)
    out = np.empty(len(p), np.int32)
    check(lib.vg_points_in_boxes_host(_F32, _np_ptr(p), 3, len(p), _np_ptr(b), len(b), 1, _np_ptr(out)), 'vg_points_in_boxes_host')
    return out.astype(np.int64)


def points_in_boxes(points, boxes):
    """pointcloud_utils.points_in_boxes (:516-522): numpy points [N, >=3] and boxes [M, >=7] (both cast to float32 as there) -> numpy
    int64 [N], the box index per point from the GPU."""
    import torch
    p, b = _host_arrays(points, boxes)
    dev = torch.device('cuda', torch.cuda.current_device())
    idx = points_in_boxes_gpu(torch.from_numpy(p).unsqueeze(0).to(dev), torch.from_numpy(b).unsqueeze(0).to(dev))
    return idx.long().squeeze(0).cpu().numpy()


def get_box_heights(points, boxes, membership=points_in_boxes):
    """pointcloud_utils.get_box_heights (:144-158): a copy of `boxes` in which every box that owns a point has its z centre and height
    set to the extent of ITS points (first-hit membership, from the GPU); the z minimum / maximum are taken from the caller's array in
    its dtype, on the host, as there.  Boxes without points are unchanged.  membership: the function that assigns the points
    (`points_in_boxes_host` keeps the call off the GPU)."""
    points, boxes = np.asarray(points), np.asarray(boxes)
    out = boxes.copy()
    idx = membership(points, boxes)
    z = points[:, 2]
    for i in np.unique(idx[idx >= 0]):                     # the boxes that own a point
        zi = z[idx == i]
        lo, hi = zi.min(), zi.max()                        # scalars of the points' dtype: the arithmetic below runs in it
        out[i, 2], out[i, 5] = lo + (hi - lo) / 2, hi - lo
    return out
