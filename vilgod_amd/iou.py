"""Rotated-box IoU on the GPU: pcdet's `boxes_iou3d_gpu` / `boxes_iou_bev` call shape over vg_boxes_iou3d (csrc/iou.hip).

    from vilgod_amd.iou import boxes_iou3d            # instead of pcdet.ops.iou3d_nms.iou3d_nms_utils.boxes_iou3d_gpu
    iou = boxes_iou3d(boxes_a, boxes_b)                # CUDA tensors [N, >=7], [M, >=7] -> [N, M] in the input dtype

The reference reaches that op in src/utils/tracking_utils.py:9-20, src/vilgod/zero_shot_detector.py:737-739 and
src/datasets/waymo_dataset.py:300.  Boxes are [x, y, z, dx, dy, dz, heading]; the arithmetic is float64 whatever the input dtype.
`iou_groups` runs many independent matrices in one launch (the evaluation: one per frame and object type); `iou_groups_host` is the
same per-pair code on the CPU (vg_boxes_iou3d_host), bit for bit.  There is no fallback from one to the other.
"""
import ctypes

import numpy as np

from ._lib import lib, check, ptr, stream_ptr, _DEFINES

MODE_3D, MODE_BEV, MODE_BEV_AREA = _DEFINES['IOU_3D'], _DEFINES['IOU_BEV'], _DEFINES['IOU_BEV_AREA']
_F32, _F64 = _DEFINES['IOU_F32'], _DEFINES['IOU_F64']


def group_out_offsets(a_off, b_off):
    """-> (out_off [G] int64, total): the groups' [na_g, nb_g] matrices packed one behind the other."""
    a_off, b_off = np.asarray(a_off, np.int64), np.asarray(b_off, np.int64)
    if a_off.ndim != 1 or a_off.shape != b_off.shape or len(a_off) < 1:
        raise ValueError('a_off and b_off must be 1-D, of equal length G + 1')
    sizes = np.diff(a_off) * np.diff(b_off)
    ends = np.cumsum(sizes)
    return (ends - sizes).astype(np.int64), int(ends[-1]) if len(ends) else 0


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def iou_groups_host(a, a_off, b, b_off, mode=MODE_3D):
    """numpy [Na, >=7], [Nb, >=7] (float32 or float64, one dtype) with group offsets [G+1] -> (flat float64 result, out_off [G])
    through the host entry point: group g's row-major [na_g, nb_g] matrix starts at out_off[g]."""
    a, b = np.asarray(a), np.asarray(b)
    dt = np.float32 if a.dtype == np.float32 and b.dtype == np.float32 else np.float64
    a = np.ascontiguousarray(a.reshape(-1, a.shape[-1] if a.ndim == 2 else 7)[:, :7], dt)
    b = np.ascontiguousarray(b.reshape(-1, b.shape[-1] if b.ndim == 2 else 7)[:, :7], dt)
    out_off, total = group_out_offsets(a_off, b_off)
    a_off, b_off = np.ascontiguousarray(a_off, np.int32), np.ascontiguousarray(b_off, np.int32)
    if a_off[-1] > len(a) or b_off[-1] > len(b):
        raise ValueError('group offsets reach past the boxes')
    out = np.zeros(total, np.float64)
    check(lib.vg_boxes_iou3d_host(_F32 if dt == np.float32 else _F64, _np_ptr(a), _np_ptr(a_off), _np_ptr(b), _np_ptr(b_off),
                                  len(a_off) - 1, _np_ptr(out_off), int(mode), _np_ptr(out)), 'vg_boxes_iou3d_host')
    return out, out_off


def iou_groups(a, a_off, b, b_off, mode=MODE_3D, stream=None):
    """CUDA tensors [Na, >=7], [Nb, >=7] (float32 or float64, one dtype) with group offsets [G+1] (any integer sequence) ->
    (flat float64 CUDA tensor, out_off [G] numpy int64) in ONE launch: group g's row-major [na_g, nb_g] matrix starts at out_off[g].
    `stream`: a torch stream on which the boxes are ready (default: the current one)."""
    import torch
    if not (a.is_cuda and b.is_cuda):
        raise ValueError('iou_groups takes CUDA tensors (iou_groups_host is the CPU form)')
    if a.dtype != b.dtype or a.dtype not in (torch.float32, torch.float64):
        raise ValueError(f'boxes must share one dtype, float32 or float64 (got {a.dtype}, {b.dtype})')
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] < 7 or b.shape[1] < 7:
        raise ValueError('boxes must be [N, >=7]')
    out_off, total = group_out_offsets(a_off, b_off)
    a_off, b_off = np.ascontiguousarray(a_off, np.int32), np.ascontiguousarray(b_off, np.int32)
    if a_off[-1] > len(a) or b_off[-1] > len(b):
        raise ValueError('group offsets reach past the boxes')
    dev = a.device
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(stream):          # the copies and the result's zero fill go to the launch's stream
        a, b = a[:, :7].contiguous(), b[:, :7].contiguous()
        d_a_off, d_b_off = torch.from_numpy(a_off).to(dev), torch.from_numpy(b_off).to(dev)
        d_out_off = torch.from_numpy(out_off).to(dev)
        out = torch.zeros(total, dtype=torch.float64, device=dev)
        check(lib.vg_boxes_iou3d(_F32 if a.dtype == torch.float32 else _F64, ptr(a), ptr(d_a_off), ptr(b), ptr(d_b_off), len(a_off) - 1,
                                 ptr(d_out_off), int(mode), ptr(out), stream_ptr(stream)), 'vg_boxes_iou3d')
    return out, out_off


def _matrix(a, b, mode):
    out, _ = iou_groups(a, [0, a.shape[0]], b, [0, b.shape[0]], mode)
    return out.reshape(a.shape[0], b.shape[0]).to(a.dtype)


def boxes_iou3d(boxes_a, boxes_b):
    """[N, >=7], [M, >=7] CUDA tensors -> [N, M] 3-D IoU in the input dtype (pcdet's boxes_iou3d_gpu)."""
    return _matrix(boxes_a, boxes_b, MODE_3D)


def boxes_iou_bev(boxes_a, boxes_b):
    """[N, >=7], [M, >=7] CUDA tensors -> [N, M] bird's-eye-view IoU in the input dtype (pcdet's boxes_iou_bev)."""
    return _matrix(boxes_a, boxes_b, MODE_BEV)
