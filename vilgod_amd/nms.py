"""Rotated-box NMS on the GPU: pcdet's `nms_gpu` / `nms_normal_gpu` call shape over vg_boxes_nms (csrc/nms.hip).

    from vilgod_amd.nms import nms_gpu                 # instead of pcdet.ops.iou3d_nms.iou3d_nms_utils.nms_gpu
    keep, _ = nms_gpu(boxes, scores, thresh=0.1)       # CUDA tensors [N, >=7], [N] -> int64 indices into boxes, best first

The reference imports that module in src/utils/tracking_utils.py:6, src/vilgod/zero_shot_detector.py:17 and
src/datasets/waymo_dataset.py:3.  Boxes are [x, y, z, dx, dy, dz, heading]; the arithmetic is float64 whatever the input dtype.

The rules (include/vilgod_hip.h has them in full): rows are ranked by (score descending, row index ascending); a row with a NaN
score or a non-finite x, y, dx, dy or heading is never kept and suppresses nothing; with `pre_maxsize` only the first that many
ranked rows take part; a row is kept iff no earlier-kept row p has v(row, p) > thresh, strictly, where v is the BEV IoU of
`boxes_iou_bev` ('rotated') or the axis-aligned BEV IoU with the headings ignored ('normal'), the later row as `a`.

`nms_groups` runs many independent passes in one call (one per frame and class) and leaves everything on the device without a
synchronisation; `nms_groups_host` is the same per-pair code on the CPU (vg_boxes_nms_host), bit for bit.  There is no fallback from
one to the other.  A group holds at most MAX_GROUP rows.
"""
import ctypes

import numpy as np

from ._lib import lib, check, ptr, stream_ptr, _DEFINES

MODE_ROTATED, MODE_NORMAL = _DEFINES['NMS_ROTATED'], _DEFINES['NMS_NORMAL']
MAX_GROUP = _DEFINES['NMS_MAX_GROUP']
_F32, _F64 = _DEFINES['NMS_F32'], _DEFINES['NMS_F64']
_MODES = {'rotated': MODE_ROTATED, 'normal': MODE_NORMAL}


def _mode(mode):
    if mode not in _MODES:
        raise ValueError(f"mode: 'rotated' or 'normal', got {mode!r}")
    return _MODES[mode]


def _pre_max(pre_maxsize):
    if pre_maxsize is None:
        return 0
    if int(pre_maxsize) != pre_maxsize or pre_maxsize < 1:
        raise ValueError(f'pre_maxsize: None or a positive integer, got {pre_maxsize!r}')
    return int(min(pre_maxsize, 2 ** 31 - 1))


def _offsets(off, n_rows):
    """-> (off as contiguous int32 [G + 1], the largest group): non-decreasing, inside [0, n_rows], no group above MAX_GROUP"""
    off = np.asarray(off)
    if off.ndim != 1 or len(off) < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError('off: a 1-D integer sequence of G + 1 entries')
    off = off.astype(np.int64)
    sizes = np.diff(off)
    if off[0] < 0 or off[-1] > n_rows or np.any(sizes < 0):
        raise ValueError(f'off: must be non-decreasing inside [0, {n_rows}]')
    largest = int(sizes.max()) if len(sizes) else 0
    if largest > MAX_GROUP:
        raise ValueError(f'off: a group of {largest} rows, the largest a call takes is {MAX_GROUP}')
    return np.ascontiguousarray(off, np.int32), largest


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def nms_groups_host(boxes, scores, off, thresh, mode='rotated', pre_maxsize=None):
    """numpy boxes [N, >=7] and scores [N] (each float32 or float64) with group offsets [G + 1] -> (keep int32 [N]: group g's kept
    rows as indices into boxes, best first, from off[g], then -1; slots outside every group are -1 too, counts int32 [G]) through
    the host entry point.  No GPU needed."""
    boxes, scores = np.asarray(boxes), np.asarray(scores)
    if boxes.ndim != 2 or boxes.shape[1] < 7:
        raise ValueError(f'boxes: [N, >=7], got shape {boxes.shape}')
    if scores.shape != (len(boxes),):
        raise ValueError(f'scores: [{len(boxes)}], got shape {scores.shape}')
    m, pre = _mode(mode), _pre_max(pre_maxsize)
    off, largest = _offsets(off, len(boxes))
    boxes = np.ascontiguousarray(boxes[:, :7], np.float32 if boxes.dtype == np.float32 else np.float64)
    scores = np.ascontiguousarray(scores, np.float32 if scores.dtype == np.float32 else np.float64)
    keep, counts = np.full(len(boxes), -1, np.int32), np.zeros(len(off) - 1, np.int32)
    check(lib.vg_boxes_nms_host(_F32 if boxes.dtype == np.float32 else _F64, _np_ptr(boxes), _F32 if scores.dtype == np.float32 else _F64,
                                _np_ptr(scores), _np_ptr(off), len(off) - 1, len(boxes), largest, m, float(thresh), pre, _np_ptr(keep),
                                _np_ptr(counts)), 'vg_boxes_nms_host')
    return keep, counts


def nms_groups(boxes, scores, off, thresh, mode='rotated', pre_maxsize=None, stream=None, max_group=None):
    """CUDA tensors boxes [N, >=7] and scores [N] (each float32 or float64) with group offsets [G + 1] -> (keep int32 [N], counts
    int32 [G]) as nms_groups_host gives them, both on the device, with no synchronisation: three launches on `stream` (a torch stream on
    which the inputs are ready; default: the current one).
    off: an integer sequence, checked here and uploaded; or an int32 CUDA tensor with `max_group`, the caller's bound on any group's
    size -- nothing is then copied in either direction (the call can be captured into a graph), and a group the table describes
    wrongly comes back with count -1 and -1 in its rows."""
    import torch
    if not (boxes.is_cuda and scores.is_cuda):
        raise ValueError('boxes and scores must be CUDA tensors (nms_groups_host is the CPU form)')
    if boxes.dtype not in (torch.float32, torch.float64) or boxes.dim() != 2 or boxes.shape[1] < 7:
        raise ValueError(f'boxes: [N, >=7] float32 or float64, got {tuple(boxes.shape)} {boxes.dtype}')
    if scores.dtype not in (torch.float32, torch.float64) or scores.shape != (boxes.shape[0],):
        raise ValueError(f'scores: [{boxes.shape[0]}] float32 or float64, got {tuple(scores.shape)} {scores.dtype}')
    m, pre = _mode(mode), _pre_max(pre_maxsize)
    n, dev = boxes.shape[0], boxes.device
    on_device = torch.is_tensor(off) and off.is_cuda
    if on_device:
        if off.dtype != torch.int32 or off.dim() != 1 or off.numel() < 1 or not off.is_contiguous():
            raise ValueError('off: a device table is a contiguous 1-D int32 tensor of G + 1 entries')
        if max_group is None or not 0 <= int(max_group) <= MAX_GROUP:
            raise ValueError(f'max_group: 0 .. {MAX_GROUP}, required with a device table, got {max_group!r}')
        largest = int(max_group)
    else:
        off, largest = _offsets(off.cpu().numpy() if torch.is_tensor(off) else off, n)
        if max_group is not None:
            if not largest <= int(max_group) <= MAX_GROUP:
                raise ValueError(f'max_group: {largest} .. {MAX_GROUP} for this table, got {max_group!r}')
            largest = int(max_group)
    groups = len(off) - 1
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(stream):          # the copies and the fills go to the launches' stream
        boxes, scores = boxes[:, :7].contiguous(), scores.contiguous()
        d_off = off if on_device else torch.from_numpy(off).to(dev)
        keep = torch.full((n,), -1, dtype=torch.int32, device=dev)
        counts = torch.zeros(groups, dtype=torch.int32, device=dev)
        work = torch.empty(int(lib.vg_boxes_nms_work_bytes(n, largest, groups)), dtype=torch.uint8, device=dev)
        check(lib.vg_boxes_nms(_F32 if boxes.dtype == torch.float32 else _F64, ptr(boxes), _F32 if scores.dtype == torch.float32 else _F64,
                               ptr(scores), ptr(d_off), groups, n, largest, m, float(thresh), pre, ptr(work), ptr(keep), ptr(counts),
                               stream_ptr(stream)), 'vg_boxes_nms')
    return keep, counts


def _single(boxes, scores, thresh, pre_maxsize, mode):
    import torch
    if boxes.shape[0] > MAX_GROUP:
        raise ValueError(f'boxes: {boxes.shape[0]} rows, the largest a call takes is {MAX_GROUP} (cut them by score first)')
    if boxes.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64, device=boxes.device), None
    keep, counts = nms_groups(boxes, scores, [0, boxes.shape[0]], thresh, mode, pre_maxsize)
    return keep[:int(counts[0])].long(), None                         # the one read-back: the count


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """[N, >=7] boxes and [N] scores, CUDA tensors -> (int64 indices into boxes of the kept rows, best first, None): pcdet's nms_gpu.
    Only the first 7 columns of boxes are read."""
    return _single(boxes, scores, thresh, pre_maxsize, 'rotated')


def nms_normal_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """... with the headings ignored (axis-aligned BEV boxes): pcdet's nms_normal_gpu."""
    return _single(boxes, scores, thresh, pre_maxsize, 'normal')
