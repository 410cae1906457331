"""Oriented extents of tracked clusters (csrc/oriented_extent.hip): the per-point part of the motion-aligned boxes of moving tracks,
the `else` branch of the reference's fit_bounding_boxes_simple (src/vilgod/zero_shot_detector.py:576-603).

    PseudoLabelPipeline.oriented_extents(d_X, d_index, d_seg, pair_cluster, center3, rot4)     # the kernel, CUDA in, CUDA out
    oriented_extents_host(points, index, seg, pair_cluster, center3, rot4)                    # the same per-point code on the CPU

A pair is (cluster, direction); per pair {min x', max x', min y', max y', min z, max z} in float64, with x', y' what
`np.dot(points[:, :3] - center, rot)` gives for float32 points and centre (include/vilgod_hip.h states the chain).
tracking.moving_boxes takes these extents instead of the points.  There is no fallback from one form to the other.
"""
import ctypes

import numpy as np

from ._lib import lib, check, _DEFINES

OEXT_BLOCK = _DEFINES['OEXT_BLOCK']         # threads per workgroup of the kernel, one workgroup per pair (the tests straddle it)


def moving_boxes_mode(value):
    """device.moving_boxes: 'host' or 'device' (None, an absent key = 'host'); anything else is a ValueError."""
    value = 'host' if value is None else str(value)
    if value not in ('host', 'device'):
        raise ValueError(f"device.moving_boxes: 'host' or 'device', not {value!r}")
    return value


def pair_arrays(n_clusters, pair_cluster, center3, rot4):
    """The per-pair inputs as the entry points read them -> (int32 [n_pairs] or None, float32 [n_pairs,3], float64 [n_pairs,4])."""
    center3 = np.ascontiguousarray(center3, dtype=np.float32).reshape(-1, 3)
    rot4 = np.ascontiguousarray(rot4, dtype=np.float64).reshape(-1, 4)
    if pair_cluster is not None:
        pair_cluster = np.ascontiguousarray(pair_cluster, dtype=np.int32).reshape(-1)
    n_pairs = n_clusters if pair_cluster is None else len(pair_cluster)
    if len(center3) != n_pairs or len(rot4) != n_pairs:
        raise ValueError(f'oriented_extents: {n_pairs} pairs, {len(center3)} centres, {len(rot4)} rotations')
    return pair_cluster, center3, rot4


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


def oriented_extents_host(points, index, seg, pair_cluster, center3, rot4):
    """vg_cluster_oriented_extents_host: points [N, >=3] float32 (rows of any width), packed cluster lists (index, seg), the pairs'
    clusters (None: pair p is cluster p), float32 centres [n_pairs,3], float64 rotations [n_pairs,4] -> [n_pairs,6] float64."""
    points = np.ascontiguousarray(points, dtype=np.float32)
    if points.ndim != 2:
        raise ValueError(f'oriented_extents_host: points [N, >=3], got {points.ndim} dimensions')
    index = np.ascontiguousarray(index, dtype=np.int32)
    seg = np.ascontiguousarray(seg, dtype=np.int32)
    C = len(seg) - 1
    pair_cluster, center3, rot4 = pair_arrays(C, pair_cluster, center3, rot4)
    n_pairs = len(center3)
    out = np.empty((n_pairs, 6), np.float64)
    check(lib.vg_cluster_oriented_extents_host(_np_ptr(points), points.shape[1], _np_ptr(index), _np_ptr(seg), C, _np_ptr(pair_cluster),
                                               n_pairs, _np_ptr(center3), _np_ptr(rot4), _np_ptr(out)), 'vg_cluster_oriented_extents_host')
    return out
