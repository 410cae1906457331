"""Per-frame state as structure-of-arrays, materialised into the reference's dict layout only when a
pickle is written (SURVEY §8a row T1, §8b "Output 1").

Mirrors what `LidarFrame` (src/vilgod/lidar_frame.py:15-59, 124-147) and `Detection`
(src/dataclass/objects.py:37-103, 136-142) hold and serialise:
  frame dict keys   `_detections`, `_ground_point_indices`, `_entropy_scores`, `_entropy_indices`, `_gt_cluster_mapping`
  detection keys    `cluster_id`, `_bounding_box`, `valid`, `static`, `gt_assigned`, `cluster_points_index`,
                    `object_class_predictions`, `tid`, `static_track`, `object_class_predictions_detailed`,
                    `object_class_predictions_score`, `object_class`, `object_class_score`
                    (a key is present only when its value is not None -- objects.py:95-100)
"""
import numpy as np

INDEX_WO_GROUND, INDEX_ALL_POINTS = 'points_ref_wo_ground', 'points_ref'      # FrameState.index_space

DETECTION_FIELDS = ['cluster_id', '_bounding_box', 'valid', 'static', 'gt_assigned', 'cluster_points_index',
                    'object_class_predictions', 'tid', 'static_track', 'object_class_predictions_detailed',
                    'object_class_predictions_score', 'object_class', 'object_class_score']       # objects.py:90-93


def pack_clusters(labels, probs, threshold):
    """lidar_frame.py:163-167, 230-237 as arrays: labels of low-probability points -> -1; clusters in ascending
    label order; each cluster's point indices ascending.  Returns (cluster_ids, packed index int32, seg_off int32).
    One counting sort on the host (csrc/hdbscan_tree.cpp vg_pack_clusters_host): the numpy form below -- a stable argsort of ~80k labels --
    was 2 ms of a frame's 12.6 ms front-stage latency (round 5)."""
    import ctypes
    from ._lib import lib, check
    labels = np.asarray(labels)
    if labels.size and (int(labels.max()) > np.iinfo(np.int32).max or int(labels.min()) < np.iinfo(np.int32).min):
        return pack_clusters_numpy(labels, probs, threshold)        # (labels beyond int32 would wrap in the cast below)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    n = len(labels)
    pr = None if probs is None else np.ascontiguousarray(probs, dtype=np.float64)
    ids = np.empty(n, np.int64)
    index = np.empty(n, np.int32)
    seg = np.empty(n + 1, np.int32)
    nc = ctypes.c_int32(0)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    check(lib.vg_pack_clusters_host(p(labels), p(pr), n, float(threshold), p(ids), p(index), p(seg), ctypes.byref(nc)),
          'vg_pack_clusters_host')
    c = nc.value
    return ids[:c].copy(), index[:int(seg[c])].copy(), seg[:c + 1].copy()


def pack_clusters_numpy(labels, probs, threshold):
    """The same grouping in numpy (what `pack_clusters` computed before round 5; tests compare the two)."""
    labels = np.asarray(labels).copy()
    if probs is not None:
        labels[np.asarray(probs) < threshold] = -1
    keep = np.flatnonzero(labels >= 0)
    if keep.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(1, np.int32)
    order = keep[np.argsort(labels[keep], kind='stable')]          # ascending label, then ascending index
    sl = labels[order]
    starts = np.flatnonzero(np.r_[True, sl[1:] != sl[:-1]])
    seg = np.r_[starts, len(order)].astype(np.int32)
    return sl[starts].astype(np.int64), order.astype(np.int32), seg


PACK_MAX_LABEL_BOUND = 1 << 24      # include/vilgod_hip.h vg_pack_clusters: label_bound and n go up to 2^24
_PACK_WORK = {}                     # (device, stream) -> work buffer of pack_clusters_device / select_clusters_device callers without their own


def _pack_work(nbytes, device, work):
    """A work buffer of at least nbytes: the caller's, or one kept per (device, current stream) -- calls on one stream are ordered."""
    import torch
    if work is not None:
        if work.numel() * work.element_size() < nbytes:
            raise ValueError(f'work buffer: {work.numel() * work.element_size()} bytes, {nbytes} needed')
        return work
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    w = _PACK_WORK.get(key)
    if w is None or w.numel() < nbytes:
        w = _PACK_WORK[key] = torch.empty(max(int(nbytes), 1 << 16), dtype=torch.uint8, device=device)
    return w


def pack_clusters_device(d_labels, d_probs, threshold, label_bound=None, work=None, out=None):
    """`pack_clusters` on the device (csrc/pack.hip vg_pack_clusters): d_labels CUDA int32 [n], d_probs CUDA float64 [n] or None.
    label_bound: exclusive upper bound of the labels (default n: a partition of n points has at most n parts).
    -> (ids int64 [n], index int32 [n], seg int32 [n + 1], counts int32 [3]) CUDA tensors, queued on the current stream, nothing waited
    for.  counts = (C, P, overflow); the lists are ids[:C], index[:P], seg[:C + 1], the rest is not written; overflow != 0: a label was
    >= label_bound and the lists must not be used.  work: uint8 CUDA scratch of vg_pack_clusters_work_bytes(n) bytes (default: one kept
    per stream); out: (ids, index, seg, counts) tensors to write into."""
    import torch
    from ._lib import lib, check, ptr, stream_ptr
    if not (d_labels.is_cuda and d_labels.dtype == torch.int32 and d_labels.dim() == 1 and d_labels.is_contiguous()):
        raise ValueError('d_labels: contiguous CUDA int32 [n]')
    n = d_labels.numel()
    if d_probs is not None and not (d_probs.is_cuda and d_probs.dtype == torch.float64 and d_probs.is_contiguous() and d_probs.numel() == n):
        raise ValueError('d_probs: contiguous CUDA float64 [n]')
    dev = d_labels.device
    bound = n if label_bound is None else int(label_bound)
    nbytes = lib.vg_pack_clusters_work_bytes(n)
    if nbytes < 0:
        raise ValueError(f'vg_pack_clusters: {n} points (at most {PACK_MAX_LABEL_BOUND})')
    work = _pack_work(nbytes, dev, work)
    if out is None:
        out = (torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(n + 1, dtype=torch.int32, device=dev), torch.empty(3, dtype=torch.int32, device=dev))
    ids, index, seg, counts = out
    check(lib.vg_pack_clusters(ptr(d_labels), ptr(d_probs), n, float(threshold), bound, ptr(work), work.numel(), ptr(ids), ptr(index),
                               ptr(seg), ptr(counts), stream_ptr()), 'vg_pack_clusters')
    return ids, index, seg, counts


def select_clusters_device(d_index, d_seg, n_clusters, d_valid, n_index=None, work=None, out=None):
    """The packed sub-lists of the clusters with d_valid[c] != 0 (csrc/pack.hip vg_pack_select): d_index CUDA int32, d_seg CUDA int32
    [>= n_clusters + 1], d_valid CUDA uint8 [n_clusters] as the filter kernels write it.  n_index: entries of d_index (default: its
    length).  -> (out_index int32 [n_index], out_seg int32 [n_clusters + 1], counts int32 [2] = kept clusters K, kept points Q) CUDA
    tensors, queued on the current stream; only out_index[:Q] and out_seg[:K + 1] are written."""
    import torch
    from ._lib import lib, check, ptr, stream_ptr
    C = int(n_clusters)
    n_index = d_index.numel() if n_index is None else int(n_index)
    if not (d_index.is_cuda and d_index.dtype == torch.int32 and d_index.is_contiguous() and d_index.numel() >= n_index):
        raise ValueError('d_index: contiguous CUDA int32 [>= n_index]')
    if not (d_seg.is_cuda and d_seg.dtype == torch.int32 and d_seg.is_contiguous() and d_seg.numel() >= C + 1):
        raise ValueError('d_seg: contiguous CUDA int32 [>= n_clusters + 1]')
    if not (d_valid.is_cuda and d_valid.dtype == torch.uint8 and d_valid.is_contiguous() and d_valid.numel() >= C):
        raise ValueError('d_valid: contiguous CUDA uint8 [n_clusters]')
    dev = d_index.device
    work = _pack_work(lib.vg_pack_select_work_bytes(C), dev, work)
    if out is None:
        out = (torch.empty(n_index, dtype=torch.int32, device=dev), torch.empty(C + 1, dtype=torch.int32, device=dev),
               torch.empty(2, dtype=torch.int32, device=dev))
    o_index, o_seg, counts = out
    check(lib.vg_pack_select(ptr(d_index), ptr(d_seg), C, n_index, ptr(d_valid), ptr(work), work.numel(), ptr(o_index), ptr(o_seg),
                             ptr(counts), stream_ptr()), 'vg_pack_select')
    return o_index, o_seg, counts


def sublist_offsets(seg_off, rows):
    """Offsets int32 [len(rows) + 1] of the packed lists of the clusters `rows` alone (any order; no rows: [0])."""
    rows = np.asarray(rows, dtype=np.int64)
    return np.r_[0, np.cumsum(seg_off[rows + 1] - seg_off[rows])].astype(np.int32)


def cluster_sublists(index, seg_off, rows):
    """The packed lists of the clusters `rows` alone, in the order of `rows` (empty clusters allowed) -> (index int32, seg int32)."""
    parts = [index[seg_off[c]:seg_off[c + 1]] for c in rows]
    sub = np.concatenate(parts) if parts else np.zeros(0, np.int32)
    return np.ascontiguousarray(sub, dtype=np.int32), sublist_offsets(seg_off, rows)


def select_rows_device(d_index, d_seg, n_clusters, seg, keep):
    """`cluster_sublists` cut on the device from the lists held there (select_clusters_device).  keep: the clusters as STRICTLY INCREASING
    host rows, or as the CUDA uint8 [n_clusters] verdict a filter kernel left on the device (no upload then).  seg: their
    `sublist_offsets` on the host: it sizes what the kernel writes, so nothing is read back.  -> (d_index, d_seg [len(seg)]) CUDA int32."""
    import torch
    if not isinstance(keep, torch.Tensor):
        keep = torch.from_numpy(np.isin(np.arange(n_clusters), keep).astype(np.uint8)).to(d_index.device)
    o_index, o_seg, _ = select_clusters_device(d_index, d_seg, n_clusters, keep)
    return o_index[:int(seg[-1])], o_seg[:len(seg)]


def vote(class_ids, scores, class_names_sorted):
    """LidarFrame.update_object_classes (lidar_frame.py:269-285) for all detections at once.
    class_ids: [C,V] indices into `class_names_sorted` (ALPHABETICAL order = np.unique order); scores [C,V] float32.  V counts every
    entry of a detection: views x clip.top_k, view-major (what `cls_result_list.reshape((length, -1))` gives upstream).
    Returns (winner index [C], score [C] float32).
      no tie for the highest count -> that name (first in alphabetical order), mean score of its views
      tie -> the name with the highest mean score among ALL names present, scanned alphabetically with `>`
             (max_score starts at 0).
    A name's mean is numpy's float32 np.mean of its entries in column order.  Below 8 entries that is the sequential sum formed
    here for all rows at once; from 8 entries on numpy adds pairwise (eight accumulators, then the remainder), which no longer is
    the sequential sum: those (row, name) pairs -- none unless V >= 8 -- get np.mean of the selection itself."""
    C, V = class_ids.shape
    K = len(class_names_sorted)
    counts = np.zeros((C, K), np.int64)
    sums = np.zeros((C, K), np.float32)
    for v in range(V):                                    # sequential float32 accumulation like np.mean on <8 items
        np.add.at(counts, (np.arange(C), class_ids[:, v]), 1)
        cur = sums[np.arange(C), class_ids[:, v]]
        sums[np.arange(C), class_ids[:, v]] = cur + scores[:, v].astype(np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        means = (sums / counts.astype(np.float32)).astype(np.float32)
    if V >= 8:
        sc32 = np.asarray(scores, np.float32)
        for c, k in zip(*np.nonzero(counts >= 8)):
            means[c, k] = np.mean(sc32[c][class_ids[c] == k])
    mx = counts.max(axis=1)
    tie = (counts == mx[:, None]).sum(axis=1) > 1
    win = counts.argmax(axis=1)                           # first maximum = alphabetical first
    score = means[np.arange(C), win]
    for c in np.flatnonzero(tie):
        best, best_s = -1, np.float32(0)
        for k in range(K):
            if counts[c, k] > 0 and means[c, k] > best_s:
                best, best_s = k, means[c, k]
        win[c], score[c] = best, best_s
    return win, score


def static_from_entropy(ent_full, index, seg_off, percentile=30, min_percentile_pp_score=0.5):
    """`Detection.static = not filter_by_ephemeral_score(entropy[cluster_points_index], ...)` for every cluster
    (lidar_frame.py:238-243; cluster_utils.py:62-64): static <=> np.percentile(scores, percentile) > min score.
    np.percentile(method='linear') on a float32 array: virtual index t*(n-1), neighbours a <= b, float64
    a + (b-a)*g for g < 0.5 else b - (b-a)*(1-g).  ent_full float32 [M]; packed cluster index / offsets.  -> bool [C]."""
    C = len(seg_off) - 1
    if C == 0:
        return np.zeros(0, bool)
    vals = np.asarray(ent_full, np.float32)[index]
    seg_id = np.repeat(np.arange(C), np.diff(seg_off))
    order = np.lexsort((vals, seg_id))
    sv = vals[order].astype(np.float64)
    n = np.diff(seg_off).astype(np.int64)
    virt = (percentile / 100.0) * (n - 1)
    lo = np.floor(virt).astype(np.int64)
    g = virt - lo
    hi = np.minimum(lo + 1, n - 1)
    a, b = sv[seg_off[:-1] + lo], sv[seg_off[:-1] + hi]
    d = b - a
    q = np.where(g >= 0.5, b - d * (1 - g), a + d * g)
    return q > min_percentile_pp_score


class FrameState:
    def __init__(self, fnr, pose, ref_pose):
        self.fnr = fnr
        self.pose = np.asarray(pose, dtype=np.float64)
        self.ref_pose = np.asarray(ref_pose, dtype=np.float64)
        self.transform_to_ref = np.linalg.inv(self.ref_pose) @ self.pose          # lidar_frame.py:25
        self.transform_to_ego = np.linalg.inv(self.pose) @ self.ref_pose          # lidar_frame.py:26
        self.ground_point_indices = None
        self.n_points = 0
        self.ground_plane_model_ref = None
        self.entropy_scores = None                     # kept values (< 0.9), float64   (lidar_frame.py:256-258)
        self.entropy_indices = None                    # their indices into points_ref_wo_ground
        self.n_nonground = 0
        self.clear_detections()

    def clear_detections(self):
        self.cluster_ids = np.zeros(0, np.int64)
        self.index = np.zeros(0, np.int32)            # indices into points_ref_wo_ground
        self.seg_off = np.zeros(1, np.int32)
        self.valid = np.zeros(0, bool)
        self.static = np.zeros(0, bool)
        self.tid = np.zeros(0, np.int64)
        self.static_track = np.zeros(0, np.int8)       # -1 = None (never tracked), 0 = moving track, 1 = static track (objects.py:59)
        self.boxes = None                              # [C,7] float64 ref frame, NaN rows = no box
        self.cls = {}                                  # key -> dict(pred, detailed, score [C,V]; name, final [C]; has [C])
        self.filtered = False
        self.filter_dict = {}                          # Detection.filter_dict (objects.py:168), name -> bool [C]: every active filter's own
                                                       # verdict, written only when vg_cluster_filter_ex ran (not serialised, like the reference)
        self.index_space = INDEX_WO_GROUND             # the point table `index` refers to (set_proposals: INDEX_ALL_POINTS)

    @property
    def n_detections(self):
        return len(self.cluster_ids)

    def set_clusters(self, cluster_ids, index, seg_off):
        self.clear_detections()
        C = len(cluster_ids)
        self.cluster_ids, self.index, self.seg_off = cluster_ids, index, seg_off
        self.valid = np.ones(C, bool)                  # Detection.valid default (objects.py:57)
        self.static = np.ones(C, bool)                 # :58
        self.tid = np.full(C, -1, np.int64)            # :64
        self.static_track = np.full(C, -1, np.int8)

    def set_proposals(self, proposals_ref, box_idx, names=None):
        """generate_detections(None, proposals=..., names=...) (lidar_frame.py:156-167, 232-248) as arrays: one detection per proposal
        that owns at least one point.  proposals_ref [P, >=7]: the boxes in the reference frame; box_idx [n_points]: per point of
        `points_ref` (ALL points, ground included) the proposal that owns it or -1 (points_in_boxes); alternatively the packed lists
        (ids, index, seg_off) of that membership as `pack_clusters` returns them.  cluster_ids are the proposal indices (ascending,
        with gaps), boxes[c] = proposals_ref[cid, :7]; with `names`, object_class['proposal'] = names[cid] shows in `detection_dict`
        (that key of the five alone: no predictions, no score).  The lists index `points_ref`: `index_space` says so, and
        `require_index_space` lets a stage that reads `points_ref_wo_ground` refuse the frame."""
        proposals_ref = np.asarray(proposals_ref)
        if proposals_ref.ndim != 2 or proposals_ref.shape[1] < 7:
            raise ValueError('proposals_ref: [P, >=7]')
        P = len(proposals_ref)
        if isinstance(box_idx, tuple):
            ids, index, seg = box_idx
        else:
            box_idx = np.asarray(box_idx)
            if box_idx.ndim != 1:
                raise ValueError('box_idx: [n_points], one proposal index (or -1) per point')
            ids, index, seg = pack_clusters_numpy(box_idx, None, 0.0)
        ids = np.asarray(ids, dtype=np.int64)
        if len(ids) and (ids.min() < 0 or ids.max() >= P):
            raise ValueError(f'box_idx: proposal indices outside 0 .. {P - 1}')
        if names is not None and len(names) != P:
            raise ValueError(f'names: {len(names)} entries for {P} proposals')
        self.set_clusters(ids, np.asarray(index, dtype=np.int32), np.asarray(seg, dtype=np.int32))
        self.index_space = INDEX_ALL_POINTS
        self.boxes = np.array(proposals_ref[ids, :7], dtype=np.float64)
        if names is not None:
            C = len(ids)
            name = np.empty(C, object)
            name[:] = [names[int(c)] for c in ids]
            self.cls['proposal'] = dict(has=np.ones(C, bool), name=name, name_only=True)

    def require_index_space(self, space, what):
        """ValueError unless the detections' lists index the point table `space` (INDEX_WO_GROUND / INDEX_ALL_POINTS)."""
        have = getattr(self, 'index_space', INDEX_WO_GROUND)
        if have != space:
            raise ValueError(f'{what} reads {space}, but this frame\'s detections index {have} '
                             f'({"set_proposals" if have == INDEX_ALL_POINTS else "set_clusters"} built them)')

    def cluster_index(self, c):
        return self.index[self.seg_off[c]:self.seg_off[c + 1]]

    def sublists(self, rows):
        return cluster_sublists(self.index, self.seg_off, rows)

    def set_classes(self, key, which, pred, detailed, score, name, final_score):
        """which: bool [C] detections that were classified; the arrays have one row per True entry."""
        C = self.n_detections
        V = pred.shape[1] if len(pred) else 0
        e = dict(has=which.copy(), pred=np.empty((C, V), object), detailed=np.empty((C, V), object),
                 score=np.zeros((C, V), np.float32), name=np.empty(C, object), final=np.zeros(C, np.float64),
                 final_py=np.zeros(C, bool))
        # `final`: the vote's mean is a numpy float32 upstream (lidar_frame.py:276-283); propagate_labels may replace it by a
        # python float constant (0.5 / 0.7 / 1.0, zero_shot_detector.py:781-812), which decides the dtype of the result dict's
        # score array (:855) -- held here as float64 values (float32 means are exact in it) + a flag "python float"
        rows = np.flatnonzero(which)
        e['pred'][rows], e['detailed'][rows], e['score'][rows] = pred, detailed, score
        e['name'][rows], e['final'][rows] = name, final_score
        self.cls[key] = e

    def final_score(self, key, c):
        """Detection.object_class_score[key] with upstream's type: numpy float32 (vote) or python float (propagated constant)."""
        e = self.cls[key]
        return float(e['final'][c]) if e['final_py'][c] else np.float32(e['final'][c])

    def set_final_score(self, key, c, value):
        e = self.cls[key]
        e['final'][c] = value
        e['final_py'][c] = not isinstance(value, np.floating)

    # ---- reference-compatible (de)serialisation ---------------------------------------------------------
    def detection_dict(self, c):
        d = {'cluster_id': self.cluster_ids[c]}
        if self.boxes is not None and not np.isnan(self.boxes[c, 0]):
            d['_bounding_box'] = self.boxes[c].copy()
        # objects.py:158-181: the filters' numpy `&` leaves a numpy bool; the constructor default is the python True (:57)
        d['valid'] = np.bool_(self.valid[c]) if self.filtered else bool(self.valid[c])
        d['static'] = bool(self.static[c])
        d['gt_assigned'] = False
        d['cluster_points_index'] = self.cluster_index(c).astype(np.int64)
        named = [k for k, e in self.cls.items() if e['has'][c]]
        has = [k for k in named if not self.cls[k].get('name_only')]       # (set_proposals' entry carries object_class alone)
        if has:
            d['object_class_predictions'] = {k: self.cls[k]['pred'][c].astype(str) for k in has}
        d['tid'] = int(self.tid[c])
        if self.static_track[c] >= 0:
            d['static_track'] = bool(self.static_track[c])
        if has:
            d['object_class_predictions_detailed'] = {k: self.cls[k]['detailed'][c].astype(str) for k in has}
            d['object_class_predictions_score'] = {k: self.cls[k]['score'][c].copy() for k in has}
        if named:
            # an element of np.unique's result, lidar_frame.py:269-283; a proposal's name is the caller's own object (:246-247)
            d['object_class'] = {k: self.cls[k]['name'][c] if self.cls[k].get('name_only') else np.str_(self.cls[k]['name'][c]) for k in named}
        if has:
            d['object_class_score'] = {k: self.final_score(k, c) for k in has}
        return d

    @property
    def serialize(self):
        """lidar_frame.py:41-59."""
        frame = {'_detections': [self.detection_dict(c) for c in range(self.n_detections)]}
        if self.ground_point_indices is not None:
            frame['_ground_point_indices'] = self.ground_point_indices
        if self.entropy_scores is not None:
            frame['_entropy_scores'] = self.entropy_scores
            frame['_entropy_indices'] = self.entropy_indices
        frame['_gt_cluster_mapping'] = {}
        return frame

    # ---- compact form: what `serialize` reads, as a handful of arrays (the state-writer process builds the dicts from it) ----------
    _COMPACT_SHARED = ('cluster_ids', 'index', 'seg_off', 'ground_point_indices', 'entropy_scores', 'entropy_indices')
    _COMPACT_COPIED = ('valid', 'static', 'tid', 'static_track')

    def compact(self):
        """Everything `serialize` reads, detached from later changes: the arrays that later stages rewrite in place (flags, boxes,
        class results) are copied, the bulk that never changes once written (cluster membership, ground set, entropy scores) is
        shared.  ~15 arrays per frame instead of ~90 dicts of a dozen objects: cheap to make, cheap to send to another process."""
        d = {k: getattr(self, k) for k in self._COMPACT_SHARED}
        d.update({k: getattr(self, k).copy() for k in self._COMPACT_COPIED})
        d['boxes'] = None if self.boxes is None else self.boxes.copy()
        d['filtered'] = bool(self.filtered)
        d['cls'] = {k: {f: v.copy() if isinstance(v, np.ndarray) else v for f, v in e.items()} for k, e in self.cls.items()}
        return d

    @classmethod
    def from_compact(cls, d):
        """A FrameState that can `serialize` (nothing else: no poses)."""
        fs = cls.__new__(cls)
        for k in cls._COMPACT_SHARED + cls._COMPACT_COPIED + ('boxes', 'filtered', 'cls'):
            setattr(fs, k, d[k])
        return fs

    def sync(self, data):
        """lidar_frame.py:124-147 + objects.py:136-142: restore from a serialised frame dict."""
        if '_ground_point_indices' in data:
            self.ground_point_indices = np.asarray(data['_ground_point_indices'])
        if data.get('_entropy_scores') is not None:
            self.entropy_scores = np.asarray(data['_entropy_scores'])
            self.entropy_indices = np.asarray(data['_entropy_indices'])
        dets = data.get('_detections')
        if not dets:
            return
        C = len(dets)
        idx = [np.asarray(d['cluster_points_index'], dtype=np.int32) for d in dets]
        self.set_clusters(np.array([d['cluster_id'] for d in dets], dtype=np.int64),
                          np.concatenate(idx) if idx else np.zeros(0, np.int32),
                          np.r_[0, np.cumsum([len(i) for i in idx])].astype(np.int32))
        self.valid = np.array([bool(d.get('valid', True)) for d in dets])
        self.static = np.array([bool(d.get('static', True)) for d in dets])
        self.tid = np.array([int(d.get('tid', -1)) for d in dets], dtype=np.int64)
        self.static_track = np.array([-1 if d.get('static_track') is None else int(bool(d['static_track'])) for d in dets], dtype=np.int8)
        self.filtered = bool((~self.valid).any())      # zero_shot_detector.py:265-274: any invalid detection = already filtered
        if any('_bounding_box' in d for d in dets):
            self.boxes = np.full((C, 7), np.nan)
            for c, d in enumerate(dets):
                if '_bounding_box' in d:
                    self.boxes[c] = d['_bounding_box']
        keys = sorted({k for d in dets for k in (d.get('object_class') or {})})
        for k in keys:
            has = np.array([k in (d.get('object_class') or {}) for d in dets])
            rows = [d for d in dets if k in (d.get('object_class') or {})]
            if not any(k in (r.get('object_class_predictions') or {}) for r in rows):      # a name alone: set_proposals' entry
                name = np.empty(C, object)
                name[np.flatnonzero(has)] = [r['object_class'][k] for r in rows]
                self.cls[k] = dict(has=has, name=name, name_only=True)
                continue
            self.set_classes(k, has,
                             np.array([r['object_class_predictions'][k] for r in rows], dtype=object),
                             np.array([r['object_class_predictions_detailed'][k] for r in rows], dtype=object),
                             np.array([r['object_class_predictions_score'][k] for r in rows], dtype=np.float32),
                             np.array([r['object_class'][k] for r in rows], dtype=object),
                             np.array([r['object_class_score'][k] for r in rows], dtype=np.float64))
            for c, r in zip(np.flatnonzero(has), rows):
                self.cls[k]['final_py'][c] = not isinstance(r['object_class_score'][k], np.floating)
