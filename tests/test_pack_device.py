"""Cluster packing and valid-cluster selection on the device (csrc/pack.hip: vg_pack_clusters, vg_pack_select) and the opt-in
`pack='device'` mode of the pipeline built on them.

The reference of every comparison is `frame_state.pack_clusters_numpy` (the plain numpy restatement of lidar_frame.py:163-167,
230-237 that test_host.py pins the host kernel with) and plain numpy concatenation for the selection -- never the device code against
itself.  Every comparison is exact: integer outputs, `np.array_equal`, dtypes included."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from vilgod_amd import synthetic

SENT = -7777          # pre-fill of every output: what the kernels must not touch keeps it
GUARD = 64            # sentinel elements in front of and behind every output buffer

SIZES = [0, 1, 63, 64, 65, 1_000, 78_775, 400_000, 1 << 20]
PROB_MODES = ['none', 'uniform', 'empties', 'equal', 'nan']


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_pack_entries():
    from vilgod_amd import _lib
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('vg_pack_clusters', 'vg_pack_clusters_work_bytes', 'vg_pack_select', 'vg_pack_select_work_bytes'):
        assert name in protos, name
        assert hasattr(lib, name), name
    assert [a for _, a in protos['vg_pack_clusters'][1]] == ['d_labels', 'd_probs', 'n', 'threshold', 'label_bound', 'd_work', 'work_bytes',
                                                            'd_ids', 'd_index', 'd_seg', 'd_counts', 'stream']
    assert [a for _, a in protos['vg_pack_select'][1]] == ['d_index', 'd_seg', 'n_clusters', 'n_index', 'd_valid', 'd_work', 'work_bytes',
                                                          'd_out_index', 'd_out_seg', 'd_counts', 'stream']
    # the size queries are host arithmetic: no GPU needed
    assert _lib.lib.vg_pack_clusters_work_bytes(0) > 0
    assert _lib.lib.vg_pack_clusters_work_bytes(1 << 20) >= 16 * (1 << 20)
    assert _lib.lib.vg_pack_clusters_work_bytes(-1) < 0 and _lib.lib.vg_pack_clusters_work_bytes((1 << 24) + 1) < 0
    assert _lib.lib.vg_pack_select_work_bytes(700) >= 4 * 700 and _lib.lib.vg_pack_select_work_bytes(-1) < 0
    src = open(os.path.join(ROOT, 'include', 'vilgod_hip.h')).read()
    doc = src[src.index('The same grouping ON THE DEVICE'):src.index('int vg_pack_select(')]
    assert 'lidar_frame.py:163-167' in doc and 'zero_shot_detector.py:' in doc          # cites the reference like the other entries


def test_pack_mode_is_parsed_without_a_gpu():
    from vilgod_amd.pipeline import PseudoLabelPipeline
    from vilgod_amd import frame_state
    assert PseudoLabelPipeline.parse_pack('host') == 'host' and PseudoLabelPipeline.parse_pack('device') == 'device'
    assert PseudoLabelPipeline.parse_pack(None) == 'host'
    for bad in ('gpu', 'Device', '', 1):
        with pytest.raises(ValueError):
            PseudoLabelPipeline.parse_pack(bad)
    assert inspect.signature(PseudoLabelPipeline.__init__).parameters['pack'].default == 'host'
    assert callable(frame_state.pack_clusters_device) and callable(frame_state.select_clusters_device)
    # the shipped configuration names the mode, with the host path as its default; the entry point and the stage dispatcher read it
    text = open(os.path.join(ROOT, 'tools', 'configs', 'preprocessing.yaml')).read()
    assert re.search(r'^\s+pack:\s*host\b', text, flags=re.M)
    for rel in ('tools/preprocess_data.py', 'vilgod_amd/zero_shot_detector.py'):
        assert "pack=dev.get('pack', 'host')" in open(os.path.join(ROOT, rel)).read(), rel


def test_pack_kernels_are_built_for_the_device_and_do_not_spill():
    from vilgod_amd import build
    asm = build._device_asm('pack.hip')
    for k in ('k_pack_hist', 'k_pack_scan', 'k_pack_scatter', 'k_pack_head_count', 'k_pack_head_write', 'k_pack_select_scan',
              'k_pack_select_copy'):
        assert re.search(r'^_Z\S*' + k + r'\S*:', asm, flags=re.M), k
    assert 'gfx950' in asm
    assert build.check_scratch('pack.hip', 'k_pack') == []
    assert build.check_isa(sources=['pack.hip']) == []


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def _guarded(n, dtype, dev):
    full = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=dev)
    return full, full[GUARD:GUARD + n]


def _guards_intact(full, n):
    h = full.cpu().numpy()
    return bool((h[:GUARD] == SENT).all() and (h[GUARD + n:] == SENT).all())


def _pack(labels, probs, thr, bound, dev):
    """-> (ids, index, seg, counts) host copies of the whole capacity + whether every guard zone survived"""
    from vilgod_amd.frame_state import pack_clusters_device
    n = len(labels)
    d_lab = torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(dev)
    d_pr = None if probs is None else torch.from_numpy(np.ascontiguousarray(probs, np.float64)).to(dev)
    f_ids, ids = _guarded(n, torch.int64, dev)
    f_idx, idx = _guarded(n, torch.int32, dev)
    f_seg, seg = _guarded(n + 1, torch.int32, dev)
    f_cnt, cnt = _guarded(3, torch.int32, dev)
    pack_clusters_device(d_lab, d_pr, thr, label_bound=bound, out=(ids, idx, seg, cnt))
    torch.cuda.synchronize()
    ok = _guards_intact(f_ids, n) and _guards_intact(f_idx, n) and _guards_intact(f_seg, n + 1) and _guards_intact(f_cnt, 3)
    return ids.cpu().numpy(), idx.cpu().numpy(), seg.cpu().numpy(), cnt.cpu().numpy(), ok


def _check_pack(labels, probs, thr, bound, dev, what):
    from vilgod_amd.frame_state import pack_clusters_numpy
    ids, idx, seg, cnt, ok = _pack(labels, probs, thr, bound, dev)
    w_ids, w_idx, w_seg = pack_clusters_numpy(np.asarray(labels, np.int32), probs, thr)
    C, P = len(w_ids), len(w_idx)
    assert ok, what
    assert cnt.dtype == np.int32 and cnt.tolist() == [C, P, 0], (what, cnt.tolist(), C, P)
    assert ids.dtype == np.int64 and idx.dtype == np.int32 and seg.dtype == np.int32
    assert np.array_equal(ids[:C], w_ids), what
    assert np.array_equal(idx[:P], w_idx), what
    assert np.array_equal(seg[:C + 1], w_seg), what
    assert (ids[C:] == SENT).all() and (idx[P:] == SENT).all() and (seg[C + 1:] == SENT).all(), what      # nothing beyond is written
    return w_ids, w_idx, w_seg


def _labels(family, n, rng):
    """-> (labels int32 [n], exclusive label bound) or None when the family has no such size"""
    if family == 'noise':
        return np.full(n, -1, np.int32), 8
    if family == 'one':
        return np.zeros(n, np.int32), 1
    if family == 'identity':                       # n clusters of one point
        return np.arange(n, dtype=np.int32), max(n, 1)
    if family == 'random700':
        lab = rng.integers(0, 700, n).astype(np.int32)
        lab[rng.random(n) < 0.4] = -1
        return lab, 700
    if family == 'sparse':                         # labels with gaps
        lab = np.array([3, 7, 500, -1], np.int32)[rng.integers(0, 4, n)]
        return lab, 512
    if family == 'big':                            # one cluster of 20k points among 90 small ones
        if n < 30_000:
            return None
        lab = np.full(n, -1, np.int32)
        perm = rng.permutation(n)
        lab[perm[:20_000]] = 45
        small = np.delete(np.arange(91), 45)
        lab[perm[20_000:20_000 + 90 * 40]] = np.repeat(small, 40)
        return lab, 91
    raise KeyError(family)


def _probs(mode, labels, rng):
    """-> (probs float64 or None, threshold)"""
    n = len(labels)
    if mode == 'none':
        return None, 0.3
    if mode == 'uniform':
        return rng.random(n), 0.3
    if mode == 'empties':                          # every point of the odd labels lies below the threshold: those ids must vanish
        p = 0.5 + 0.5 * rng.random(n)
        p[(labels % 2) == 1] = 0.1
        return p, 0.3
    if mode == 'equal':                            # exactly the threshold is kept (strict <)
        thr = 0.3
        p = np.full(n, thr)
        p[rng.random(n) < 0.25] = np.nextafter(thr, 0.0)
        p[rng.random(n) < 0.25] = np.nextafter(thr, 1.0)
        return p, thr
    if mode == 'nan':                              # NaN < threshold is false: the point stays
        p = rng.random(n)
        p[rng.random(n) < 0.3] = np.nan
        return p, 0.3
    raise KeyError(mode)


# ---- GPU: grouping ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('family', ['noise', 'one', 'identity', 'random700', 'sparse', 'big'])
def test_grouping_equals_numpy_for_every_size_and_probability_mode(cuda, family):
    """Sizes 0 .. 2^20 around the 64-lane wave and the 2048-point tile, every probability mode.  ('big' needs room for its 20 000-point
    cluster and its 90 clusters of 40: the three sizes from 78 775 up.)"""
    rng = np.random.default_rng(11)
    done = 0
    for n in SIZES:
        made = _labels(family, n, rng)
        if made is None:
            continue
        labels, bound = made
        for mode in PROB_MODES:
            probs, thr = _probs(mode, labels, rng)
            w_ids, _, _ = _check_pack(labels, probs, thr, bound, cuda, (family, n, mode))
            if mode == 'empties' and family in ('identity', 'random700', 'sparse', 'big') and n >= 1000:
                assert len(w_ids) and (w_ids % 2 == 0).all()
            done += 1
    assert done == len(PROB_MODES) * (3 if family == 'big' else len(SIZES))


def _bench_frame_labels(cuda):
    """labels / probabilities the pipeline's own cluster() returns for the frame behind tests/golden/cluster_full_golden.json"""
    from vilgod_amd.pipeline import PseudoLabelPipeline
    pipe = PseudoLabelPipeline(device=cuda, max_points=151_000, clip_model_path='/nonexistent', box_mode='fast', box_workers=0)
    poses = synthetic.make_poses(2)
    fs, d_ref, d_X, gidx = pipe.prepare(synthetic.make_frame(7, 150_000, n_objects=60), poses[1], poses[0])
    labels, probs = pipe.cluster(d_X)
    assert isinstance(labels, np.ndarray)          # the default mode hands host arrays on
    return pipe, labels, probs


@pytest.mark.gpu
def test_grouping_of_the_pipelines_own_labels(cuda):
    pipe, labels, probs = _bench_frame_labels(cuda)
    print('own labels:', len(labels), 'points,', int(labels.max()) + 1, 'labels,', int((labels < 0).sum()), 'noise points')
    assert len(labels) == 78_775 and int(labels.max()) + 1 == 90
    rng = np.random.default_rng(5)
    n = len(labels)
    _check_pack(labels, probs, pipe.prob_threshold, n // 15 + 1, cuda, 'own, own probabilities')       # the bound the pipeline passes
    for mode in PROB_MODES:
        p, thr = _probs(mode, labels, rng)
        _check_pack(labels, p, thr, 90, cuda, ('own', mode))


@pytest.mark.gpu
def test_label_beyond_the_bound_sets_the_flag_and_writes_nothing_out_of_bounds(cuda):
    rng = np.random.default_rng(3)
    for n, bound, bad in ((1000, 512, 512), (78_775, 700, 1 << 30), (5000, 0, 0), (70_000, 1 << 16, 1 << 16)):
        labels = rng.integers(0, max(bound, 1), n).astype(np.int32)
        labels[rng.integers(0, n, 7)] = bad
        ids, idx, seg, cnt, ok = _pack(labels, None, 0.3, bound, cuda)
        assert ok and cnt[2] != 0, (n, bound)
        C, P = int(cnt[0]), int(cnt[1])
        assert 0 <= C <= n and 0 <= P <= n and (idx[P:] == SENT).all() and (ids[C:] == SENT).all() and (seg[C + 1:] == SENT).all()


@pytest.mark.gpu
def test_pipeline_falls_back_to_the_host_lists_for_labels_beyond_the_bound(cuda):
    from vilgod_amd.pipeline import PseudoLabelPipeline
    host = PseudoLabelPipeline(device=cuda, max_points=61_000, clip_model_path='/nonexistent', box_mode='fast', box_workers=0)
    dev = PseudoLabelPipeline(device=cuda, max_points=61_000, clip_model_path='/nonexistent', box_mode='fast', box_workers=0, clip=host.clip,
                              pack='device')
    pts = synthetic.make_frame(71, 60_000, n_objects=30)
    poses = synthetic.make_poses(2)
    out = []
    for pipe in (host, dev):
        pipe.new_sequence()
        fs, d_ref, d_X, gidx = pipe.prepare(pts, poses[1], poses[0])
        labels, probs = pipe.cluster(d_X)
        if pipe is dev:
            assert isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int32
            far = torch.where(labels >= 0, labels * 1000, labels)            # ids far beyond n / min_cluster_size
            assert dev.pack_device(far, probs) is None
        else:
            far = np.where(labels >= 0, labels * 1000, labels)
        out.append(pipe.label(fs, d_ref, d_X, gidx, far, probs))
    (fa, ra), (fb, rb) = out
    assert fa.n_detections > 10 and int(fa.cluster_ids.max()) >= 1000
    _same_frame(fa, ra, None, fb, rb, None)


# ---- GPU: determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_same_input_same_bits_also_beside_a_busy_stream(cuda):
    from vilgod_amd.hdbscan import HDBSCAN
    rng = np.random.default_rng(8)
    labels, bound = _labels('random700', 400_000, rng)
    probs, thr = _probs('uniform', labels, rng)
    a = _pack(labels, probs, thr, bound, cuda)
    b = _pack(labels, probs, thr, bound, cuda)
    model = HDBSCAN(min_cluster_size=15, max_points=61_000, device=cuda)
    X = torch.from_numpy(synthetic.make_frame(70, 60_000, n_objects=30)[:, :3].copy()).to(cuda)
    busy, side = torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize()
    tree = []

    def other_stream():                                     # vg_cluster_mst_nd: several ms of kernels (and its own waits) on `busy`
        torch.cuda.set_device(cuda)
        with torch.cuda.stream(busy):
            tree.append(model.mst(X, stream=busy))
    import threading
    th = threading.Thread(target=other_stream)
    th.start()
    with torch.cuda.stream(side):
        c = _pack(labels, probs, thr, bound, cuda)
    th.join()
    torch.cuda.synchronize()
    assert tree and tree[0][0].numel() == X.shape[0] - 1
    for other in (b, c):
        assert other[4]
        for x, y in zip(a[:4], other[:4]):
            assert np.array_equal(x, y)


# ---- GPU: selection -------------------------------------------------------------------------------------------------------------------
def _check_select(index, seg, keep, dev, what):
    from vilgod_amd.frame_state import select_clusters_device
    C, P = len(seg) - 1, len(index)
    d_index = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev)
    d_seg = torch.from_numpy(np.ascontiguousarray(seg, np.int32)).to(dev)
    d_valid = torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).to(dev)          # the dtype vg_cluster_filter[_ex] write
    f_oi, oi = _guarded(P, torch.int32, dev)
    f_os, osg = _guarded(C + 1, torch.int32, dev)
    f_cnt, cnt = _guarded(2, torch.int32, dev)
    select_clusters_device(d_index, d_seg, C, d_valid, n_index=P, out=(oi, osg, cnt))
    torch.cuda.synchronize()
    rows = np.flatnonzero(keep)
    parts = [index[seg[c]:seg[c + 1]] for c in rows]
    w_index = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    w_seg = np.r_[0, np.cumsum([len(p) for p in parts])].astype(np.int32)
    K, Q = len(rows), len(w_index)
    assert _guards_intact(f_oi, P) and _guards_intact(f_os, C + 1) and _guards_intact(f_cnt, 2), what
    h_oi, h_os = oi.cpu().numpy(), osg.cpu().numpy()
    assert cnt.cpu().numpy().tolist() == [K, Q], what
    assert h_oi.dtype == np.int32 and h_os.dtype == np.int32
    assert np.array_equal(h_oi[:Q], w_index) and np.array_equal(h_os[:K + 1], w_seg), what
    assert (h_oi[Q:] == SENT).all() and (h_os[K + 1:] == SENT).all(), what


@pytest.mark.gpu
def test_selection_equals_numpy_concatenation(cuda):
    from vilgod_amd.frame_state import pack_clusters_numpy
    rng = np.random.default_rng(21)
    cases = [('random700', 78_775), ('big', 78_775), ('identity', 1_000), ('sparse', 65), ('noise', 1_000), ('identity', 400_000), ('one', 0)]
    for family, n in cases:
        labels, _ = _labels(family, n, rng)
        _, index, seg = pack_clusters_numpy(labels, None, 0.3)
        C = len(seg) - 1
        masks = {'none': np.zeros(C, np.uint8), 'all': np.ones(C, np.uint8), 'random': (rng.random(C) < 0.5).astype(np.uint8),
                 'bytes': rng.integers(0, 256, C).astype(np.uint8) * (rng.random(C) < 0.7)}       # any non-zero byte keeps
        if C:
            largest = np.zeros(C, np.uint8)
            largest[int(np.argmax(np.diff(seg)))] = 1
            masks['largest'] = largest
        for name, keep in masks.items():
            _check_select(index, seg, keep.astype(np.uint8), cuda, (family, n, name))
    # frame_state.select_rows_device (the pipeline's and the stage dispatcher's cut of some clusters, trimmed to what the kernel wrote)
    # against the host's cluster_sublists, itself pinned to the written-out concatenation in test_host.py
    from test_host import sublist_case_700
    from vilgod_amd.frame_state import cluster_sublists, select_rows_device
    index700, seg700, rows700 = sublist_case_700()
    three = (np.array([5, 1, 4, 9, 9, 2, 7], np.int32), np.array([0, 2, 3, 7], np.int32))
    for index, seg, rows, on_device in [(np.array([3, 0, 2], np.int32), np.array([0, 3], np.int32), [0], False), (*three, [1], False),
                                        (*three, [0, 1, 2], False), (index700, seg700, np.arange(700), False),
                                        (index700, seg700, rows700, False), (index700, seg700, rows700, True)]:
        C = len(seg) - 1
        w_index, w_seg = cluster_sublists(index, seg, rows)
        keep = rows
        if on_device:                                       # the verdict as a filter kernel leaves it: uint8 [C], already on the device
            keep = torch.from_numpy(np.isin(np.arange(C), rows).astype(np.uint8)).to(cuda)
        g_index, g_seg = select_rows_device(torch.from_numpy(index).to(cuda), torch.from_numpy(seg).to(cuda), C, w_seg, keep)
        assert g_index.dtype == torch.int32 and g_seg.dtype == torch.int32 and g_index.is_cuda and g_seg.is_cuda
        assert np.array_equal(g_index.cpu().numpy(), w_index) and np.array_equal(g_seg.cpu().numpy(), w_seg), (C, len(rows), on_device)


# ---- GPU: refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bad_arguments_are_refused_and_leave_the_outputs_alone(cuda):
    from vilgod_amd._lib import lib, ptr, stream_ptr
    n = 1000
    lab = torch.zeros(n, dtype=torch.int32, device=cuda)
    pr = torch.ones(n, dtype=torch.float64, device=cuda)
    wb = lib.vg_pack_clusters_work_bytes(n)
    work = torch.empty(wb, dtype=torch.uint8, device=cuda)
    ids = torch.full((n,), SENT, dtype=torch.int64, device=cuda)
    idx = torch.full((n,), SENT, dtype=torch.int32, device=cuda)
    seg = torch.full((n + 1,), SENT, dtype=torch.int32, device=cuda)
    cnt = torch.full((3,), SENT, dtype=torch.int32, device=cuda)
    good = dict(d_labels=ptr(lab), d_probs=ptr(pr), n=n, threshold=0.3, label_bound=8, d_work=ptr(work), work_bytes=wb, d_ids=ptr(ids),
                d_index=ptr(idx), d_seg=ptr(seg), d_counts=ptr(cnt))
    order = ['d_labels', 'd_probs', 'n', 'threshold', 'label_bound', 'd_work', 'work_bytes', 'd_ids', 'd_index', 'd_seg', 'd_counts']
    bad = [dict(d_labels=None), dict(d_work=None), dict(d_ids=None), dict(d_index=None), dict(d_seg=None), dict(d_counts=None), dict(n=-1),
           dict(label_bound=-1), dict(label_bound=(1 << 24) + 1), dict(work_bytes=wb - 1), dict(work_bytes=0), dict(n=(1 << 24) + 1)]
    for change in bad:
        a = {**good, **change}
        assert lib.vg_pack_clusters(*[a[k] for k in order], stream_ptr()) == 1, change
    sel_work = torch.empty(lib.vg_pack_select_work_bytes(4), dtype=torch.uint8, device=cuda)
    s_index = torch.arange(8, dtype=torch.int32, device=cuda)
    s_seg = torch.tensor([0, 2, 4, 6, 8], dtype=torch.int32, device=cuda)
    s_valid = torch.ones(4, dtype=torch.uint8, device=cuda)
    o_index = torch.full((8,), SENT, dtype=torch.int32, device=cuda)
    o_seg = torch.full((5,), SENT, dtype=torch.int32, device=cuda)
    o_cnt = torch.full((2,), SENT, dtype=torch.int32, device=cuda)
    sgood = dict(d_index=ptr(s_index), d_seg=ptr(s_seg), n_clusters=4, n_index=8, d_valid=ptr(s_valid), d_work=ptr(sel_work),
                 work_bytes=sel_work.numel(), d_out_index=ptr(o_index), d_out_seg=ptr(o_seg), d_counts=ptr(o_cnt))
    sorder = ['d_index', 'd_seg', 'n_clusters', 'n_index', 'd_valid', 'd_work', 'work_bytes', 'd_out_index', 'd_out_seg', 'd_counts']
    sbad = [dict(d_index=None), dict(d_seg=None), dict(d_valid=None), dict(d_work=None), dict(d_out_index=None), dict(d_out_seg=None),
            dict(d_counts=None), dict(n_clusters=-1), dict(n_index=-1), dict(work_bytes=3)]
    for change in sbad:
        a = {**sgood, **change}
        assert lib.vg_pack_select(*[a[k] for k in sorder], stream_ptr()) == 1, change
    torch.cuda.synchronize()
    for t in (ids, idx, seg, cnt, o_index, o_seg, o_cnt):
        assert (t == SENT).all()
    # ... and the same buffers work once the arguments are right; n == 0 succeeds with d_seg[0] = 0 and zero counts
    assert lib.vg_pack_clusters(*[good[k] for k in order], stream_ptr()) == 0
    assert lib.vg_pack_select(*[sgood[k] for k in sorder], stream_ptr()) == 0
    torch.cuda.synchronize()
    assert cnt.tolist() == [1, n, 0] and seg[:2].tolist() == [0, n] and o_cnt.tolist() == [4, 8] and o_index.tolist() == list(range(8))
    seg.fill_(SENT)
    cnt.fill_(SENT)
    zero = {**good, 'n': 0, 'd_labels': None, 'd_probs': None, 'd_ids': None, 'd_index': None}
    assert lib.vg_pack_clusters(*[zero[k] for k in order], stream_ptr()) == 0
    torch.cuda.synchronize()
    assert cnt.tolist() == [0, 0, 0] and seg[0].item() == 0 and (seg[1:] == SENT).all()


# ---- GPU: the pipeline in both modes ----------------------------------------------------------------------------------------------------
def _same_frame(fa, ra, pa, fb, rb, pb):
    """everything the frame state and the results hold: same arrays, same dtypes"""
    for k in ('cluster_ids', 'index', 'seg_off', 'valid', 'static', 'tid', 'static_track'):
        x, y = getattr(fa, k), getattr(fb, k)
        assert x.dtype == y.dtype and np.array_equal(x, y), k
    assert np.array_equal(fa.ground_point_indices, fb.ground_point_indices)
    assert fa.filtered == fb.filtered and set(fa.filter_dict) == set(fb.filter_dict)
    for k in fa.filter_dict:
        assert np.array_equal(fa.filter_dict[k], fb.filter_dict[k]), k
    assert (fa.boxes is None) == (fb.boxes is None)
    if fa.boxes is not None:
        assert np.array_equal(fa.boxes, fb.boxes, equal_nan=True)
    assert set(fa.cls) == set(fb.cls)
    for key in fa.cls:
        for f in fa.cls[key]:
            x, y = fa.cls[key][f], fb.cls[key][f]
            assert x.dtype == y.dtype and np.array_equal(x, y), (key, f)
    assert set(ra) == set(rb)
    for k in ra:
        assert ra[k].dtype == rb[k].dtype and np.array_equal(ra[k], rb[k]), k
    if pa is not None:
        assert np.array_equal(pa.cpu().numpy(), pb.cpu().numpy())          # per-crop probabilities


def _pair(cuda, cfg=None, **kw):
    from vilgod_amd.pipeline import PseudoLabelPipeline
    host = PseudoLabelPipeline(cfg, device=cuda, clip_model_path='/nonexistent', **kw)
    dev = PseudoLabelPipeline(cfg, device=cuda, clip_model_path='/nonexistent', clip=host.clip, pack='device', **kw)
    assert host.pack == 'host' and dev.pack == 'device'
    return host, dev


@pytest.mark.gpu
def test_pipeline_20k_frame_equal_in_both_modes(cuda):
    """the frame of test_pipeline.py's oracle test, in its parity configuration (fp32 tower, reference boxes and view angle)"""
    from vilgod_amd.pipeline import default_preprocessor_cfg
    host, dev = _pair(cuda, default_preprocessor_cfg(), vit_dtype='f32', max_points=25_000, angle_mode='reference')
    pts = synthetic.make_frame(3, 20_000, n_objects=12)
    poses = synthetic.make_poses(2, seed=4)
    fa, ra = host.process_frame(pts, poses[1], poses[0], fnr=1)
    pa = host.last_probs
    fb, rb = dev.process_frame(pts, poses[1], poses[0], fnr=1, timing=True)
    assert fa.n_detections > 5 and fa.valid.sum() > 2 and len(ra['name']) > 0
    _same_frame(fa, ra, pa, fb, rb, dev.last_probs)
    assert {'pack_clusters+h2d', 'valid_lists'} <= set(dev.latency)          # the two modes' latency tables line up
    assert type(fa.serialize['_detections'][0]['cluster_id']) is type(fb.serialize['_detections'][0]['cluster_id'])


@pytest.mark.gpu
def test_three_150k_frames_in_flight_equal_in_both_modes(cuda):
    host, dev = _pair(cuda, vit_dtype='f16', max_points=160_000)
    poses = synthetic.make_poses(4)
    frames = [synthetic.make_frame(f, 150_000) for f in range(3)]
    host.new_sequence()
    dev.new_sequence()
    a = host.process_frames([host.upload(f) for f in frames], poses[1:4], poses[0], n_workers=3)
    b = dev.process_frames([dev.upload(f) for f in frames], poses[1:4], poses[0], n_workers=3)
    n_valid = 0
    for (fa, ra, pa), (fb, rb, pb) in zip(a, b):
        _same_frame(fa, ra, pa, fb, rb, pb)
        n_valid += int(fa.valid.sum())
    assert n_valid > 30


@pytest.mark.gpu
def test_sequence_with_entropy_and_two_frame_clustering_equal_in_both_modes(cuda):
    from vilgod_amd.pipeline import default_preprocessor_cfg
    host, dev = _pair(cuda, default_preprocessor_cfg(), vit_dtype='f16', max_points=25_000)
    frames, poses = synthetic.make_sequence(seed=2, n_frames=6, n_points=12_000, n_objects=8)
    ent_args = dict(n_neighbouring_frames=3, skip_frames=0)
    a = host.process_sequence(frames, poses, poses[0], entropy_args=ent_args, n_frames=2, seed=0)
    b = dev.process_sequence(frames, poses, poses[0], entropy_args=ent_args, n_frames=2, seed=0)
    c = dev.process_sequence(frames, poses, poses[0], entropy_args=ent_args, n_frames=2, seed=0, n_workers=2)
    assert sum(int(fa.n_detections) for fa, _ in a) > 10 and sum(int((~fa.static).sum()) for fa, _ in a) > 0
    for (fa, ra), (fb, rb), (fc, rc) in zip(a, b, c):
        _same_frame(fa, ra, None, fb, rb, None)
        _same_frame(fa, ra, None, fc, rc, None)
        assert np.array_equal(fa.entropy_indices, fb.entropy_indices) and np.array_equal(fa.entropy_scores, fb.entropy_scores)


@pytest.mark.gpu
def test_host_hierarchy_equal_in_both_modes(cuda):
    """hierarchy='host': the labels arrive as host arrays, are uploaded (12 bytes per point) and packed on the device all the same"""
    host, dev = _pair(cuda, vit_dtype='f16', max_points=61_000, hierarchy='host', box_mode='fast', box_workers=0)
    poses = synthetic.make_poses(3)
    for f in range(2):
        pts = synthetic.make_frame(70 + f, 60_000, n_objects=30)
        fa, ra = host.process_frame(pts, poses[f + 1], poses[0], fnr=f)
        pa = host.last_probs
        fb, rb = dev.process_frame(pts, poses[f + 1], poses[0], fnr=f)
        assert fa.valid.sum() > 5
        _same_frame(fa, ra, pa, fb, rb, dev.last_probs)


@pytest.mark.gpu
def test_non_shipped_filter_set_equal_in_both_modes(cuda):
    """a filter set that runs vg_cluster_filter_ex: its verdict bytes feed vg_pack_select as they are"""
    from vilgod_amd.pipeline import default_preprocessor_cfg
    cfg = default_preprocessor_cfg()
    cl = cfg['clustering']
    cl['filters'] = cl['filters'] + [dict(name='filter_by_aspect_ratio', args=dict(logic='or', min_aspect_ratio=1.0, max_aspect_ratio=5.0)),
                                     dict(name='filter_by_area', args=dict(logic='and', min_area=0.35))]
    cl['filters_active'] = [f['name'] for f in cl['filters']]
    host, dev = _pair(cuda, cfg, vit_dtype='f16', max_points=61_000)
    assert host._filters['entry'] == 'vg_cluster_filter_ex'
    poses = synthetic.make_poses(2)
    pts = synthetic.make_frame(72, 60_000, n_objects=30)
    fa, ra = host.process_frame(pts, poses[1], poses[0], fnr=1)
    pa = host.last_probs
    fb, rb = dev.process_frame(pts, poses[1], poses[0], fnr=1)
    assert 0 < fa.valid.sum() < fa.n_detections and set(fa.filter_dict) == set(cl['filters_active'])
    _same_frame(fa, ra, pa, fb, rb, dev.last_probs)


# ---- GPU: the entry point ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_with_device_pack_writes_the_default_runs_pickles(cuda, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import preprocess_data
    from test_cli import OVR, _load, _same_outputs
    roots = {}
    for mode in ('host', 'device'):
        roots[mode] = str(tmp_path / mode)
        preprocess_data.main(['preprocessor=waymo', f'dataset.DATA_PATH={roots[mode]}'] + ([] if mode == 'host' else ['device.pack=device']) + OVR)
    a, ia, sa = _load(roots['host'])
    b, ib, sb = _load(roots['device'])
    assert ia == ib and len(a) == len(b) == 6 and sum(len(fr['name']) for fr in a) > 0
    _same_outputs(a, sa, b, sb)
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            assert x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k])
    for x, y in zip(sa, sb):
        assert set(x) == set(y)
        assert np.array_equal(x['_entropy_scores'], y['_entropy_scores']) and np.array_equal(x['_entropy_indices'], y['_entropy_indices'])
        for d, e in zip(x['_detections'], y['_detections']):
            assert list(d) == list(e)
            assert d['cluster_id'] == e['cluster_id'] and type(d['cluster_id']) is type(e['cluster_id'])
            assert d['cluster_points_index'].dtype == e['cluster_points_index'].dtype
