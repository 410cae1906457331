"""Motion-aligned track boxes from oriented extents, CPU side: vg_cluster_oriented_extents_host (the kernel's per-point code,
csrc/oriented_extent_point.inc) against the exact reference of tests/moving_boxes_ref.py, and tracking.moving_boxes /
fit_track_boxes fed with its extents against the forms that read the points -- every comparison is for equal values, none has a
tolerance of its own (the golden boxes keep the atol=2e-5 tests/test_tracking.py gives them)."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

import moving_boxes_ref as R
from oracle import segment_oracle as so
from oracle import tracking_oracle
from vilgod_amd import build, synthetic, tracking
from vilgod_amd import oriented_extents as oe
from vilgod_amd._lib import HEADER, lib, parse_header

B = oe.OEXT_BLOCK


def host(case):
    return oe.oriented_extents_host(case['points'], case['index'], case['seg'], case['pair_cluster'], case['center3'], case['rot4'])


@pytest.fixture(scope='module')
def cases():
    return dict(R.kernel_cases(B))


def test_header_declares_and_library_exports_the_entries():
    protos = parse_header()
    assert len(protos['vg_cluster_oriented_extents'][1]) == 11 and len(protos['vg_cluster_oriented_extents_host'][1]) == 10
    assert lib.vg_cluster_oriented_extents and lib.vg_cluster_oriented_extents_host
    assert lib.vg_abi_version() >= 1
    assert B == int(re.search(r'^#define\s+VG_OEXT_BLOCK\s+(\d+)', open(HEADER).read(), flags=re.M).group(1))
    assert B % 64 == 0 and 64 <= B <= 1024
    assert build.SOURCES['oriented_extent.hip'] == ['-ffp-contract=off']


def test_kernel_is_built_without_scratch_and_without_unencodable_constants():
    assert build.check_scratch('oriented_extent.hip', '') == []
    assert build.check_isa(sources=['oriented_extent.hip']) == []
    assert 'k_cluster_oriented_extents' in build._device_asm('oriented_extent.hip')


CASE_NAMES = ['sizes', 'large', 'pairs300', 'pairs1', 'pairs0', 'identity', 'out_of_range', 'geometry', 'nonfinite']


# (the 20 001-point clusters go through the exact reference once, at stride 5: 60 000 exact points take seconds)
@pytest.mark.parametrize('name,stride', [(n, s) for n in CASE_NAMES for s in (3, 5) if (n, s) != ('large', 3)])
def test_host_entry_point_equals_the_exact_reference_bit_for_bit(cases, name, stride):
    case = R.with_stride(cases[name], stride)
    got = host(case)
    want = R.ref_extents(case['points'], case['index'], case['seg'], case['pair_cluster'], case['center3'], case['rot4'])
    assert got.shape == want.shape == (len(case['center3']), 6)
    bad = np.argwhere(R.bits(got) != R.bits(want))
    assert len(bad) == 0, (name, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    nan = np.isnan(want).all(axis=1)
    assert not np.isnan(want[~nan]).any()
    if name == 'sizes':
        assert nan.sum() == 6                                            # the three empty clusters, two pairs each
        assert (want[~nan, 1] > want[~nan, 0]).sum() >= 2 * 3 * 8 and np.all(want[~nan, 1] >= want[~nan, 0])
    if name == 'out_of_range':
        assert nan.tolist() == [False, True, False, False, True, False]
    if name == 'geometry':
        ok = want[~nan]
        assert (ok[:, 1] < 0).any() and (ok[:, 0] > 0).any() and ((ok[:, 0] < 0) & (ok[:, 1] > 0)).any()      # all negative, all positive, straddling
        assert (ok[:, 0] == ok[:, 1]).sum() >= 8                                                             # identical points
    if name == 'nonfinite':
        assert nan.tolist() == [False, False, True, True, False, False, True, True, True, True, True, False]
    if name == 'identity':
        assert case['pair_cluster'] is None and len(want) == 40
    if name == 'pairs300':
        assert len(want) == 300 and len(set(case['pair_cluster'].tolist())) < 41 and np.any(np.diff(case['index']) < 0)


def test_minimum_and_maximum_are_the_projections_numpy_computes(cases):
    """the restated chain IS np.dot's: on the geometry case every extent equals the min / max of np.dot(points - centre, rot)"""
    case = cases['geometry']
    got = host(case)
    for p, c in enumerate(case['pair_cluster']):
        pts = case['points'][case['index'][case['seg'][c]:case['seg'][c + 1]], :3]
        rot = np.eye(3)
        rot[:2, :2] = case['rot4'][p].reshape(2, 2)
        proj = np.dot(pts - case['center3'][p], rot)
        want = [proj[:, 0].min(), proj[:, 0].max(), proj[:, 1].min(), proj[:, 1].max(), pts[:, 2].min(), pts[:, 2].max()]
        assert np.array_equal(got[p], np.array(want, dtype=np.float64)), p


def test_moving_boxes_from_extents_equal_the_forms_that_read_the_points():
    """the 200 seeded tracks of tests/test_tracking.py: extents from the host entry point, no points -> the same boxes, bit for bit,
    as tracking.moving_boxes and the line-by-line oracle give from the points"""
    n_box = 0
    for trial, dirs, pts, T in R.seeded_tracks():
        c3 = [np.median(p[:, :3], axis=0) for p in pts]
        n = [len(p) for p in pts]
        seg = np.r_[0, np.cumsum(n)]
        rot4 = tracking.direction_rotations(dirs)[1][:, :2, :2].reshape(-1, 4)
        E = oe.oriented_extents_host(np.concatenate(pts), np.arange(seg[-1]), seg, None, c3, rot4)
        R.assert_float32_safe(E, trial)                                # (every cluster of every track: none is left out)
        want = tracking.moving_boxes(pts, dirs, T, centers3=c3)
        got = tracking.moving_boxes(None, dirs, T, centers3=c3, extents=E, counts=n)
        assert got.dtype == want.dtype and np.array_equal(got, want), trial
        assert np.array_equal(got, tracking_oracle.moving_boxes(pts, dirs, T, centers3=c3)), trial
        packed = tracking.moving_boxes_packed(None, None, dirs, T, c3, extents=E, counts=n)
        assert np.array_equal(packed, want), trial
        n_box += 1
    assert n_box > 50
    with pytest.raises(ValueError):
        tracking.moving_boxes(None, dirs, T, centers3=c3, extents=E)


# ---- the golden scene of tests/test_tracking.py ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gold(golden_dir):
    with open(os.path.join(golden_dir, 'track_golden.pkl'), 'rb') as f:
        return pickle.load(f)


@pytest.fixture(scope='module')
def scene():
    frames, poses = synthetic.make_sequence(seed=11, n_frames=18, n_points=5000, n_objects=9, moving_frac=0.6)
    X = []
    for f, p in zip(frames, poses):
        pr = so.apply_transform(f, np.linalg.inv(poses[0]) @ p)
        X.append(np.ascontiguousarray(pr[pr[:, 2] > 0.25]))
    return frames, poses, X


def run_tracker(gold, X):
    tr = tracking.Tracker(mode='cluster_center', max_distance=1.0, min_length=5, max_missed=3)
    med, cnt, idx_of = {}, {}, {}
    for fnr, dets in enumerate(gold['clusters']):
        keys = [(fnr, cid) for cid, _ in dets]
        for (cid, idx) in dets:
            med[(fnr, cid)] = np.median(X[fnr][idx], axis=0)
            cnt[(fnr, cid)] = len(idx)
            idx_of[(fnr, cid)] = np.asarray(idx)
        centers = np.array([med[k] for k in keys]) if keys else np.zeros((0, 5), np.float32)
        tr.next(fnr, keys, centers, [cnt[k] for k in keys], lambda k: (med[k], cnt[k]))
    tr.finish()
    return tr, med, cnt, idx_of


def host_extents_of(X, idx_of, seen=None):
    """a fit_track_boxes `moving_extents` on the host entry point: one call per frame over that frame's pairs"""
    def extents(pairs):
        out = np.empty((len(pairs), 6))
        for fnr in sorted({k[0] for _, _, k, _, _ in pairs}):
            js = [j for j, p in enumerate(pairs) if p[2][0] == fnr]
            keys = sorted({pairs[j][2] for j in js})
            seg = np.r_[0, np.cumsum([len(idx_of[k]) for k in keys])]
            out[js] = oe.oriented_extents_host(X[fnr], np.concatenate([idx_of[k] for k in keys]), seg, [keys.index(pairs[j][2]) for j in js],
                                               [pairs[j][4] for j in js], [pairs[j][3] for j in js])
        R.assert_float32_safe(out)                                     # (every pair of every moving track)
        if seen is not None:
            seen.extend(pairs)
        return out
    return extents


def track_state(tr, tab):
    return ([(t.static, [None if b is None else np.asarray(b).tobytes() for b in t.clone_box], list(t.clone_static_track)) for t in tr.tracks_valid],
            {k: np.asarray(v).tobytes() for k, v in tab.box.items()}, dict(tab.static_track))


def test_fit_track_boxes_from_extents_leaves_the_same_state_and_gathers_no_moving_cluster(gold, scene):
    frames, poses, X = scene
    to_ego = lambda f: np.linalg.inv(poses[f]) @ poses[0]
    rect = lambda xy: so.minimum_bounding_rectangle(xy, all_edges=False)
    states = []
    for mode in ('points', 'extents'):
        tr, med, cnt, idx_of = run_tracker(gold, X)
        tab = tracking.DetectionTable()
        stat = {}
        for fnr, (dets, flags) in enumerate(zip(gold['clusters'], gold['static'])):
            for (cid, _), st in zip(dets, flags):
                stat[(fnr, cid)] = st
                tab.valid[(fnr, cid)] = True
        asked, seen = [], []

        def points_of(k):
            asked.append(k)
            return X[k[0]][idx_of[k]]
        how = dict(moving_extents=host_extents_of(X, idx_of, seen), count_of=cnt.__getitem__) if mode == 'extents' else {}
        tracking.fit_track_boxes(tr, tab, points_of, stat.__getitem__, to_ego, rect, median_of=med.__getitem__, **how)
        states.append(track_state(tr, tab))
        moving = [t for t in tr.tracks_valid if not t.static]
        assert len(moving) > 0
        if mode == 'extents':
            rest = [k for t in tr.tracks_valid if t.static for k in t.source]
            assert asked == rest                                       # the points of the other tracks, once each, and of no moving track
            only_moving = {k for t in moving for k in t.source} - set(rest)
            assert only_moving and not only_moving & set(asked)
            assert [p[2] for p in seen] == [k for t in moving for k in t.source]       # one call, every entry of every moving track
            assert all(t is tr.tracks_valid[p[0]] and t.source[p[1]] == p[2] for p in seen for t in [tr.tracks_valid[p[0]]])
            for t, g in zip(tr.tracks, gold['tracks']):
                assert t.static == g['track_static_fit']
                got = np.array([t.clone_box[i] if t.prediction[i] else tab.box[t.source[i]] for i in range(len(t))], dtype=np.float64)
                assert np.allclose(got, g['boxes_fit'], rtol=0, atol=2e-5), np.abs(got - g['boxes_fit']).max()
    assert states[0] == states[1]
    with pytest.raises(ValueError):
        tracking.fit_track_boxes(tr, tab, points_of, stat.__getitem__, to_ego, rect, moving_extents=lambda pairs: None)


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_empty_work(cases):
    case = cases['pairs300']
    base = dict(p=case['points'], stride=5, i=case['index'], s=case['seg'], C=40, pc=case['pair_cluster'], n=300,
                c=case['center3'], r=case['rot4'])
    guard = np.full((302, 6), -7.0)

    def call(**kw):
        a = dict(base, **kw)
        ptr = lambda v: None if v is None else v.ctypes.data_as(ctypes.c_void_p)
        out = None if a.get('o', 0) is None else ptr(guard[1:])
        return lib.vg_cluster_oriented_extents_host(ptr(a['p']), a['stride'], ptr(a['i']), ptr(a['s']), a['C'], ptr(a['pc']), a['n'],
                                                    ptr(a['c']), ptr(a['r']), out)
    assert call(n=-1) == 1 and call(C=-1) == 1
    assert call(stride=2) == 1 and call(stride=0) == 1 and call(stride=-5) == 1
    assert call(p=None) == 1 and call(i=None) == 1 and call(s=None) == 1 and call(c=None) == 1 and call(r=None) == 1 and call(o=None) == 1
    assert call(pc=None) == 1                                           # identity needs n_pairs == n_clusters
    assert call(pc=None, n=41) == 1 and call(pc=None, n=39) == 1
    assert np.all(guard == -7.0)                                        # nothing was written by a refused call
    assert call(n=0) == 0 and call(n=0, pc=None, c=None, r=None, o=None) == 0 and np.all(guard == -7.0)
    assert call(n=0, stride=2) == 1
    assert call(C=0, p=None, i=None, s=None) == 0                       # no cluster: every pair is out of range, nothing is read
    assert np.isnan(guard[1:301]).all() and np.all(guard[[0, 301]] == -7.0)
    assert call() == 0 and np.array_equal(R.bits(guard[1:301]), R.bits(host(case)))
    assert call(pc=None, n=40) == 0


def test_the_config_key_takes_host_or_device():
    assert oe.moving_boxes_mode(None) == 'host' and oe.moving_boxes_mode('host') == 'host' and oe.moving_boxes_mode('device') == 'device'
    for bad in ('bogus', 'Device', '', 1):
        with pytest.raises(ValueError, match=r'device\.moving_boxes'):
            oe.moving_boxes_mode(bad)

    # the stage dispatcher reads the key where it reads device.pack, before it builds anything
    from vilgod_amd import zero_shot_detector as zsd

    class Cfg(dict):
        __getattr__ = dict.__getitem__
    cfg = Cfg(device={'moving_boxes': 'bogus'}, pipeline=[], preprocessor=None, paths=Cfg(clip_model='/nonexistent'))
    with pytest.raises(ValueError, match=r'device\.moving_boxes'):
        zsd.ZeroShotDetector(Cfg(sequence_length=1), 'seq', cfg, None)
    text = open(os.path.join(os.path.dirname(HEADER), '..', 'tools', 'configs', 'preprocessing.yaml')).read()
    assert re.search(r'^\s+moving_boxes:\s*host\b', text, flags=re.M)
