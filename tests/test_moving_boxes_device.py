"""Motion-aligned track boxes from oriented extents, GPU side: k_cluster_oriented_extents (csrc/oriented_extent.hip) against the host
entry point -- which tests/test_moving_boxes_host.py holds against the exact reference on the same cases -- bit for bit, then
ZeroShotDetector's tracked box stage and the command line in device.moving_boxes=device against the default mode, for equal values."""
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

import moving_boxes_ref as R
from conftest import ROOT
from oracle import segment_oracle as so
from vilgod_amd import oriented_extents as oe
from vilgod_amd import synthetic
from vilgod_amd._lib import HEADER

pytestmark = pytest.mark.gpu

B = int(re.search(r'^#define\s+VG_OEXT_BLOCK\s+(\d+)', open(HEADER).read(), flags=re.M).group(1))
CASE_NAMES = ['sizes', 'large', 'pairs300', 'pairs1', 'pairs0', 'identity', 'out_of_range', 'geometry', 'nonfinite']
GUARD = 3


@pytest.fixture(scope='module')
def cases():
    return dict(R.kernel_cases(B))


@pytest.fixture(scope='module')
def pipe(cuda):
    from vilgod_amd.pipeline import PseudoLabelPipeline
    return PseudoLabelPipeline(device=torch.device('cuda:0'), max_points=70000, clip_model_path='/nonexistent', box_mode='reference')


def launch(pipe, case, tensors=False):
    """the case through PseudoLabelPipeline.oriented_extents into the middle of a NaN-filled buffer -> (extents, guard rows)"""
    dev = pipe.device
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    full = torch.full((len(case['center3']) + 2 * GUARD, 6), float('nan'), dtype=torch.float64, device=dev)
    out = full[GUARD:len(full) - GUARD]
    per_pair = (case['pair_cluster'], case['center3'], case['rot4'])
    got = pipe.oriented_extents(up(case['points']), up(case['index']), up(case['seg']), *(map(up, per_pair) if tensors else per_pair), out=out)
    assert got is out
    full = full.cpu().numpy()
    return full[GUARD:len(full) - GUARD], np.r_[full[:GUARD], full[len(full) - GUARD:]]


@pytest.mark.parametrize('stride', [3, 5])
@pytest.mark.parametrize('name', CASE_NAMES)
def test_kernel_equals_the_host_entry_point_bit_for_bit(pipe, cases, name, stride):
    case = R.with_stride(cases[name], stride)
    want = oe.oriented_extents_host(case['points'], case['index'], case['seg'], case['pair_cluster'], case['center3'], case['rot4'])
    got, guard = launch(pipe, case)
    assert got.shape == want.shape
    bad = np.argwhere(R.bits(got) != R.bits(want))
    assert len(bad) == 0, (name, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(R.bits(guard), R.bits(np.full((2 * GUARD, 6), float('nan'))))      # the rows before and after keep their NaN
    again, _ = launch(pipe, case, tensors=True)                                            # a second launch: the same bits
    assert np.array_equal(R.bits(again), R.bits(got))
    if name not in ('pairs0',):
        assert np.isfinite(want).any()
    if name in ('sizes', 'out_of_range', 'nonfinite'):
        assert np.isnan(want).all(axis=1).any() and not np.isnan(want).all()


def test_a_fresh_result_tensor_and_the_argument_checks(pipe, cases):
    case = cases['geometry']
    dev = pipe.device
    up = lambda a: torch.from_numpy(a).to(dev)
    X, index, seg = up(case['points']), up(case['index']), up(case['seg'])
    got = pipe.oriented_extents(X, index, seg, case['pair_cluster'], case['center3'], case['rot4'])
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (len(case['center3']), 6)
    want = oe.oriented_extents_host(case['points'], case['index'], case['seg'], case['pair_cluster'], case['center3'], case['rot4'])
    assert np.array_equal(R.bits(got.cpu().numpy()), R.bits(want))
    with pytest.raises(ValueError):
        pipe.oriented_extents(X, index, seg, case['pair_cluster'], case['center3'][:-1], case['rot4'])
    with pytest.raises(ValueError):
        pipe.oriented_extents(X, index, seg, up(case['pair_cluster']), up(case['center3']), up(case['rot4']).float())
    with pytest.raises(ValueError):
        pipe.oriented_extents(X, index, seg, case['pair_cluster'], case['center3'], case['rot4'],
                              out=torch.empty((len(case['center3']), 6), dtype=torch.float32, device=dev))


# ---- the tracked box stage of ZeroShotDetector on the golden scene of tests/test_tracking.py -----------------------------------
class Cfg(dict):
    __getattr__ = dict.__getitem__


def _detector(pipe, gold, scene, mode, tmp_path):
    from vilgod_amd import zero_shot_detector as zsd
    frames, poses, X = scene
    ds = Cfg(sequence_length=len(X), sequence_infos=[{'pose': p} for p in poses], class_names=['Vehicle', 'Pedestrian', 'Cyclist'])
    track = {'mode': 'cluster_center', 'min_length': 5, 'max_missed': 3,
             'assignment': {'method': 'assign_detections_greedy', 'max_distance': 1.0}}
    cfg = Cfg(device={'moving_boxes': mode, 'async_state_write': False, 'frames_in_flight': 1}, pipeline=[],
              pipeline_active=['track_clusters', 'fit_bounding_boxes_simple'],
              preprocessor=Cfg(tracking=Cfg(cluster=track)), paths=Cfg(clip_model='/nonexistent', sequence_data=str(tmp_path / mode)),
              postfix=Cfg(sequence_data='.pkl'))
    import logging
    det = zsd.ZeroShotDetector(ds, 'golden', cfg, logging.getLogger('test_moving_boxes'), pipeline=pipe)
    for fnr, (dets, flags) in enumerate(zip(gold['clusters'], gold['static'])):
        fs = det.lidar_frame_list[fnr]
        d_X = torch.from_numpy(X[fnr]).to(pipe.device)
        det._dev[fnr] = {'ref': d_X, 'X': d_X}                       # the scene's points ARE points_ref_wo_ground
        if dets:
            fs.set_clusters(np.array([cid for cid, _ in dets], np.int64), np.concatenate([np.asarray(i) for _, i in dets]).astype(np.int32),
                            np.r_[0, np.cumsum([len(i) for _, i in dets])].astype(np.int32))
            fs.static = np.array(flags, dtype=bool)
    return det


def test_tracked_box_stage_is_the_same_in_both_modes(pipe, golden_dir, tmp_path, monkeypatch):
    from vilgod_amd import boxes as vboxes
    from vilgod_amd import zero_shot_detector as zsd
    with open(os.path.join(golden_dir, 'track_golden.pkl'), 'rb') as f:
        gold = pickle.load(f)
    frames, poses = synthetic.make_sequence(seed=11, n_frames=18, n_points=5000, n_objects=9, moving_frac=0.6)
    X = []
    for f, p in zip(frames, poses):
        pr = so.apply_transform(f, np.linalg.inv(poses[0]) @ p)
        X.append(np.ascontiguousarray(pr[pr[:, 2] > 0.25]))
    calls = {'gather': 0, 'submit': 0, 'extents': 0}
    gather, submit, extents = zsd.ZeroShotDetector._cluster_points_host, vboxes.submit_moving_boxes, type(pipe).oriented_extents

    def count(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapped
    monkeypatch.setattr(zsd.ZeroShotDetector, '_cluster_points_host', count('gather', gather))
    monkeypatch.setattr(vboxes, 'submit_moving_boxes', count('submit', submit))
    monkeypatch.setattr(type(pipe), 'oriented_extents', count('extents', extents))
    state = {}
    for mode, drop_medians in (('host', False), ('device', False), ('device', True)):
        for k in calls:
            calls[k] = 0
        det = _detector(pipe, gold, (frames, poses, X), mode, tmp_path)
        assert det.moving_boxes == mode
        det.track_clusters()
        assert len(det.tracker.tracks) == len(gold['tracks'])
        if drop_medians:
            det._med = {}                                             # the tracker stage left no medians: the box stage asks the kernel itself
        det.fit_bounding_boxes_simple(None)
        assert det._host_X3 == {}
        if mode == 'host':
            assert calls['gather'] > 0 and calls['submit'] > 0 and calls['extents'] == 0
        else:
            assert calls['gather'] == 0 and calls['submit'] == 0
            moving_frames = {k[0] for t in det.tracker.tracks_valid if not t.static for k in t.source}
            assert calls['extents'] == len(moving_frames) > 0         # one launch per frame that holds an entry of a moving track
        state[(mode, drop_medians)] = [(fs.boxes, fs.static_track.copy(), fs.valid.copy()) for fs in det.lidar_frame_list]
        assert sum(int((st == 0).sum()) for _, st, _ in state[(mode, drop_medians)]) > 0      # entries of moving tracks exist
        for t, g in zip(det.tracker.tracks, gold['tracks']):
            assert t.static == g['track_static_fit']
    want = state[('host', False)]
    for key in (('device', False), ('device', True)):
        for (b0, s0, v0), (b1, s1, v1) in zip(want, state[key]):
            assert (b0 is None) == (b1 is None) and (b0 is None or np.array_equal(b0, b1, equal_nan=True))
            assert np.array_equal(s0, s1) and np.array_equal(v0, v1)


# ---- the command line -------------------------------------------------------------------------------------------------------------
OVR = ['dataset.SYNTHETIC.frames_per_sequence=6', 'dataset.SYNTHETIC.points_per_frame=20000', 'dataset.SYNTHETIC.objects_per_frame=10',
       'dataset.SYNTHETIC.n_sequences=1', 'end_sequence=0', 'device.max_points=24000', 'paths.clip_model=/nonexistent']     # tests/test_cli.py's
STAGES = ['mask_ground_points', 'calculate_entropy_scores', 'spatial_clustering', 'filter_detections', 'track_clusters',
          'classification', 'fit_bounding_boxes_simple', 'propagate_labels', 'evaluate_sequence']


def _load(root, seq='synthetic_train_0000'):
    out = []
    for path in (f'{root}/preprocessed_data/results/vilgod_mi355x/{"_".join(STAGES)}/{seq}.pkl',
                 f'{root}/preprocessed_data/results/vilgod_mi355x/{"_".join(STAGES)}/{seq}_indices.pkl',
                 f'{root}/preprocessed_data/vilgod_mi355x_seq/{seq}.pkl'):
        with open(path, 'rb') as f:
            out.append(pickle.load(f))
    return out


def test_cli_in_device_mode_writes_the_default_run_s_pickles(cuda, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import preprocess_data
    roots = {}
    for mode in ('host', 'device'):
        roots[mode] = str(tmp_path / mode)
        extra = ['device.moving_boxes=device'] if mode == 'device' else []          # the default run names no mode
        preprocess_data.main(['preprocessor=waymo', f'dataset.DATA_PATH={roots[mode]}'] + extra + OVR)
    (a, ia, sa), (b, ib, sb) = _load(roots['host']), _load(roots['device'])
    assert ia == ib and len(a) == len(b) == 6 and sum(len(fr['name']) for fr in a) > 0
    assert any(fr['moving'].any() for fr in a)                                     # a moving track reached the result
    for x, y in zip(a, b):
        assert np.array_equal(x['name'], y['name']) and np.array_equal(x['moving'], y['moving'])
        assert np.array_equal(x['boxes_lidar'], y['boxes_lidar']) and np.array_equal(x['score'], y['score'])
    for x, y in zip(sa, sb):
        assert len(x['_detections']) == len(y['_detections'])
        for d, e in zip(x['_detections'], y['_detections']):
            assert np.array_equal(d['cluster_points_index'], e['cluster_points_index']) and d['valid'] == e['valid']
            assert d['static'] == e['static'] and d.get('static_track') == e.get('static_track') and d['tid'] == e['tid']
            assert ('_bounding_box' in d) == ('_bounding_box' in e) and ('_bounding_box' not in d or np.array_equal(d['_bounding_box'], e['_bounding_box']))
