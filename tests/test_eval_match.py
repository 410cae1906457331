"""The evaluation's matcher switch (vilgod_amd/evaluation.py detection_metrics(..., match=...)): the grouped assignment solver
(vilgod_amd/lap.py) in place of the scipy loop.  On the CPU the solver's host form drives the counting loop (match='reference') and
must give the scipy loop's matched pairs at every (frame, type, score cut-off) of the seeded scenes, whose best assignment leads by
1e-6 (test_iou_host.py::test_scene_seeds_meet_their_conditions); on the GPU all four (iou, match) combinations agree, and the command
line takes device.eval_match."""
import json
import logging
import os
import sys

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import iou_ref as R
from conftest import GOLDEN, ROOT
from vilgod_amd import evaluation as ev


def _scene_cfg():
    return ev.build_config(difficulties=[1, 2], breakdown_range=True, iou_thresholds=R.SCENE_THRESHOLDS[1:])


def _golden_calls():
    G = json.load(open(f'{GOLDEN}/eval_golden.json'))
    cfg = ev.build_config(difficulties=[1, 2], breakdown_range=False, iou_thresholds=[G['iou_threshold']] * 4)
    for case in G['cases']:
        gt, pd = np.array(case['gt'], np.float64), np.array(case['pd'], np.float64)
        yield case, (np.zeros(len(pd), np.int64), pd, np.ones(len(pd), int), np.array(case['score']),
                     np.zeros(len(gt), np.int64), gt, np.ones(len(gt), int), np.array(case['gt_level'], np.int8), cfg)


# ---- CPU: the solver's host form under the counting loop ------------------------------------------------------------------------------
def test_order_and_prefixes_describe_every_kept_set():
    cutoffs = ev.build_config()['score_cutoffs']
    scores = np.array([0.5, 0.9, 0.5, 0.123, 1.0, 0.0, 0.9])
    order, prefixes = ev.match_order_and_prefixes(scores, cutoffs)
    assert order.tolist() == [4, 1, 6, 0, 2, 3, 5]                            # score descending, index ascending among equals
    sizes = sorted({int(np.count_nonzero(scores >= c)) for c in cutoffs} - {0})
    assert prefixes.tolist() == sizes == [1, 3, 5, 6, 7]
    for c in cutoffs:
        keep = np.flatnonzero(scores >= c)
        assert sorted(order[:len(keep)].tolist()) == keep.tolist()           # every kept set is a prefix of the order
    order, prefixes = ev.match_order_and_prefixes(np.zeros(0), cutoffs)
    assert len(order) == 0 and len(prefixes) == 0


def test_reference_matcher_gives_the_scipy_loops_pairs_at_every_cutoff():
    cfg = _scene_cfg()
    cutoffs = np.asarray(cfg['score_cutoffs'])
    n_pairs = n_sets = 0
    for seed in R.SCENE_SEEDS:
        pf, pb, pt, ps, gf, gb, gt, _ = R.scene(seed)
        groups, ws = [], []
        for f in range(3):
            for t in (1, 2, 4):
                pi, gi = np.flatnonzero((pf == f) & (pt == t)), np.flatnonzero((gf == f) & (gt == t))
                iou = ev.iou3d_matrix(pb[pi], gb[gi])
                w = np.where((iou >= cfg['iou_thresholds'][t]) & (iou > 0), iou, 0.0)
                groups.append((w, ps[pi]))
        tables = ev._match_tables(groups, cutoffs, 'reference')
        for (w, sc), table in zip(groups, tables):
            for cut in cutoffs:
                keep = np.flatnonzero(sc >= cut)
                want = set()
                if len(keep) and w.shape[1]:
                    rr, cc = linear_sum_assignment(-w[keep])
                    want = {(int(keep[r]), int(c)) for r, c in zip(rr, cc) if w[keep[r], c] > 0}
                got = set()
                if len(keep):
                    col = table[len(keep)]
                    assert np.all(col[np.setdiff1d(np.arange(len(sc)), keep)] == -1)
                    got = {(int(i), int(col[i])) for i in keep if col[i] >= 0 and w[i, col[i]] > 0}
                assert got == want, (seed, cut)
                n_pairs += len(want)
                n_sets += 1
    assert n_pairs > 2000 and n_sets == 20 * 9 * 101


def test_reference_matcher_gives_the_default_metrics_exactly():
    cfg = _scene_cfg()
    for seed in R.SCENE_SEEDS:
        args = R.scene(seed) + (cfg,)
        assert ev.detection_metrics(*args, match='reference') == ev.detection_metrics(*args)
    for case, args in _golden_calls():
        ref, host = ev.detection_metrics(*args, match='reference'), ev.detection_metrics(*args, match='host')
        assert ref == host == ev.detection_metrics(*args), case['name']


def test_a_bogus_matcher_is_refused():
    args = R.scene(0) + (_scene_cfg(),)
    with pytest.raises(ValueError, match='match'):
        ev.detection_metrics(*args, match='bogus')
    with pytest.raises(ValueError, match='match'):
        ev.waymo_evaluation([], [], class_name=['Vehicle'], match='bogus')
    assert ev.MATCH_BACKENDS == ('host', 'device', 'reference')


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_all_four_combinations_on_the_seeded_scenes(cuda):
    cfg = _scene_cfg()
    n_positive = 0
    for seed in R.SCENE_SEEDS:
        args = R.scene(seed) + (cfg,)
        host = ev.detection_metrics(*args, iou='host', match='host')
        assert ev.detection_metrics(*args, iou='host', match='device') == host           # the matcher's input is identical
        for iou in ('host', 'device'):
            for match in ('host', 'device'):
                got = ev.detection_metrics(*args, iou=iou, match=match)
                assert list(got) == list(host)
                for k in host:
                    assert abs(got[k][0] - host[k][0]) <= 1e-12, (seed, iou, match, k, got[k], host[k])
        n_positive += sum(v[0] > 0 for v in host.values())
    assert n_positive > 100


@pytest.mark.gpu
def test_all_four_combinations_on_the_hand_computed_cases(cuda):
    names = []
    for case, args in _golden_calls():
        host = ev.detection_metrics(*args, iou='host', match='host')
        assert ev.detection_metrics(*args, iou='host', match='device') == host, case['name']
        for iou in ('host', 'device'):
            for match in ('host', 'device'):
                got = ev.detection_metrics(*args, iou=iou, match=match)
                assert list(got) == list(host)
                for k in host:
                    assert abs(got[k][0] - host[k][0]) <= 1e-12, (case['name'], iou, match, k)
        names.append(case['name'])
    assert 'hungarian_not_greedy' in names


def _eval_lines(caplog):
    return [r.getMessage() for r in caplog.records if ' AP ' in r.getMessage() or ' APH ' in r.getMessage()]


@pytest.mark.gpu
def test_cli_logs_the_same_evaluation_lines_with_the_device_matcher(cuda, tmp_path, caplog):
    """tools/preprocess_data.py on the synthetic set of test_iou_device.py::test_cli_logs_the_same_evaluation_lines:
    device.eval_match=device (alone and with device.eval_iou=device) logs the evaluation lines of the default; a bogus value is refused"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import preprocess_data
    stages = ['mask_ground_points', 'spatial_clustering', 'filter_detections', 'classification', 'fit_bounding_boxes_simple', 'evaluate_sequence']

    def run(mode, extra):
        root = str(tmp_path / mode)
        caplog.clear()
        with caplog.at_level(logging.INFO):
            res = preprocess_data.main(['preprocessor=waymo', f'dataset.DATA_PATH={root}', 'pipeline_active=[' + ','.join(stages) + ']',
                                        'pipeline.2.args.n_frames=1', 'dataset.SYNTHETIC.frames_per_sequence=2',
                                        'dataset.SYNTHETIC.points_per_frame=20000', 'dataset.SYNTHETIC.objects_per_frame=10',
                                        'dataset.SYNTHETIC.n_sequences=1', 'end_sequence=0', 'device.max_points=24000',
                                        'paths.clip_model=/nonexistent'] + extra)
        assert len(res) == 2 and sum(len(fr['name']) for fr in res) > 0
        return _eval_lines(caplog)
    lines = {'default': run('default', []), 'match': run('match', ['device.eval_match=device']),
             'both': run('both', ['device.eval_match=device', 'device.eval_iou=device'])}
    assert any('Vehicle AP  L2:' in ln for ln in lines['default']) and any(not ln.endswith(' 0.00') for ln in lines['default'])
    assert lines['match'] == lines['default'] and lines['both'] == lines['default']
    with pytest.raises(ValueError, match='match'):
        run('bogus', ['device.eval_match=bogus'])
