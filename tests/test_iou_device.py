"""The rotated-box IoU kernel (csrc/iou.hip k_boxes_iou) on the GPU: against the 60-digit reference of tests/golden/make_iou.py under
the bar of tests/iou_ref.py (per pair min(max(8 * E_host[family], 2^-50), 2^-50 + 2^-44 R^2 / U); E_host = 5.551e-16 / 4.286e-10 /
4.286e-10 / 2.776e-16 / 3.343e-14 for A .. E), bit for bit against the host entry point (the same pair body, no library maths, no
contraction), at the lane / wave / workgroup edges of its flat work mapping, and through the evaluation's opt-in switch.
The share of the bar each family uses is printed (`pytest -s`)."""
import logging
import os
import sys

import numpy as np
import pytest

import iou_ref as R
from conftest import GOLDEN, ROOT
from vilgod_amd import evaluation as ev, iou

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g():
    return R.fixture()


@pytest.fixture(scope='module')
def device_values(g, cuda):
    """every fixture pair in ONE grouped launch per mode (one group per pair): {mode: [P] numpy}"""
    import torch
    a, b = torch.from_numpy(g['a']).to(cuda), torch.from_numpy(g['b']).to(cuda)
    off = R.one_group_per_pair(len(g['a']))
    return {mode: iou.iou_groups(a, off, b, off, mode)[0].cpu().numpy() for mode in (0, 1, 2)}


def test_every_family_meets_the_bar(g, device_values):
    R.check_against_bar(g, device_values, 'device')


def test_kernel_bits_equal_the_host_entry_points(g, device_values):
    off = R.one_group_per_pair(len(g['a']))
    for mode in (0, 1, 2):
        host, _ = iou.iou_groups_host(g['a'], off, g['b'], off, mode)
        diff = np.flatnonzero(host.view(np.uint64) != device_values[mode].view(np.uint64))
        assert len(diff) == 0, (mode, len(diff), diff[:5], host[diff[:5]], device_values[mode][diff[:5]])


def _boxes(g, n):
    return R.crowd(n)


@pytest.mark.parametrize('na,nb', [(1, 65), (65, 1), (64, 64), (257, 3)])
def test_matrix_shapes_across_lane_wave_and_workgroup_edges(g, cuda, na, nb):
    import torch
    a = _boxes(g, na)[0]
    b = _boxes(g, nb)[1]
    got = iou.boxes_iou3d(torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda))
    assert got.shape == (na, nb) and got.dtype == torch.float64
    want, _ = iou.iou_groups_host(a, [0, na], b, [0, nb])
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert np.count_nonzero(want) >= 3


def test_groups_with_empty_ones_and_a_thousand_single_pairs(g, cuda, device_values):
    import torch
    a, b = _boxes(g, 400)
    # seven groups: empty first, in the middle (no a rows, no b rows, neither) and last; sizes that straddle a 256-lane workgroup
    a_off, b_off = [0, 0, 70, 73, 73, 73, 330, 330], [0, 5, 9, 100, 100, 140, 143, 143]
    got, off = iou.iou_groups(torch.from_numpy(a).to(cuda), a_off, torch.from_numpy(b).to(cuda), b_off)
    want, off_h = iou.iou_groups_host(a, a_off, b, b_off)
    assert np.array_equal(off, off_h) and (np.diff(a_off) * np.diff(b_off)).tolist() == [0, 280, 273, 0, 0, 771, 0]
    assert got.cpu().numpy().tobytes() == want.tobytes() and np.count_nonzero(want) > 10
    # 1000 groups of 1 x 1
    sel = np.flatnonzero(g['family'] == 4)[:1000]
    one = R.one_group_per_pair(1000)
    got, _ = iou.iou_groups(torch.from_numpy(g['a'][sel]).to(cuda), one, torch.from_numpy(g['b'][sel]).to(cuda), one)
    assert got.cpu().numpy().tobytes() == device_values[0][sel].tobytes()
    # nothing to do
    e = torch.zeros((0, 7), dtype=torch.float64, device=cuda)
    assert iou.boxes_iou3d(e, torch.from_numpy(b[:5]).to(cuda)).shape == (0, 5)
    assert iou.boxes_iou3d(torch.from_numpy(a[:5]).to(cuda), e).shape == (5, 0)
    assert iou.iou_groups(e, [0], e, [0])[0].shape == (0,)


def test_output_outside_the_ranges_stays_untouched_and_bad_arguments_launch_nothing(g, cuda):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr
    a, b = _boxes(g, 40)
    d_a, d_b = torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda)
    a_off = torch.tensor([0, 20, 20, 40], dtype=torch.int32, device=cuda)
    b_off = torch.tensor([0, 15, 30, 40], dtype=torch.int32, device=cuda)
    out_off = torch.tensor([3, 310, 700], dtype=torch.int64, device=cuda)           # slack in front, between the groups and behind
    out = torch.full((1000,), -7.25, dtype=torch.float64, device=cuda)

    def call(dtype=1, mode=0, a_=d_a, ao=a_off, bo=b_off, oo=out_off, n=3, o=out):
        rc = lib.vg_boxes_iou3d(dtype, ptr(a_), ptr(ao), ptr(d_b), ptr(bo), n, ptr(oo), mode, ptr(o), stream_ptr())
        torch.cuda.synchronize()
        return rc

    bad_a = torch.tensor([0, 20, 10, 40], dtype=torch.int32, device=cuda)
    bad_o = torch.tensor([3, 200, 700], dtype=torch.int64, device=cuda)             # group 0 ends at 303
    assert call(dtype=2) == 1 and call(mode=3) == 1 and call(ao=bad_a) == 1 and call(oo=bad_o) == 1 and call(n=-1) == 1
    assert call(a_=None) == 1 and call(o=None) == 1
    assert torch.all(out == -7.25)
    assert call() == 0
    got = out.cpu().numpy()
    written = np.zeros(1000, bool)
    written[3:303] = True
    written[700:900] = True
    assert np.all(got[~written] == -7.25) and np.all(got[written] >= 0)
    want, _ = iou.iou_groups_host(a, [0, 20, 20, 40], b, [0, 15, 30, 40])
    assert np.concatenate([got[3:303], got[700:900]]).tobytes() == want.tobytes()
    empty = torch.zeros(2, dtype=torch.int32, device=cuda)
    assert call(a_=None, ao=empty, bo=empty, oo=out_off, n=1, o=None) == 0           # only empty groups: nothing read, nothing launched
    assert lib.vg_boxes_iou3d(1, None, None, None, None, 0, None, 0, None, stream_ptr()) == 0


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_pcdet_call_shape_returns_the_input_dtype(g, cuda, dtype):
    import torch
    a, b = _boxes(g, 30)
    a, b = a.astype(dtype), b.astype(dtype)
    extra = np.concatenate([a, np.full((30, 2), 9.0, dtype)], axis=1)                # [N, 9]: velocity columns behind the box are ignored
    for fn, mode in ((iou.boxes_iou3d, 0), (iou.boxes_iou_bev, 1)):
        got = fn(torch.from_numpy(extra).to(cuda), torch.from_numpy(b).to(cuda))
        assert got.dtype == getattr(torch, dtype) and got.shape == (30, 30) and got.is_cuda
        want, _ = iou.iou_groups_host(a, [0, 30], b, [0, 30], mode)
        assert torch.equal(got.cpu(), torch.from_numpy(want.reshape(30, 30)).to(getattr(torch, dtype)))
    with pytest.raises(ValueError):
        iou.boxes_iou3d(torch.from_numpy(a).to(cuda), torch.from_numpy(b.astype('float64' if dtype == 'float32' else 'float32')).to(cuda))
    with pytest.raises(ValueError):
        iou.boxes_iou3d(torch.from_numpy(a), torch.from_numpy(b))


def test_launch_on_another_stream(g, cuda):
    import torch
    a, b = _boxes(g, 100)
    d_a, d_b = torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    got, _ = iou.iou_groups(d_a, [0, 50, 100], d_b, [0, 50, 100], stream=side)
    side.synchronize()
    want, _ = iou.iou_groups_host(a, [0, 50, 100], b, [0, 50, 100])
    assert got.cpu().numpy().tobytes() == want.tobytes()


# ---- the evaluation's switch ---------------------------------------------------------------------------------------------------
def test_detection_metrics_on_the_hand_computed_cases(cuda):
    import json
    G = json.load(open(f'{GOLDEN}/eval_golden.json'))
    cfg = ev.build_config(difficulties=[1, 2], breakdown_range=False, iou_thresholds=[G['iou_threshold']] * 4)
    for case in G['cases']:
        gt, pd = np.array(case['gt'], np.float64), np.array(case['pd'], np.float64)
        args = (np.zeros(len(pd), np.int64), pd, np.ones(len(pd), int), np.array(case['score']),
                np.zeros(len(gt), np.int64), gt, np.ones(len(gt), int), np.array(case['gt_level'], np.int8), cfg)
        dev, host = ev.detection_metrics(*args, iou='device'), ev.detection_metrics(*args, iou='host')
        assert list(dev) == list(host)
        tol = case.get('tol', 1e-9)
        for k, want in case['expect'].items():
            assert abs(dev[f'OBJECT_TYPE_TYPE_VEHICLE_LEVEL_{k}'][0] - want) <= tol, (case['name'], k)
        for k in host:
            assert abs(dev[k][0] - host[k][0]) <= tol, (case['name'], k)


def test_detection_metrics_on_seeded_scenes(cuda):
    """20 scenes whose host IoUs keep 1e-6 from every threshold and whose best assignment leads by 1e-6 (asserted on the CPU:
    test_iou_host.py::test_scene_seeds_meet_their_conditions): the two IoUs differ by ~1e-15, so the same pairs match"""
    cfg = ev.build_config(difficulties=[1, 2], breakdown_range=True, iou_thresholds=R.SCENE_THRESHOLDS[1:])
    n_positive = 0
    for seed in R.SCENE_SEEDS:
        args = R.scene(seed) + (cfg,)
        dev, host = ev.detection_metrics(*args, iou='device'), ev.detection_metrics(*args, iou='host')
        assert list(dev) == list(host)
        for k in host:
            assert abs(dev[k][0] - host[k][0]) <= 1e-12, (seed, k, dev[k], host[k])
        n_positive += sum(v[0] > 0 for v in host.values())
    assert n_positive > 100


class _Frames:
    """what filter_for_evaluation reads of a data set"""
    point_cloud_range = np.array([-75.0, -75.0, -2.0, 75.0, 75.0, 4.0])

    def __init__(self, annos):
        self.infos = [{'annos': a} for a in annos]
        self.index_mapping = list(range(len(annos)))


def test_moving_static_removal_keeps_the_same_detections(cuda):
    rng = np.random.default_rng(11)
    annos, dets = [], []
    for f in range(2):
        n = 8
        gt = np.c_[rng.uniform(-40, 40, (n, 2)), rng.uniform(-0.5, 0.5, n), rng.uniform(3.5, 5, n), rng.uniform(1.6, 2.2, n), rng.uniform(1.4, 1.8, n),
                   rng.uniform(-np.pi, np.pi, n)].astype(np.float32)
        moving = np.arange(n) % 2 == 0
        annos.append(dict(name=np.array(['Vehicle'] * n), gt_boxes_lidar=gt, num_points_in_gt=np.full(n, 50), difficulty=np.ones(n, np.int32),
                          moving=moving))
        near = gt[:6].astype(np.float64) + np.c_[rng.normal(0, 0.3, (6, 2)), np.zeros((6, 4)), rng.normal(0, 0.1, 6)]       # on ground truth of both kinds
        far = np.c_[rng.uniform(50, 70, (4, 2)), np.zeros(4), np.full((4, 3), 2.0), rng.uniform(-3, 3, 4)]                    # on nothing
        boxes = np.concatenate([near, far])
        dets.append(dict(boxes_lidar=boxes, name=np.array(['Vehicle'] * 10), score=rng.uniform(0.1, 0.9, 10), moving=np.zeros(10, bool)))
        # the scene's premise: every detection the removal takes overlaps static ground truth by more than 1e-6, the others by nothing
        iou = ev.iou3d_matrix(boxes.astype(np.float32), gt[~moving])
        assert np.all((iou.max(axis=1) > 1e-6) | (iou.sum(axis=1) == 0))
    ds = _Frames(annos)
    kw = dict(eval_range=[-75.0, -75.0, 75.0, 75.0], moving=True, static=False)
    d_host, g_host = ev.filter_for_evaluation(ds, dets, ['Vehicle'], **kw, iou='host')
    d_dev, g_dev = ev.filter_for_evaluation(ds, dets, ['Vehicle'], **kw, iou='device')
    for x, y in zip(d_host + g_host, d_dev + g_dev):
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k
    assert [len(d['score']) for d in d_host] == [7, 7]               # three detections per frame sat on static ground truth
    with pytest.raises(ValueError):
        ev.filter_for_evaluation(ds, dets, ['Vehicle'], **kw, iou='bogus')


def _eval_lines(caplog):
    return [r.getMessage() for r in caplog.records if ' AP ' in r.getMessage() or ' APH ' in r.getMessage()]


def test_cli_logs_the_same_evaluation_lines(cuda, tmp_path, caplog):
    """tools/preprocess_data.py on the one-sequence synthetic set of tests/test_image_size.py (coherent here, so that it carries ground
    truth, with the box fit and the evaluation added to the stage list): device.eval_iou=device logs the evaluation lines of the default"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import preprocess_data
    stages = ['mask_ground_points', 'spatial_clustering', 'filter_detections', 'classification', 'fit_bounding_boxes_simple', 'evaluate_sequence']
    lines = {}
    for mode, extra in (('default', []), ('host', ['device.eval_iou=host']), ('device', ['device.eval_iou=device'])):
        root = str(tmp_path / mode)
        caplog.clear()
        with caplog.at_level(logging.INFO):
            res = preprocess_data.main(['preprocessor=waymo', f'dataset.DATA_PATH={root}', 'pipeline_active=[' + ','.join(stages) + ']',
                                        'pipeline.2.args.n_frames=1', 'dataset.SYNTHETIC.frames_per_sequence=2',
                                        'dataset.SYNTHETIC.points_per_frame=20000', 'dataset.SYNTHETIC.objects_per_frame=10',
                                        'dataset.SYNTHETIC.n_sequences=1', 'end_sequence=0', 'device.max_points=24000',
                                        'paths.clip_model=/nonexistent'] + extra)
        assert len(res) == 2 and sum(len(fr['name']) for fr in res) > 0
        lines[mode] = _eval_lines(caplog)
    assert any('Vehicle AP  L2:' in ln for ln in lines['default']) and any(not ln.endswith(' 0.00') for ln in lines['default'])
    assert lines['host'] == lines['default'] and lines['device'] == lines['default']
