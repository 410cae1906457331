"""The box NMS kernels (csrc/nms.hip k_nms_rank, k_nms_mask, k_nms_reduce) on the GPU: bit for bit against vg_boxes_nms_host -- the same
per-pair and per-row text, which tests/test_nms_host.py holds to the numpy reference -- on every case of that file, at the cap, over
many groups, with a poisoned work buffer and from a captured graph; the pcdet call shapes; PseudoLabelPipeline.label_proposals with
its `nms` argument."""
import numpy as np
import pytest

import nms_ref as R
from vilgod_amd import iou, nms

pytestmark = pytest.mark.gpu


def _same(c, cuda, label, **kw):
    st_h, keep_h, counts_h = R.host_raw(c)
    st_d, keep_d, counts_d = R.device_raw(c, cuda, **kw)
    assert st_h == 0 and st_d == 0, label
    assert counts_d.tobytes() == counts_h.tobytes(), (label, counts_d[:8], counts_h[:8])
    assert keep_d.tobytes() == keep_h.tobytes(), (label, np.flatnonzero(keep_d != keep_h)[:5])
    return keep_h, counts_h


@pytest.fixture(scope='module')
def cases():
    return R.all_cases()


def test_every_host_case_equals_the_host_bit_for_bit(cases, cuda):
    for name, c in cases.items():
        keep, counts = _same(c, cuda, name)
        off = c['off']
        assert np.all(keep[:off[0]] == R.SENTINEL) and np.all(keep[off[-1]:] == R.SENTINEL), name      # slots of no group: untouched
    assert len(cases) > 80
    c = cases['r:small_max_group']
    assert R.host_raw(c)[2][1] == -1


def test_refusals_launch_nothing(cuda):
    n = nms.MAX_GROUP + 1
    c = R.case(R.far_boxes(n), np.linspace(1, 0, n), [0, n], 0.5)
    st, keep, counts = R.device_raw(c, cuda)                                     # max_group above the cap: VG_ERR_ARG, nothing written
    assert st == 1 and np.all(keep == R.SENTINEL) and np.all(counts == R.SENTINEL)
    st, keep, counts = R.device_raw(dict(c, max_group=nms.MAX_GROUP), cuda)     # the group is above max_group: marked by the kernels, no fault
    assert st == 0 and counts[0] == -1 and np.all(keep == -1)
    assert R.host_raw(dict(c, max_group=nms.MAX_GROUP))[2][0] == -1


@pytest.mark.parametrize('n', [4096, 4095])
def test_one_group_at_the_cap(cuda, n):
    assert nms.MAX_GROUP == 4096
    c = R.case(R.crowd(n, 7), R.crowd_scores(n, 7), [0, n], 0.5)          # about 2400 rows survive
    keep, counts = _same(c, cuda, n)
    print(f'n {n}: {counts[0]} kept')
    assert 64 < counts[0] < n - 64
    assert np.any(keep[:counts[0]] >= n - 64)                   # rows of the last word among them
    _same(dict(c, mode='normal', thresh=0.3), cuda, (n, 'normal'))


def test_199_groups_of_100_in_one_call(cuda):
    boxes = np.concatenate([R.crowd(100, 100 + g) for g in range(199)])
    scores = np.random.default_rng(12).uniform(0, 1, len(boxes)).astype(np.float32)
    c = R.case(boxes.astype(np.float32), scores, 100 * np.arange(200), 0.3)
    keep, counts = _same(c, cuda, '199 x 100')
    assert np.all(counts > 1) and np.all(counts < 100) and len(set(counts)) > 5
    # through the Python entry point, nothing read back by it
    import torch
    k, n = nms.nms_groups(torch.from_numpy(c['boxes']).to(cuda), torch.from_numpy(scores).to(cuda), c['off'], 0.3)
    assert k.is_cuda and n.is_cuda and k.dtype == torch.int32 and n.dtype == torch.int32
    assert np.array_equal(k.cpu().numpy(), keep) and np.array_equal(n.cpu().numpy(), counts)


def test_two_runs_and_a_poisoned_work_buffer_give_the_same(cases, cuda):
    for name in ('r:seams_f64', 'n:seams_f32', 'r:pre_max_65', 'r:padding_f64', 'crowd_512_0_0.5_float32'):
        c = cases[name]
        first = R.device_raw(c, cuda)
        again = R.device_raw(c, cuda)
        poisoned = R.device_raw(c, cuda, work_fill=0xFF)       # a mask word read without having been written would show
        for other in (again, poisoned):
            assert other[0] == 0 and other[1].tobytes() == first[1].tobytes() and other[2].tobytes() == first[2].tobytes(), name
        _same(c, cuda, name, work_fill=0xFF)


def test_captured_graph_replays_with_new_scores(cuda):
    import torch
    c = R.seam_case('rotated', np.float32, seed=1)
    d_boxes, d_scores = torch.from_numpy(c['boxes']).to(cuda), torch.from_numpy(c['scores']).to(cuda)
    d_off = torch.from_numpy(c['off'].astype(np.int32)).to(cuda)
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):                              # warm-up outside the capture
        nms.nms_groups(d_boxes, d_scores, d_off, c['thresh'], max_group=c['max_group'])
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize(cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                              # one stream: the three launches and the fills in front of them
        keep, counts = nms.nms_groups(d_boxes, d_scores, d_off, c['thresh'], max_group=c['max_group'])
    for scores in (c['scores'], np.random.default_rng(13).uniform(0, 1, len(c['scores'])).astype(np.float32)):
        d_scores.copy_(torch.from_numpy(scores).to(cuda))
        graph.replay()
        torch.cuda.synchronize(cuda)
        want_keep, want_counts = nms.nms_groups_host(c['boxes'], scores, c['off'], c['thresh'])
        assert np.array_equal(counts.cpu().numpy(), want_counts) and np.array_equal(keep.cpu().numpy(), want_keep)
    assert not np.array_equal(want_keep, nms.nms_groups_host(c['boxes'], c['scores'], c['off'], c['thresh'])[0])


def test_pcdet_call_shapes_against_the_numpy_reference(cuda):
    import torch
    b = np.c_[R.crowd(300, 3, np.float32), np.zeros((300, 2), np.float32)]          # [N, 9]: only the first 7 columns are read
    s = R.crowd_scores(300, 3, np.float32)
    for fn, mode, boxes in ((nms.nms_gpu, 'rotated', b), (nms.nms_normal_gpu, 'normal', np.c_[R.grid_crowd(300, 5), np.zeros((300, 2))])):
        for pre in (None, 100):
            out = fn(torch.from_numpy(boxes).to(cuda), torch.from_numpy(s).to(cuda), 0.3, pre_maxsize=pre, post_max_size=None)
            assert isinstance(out, tuple) and len(out) == 2 and out[1] is None
            keep = out[0]
            assert keep.is_cuda and keep.dtype == torch.int64 and keep.dim() == 1
            w_keep, w_counts = R.reference(R.case(boxes[:, :7], s, [0, 300], 0.3, mode, pre_max=pre))
            assert 1 < w_counts[0] < 300
            assert np.array_equal(keep.cpu().numpy(), w_keep[:w_counts[0]])
            assert np.all(np.diff(s[keep.cpu().numpy()].astype(np.float64)) <= 0)     # best first
    keep, none = nms.nms_gpu(torch.zeros((0, 7), device=cuda), torch.zeros(0, device=cuda), 0.5)
    assert keep.shape == (0,) and keep.dtype == torch.int64 and none is None
    with pytest.raises(ValueError, match='boxes'):
        nms.nms_gpu(torch.zeros((nms.MAX_GROUP + 1, 7), device=cuda), torch.zeros(nms.MAX_GROUP + 1, device=cuda), 0.5)
    with pytest.raises(ValueError, match='max_group'):
        nms.nms_groups(torch.zeros((4, 7), device=cuda), torch.zeros(4, device=cuda), torch.tensor([0, 4], dtype=torch.int32, device=cuda), 0.5)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------
def _proposals(meta):
    props = [[*o['center'], o['dims'][0] + 0.3, o['dims'][1] + 0.3, o['dims'][2] + 0.3, o['yaw']] for o in meta['objects']]
    props.insert(5, [74.0, -74.0, 40.0, 2.0, 2.0, 2.0, 0.3])                                                           # owns no point
    return np.array(props, np.float64)


def _equal_results(a, b):
    assert list(a) == list(b)
    for k in a:
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_label_proposals_with_nms_on_a_20k_frame(cuda):
    from vilgod_amd import synthetic
    from vilgod_amd.pipeline import PseudoLabelPipeline
    pts, meta = synthetic.make_frame(12, 20_000, n_objects=12, return_meta=True)
    poses = synthetic.make_poses(2)
    pose, ref_pose = poses[1], poses[0]
    props = _proposals(meta)
    P = len(props)
    names = [f'p{k}' for k in range(P)]
    scores = np.random.default_rng(14).uniform(0.3, 0.9, P)
    # every proposal duplicated with a 5 cm shift and a lower score, the duplicates in FRONT (the lowest-index rule favours them)
    dups = props.copy()
    dups[:, 0] += 0.05
    both, both_scores, both_names = np.r_[dups, props], np.r_[0.5 * scores, scores], [f'd{k}' for k in range(P)] + names
    bev = iou.iou_groups_host(both, [0, 2 * P], both, [0, 2 * P], iou.MODE_BEV)[0].reshape(2 * P, 2 * P)
    twin = np.zeros((2 * P, 2 * P), bool)
    twin[np.arange(P), P + np.arange(P)] = twin[P + np.arange(P), np.arange(P)] = True
    assert np.all(bev[twin] > 0.5) and np.all(bev[~twin & ~np.eye(2 * P, dtype=bool)] < 0.5)
    pipe = PseudoLabelPipeline(device=cuda, max_points=24_000, clip_model_path='/nonexistent', box_mode='fast', box_workers=0)

    fs0, res0 = pipe.label_proposals(pts, pose, ref_pose, props, names=names, fnr=1)            # the un-duplicated list
    probs0 = pipe.last_probs.cpu().numpy()
    rows0 = pipe.proposal_rows(fs0)
    assert len(res0['name']) > 0 and fs0.n_detections == P - 1

    fs1, res1 = pipe.label_proposals(pts, pose, ref_pose, both, names=both_names, fnr=1, scores=both_scores, nms={'thresh': 0.5})
    _equal_results(res1, res0)
    assert pipe.last_probs.cpu().numpy().tobytes() == probs0.tobytes()
    for k in ('cluster_ids', 'index', 'seg_off', 'boxes'):
        assert np.array_equal(getattr(fs1, k), getattr(fs0, k)) and getattr(fs1, k).dtype == getattr(fs0, k).dtype, k
    e1, e0 = fs1.cls[pipe.cls_key], fs0.cls[pipe.cls_key]
    for k in ('has', 'pred', 'detailed', 'score', 'name', 'final'):
        assert np.array_equal(e1[k], e0[k]) and (e1[k].dtype == object or e1[k].tobytes() == e0[k].tobytes()), k
    assert np.array_equal(pipe.proposal_rows(fs1), P + rows0)                                   # the original, higher-scored rows
    assert np.array_equal(fs1.proposal_index, P + np.arange(P))
    assert [d['object_class']['proposal'] for d in fs1.serialize['_detections']] == [names[i] for i in fs0.cluster_ids]
    # the other mode and a float32 list go the same way
    fs2, res2 = pipe.label_proposals(pts, pose, ref_pose, both, fnr=1, scores=both_scores.astype(np.float32), nms={'thresh': 0.5, 'mode': 'normal', 'pre_maxsize': None})
    assert np.array_equal(pipe.proposal_rows(fs2), P + rows0)

    # without nms the duplicated list gives what it gives today: the duplicates in front own the points
    fs3, res3 = pipe.label_proposals(pts, pose, ref_pose, both, names=both_names, fnr=1)
    probs3 = pipe.last_probs.cpu().numpy()
    fs4, res4 = pipe.label_proposals(pts, pose, ref_pose, both, names=both_names, fnr=1, scores=both_scores)
    _equal_results(res3, res4)
    assert pipe.last_probs.cpu().numpy().tobytes() == probs3.tobytes() and np.array_equal(fs3.cluster_ids, fs4.cluster_ids)
    assert np.any(fs3.cluster_ids < P) and fs3.proposal_index is None and set(pipe.proposal_rows(fs3)) <= set(fs3.cluster_ids)
    # everything suppressed but one
    fs5, res5 = pipe.label_proposals(pts, pose, ref_pose, both, fnr=1, scores=both_scores, nms={'thresh': -1.0})
    assert fs5.n_detections <= 1 and len(fs5.proposal_index) == 1 and fs5.proposal_index[0] == np.argmax(both_scores)
