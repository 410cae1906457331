"""The points-in-boxes kernel (csrc/points_in_boxes.hip k_points_in_boxes) on the GPU: against the 60-digit fixture of
tests/golden/make_points_in_boxes.py on every point of families A-D (the tie-zone bound that keeps family B decidable is derived in
tests/test_points_in_boxes_host.py), bit for bit against the host entry point on every launch below (the same per-pair code, no
library maths, no contraction), at the lane / wave / workgroup / chunk edges of its launch, along the chunk loop's barrier path, and
through PseudoLabelPipeline.label_proposals."""
import numpy as np
import pytest

import pib_ref as R
from vilgod_amd import points_in_boxes as pib

pytestmark = pytest.mark.gpu
CHUNK = pib.PIB_CHUNK


@pytest.fixture(scope='module')
def g():
    return R.fixture()


def _device(cuda, points, boxes):
    import torch
    return pib.points_in_boxes_gpu(torch.from_numpy(points).to(cuda), torch.from_numpy(boxes).to(cuda)).cpu().numpy()


@pytest.mark.parametrize('family', R.FAMILIES)
def test_kernel_equals_the_fixture_and_the_host_on_every_point(g, cuda, family):
    pts, boxes, want = g[f'{family}_points'], g[f'{family}_boxes'], g[f'{family}_expect']
    got = _device(cuda, pts, boxes)                                    # one batched launch: a set per batch element
    assert got.dtype == np.int32 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (family, len(bad), bad[:5], got[got != want][:5], want[got != want][:5])
    assert got.tobytes() == R.host_batched(pts, boxes).tobytes()


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 513])
def test_launch_edges_equal_the_host_bit_for_bit(cuda, n):
    for m in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        for batch in (1, 3):
            dtype = np.float32 if (m + batch) % 2 else np.float64
            pts, boxes = R.scene(n, m, batch, seed=1000 * n + 10 * m + batch, dtype=dtype)
            want = R.host_batched(pts, boxes)
            got = _device(cuda, pts, boxes)
            assert got.tobytes() == want.tobytes(), (n, m, batch, np.argwhere(got != want)[:5])
            if m == 0:
                assert np.all(got == -1)
                continue
            share = np.mean(want >= 0)
            print(f'N {n} M {m} B {batch}: {share:.2f} of the points inside a box')
            assert share >= 0.2, (n, m, batch, share)
            if batch == 3 and n >= 63:
                assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])      # a different answer per element
            if m > 2 * CHUNK and n >= 255:
                assert want.max() >= CHUNK                             # answers from beyond the first chunk


def test_point_stride_five_and_boxes_with_nine_columns(cuda):
    pts, boxes = R.scene(300, CHUNK + 3, 2, seed=77, point_cols=5, box_cols=9, dtype=np.float32)
    want = R.host_batched(pts, boxes)
    assert np.mean(want >= 0) >= 0.2
    assert _device(cuda, pts, boxes).tobytes() == want.tobytes()
    # non-contiguous views: every other point, the columns of a wider table
    import torch
    d_p, d_b = torch.from_numpy(pts).to(cuda), torch.from_numpy(boxes).to(cuda)
    got = pib.points_in_boxes_gpu(d_p[:, ::2, 1:4], d_b[:, :, 2:]).cpu().numpy()
    assert got.tobytes() == R.host_batched(np.ascontiguousarray(pts[:, ::2, 1:4]), np.ascontiguousarray(boxes[:, :, 2:])).tobytes()


def test_launch_on_another_stream(cuda):
    import torch
    pts, boxes = R.scene(513, CHUNK + 1, 1, seed=5, dtype=np.float64)
    d_p, d_b = torch.from_numpy(pts).to(cuda), torch.from_numpy(boxes).to(cuda)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        got = pib.points_in_boxes_gpu(d_p, d_b)
    side.synchronize()
    assert got.cpu().numpy().tobytes() == R.host_batched(pts, boxes).tobytes()


def test_numpy_form_and_box_heights(g, cuda):
    pts, props = g['E_points'], g['E_proposals']
    got = pib.points_in_boxes(pts, props)
    assert got.dtype == np.int64 and np.array_equal(got, pib.points_in_boxes_host(pts, props))
    heights = pib.get_box_heights(pts, props)
    assert np.array_equal(heights, g['E_heights'])
    assert np.array_equal(pib.points_in_boxes(pts, np.zeros((0, 7))), np.full(len(pts), -1))
    assert pib.points_in_boxes(np.zeros((0, 3)), props).shape == (0,)


# ---- the chunk loop ---------------------------------------------------------------------------------------------------------------
def test_only_box_is_the_last_of_the_third_chunk(cuda):
    boxes = R.far_boxes(3 * CHUNK)
    boxes[-1] = [0.5, -0.25, 0.1, 2.0, 1.0, 1.0, 0.7]
    pts = np.array([[0.5, -0.25, 0.1], [0.6, -0.2, 0.3], [40.0, 40.0, 0.0]], np.float32)
    got = _device(cuda, pts[None], boxes[None])[0]
    assert got.tolist() == [3 * CHUNK - 1, 3 * CHUNK - 1, -1]
    assert got.tobytes() == R.host_batched(pts[None], boxes[None]).tobytes()


def test_box_zero_wins_over_a_box_of_the_second_chunk(cuda):
    boxes = R.far_boxes(2 * CHUNK)
    boxes[0] = [0.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0]
    boxes[CHUNK + 17] = [0.2, 0.1, 0.0, 2.0, 2.0, 2.0, 0.4]
    pts = np.array([[0.1, 0.1, 0.0],            # inside both
                    [1.05, 0.3, 0.0]], np.float32)   # inside the second alone
    got = _device(cuda, pts[None], boxes[None])[0]
    assert got.tolist() == [0, CHUNK + 17]
    assert got.tobytes() == R.host_batched(pts[None], boxes[None]).tobytes()


def test_one_workgroup_whose_lanes_finish_in_different_chunks(cuda):
    """lane 0 finds its box in chunk 0 and then only keeps the barriers company; lane 255 finds its in the last chunk"""
    m = 2 * CHUNK + 1
    boxes = R.far_boxes(m)
    pts = np.zeros((256, 3), np.float32)
    pts[:, 0] = -500.0 - 10.0 * np.arange(256)                         # nobody's
    owner = {0: 5, 1: CHUNK, 63: CHUNK - 1, 64: CHUNK + 1, 128: 2 * CHUNK - 1, 254: 0, 255: m - 1}
    for lane, j in owner.items():
        pts[lane] = boxes[j, :3] + np.array([0.3, -0.2, 0.1])
    want = np.full(256, -1, np.int32)
    for lane, j in owner.items():
        want[lane] = j
    got = _device(cuda, pts[None], boxes[None])[0]
    assert np.array_equal(got, want)
    assert got.tobytes() == R.host_batched(pts[None], boxes[None]).tobytes()


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------
def _proposals(meta):
    props = [[*o['center'], o['dims'][0] + 0.3, o['dims'][1] + 0.3, o['dims'][2] + 0.3, o['yaw']] for o in meta['objects']]
    first = props[0]
    props.insert(0, [first[0] + 0.3, first[1] - 0.2, first[2], first[3], first[4] + 0.4, first[5], first[6] + 0.2])      # overlaps the next one
    props.insert(5, [74.0, -74.0, 40.0, 2.0, 2.0, 2.0, 0.3])                                                           # owns no point
    return np.array(props, np.float64)


def _equal_results(a, b):
    assert list(a) == list(b)
    for k in a:
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_label_proposals_on_a_20k_frame(cuda):
    import torch
    from vilgod_amd import synthetic
    from vilgod_amd.frame_state import FrameState, pack_clusters, INDEX_ALL_POINTS
    from vilgod_amd.pipeline import PseudoLabelPipeline
    from vilgod_amd.sequence_datasets import apply_transform
    pts, meta = synthetic.make_frame(12, 20_000, n_objects=12, return_meta=True)
    poses = synthetic.make_poses(2)
    pose, ref_pose = poses[1], poses[0]
    props = _proposals(meta)
    names = [f'p{k}' for k in range(len(props))]
    kw = dict(device=cuda, max_points=24_000, clip_model_path='/nonexistent', box_mode='fast', box_workers=0)
    host = PseudoLabelPipeline(pack='host', **kw)
    dev = PseudoLabelPipeline(pack='device', clip=host.clip, **kw)
    # (the ground segmentation carries state from frame to frame: the yardstick is a pipeline that runs the same two frames and nothing else)
    plain = PseudoLabelPipeline(pack='host', clip=host.clip, **kw)
    before = host.process_frame(pts, pose, ref_pose, fnr=1)
    plain_before = plain.process_frame(pts, pose, ref_pose, fnr=1)

    fs, res = host.label_proposals(pts, pose, ref_pose, props, names=names, fnr=1)
    probs = host.last_probs.cpu().numpy()
    # the lists equal the host's lists from points_in_boxes_host
    d_ref = host.to_ref(host.upload(pts), fs.transform_to_ref)
    ref = d_ref.cpu().numpy()
    props_ref = apply_transform(props, fs.transform_to_ref, box=True)
    ids, index, seg = pack_clusters(pib.points_in_boxes_host(ref, props_ref), None, 0.0)
    assert 5 not in ids and len(ids) == len(props) - 1 and 0 in ids and 1 in ids
    assert fs.index_space == INDEX_ALL_POINTS and fs.n_points == len(pts)
    assert np.array_equal(fs.cluster_ids, ids) and np.array_equal(fs.index, index) and np.array_equal(fs.seg_off, seg)
    assert np.array_equal(fs.boxes, props_ref[ids, :7])
    # classification and vote: the same kernels on the host-built lists
    want_fs = FrameState(1, pose, ref_pose)
    want_fs.set_proposals(props_ref, (ids, index, seg), names)
    w_probs, w_top1, w_score = host.classify(d_ref, *host.lists_to_device(index, seg), want_fs.transform_to_ego)
    w_names, w_win, w_final = host.vote_classes(want_fs, host.cls_key, np.ones(len(ids), bool), w_top1.cpu().numpy(), w_score.cpu().numpy())
    assert probs.tobytes() == w_probs.cpu().numpy().tobytes() and probs.shape[0] == len(ids) * host.projection.num_views
    e, w = fs.cls[host.cls_key], want_fs.cls[host.cls_key]
    for k in ('has', 'pred', 'detailed', 'score', 'name', 'final'):
        assert np.array_equal(e[k], w[k]) and (e[k].dtype == object or e[k].tobytes() == w[k].tobytes()), k
    keep = np.array([w_names[i] in host.class_names for i in w_win], bool)
    assert keep.any()
    _equal_results(res, {'boxes_lidar': props[ids[keep], :7], 'name': np.array([str(w_names[i]) for i in w_win[keep]]),
                         'score': np.array(w_final[keep]), 'moving': np.zeros(int(keep.sum()), bool)})
    assert np.array_equal(host.proposal_rows(fs), ids[keep])
    dets = fs.serialize['_detections']
    assert [d['object_class']['proposal'] for d in dets] == [names[i] for i in ids] and all(host.cls_key in d['object_class'] for d in dets)
    # pack='device' gives the same frame
    fs_d, res_d = dev.label_proposals(pts, pose, ref_pose, props, names=names, fnr=1)
    _equal_results(res, res_d)
    assert np.array_equal(fs_d.cluster_ids, ids) and np.array_equal(fs_d.index, index) and np.array_equal(fs_d.seg_off, seg)
    assert dev.last_probs.cpu().numpy().tobytes() == probs.tobytes()
    # nothing to label
    for p_, pts_ in ((np.zeros((0, 7)), pts), (props[5:6], pts), (props, pts[:0])):
        fs_e, res_e = host.label_proposals(pts_, pose, ref_pose, p_, fnr=1)
        assert fs_e.n_detections == 0 and len(res_e['name']) == 0 and res_e['boxes_lidar'].shape == (0, 7)
    with pytest.raises(ValueError, match='proposals'):
        host.label_proposals(pts, pose, ref_pose, np.zeros((3, 6)))
    with pytest.raises(ValueError, match='names'):
        host.label_proposals(pts, pose, ref_pose, props, names=names[:-1])
    # ordinary frames before and after it return what they return without it
    after = host.process_frame(pts, pose, ref_pose, fnr=2)
    plain_after = plain.process_frame(pts, pose, ref_pose, fnr=2)
    for mine, want in ((before, plain_before), (after, plain_after)):
        _equal_results(mine[1], want[1])
        assert len(mine[1]['name']) > 0
        assert np.array_equal(mine[0].index, want[0].index) and np.array_equal(mine[0].seg_off, want[0].seg_off)
        assert np.array_equal(mine[0].ground_point_indices, want[0].ground_point_indices)
    torch.cuda.synchronize()
